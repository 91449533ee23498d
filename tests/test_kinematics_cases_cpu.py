"""The case generator of tests/kinematics_cases.py, on the CPU: what the twin filter keeps, and that it cannot hide a class.

The GPU tests (tests/test_gpu_kinematics_edges.py) compare the kernels with the oracle on the rows the oracle reproduces itself on.  A
filter that dropped every hard row would make them pass for nothing, so the shares and the classes that must survive it are asserted
here, from the oracle alone; so are the counts that say the env-level actions really drive the limits, the clamp and the failures."""

import numpy as np
import pytest

import kinematics_cases as K

SPECIAL = ("near_pi", "small", "far", "edge")


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_twin_filter_keeps_every_class(robot):
    c = K.classified_cases(robot)
    cls, kept, ok, iters, angle0 = c["cls"], c["kept"], c["ok"], c["iters"], c["angle0"]
    # (the shares count the rows held to the oracle's success and iteration count; `kept` leaves out the near-pi rows of the 7-dof arms
    # that are exempt from the comparison of q alone -- the band count below is of `kept`: rows compared in full)
    share = {name: float(c["kept_counts"][cls == name].mean()) for name in ("wide", *SPECIAL)}
    in_band = kept & (angle0 >= np.pi - K.NEAR_PI) & (angle0 < np.pi)
    below_taylor = kept & (angle0 < K.K_TAYLOR)
    longest = int(iters[kept & ok].max())
    counts = {"rows": len(cls), "kept": int(kept.sum()), "kept failing": int((kept & ~ok).sum()),
              "kept with >= 200 iterations": int((kept & ok & (iters >= 200)).sum()), "longest kept success": longest,
              "near-pi band": int(in_band.sum()), "below kTaylor": int(below_taylor.sum()), "q-exempt": int(c["q_exempt"].sum()), "q-exempt held to the counts": int((c["q_exempt"] & c["kept_counts"]).sum())}
    branches = K.fk_branch_counts(robot)
    print(f"\n{robot}: kept shares {share}\n{robot}: {counts}\n{robot}: mat_to_quat branches (trace, x, y, z) {branches.tolist()}")
    assert (cls == "wide").sum() == K.N_WIDE and share["wide"] >= 0.75, share
    for name in SPECIAL:
        assert share[name] >= 0.5, (name, share)
    assert (cls == "far").sum() >= 4 and not ok[cls == "far"].any() and (iters[cls == "far"] == 1000).all()
    assert counts["kept failing"] >= 8 and in_band.sum() >= 8 and below_taylor.sum() >= 8, counts
    # successful rows that take 200 iterations and more.  Wide rows that take this long wander before they converge and no twin follows
    # them (0 kept of 31 / 0 / 6 / 16 such rows among 1200 wide rows of arm6 / so101 / fr3 / xarm7); the edge class has them on the 7-dof
    # arms, whose reach ends in a stretched, singular posture (up to 999 iterations).  The 5- and 6-dof arms' reach ends abruptly:
    # their rows take 200 iterations only within 1e-13 m of the edge, where the last bits of the error norm decide the success
    # (measured: the oracle's final error within 2e-17 of the threshold), which no implementation has to reproduce.  There the bar is a
    # run clearly longer than the 80 to 115 iterations of an ordinary one (a contraction by 0.9 from an error of 1 .. 10 to 1e-4).
    # The searches and their figures: profiles/kinematics_edges_tests.txt, section 4 (c) -- longest kept success 141 (arm6), 138 (so101).
    assert longest >= (200 if robot in ("fr3", "xarm7") else 120), counts
    assert (branches >= 8).all(), branches
    # the pure translations: the target's quaternion is the start pose's, bit for bit
    o = K.oracle_env(robot)
    start = K.vec7(o.sim.ik_forward(np.asarray(o.robot["q_home"], float), None) * K.tcp_offset(robot))
    pure = (cls == "small") & np.all(c["target"][:, 3:] == start[3:], axis=1)
    assert pure.sum() >= 1 and kept[pure].any() and (angle0[pure] < 1e-7).all(), (pure.sum(), angle0[pure])


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_kept_solutions_solve_the_problem(robot):
    """An anchor that does not go through the oracle's log: for every successful kept row, log6(frame(q)^-1 * target * tcp^-1) written in
    numpy on rcs_amd.common.Pose is below Pin::inverse's threshold.  "The kernel equals the oracle" then also means "solves the problem"."""
    c = K.classified_cases(robot)
    rows = np.flatnonzero(c["kept"] & c["ok"])
    res = np.array([K.residual_of_solution(robot, c["q"][r], c["target"][r]) for r in rows])
    print(f"\n{robot}: {len(rows)} solutions, largest residual {res.max():.9e}")
    # (the edge rows stop just under Pin's threshold -- the oracle's own error norm within 5e-12 of it -- and this log6 is another
    # formula: the bar leaves its round-off, 1e-6 relative, and not a differently rounded libm's last digit to decide)
    assert len(rows) >= 150 and res.max() <= 1e-4 * (1 + 1e-6), (len(rows), res.max())


@pytest.mark.parametrize("robot", K.ROBOTS)
def test_wavefront_layout(robot):
    """4 k + 3 rows; every row appears; every wavefront but the last two begins with a kept failing row and a kept quick row; one
    wavefront consists of kept failing rows only."""
    c, rows = K.classified_cases(robot), K.wavefront_layout(robot)
    assert len(rows) % 4 == 3 and set(rows.tolist()) == set(range(len(c["cls"])))
    fails, quick = c["kept"] & ~c["ok"], c["kept"] & c["ok"] & (c["iters"] <= c["iters"][c["kept"] & c["ok"]].min() + K.QUICK_ITERATIONS)
    waves = [rows[i:i + 4] for i in range(0, len(rows) - 3, 4)]
    mixed = sum(bool(fails[w[0]] and quick[w[1]] and c["ok"][w[2:]].any()) for w in waves)
    print(f"\n{robot}: {len(rows)} rows, {len(waves)} full wavefronts, {mixed} with a failing, a quick and another converging row")
    assert mixed > len(waves) // 2 and any(fails[w].all() for w in waves)


@pytest.mark.parametrize("robot,mode,relative_to", K.LIMIT_CONFIGS)
def test_limit_actions_bind(robot, mode, relative_to):
    case = K.limit_case(robot, mode, relative_to)
    print(f"\n{robot} {mode} {relative_to}: {K.limit_case_summary(case)}")
    n = K.LIMIT_ENVS * K.LIMIT_STEPS
    cut, classes = case["cut"], np.arange(K.LIMIT_ENVS) % 6
    assert 20 <= case["ik_fail"] < n // 2, case["ik_fail"]
    assert (case["split"] == K.LIMIT_STEPS).sum() >= 0.9 * K.LIMIT_ENVS, case["split"]
    if relative_to == "configured_origin":
        assert case["clamped"].sum() >= 4, case["clamped"]
    # the first step is the bare action: each class cuts what it says it cuts, and the class that EQUALS the limits cuts nothing.  So it is
    # in every step of last_step.  (configured_origin limits the pose product action * last_offset^-1, whose translation also carries
    # the turn applied to the last offset: from the second step on the translation is cut more often than the increments say.)
    steps = slice(None) if relative_to == "last_step" else slice(0, 1)
    assert np.array_equal(cut[steps, :, 0].all(axis=0), np.isin(classes, (0, 2, 5))) and np.array_equal(cut[steps, :, 0].any(axis=0), np.isin(classes, (0, 2, 5)))
    assert np.array_equal(cut[steps, :, 1].all(axis=0), np.isin(classes, (0, 3, 5))) and np.array_equal(cut[steps, :, 1].any(axis=0), np.isin(classes, (0, 3, 5)))
    assert cut[1:].any() and not cut[1:].all()
    if mode == "tquat":
        assert case["slerp_negative"] >= 20, case["slerp_negative"]  # slerp's d < 0 branch
        if relative_to == "last_step":
            assert (case["actions"][:, classes == 5, 6] < 0).all() and (case["actions"][:, classes != 5, 6] > 0).all()
    # an environment whose IK failed next to one that went on, in the same step
    fail = np.array([[not r["ik_success"] for r in row] for row in case["rec"]])
    assert (fail.any(axis=1) & ~fail.all(axis=1)).sum() >= 4
