"""The free box's substep (csrc/box_team.h: box_substep) against the CPU oracle, case by case: tests/box_cases.py.

One handle per scene, one environment per case (44 environments: neither a wavefront nor a grid row is full).  Right after it is made
the handle runs the table -- the states written, Sim.step(1) three times, then 22 substeps more -- and keeps what it read after 1, 2, 3
and 25 substeps; the tests below hold those numbers to the oracle and to the mpmath restatement of flight, and then use the same handle,
after rcsh_sim_reset_free_box, to ask that nothing but the state decides the result: not how the substeps are split into launches, not
where in the batch a case sits, not what the handle did before.

Bars (box_cases.py, the oracle's own spread on every case is 1/100 of them: test_box_cases_cpu.py): box velocity 1e-10, position and
quaternion 1e-12, robot joints 1e-9; flight against mpmath 1e-14 after one substep and 1.1e-14 after 25.  Measured on an MI355X
(profiles/box_substep/tests.txt): see the figures each test prints."""

import numpy as np
import pytest

import box_cases as B

pytestmark = pytest.mark.gpu

CASES = B.cases()
N = len(CASES)
ALONE = ("face+x-twist", "three-contacts", "noslip5-a", "flight-spin")  # the batch-of-one cases: sliding on a face, three contacts, five sweeps, flight


def _make(scene, n):
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg, xarm7_sim_robot_cfg

    if scene == "fr3_simple_pick_up":
        cfg = default_sim_robot_cfg(scene)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=n)
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
    else:
        cfg = xarm7_sim_robot_cfg(scene)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=n)
        robot = S.SimRobot(simu, None, cfg)
    robot.set_joint_position(np.tile(B.oracle(scene).home, (n, 1)))
    return simu


def _reset_box(simu):
    from rcs_amd import _lib

    _lib.check(simu._L.rcsh_sim_reset_free_box(simu._h))


def _read(simu):
    return simu.free_joint_qpos("box_joint").copy(), simu.free_joint_qvel("box_joint").copy(), simu.qpos.copy()


def _run_table(simu, rows, split=(1, 1, 1, 22)):
    """Write the rows' states and step; {substeps so far: (box qpos, box qvel, robot qpos)} after every launch."""
    simu.set_free_joint_qpos("box_joint", np.array([c["qpos"] for c in rows]))
    simu.set_free_joint_qvel("box_joint", np.array([c["qvel"] for c in rows]))
    out, k = {}, 0
    for n in split:
        simu.step(n)
        k += n
        out[k] = _read(simu)
    return out


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(scene):
        if scene not in made:
            simu = _make(scene, N)
            made[scene] = (simu, _run_table(simu, CASES))
        return made[scene]

    yield get
    for simu, _ in made.values():
        simu.close()


def _same_bits(a, b, k):
    """Box pose and velocity after k substeps, bit for bit (the robot is not the box's business: it has moved on between the runs)."""
    return np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1])


@pytest.mark.parametrize("scene", B.SCENES)
def test_designed_table_matches_the_oracle(handles, scene):
    _, fresh = handles(scene)
    ref = B.reference(scene)
    worst, late = {}, []
    for e, c in enumerate(CASES):
        w = worst.setdefault(c["cls"], np.zeros(4))
        for k in B.CHECKPOINTS:
            oq, ov, orq = ref[c["name"]][k]
            q, v, rq = fresh[k][0][e], fresh[k][1][e], fresh[k][2][e]
            d = np.array([np.abs(v - ov).max(), np.abs(q[:3] - oq[:3]).max(), np.abs(q[3:] - oq[3:]).max(), np.abs(rq - orq[: len(rq)]).max()])
            np.maximum(w, d, out=w)
            if d[0] > B.VEL_BAR or d[1] > B.POSE_BAR or d[2] > B.POSE_BAR or d[3] > B.ROBOT_BAR:
                late.append((c["name"], k, d.tolist()))
    for cls, w in worst.items():
        print(f"\n{scene} {cls}: kernel - oracle velocity {w[0]:.2e} position {w[1]:.2e} quaternion {w[2]:.2e} robot {w[3]:.2e}", end="")
    print()
    assert not late, late


@pytest.mark.parametrize("scene", B.SCENES)
def test_flight_matches_the_mpmath_restatement(handles, scene):
    _, fresh = handles(scene)
    late = []
    for e, c in enumerate(CASES):
        if not c["flight"]:
            continue
        mp = B.flight_reference(scene, c["name"])
        for k in (1, 25):
            dq, dv = float(np.abs(fresh[k][0][e] - mp[k][0]).max()), float(np.abs(fresh[k][1][e] - mp[k][1]).max())
            print(f"\n{scene} {c['name']}: kernel - mpmath after {k} substeps: pose {dq:.2e} velocity {dv:.2e}", end="")
            if max(dq, dv) > B.FLIGHT_BAR[k]:
                late.append((c["name"], k, dq, dv))
    print()
    assert not late, late


@pytest.mark.parametrize("scene", B.SCENES)
def test_one_launch_of_three_equals_three_launches_of_one(handles, scene):
    """The warm start and the remembered pose travel through LDS inside a launch and through memory between launches."""
    simu, fresh = handles(scene)
    _reset_box(simu)
    got = _run_table(simu, CASES, split=(3, 22))
    assert _same_bits(got, fresh, 3) and _same_bits(got, fresh, 25)


@pytest.mark.parametrize("scene", B.SCENES)
def test_result_does_not_depend_on_the_place_in_the_batch(handles, scene):
    """The batch reversed (every case in another team of its wavefront, next to other neighbours), and four cases alone in a batch of
    one: the quad sums must not see a neighbouring team."""
    simu, fresh = handles(scene)
    _reset_box(simu)
    got = _run_table(simu, CASES[::-1])
    for k in B.CHECKPOINTS:
        assert np.array_equal(got[k][0][::-1], fresh[k][0]) and np.array_equal(got[k][1][::-1], fresh[k][1]), k
    one = _make(scene, 1)
    for name in ALONE:
        e = B.names().index(name)
        _reset_box(one)
        got = _run_table(one, [CASES[e]])
        for k in B.CHECKPOINTS:
            assert np.array_equal(got[k][0][0], fresh[k][0][e]) and np.array_equal(got[k][1][0], fresh[k][1][e]), (name, k)
    one.close()


@pytest.mark.parametrize("scene", B.SCENES)
def test_reset_leaves_no_warm_start_behind(handles, scene):
    """After a rollout (25 substeps of the table shifted by one environment: every environment ends with another case's warm start)
    rcsh_sim_reset_free_box puts the box back, and the table's results are those of the fresh handle bit for bit."""
    simu, fresh = handles(scene)
    _run_table(simu, CASES[1:] + CASES[:1], split=(25,))
    # (what the reset is for: with the neighbour's warm start left in place Newton starts elsewhere and stops, inside the same gradient
    # test, at other bits -- within the bars, but not equal)
    stale = _run_table(simu, CASES, split=(1,))
    moved = [c["name"] for e, c in enumerate(CASES) if not np.array_equal(stale[1][1][e], fresh[1][1][e])]
    print(f"\n{scene}: without the reset {len(moved)} of {N} cases end on other bits, velocity apart by at most {np.abs(stale[1][1] - fresh[1][1]).max():.2e}")
    assert moved
    _run_table(simu, CASES[1:] + CASES[:1], split=(25,))
    _reset_box(simu)
    q0 = np.asarray(B.compiled(scene).free_bodies[0]["qpos0"])
    assert np.array_equal(simu.free_joint_qpos("box_joint"), np.tile(q0, (N, 1))) and not simu.free_joint_qvel("box_joint").any()
    got = _run_table(simu, CASES)
    for k in B.CHECKPOINTS:
        assert _same_bits(got, fresh, k), k
