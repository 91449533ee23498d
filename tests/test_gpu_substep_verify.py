"""GPU tests of the three-launch step of per-environment escalation (csrc/verify_team.h): the lean launch steps every
environment and records where each substep began, the verify launch runs the collision passes of the substeps of whoever failed the
certificate side by side, and the contact-resolving launch redoes from the copy only the environments one of those passes found touching.
RCSH_ESC_VERIFY=0 (read on every launch) selects the two launches of before: the lean launch over the environments not escalated, the
contact-resolving launch over the others, which continue from their state.

Bars: the project's 1e-9 (qpos) / 1e-8 (qvel) against the resolving oracle and between the two paths where the issue asks for them;
bit-equality where the two paths run the same kernel from the same state (an environment held in contact)."""

import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = "RCSH_ESC_VERIFY"
TRACE_CAP = 48  # kEscTraceCap (csrc/sim_kernels.h): substeps of the longest launch that takes the three-launch step
PATHS = (None, "0")  # the default, and the two launches of before


def _with_switch(value, fn, name=SWITCH):
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _fine_sim(n):
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=True), n_envs=n, resolve_robot_contacts=7)
    robot = S.SimRobot(simu, None, cfg)
    S.SimGripper(simu, default_sim_gripper_cfg())
    return simu, robot


# ---------------------------------------------------------------------------------------------------------------- 1. held contact
HELD = (1, 13, 16, 17)  # rows of parity_util.MANY_CONTACT_TARGETS: a hand driven into the floor, three arms folded onto themselves (and the floor)
HELD_WARMUP = 12        # launches towards the targets before the 30 that are compared: the contacts are made by then (asserted on the oracle)
HELD_LAUNCHES = 30
ENV_HELD = (1, 4, 6, 9)  # ... through the env layer, whose joint limits keep the folded poses out of reach: four hands driven into the floor
ENV_WARMUP = 82         # 5 degrees a launch: the last of the four touches the floor in launch 79


@functools.lru_cache(maxsize=None)
def _held(switch):
    from parity_util import MANY_CONTACT_TARGETS

    def run():
        simu, robot = _fine_sim(len(HELD))
        rec = []
        try:
            simu.step(1)
            robot.set_joint_position(MANY_CONTACT_TARGETS[list(HELD)])
            for t in range(HELD_WARMUP + HELD_LAUNCHES):
                # (the approach, under ONE path for both runs: a launch near a contact that touches nothing is stepped by the lean kernel
                # under one path and by the contact-resolving kernel under the other, and their rounding need not agree)
                _with_switch("0" if t < HELD_WARMUP else switch, lambda: simu.step(17))
                now, ever = simu.contact_escalated()
                rec.append({"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "now": now.copy(), "ever": ever.copy()})
        finally:
            simu.close()
        return rec

    return run()


@functools.lru_cache(maxsize=None)
def _held_oracle_contacts():
    """[environment, launch]: substeps of the launch in which the resolving oracle has a contact."""
    from parity_util import MANY_CONTACT_TARGETS, _many_contact_oracle
    from rcs_amd.envs import default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    cm = compile_mjcf(default_sim_robot_cfg("fr3_empty_world").mjcf_scene_path)
    out = np.zeros((len(HELD), HELD_WARMUP + HELD_LAUNCHES), dtype=int)
    for i, row in enumerate(HELD):
        o = _many_contact_oracle(cm, MANY_CONTACT_TARGETS[row])
        for t in range(out.shape[1]):
            for _ in range(17):
                o.step(1)
                out[i, t] += int(o.s.d.ncon > 0)
    return out


def test_held_contact_is_bit_equal_between_the_paths():
    """Four environments in contact in every one of 30 launches: under the default every launch is stepped by the lean launch, found
    touching and redone from the copy; under RCSH_ESC_VERIFY=0 the contact-resolving launch continues from the state.  The same kernel
    from the same state: qpos, qvel, `now` and `ever` are bit-equal after every launch (what the lean launch clobbered and the redo did
    not restore would show here)."""
    a, b = _held(None), _held("0")
    touching = _held_oracle_contacts()[:, HELD_WARMUP:]
    print(f"\nsubsteps in contact per launch (oracle), fewest per environment {touching.min(axis=1).tolist()}")
    assert (touching >= 1).all(), touching  # the precondition: every launch of every environment resolves at least one contact
    for t in range(HELD_WARMUP, HELD_WARMUP + HELD_LAUNCHES):
        assert a[t]["now"].all() and a[t]["ever"].all(), (t, a[t]["now"], a[t]["ever"])
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in ("qpos", "qvel", "now", "ever"):
            assert np.array_equal(ra[k], rb[k]), (t, k, np.abs(np.asarray(ra[k], dtype=float) - np.asarray(rb[k], dtype=float)).max())


def test_held_contact_env_layer_outputs_are_bit_equal_between_the_paths():
    """The same through the env layer, observations and info rows too: relative joint actions towards the same targets, 5 degrees a
    launch, ENV_WARMUP launches of approach under one path, then 30 launches that hold the targets."""
    from parity_util import make_oracle_envs

    recs = [_env_held(p) for p in PATHS]
    # the precondition, on the resolving oracle's env layer over the recorded actions: a penetration in every compared launch
    oenvs = make_oracle_envs(len(ENV_HELD), True)
    pen = np.zeros((len(ENV_HELD), ENV_WARMUP + HELD_LAUNCHES))
    for e, oe in enumerate(oenvs):
        oe.reset()
        for t, r in enumerate(recs[0]):
            oe.sim.s.d.pen_seen = 0.0
            oe.step({"joints": r["act"]["joints"][e], "gripper": r["act"]["gripper"][e]})
            pen[e, t] = float(oe.sim.s.d.pen_seen)
    print(f"\nenv layer: smallest per-launch penetration the oracle saw over the compared launches {pen[:, ENV_WARMUP:].min(axis=1).tolist()}")
    assert (pen[:, ENV_WARMUP:] > 1e-9).all(), pen[:, ENV_WARMUP:]
    for t, (ra, rb) in enumerate(zip(*recs)):
        if t >= ENV_WARMUP:
            assert ra["now"].all() and ra["ever"].all(), (t, ra["now"], ra["ever"])
        for k in ("qpos", "qvel", "now", "ever", "trunc"):
            assert np.array_equal(ra[k], rb[k]), (t, k)
        for grp in ("obs", "info"):
            for k in ra[grp]:
                assert np.array_equal(ra[grp][k], rb[grp][k]), (t, grp, k)


@functools.lru_cache(maxsize=None)
def _env_held(switch):
    from parity_util import MANY_CONTACT_TARGETS, make_vec_env
    from rcs_amd.envs import MAX_JOINT_MOV

    def run():
        n = len(ENV_HELD)
        tg = MANY_CONTACT_TARGETS[list(ENV_HELD)]
        venv = make_vec_env(n, True)
        rec = []
        try:
            venv.reset()
            for t in range(ENV_WARMUP + HELD_LAUNCHES):
                q = np.asarray(venv.sim.qpos)[:, :7]
                act = {"joints": np.clip(tg - q, -MAX_JOINT_MOV, MAX_JOINT_MOV), "gripper": np.ones(n, dtype=np.float32)}
                obs, _, _, trunc, info = _with_switch("0" if t < ENV_WARMUP else switch, lambda: venv.step(act))
                now, ever = venv.sim.contact_escalated()
                rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "obs": {k: np.array(v) for k, v in obs.items()},
                            "info": {k: np.array(v) for k, v in info.items()}, "trunc": np.array(trunc), "now": now.copy(), "ever": ever.copy(),
                            "act": {k: np.array(v) for k, v in act.items()}})
        finally:
            venv.close()
        return rec

    return run()


# ------------------------------------------------------------------------------------------------- 2. quiet and grazing environments
QUIET_SEEDS = (2699, 2588, 1058, 1401, 1959, 3704)  # six of test_gpu_quiet_escalated.SEEDS
# 250 launches, not 150: by launch 150 no environment of that set has been on `now & ~ever` more than three times (measured: the first
# such launches are 138 .. 248), so the precondition below -- four environments with 20 or more -- cannot hold there; by launch 250 these
# six have 56, 26, 40, 42, 20 and 24
QUIET_STEPS = 250


def _quiet_actions():
    from parity_util import synthetic_actions

    n = len(QUIET_SEEDS)
    joints, grip = np.zeros((QUIET_STEPS, n, 7)), np.zeros((QUIET_STEPS, n), dtype=np.float32)
    for i, s in enumerate(QUIET_SEEDS):
        j, g = synthetic_actions(1, QUIET_STEPS, s)
        joints[:, i], grip[:, i] = j[:, 0], g[:, 0]
    return joints, grip


@functools.lru_cache(maxsize=None)
def _quiet(switch):
    from parity_util import make_vec_env

    def run():
        n = len(QUIET_SEEDS)
        joints, grip = _quiet_actions()
        venv = make_vec_env(n, True)
        rec = []
        try:
            venv.reset()
            for t in range(QUIET_STEPS):
                obs, _, _, trunc, info = venv.step({"joints": joints[t], "gripper": grip[t]})
                now, ever = venv.sim.contact_escalated()
                rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "obs": {k: np.array(v) for k, v in obs.items()},
                            "info": {k: np.array(v) for k, v in info.items()}, "trunc": np.array(trunc), "now": now.copy(), "ever": ever.copy()})
        finally:
            venv.close()
        return rec

    return _with_switch(switch, run)


@functools.lru_cache(maxsize=None)
def _quiet_oracle():
    """The resolving oracle's env layer over the same actions, computed once: per launch qpos, qvel, observations, flags."""
    from parity_util import make_oracle_envs

    n = len(QUIET_SEEDS)
    joints, grip = _quiet_actions()
    oenvs = make_oracle_envs(n, True)
    assert oenvs[0].sim.model.resolve_contacts == 3
    for oe in oenvs:
        oe.reset()
    out = []
    for t in range(QUIET_STEPS):
        row = []
        for e, oe in enumerate(oenvs):
            oo, _, _, otrunc, oi = oe.step({"joints": joints[t, e], "gripper": grip[t, e]})
            row.append({"qpos": np.array(oe.sim.qpos), "qvel": np.array(oe.sim.qvel), "joints": np.array(oo["joints"]), "gripper": float(oo["gripper"]),
                        "collision": bool(oi["collision"]), "ik_success": bool(oi["ik_success"]), "trunc": bool(otrunc)})
        out.append(row)
    return out


def _graze_rows():
    """Two rows of the certificate cases (17-substep form) whose contact begins and ends inside one launch: one against the floor, one of
    the arm against itself, each deep enough that the resolving and the non-resolving oracle part."""
    import certificate_cases as CC

    rows = CC.by_form("step17")
    floor = next(r for r in rows if r["family"] == "floor-deep")
    self_ = next(r for r in rows if r["family"] == "self-deep")
    return [floor, self_]


@functools.lru_cache(maxsize=None)
def _graze(switch):
    import certificate_cases as CC

    def run():
        rows = _graze_rows()
        simu, robot = _fine_sim(len(rows))
        q0 = np.array([CC.start_state(r)[0] for r in rows])
        v0 = np.array([CC.start_state(r)[1] for r in rows])
        tg = np.array([CC.targets(r) for r in rows])
        rec = []
        try:
            simu.step(1)
            robot.set_joints_hard(np.ascontiguousarray(q0[:, :7]))
            simu.set_qpos(np.ascontiguousarray(q0))
            simu.set_qvel(np.ascontiguousarray(v0))
            for t in range(tg.shape[1]):
                robot.set_joint_position(np.ascontiguousarray(tg[:, t]))
                simu.step(17)
                now, ever = simu.contact_escalated()
                rec.append({"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "now": now.copy(), "ever": ever.copy()})
        finally:
            simu.close()
        return rec

    return _with_switch(switch, run)


@pytest.mark.parametrize("switch", PATHS)
def test_quiet_and_grazing_environments_match_the_oracle(switch):
    """Under either path: 1e-9 / 1e-8 against the resolving oracle and flags bit-equal, in every launch, for environments that fail the
    certificate for dozens of launches without touching anything and for two whose contact begins and ends inside one launch."""
    import certificate_cases as CC

    rec, orc = _quiet(switch), _quiet_oracle()
    n = len(QUIET_SEEDS)
    err_q, err_v, flags = np.zeros(n), np.zeros(n), np.zeros(n, dtype=int)
    for r, orow in zip(rec, orc):
        for e, o in enumerate(orow):
            q, v = r["qpos"][e], r["qvel"][e]
            err_q[e] = max(err_q[e], float(np.abs(q - o["qpos"][: q.shape[0]]).max()), float(np.abs(r["obs"]["joints"][e] - o["joints"]).max()))
            err_v[e] = max(err_v[e], float(np.abs(v - o["qvel"][: v.shape[0]]).max()))
            flags[e] += int(bool(r["info"]["collision"][e]) != o["collision"]) + int(bool(r["info"]["ik_success"][e]) != o["ik_success"])
            flags[e] += int(bool(r["trunc"][e]) != o["trunc"]) + int(float(r["obs"]["gripper"][e]) != o["gripper"])
    quiet = sum((r["now"] & ~r["ever"]).astype(int) for r in rec)
    print(f"\npath {switch}: launches in now & ~ever {quiet.tolist()}, ever {rec[-1]['ever'].astype(int).tolist()}")
    print(f"max |dq| {err_q.tolist()}\nmax |dv| {err_v.tolist()}\nflag mismatches {flags.tolist()}")
    g_rows, g_rec = _graze_rows(), _graze(switch)
    g_err = []
    for e, row in enumerate(g_rows):
        o = CC.replay(row)
        dq = max(float(np.abs(r["qpos"][e] - o["qpos"][t]).max()) for t, r in enumerate(g_rec))
        dv = max(float(np.abs(r["qvel"][e] - o["qvel"][t]).max()) for t, r in enumerate(g_rec))
        g_err.append((row["name"], dq, dv, "".join(str(int(r["now"][e])) for r in g_rec), bool(g_rec[-1]["ever"][e])))
    print("grazing (name, |dq|, |dv|, `now` after each launch, ever):", g_err)
    # the preconditions: at least 4 environments spend 20 or more launches in now & ~ever; both grazing environments end in `ever`
    assert (quiet >= 20).sum() >= 4, quiet
    assert all(g[4] for g in g_err), g_err
    assert err_q.max() <= 1e-9 and err_v.max() <= 1e-8, (err_q, err_v)
    assert flags.sum() == 0, flags
    assert max(g[1] for g in g_err) <= 1e-9 and max(g[2] for g in g_err) <= 1e-8, g_err


def test_quiet_and_grazing_flags_are_equal_between_the_paths():
    """`ever` and the info flags are equal at every launch between the default and RCSH_ESC_VERIFY=0."""
    a, b = _quiet(None), _quiet("0")
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["ever"], rb["ever"]), (t, ra["ever"], rb["ever"])
        assert np.array_equal(ra["trunc"], rb["trunc"]), t
        for k in ra["info"]:
            assert np.array_equal(ra["info"][k], rb["info"][k]), (t, k)
    for t, (ra, rb) in enumerate(zip(_graze(None), _graze("0"))):
        assert np.array_equal(ra["ever"], rb["ever"]), ("grazing", t, ra["ever"], rb["ever"])


# ------------------------------------------------------------------------------------------------------------------------ 3. shapes
SHAPE_ENV_STEPS = 90  # env steps: the hand of environment 0 reaches the floor in step 68
SHAPE_SCRIPT = (17,) * 8 + (1, 1, 1, TRACE_CAP, TRACE_CAP, TRACE_CAP + 1, TRACE_CAP + 1, 17, 17)  # substeps of the launches, in order


def _shape_targets(n, rows=(17, 13)):
    """Environment 0 (and the last one): an arm folded onto itself -- through the env layer, whose joint limits keep that pose out of
    reach, a hand driven into the floor --, touching after some launches and from then on; the others: seeded poses around home."""
    from parity_util import MANY_CONTACT_TARGETS
    from rcs_env_oracle import FR3_Q_HOME

    rng = np.random.default_rng(n)
    q = np.tile(np.asarray(FR3_Q_HOME, dtype=np.float64), (n, 1)) + rng.uniform(-0.3, 0.3, (n, 7))
    q[0] = MANY_CONTACT_TARGETS[rows[0]]
    if n > 2:
        q[n - 1] = MANY_CONTACT_TARGETS[rows[1]]
    return q


@functools.lru_cache(maxsize=None)
def _shape_fine(n, switch, verify_max=None):
    def run():
        simu, robot = _fine_sim(n)
        rec = []
        try:
            simu.step(1)
            robot.set_joint_position(_shape_targets(n))
            for k in SHAPE_SCRIPT:
                simu.step(k)
                now, ever = simu.contact_escalated()
                rec.append({"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "now": now.copy(), "ever": ever.copy()})
        finally:
            simu.close()
        return rec

    return _with_switch(verify_max, lambda: _with_switch(switch, run), "RCSH_VERIFY_MAX")


@functools.lru_cache(maxsize=None)
def _shape_env(n, switch):
    """Through the env layer: steps towards the targets, a reset under a mask (a launch with do_reset that sits some environments out --
    the folded arm among those that stay), more steps."""
    from parity_util import make_vec_env
    from rcs_amd.envs import MAX_JOINT_MOV

    def run():
        tg = _shape_targets(n, (1, 4))
        venv = make_vec_env(n, True)
        rec = []
        try:
            venv.reset()
            for t in range(SHAPE_ENV_STEPS):
                if t == SHAPE_ENV_STEPS - 10:
                    mask = np.zeros(n, dtype=np.uint8)
                    mask[1::2] = 1  # (environment 0, the folded arm, sits the reset out; n = 1: nobody is reset)
                    venv.reset(mask=mask)
                q = np.asarray(venv.sim.qpos)[:, :7]
                obs, _, _, trunc, info = venv.step({"joints": np.clip(tg - q, -MAX_JOINT_MOV, MAX_JOINT_MOV), "gripper": np.ones(n, dtype=np.float32)})
                now, ever = venv.sim.contact_escalated()
                rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "now": now.copy(), "ever": ever.copy(),
                            "joints": np.array(obs["joints"]), "collision": np.array(info["collision"])})
            # a reset of everybody: the launch with do_reset over the escalated environments too
            venv.reset()
            now, ever = venv.sim.contact_escalated()
            rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "now": now.copy(), "ever": ever.copy()})
        finally:
            venv.close()
        return rec

    return _with_switch(switch, run)


@pytest.mark.parametrize("n", (1, 5, 67))
def test_shapes_agree_between_the_paths(n):
    """n = 1, 5 and 67 (more than one mask word); launches of 1 substep, of exactly the trace's capacity and of one more (the two-launch
    step); a reset under a mask and a reset of everybody: the default against RCSH_ESC_VERIFY=0 at 1e-9 / 1e-8, `ever` equal."""
    for name, fn in (("fine", _shape_fine), ("env", _shape_env)):
        a, b = fn(n, None), fn(n, "0")
        dq = max(float(np.abs(ra["qpos"] - rb["qpos"]).max()) for ra, rb in zip(a, b))
        dv = max(float(np.abs(ra["qvel"] - rb["qvel"]).max()) for ra, rb in zip(a, b))
        work = sum(int(r["now"][0]) for r in a)
        print(f"\nn = {n} {name}: |dq| {dq:.2e} |dv| {dv:.2e}; launches after which environment 0 is escalated {work} of {len(a)}, ever {a[-2]['ever'].astype(int).sum()} of {n}")
        assert a[-2]["ever"][0] and work >= 5, (name, work)  # the folded arm gives the verify and the contact-resolving launch work
        assert dq <= 1e-9 and dv <= 1e-8, (name, dq, dv)
        for t, (ra, rb) in enumerate(zip(a, b)):
            assert np.array_equal(ra["ever"], rb["ever"]), (name, t)
            if "collision" in ra:
                assert np.array_equal(ra["collision"], rb["collision"]), (name, t)


def test_many_marked_environments_are_handed_on_unverified():
    """With more environments marked than the verify launch takes on (csrc/verify_team.h: kVerifyMaxFlagged; RCSH_VERIFY_MAX=0: any at
    all) every marked environment is redone from the copy unverified, which is what the two-launch step does with a newly marked one:
    the shapes' fine-grained script against RCSH_ESC_VERIFY=0 at 1e-9 / 1e-8, `ever` equal."""
    a, b = _shape_fine(5, None, "0"), _shape_fine(5, "0")
    dq = max(float(np.abs(ra["qpos"] - rb["qpos"]).max()) for ra, rb in zip(a, b))
    dv = max(float(np.abs(ra["qvel"] - rb["qvel"]).max()) for ra, rb in zip(a, b))
    print(f"\nhanded on unverified: |dq| {dq:.2e} |dv| {dv:.2e}; launches after which environment 0 is escalated {sum(int(r['now'][0]) for r in a)}")
    assert a[-1]["ever"][0] and dq <= 1e-9 and dv <= 1e-8, (dq, dv)
    for t, (ra, rb) in enumerate(zip(a, b)):
        assert np.array_equal(ra["ever"], rb["ever"]), t
