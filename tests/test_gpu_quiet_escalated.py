"""GPU tests of the contact-resolving launch over environments that touch nothing (per-environment escalation, csrc/sim_kernels.h:
RunOp::esc_role 2): an arm folded to within a millimetre or two of itself fails the lean launch's certificate, is stepped by the
contact-resolving kernel with a collision pass in every substep, and every one of those passes finds every pair apart.  Such a pass goes
straight to the geom pairs the slack record has due (csrc/contact_team.h: contact_collide, `pairs_only`); RCSH_CHECK_SKIP bit 6 (read on
every launch) runs the floor / box / compaction stages as before.

The environments are environments of the headline rollout (fr3_empty_world, relative +-5 deg joint actions, async control, 17 substeps a
launch), named by their seed of parity_util.synthetic_actions: over its first 280 steps each of them spends 21 to 77 launches on the
contact-resolving kernel without a contact ever being resolved.  Then the arms open (towards the home pose, 5 degrees a launch)."""

import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = (2699, 2588, 1058, 1401, 2356, 3704, 786, 1959, 2479, 3274)
STEPS = 280      # launches of the rollout
OPEN_STEPS = 10  # launches in which the arm opens
# Going back: on these inputs the parent of the pairs-only pass has every environment off the contact-resolving launch by the fifth
# launch of the opening (the last ones leave in launch index 4) and none comes back in the launches after it.
LEAVE_WITHIN = 5
SWITCH = "RCSH_CHECK_SKIP"


def _with_switch(value, fn):
    old = os.environ.get(SWITCH)
    try:
        if value is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = value
        return fn()
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


def _actions():
    from parity_util import synthetic_actions

    n = len(SEEDS)
    joints, grip = np.zeros((STEPS, n, 7)), np.zeros((STEPS, n), dtype=np.float32)
    for i, s in enumerate(SEEDS):
        j, g = synthetic_actions(1, STEPS, s)
        joints[:, i], grip[:, i] = j[:, 0], g[:, 0]
    return joints, grip


@functools.lru_cache(maxsize=None)
def _rollout(switch):
    """The kernels' rollout: per launch qpos, qvel, every observation and info array, truncation, both escalation masks, the action."""
    from parity_util import make_vec_env
    from rcs_amd.envs import MAX_JOINT_MOV
    from rcs_env_oracle import FR3_Q_HOME

    def run():
        n = len(SEEDS)
        joints, grip = _actions()
        venv = make_vec_env(n, True)
        assert venv.sim.resolve_robot_contacts == 7
        venv.reset()
        rec = []
        for t in range(STEPS + OPEN_STEPS):
            if t < STEPS:
                act = {"joints": joints[t], "gripper": grip[t]}
            else:
                q = np.asarray(venv.sim.qpos)[:, :7]
                act = {"joints": np.clip(np.asarray(FR3_Q_HOME)[None, :] - q, -MAX_JOINT_MOV, MAX_JOINT_MOV), "gripper": np.ones(n, dtype=np.float32)}
            obs, _, _, trunc, info = venv.step(act)
            now, ever = venv.sim.contact_escalated()
            rec.append({"qpos": np.array(venv.sim.qpos), "qvel": np.array(venv.sim.qvel), "obs": {k: np.array(v) for k, v in obs.items()},
                        "info": {k: np.array(v) for k, v in info.items()}, "trunc": np.array(trunc), "now": now.copy(), "ever": ever.copy(),
                        "act": {k: np.array(v) for k, v in act.items()}})
        venv.close()
        return rec

    return _with_switch(switch, run)


@functools.lru_cache(maxsize=None)
def _folded_arms(switch):
    """run_self_contact_parity(n_envs=24, seed=1, launches=40, mode=7)'s environments -- arms folded onto themselves, which DO touch --
    without its oracle: per launch qpos, qvel and both escalation masks."""
    from rcs_amd import sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_env_oracle import FR3_Q_HOME

    def run():
        n_envs = 24
        cfg = default_sim_robot_cfg("fr3_empty_world")
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=True), n_envs=n_envs, resolve_robot_contacts=7)
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
        rng = np.random.default_rng(1)
        q = np.tile(FR3_Q_HOME, (n_envs, 1))
        q[:, 0] = rng.uniform(-1, 1, n_envs)
        q[:, 1] = rng.uniform(-1.78, 0.2, n_envs)
        q[:, 3] = rng.uniform(-3.04, -2.6, n_envs)
        q[:, 4] = rng.uniform(-0.5, 0.5, n_envs)
        q[:, 5] = rng.uniform(0.55, 1.6, n_envs)
        simu.step(1)
        robot.set_joint_position(q)
        rec = []
        for _ in range(40):
            simu.step(17)
            now, ever = simu.contact_escalated()
            rec.append({"qpos": np.array(simu.qpos), "qvel": np.array(simu.qvel), "now": now.copy(), "ever": ever.copy()})
        simu.close()
        return rec

    return _with_switch(switch, run)


def _quiet_launches(rec):
    """per environment: launches spent on the contact-resolving kernel with no contact resolved so far"""
    return sum((r["now"] & ~r["ever"]).astype(int) for r in rec[:STEPS])


def test_quiet_escalated_environments_match_the_oracle():
    """Joint positions <= 1e-9, velocities <= 1e-8, flags bit-equal in every launch, for environments that sit on the contact-resolving
    launch and touch nothing (the oracle looks at every pair in every substep and sees no penetration either)."""
    from parity_util import make_oracle_envs

    rec = _rollout(None)
    n = len(SEEDS)
    oenvs = make_oracle_envs(n, True)
    assert oenvs[0].sim.model.resolve_contacts == 3
    for oe in oenvs:
        oe.reset()
    pen = np.zeros(n)
    err_q, err_v, flags = np.zeros(n), np.zeros(n), np.zeros(n, dtype=int)
    for r in rec:
        for e, oe in enumerate(oenvs):
            oe.sim.s.d.pen_seen = 0.0
            oo, _, _, otrunc, oi = oe.step({"joints": r["act"]["joints"][e], "gripper": r["act"]["gripper"][e]})
            pen[e] = max(pen[e], float(oe.sim.s.d.pen_seen))
            q, v = r["qpos"][e], r["qvel"][e]
            err_q[e] = max(err_q[e], float(np.abs(q - oe.sim.qpos[: q.shape[0]]).max()), float(np.abs(r["obs"]["joints"][e] - oo["joints"]).max()))
            err_v[e] = max(err_v[e], float(np.abs(v - oe.sim.qvel[: v.shape[0]]).max()))
            flags[e] += int(bool(r["info"]["collision"][e]) != bool(oi["collision"])) + int(bool(r["info"]["ik_success"][e]) != bool(oi["ik_success"]))
            flags[e] += int(bool(r["trunc"][e]) != bool(otrunc)) + int(float(r["obs"]["gripper"][e]) != float(oo["gripper"]))
    quiet = _quiet_launches(rec)
    ever = rec[STEPS - 1]["ever"]
    print(f"\nquiet escalated launches {quiet.tolist()}, resolved ever {ever.astype(int).tolist()}, oracle pen_seen {pen.tolist()}")
    print(f"max |dq| {err_q.tolist()}\nmax |dv| {err_v.tolist()}\nflag mismatches {flags.tolist()}")
    # the precondition: at least 8 environments escalated in at least 20 launches each, no contact ever resolved, none seen by the oracle
    ok = (quiet >= 20) & ~ever & (pen <= 1e-9)
    assert ok.sum() >= 8, (quiet, ever, pen)
    assert err_q.max() <= 1e-9 and err_v.max() <= 1e-8, (err_q, err_v)
    assert flags.sum() == 0, flags


def test_pairs_only_pass_equals_the_general_pass_bit_for_bit():
    """The same rollouts with the collision pass's shortcut (default) and with the stages it skips run in every pass (RCSH_CHECK_SKIP=64):
    every array the kernels leave is bit-equal after every launch -- environments that touch nothing, and folded arms that do (a pair the
    shortcut skipped and should have looked at would show as a contact missing here)."""
    a, b = _rollout(None), _rollout("64")
    assert len(a) == len(b) == STEPS + OPEN_STEPS
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in ("qpos", "qvel", "trunc", "now", "ever"):
            assert np.array_equal(ra[k], rb[k]), (t, k)
        for grp in ("obs", "info"):
            assert ra[grp].keys() == rb[grp].keys()
            for k in ra[grp]:
                assert np.array_equal(ra[grp][k], rb[grp][k]), (t, grp, k)
    fa, fb = _folded_arms(None), _folded_arms("64")
    for t, (ra, rb) in enumerate(zip(fa, fb)):
        for k in ("qpos", "qvel", "now", "ever"):
            assert np.array_equal(ra[k], rb[k]), ("folded arms", t, k)
    # (what was compared: quiet escalated launches in the first set, resolved contacts in the second)
    assert (_quiet_launches(a) >= 20).sum() >= 8
    assert fa[-1]["ever"].sum() >= 4, fa[-1]["ever"]


def test_opening_arm_leaves_the_contact_resolving_launch():
    """Going back: once the arms open, every environment is off the contact-resolving launch within LEAVE_WITHIN launches (the parent's
    own figure on these inputs) and stays off it."""
    rec = _rollout(None)
    assert rec[STEPS - 1]["now"].sum() >= 3, rec[STEPS - 1]["now"]  # (some are still on it when the opening begins)
    opening = rec[STEPS:]
    for k, r in enumerate(opening):
        if k >= LEAVE_WITHIN - 1:
            assert not r["now"].any(), (k, r["now"])
