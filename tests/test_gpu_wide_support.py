"""GPU tests of the hull rounds' shapes in the contact phase's narrow stage (csrc/contact_team.h: contact_collide): a lone pending pair
is refined by the whole wavefront (its hulls' support scans span 64 lanes), two pairs by 32 lanes each, three or four by a team of 16
each.  RCSH_CHECK_SKIP bit 7 (read on every launch) keeps every round on teams of 16.  The span changes how the vertices of a hull
are dealt out to lanes and how the lanes agree on the largest projection and the lowest tied index -- max and min, both exact -- so
every array the kernels leave must be BIT-equal between the two forms, after every launch.  Kernels against kernels: the 16-lane form
is held to the oracle by the rest of the suite.

Inputs (those of tests/test_gpu_quiet_escalated.py, restated here): ten environments of the headline rollout (fr3_empty_world, relative
+-5 deg joint actions, async control, 17 substeps a launch) that spend 21 to 77 of their first 280 launches on the contact-resolving
kernel with no contact ever resolved -- hull pairs within a millimetre or two, lone rounds --, then open; and 24 arms folded onto
themselves, which do touch: pad boxes and finger hulls against one link hull, rounds of two to four pairs next to lone ones.
(A support point that is wrong shows in the first set only as another size of a proven gap -- when a pair is due again, not what a step
leaves; a scratch build whose 64-lane maximum ignored half the rows passed it and failed the folded arms in launch 6:
profiles/wide_support/after.txt.)"""

import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEEDS = (2699, 2588, 1058, 1401, 2356, 3704, 786, 1959, 2479, 3274)
STEPS = 280      # launches of the rollout
OPEN_STEPS = 10  # launches in which the arm opens
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
    """Per launch: qpos, qvel, every observation and info array, truncation, both escalation masks."""
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
                        "info": {k: np.array(v) for k, v in info.items()}, "trunc": np.array(trunc), "now": now.copy(), "ever": ever.copy()})
        venv.close()
        return rec

    return _with_switch(switch, run)


@functools.lru_cache(maxsize=None)
def _folded_arms(switch):
    """24 arms folded onto themselves (rng(1)), 40 launches of 17 substeps: per launch qpos, qvel and both escalation masks."""
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


def _assert_rollouts_equal(a, b):
    assert len(a) == len(b) == STEPS + OPEN_STEPS
    for t, (ra, rb) in enumerate(zip(a, b)):
        for k in ("qpos", "qvel", "trunc", "now", "ever"):
            assert np.array_equal(ra[k], rb[k]), (t, k)
        for grp in ("obs", "info"):
            assert ra[grp].keys() == rb[grp].keys()
            for k in ra[grp]:
                assert np.array_equal(ra[grp][k], rb[grp][k]), (t, grp, k)
    # the precondition: at least 8 environments spend at least 20 launches escalated with no contact resolved
    quiet, ever = _quiet_launches(a), a[STEPS - 1]["ever"]
    print(f"\nquiet escalated launches {quiet.tolist()}, resolved ever {ever.astype(int).tolist()}")
    assert ((quiet >= 20) & ~ever).sum() >= 8, (quiet, ever)


def _assert_folded_equal(fa, fb):
    assert len(fa) == len(fb) == 40
    for t, (ra, rb) in enumerate(zip(fa, fb)):
        for k in ("qpos", "qvel", "now", "ever"):
            assert np.array_equal(ra[k], rb[k]), ("folded arms", t, k)
    # the precondition: at least 4 environments with a resolved contact at the end
    print(f"\nresolved ever {fa[-1]['ever'].astype(int).tolist()}")
    assert fa[-1]["ever"].sum() >= 4, fa[-1]["ever"]


def test_quiet_rollout_is_bit_equal_to_the_16_lane_form():
    """Environments that sit on the contact-resolving launch and touch nothing: lone hull pairs within a millimetre, round after round."""
    _assert_rollouts_equal(_rollout(None), _rollout("128"))


def test_folded_arms_are_bit_equal_to_the_16_lane_form():
    """Arms that touch themselves: rounds of one, two, three and four pairs, contacts recorded from the spans' first lanes."""
    _assert_folded_equal(_folded_arms(None), _folded_arms("128"))


def test_wide_rounds_compose_with_the_general_collision_pass():
    """Both sets with the pairs-only shortcut taken out (bit 6): bits 6 and 7 against bit 6 alone."""
    _assert_rollouts_equal(_rollout("64"), _rollout("192"))
    _assert_folded_equal(_folded_arms("64"), _folded_arms("192"))
