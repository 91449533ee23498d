"""The batched collision guard of the env layer (VecSimEnv.configure_guard / check_action, csrc/guard_team.h) against the oracle's
collision pass, the public motion query, and an oracle wrapper stack with the reference's CollisionGuard substitution in it."""

import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_collision_guard_cpu import MAX_MOV, absolute_command  # noqa: E402
from test_gpu_collision_query import BAND, _boxes, _fr3, _hand_rows  # noqa: E402

pytestmark = pytest.mark.gpu

OPEN = 0.04  # finger slides of the open hand (closed pads touch at a gap of exactly 0: such a pose is never certified)
DECISION_SEED = 11


def _venv(n, scene="fr3_empty_world", relative_to=None, async_control=True):
    """FR3 + hand, JOINTS mode; relative_to: None (absolute actions), "last_step" or "configured_origin"."""
    from rcs_amd import envs

    return envs.make_vec_env(n, async_control, relative=relative_to is not None, relative_to=relative_to or "last_step",
                             robot_cfg=envs.default_sim_robot_cfg(scene))


def _place(venv, q9, boxes=None):
    """Environments at the chain configurations q9 [N, 9] (arm joints: set_joints_hard; finger slides: qpos), cubes at `boxes`."""
    venv.robot.set_joints_hard(np.ascontiguousarray(q9[:, :7]))
    venv.sim.set_qpos(np.ascontiguousarray(q9))
    if boxes is not None:
        venv.sim.set_free_joint_qpos("box_joint", np.ascontiguousarray(boxes))


def decision_cases(orc, home, names, n=1024, seed=DECISION_SEED):
    """Test 1's environments: (q_now [n, 9], target [n, 7], class [n]) -- (a) near home, short moves; (b) above the floor, targets
    in it; (c) from home towards the folded self-contact pose of _hand_rows."""
    rng = np.random.default_rng(seed)
    base = np.concatenate([home, [OPEN, OPEN]])
    q = np.tile(base, (n, 1))
    tgt = np.tile(home, (n, 1))
    cls = np.zeros(n, dtype=int)
    k = n // 3
    q[:k, :7] += rng.uniform(-0.15, 0.15, (k, 7))
    tgt[:k] = q[:k, :7] + rng.uniform(-MAX_MOV, MAX_MOV, (k, 7))
    cls[k:2 * k] = 1
    tgt[k:2 * k, 1] = rng.uniform(1.2, 1.76, k)
    tgt[k:2 * k, 3] = rng.uniform(-1.0, -0.07, k)
    cls[2 * k:] = 2
    hand, must_hit = _hand_rows(orc, home, names)
    assert must_hit >= 3
    folded = hand[1, :7]
    m = n - 2 * k
    # (all the way to the folded pose and a little around it, or part of the way)
    tgt[2 * k:] = home + rng.uniform(0.3, 1.0, (m, 1)) * (folded - home) + rng.uniform(-0.02, 0.02, (m, 7))
    return q, tgt, cls


def oracle_samples(orc, q_from, q_to, box=None, kinds=7, samples=1001):
    """(a sampled contact?, a sample within BAND of the 1e-9 bar?) over `samples` evenly spaced points of the segment."""
    ts = np.linspace(0.0, 1.0, samples)
    d = q_to - q_from
    hit, near_bar = False, False
    for t in ts:
        p, near = orc.pairs(q_from + t * d if t < 1.0 else q_to, box)
        near_bar = near_bar or near < BAND
        hit = hit or any(p[k] for k in range(3) if kinds >> k & 1)
    return hit, near_bar


def test_decisions_against_the_oracle():
    """FR3 empty world, 1024 environments, JOINTS, absolute actions, peek only (issue's test 1).

    Ground truth: the oracle's collision pass at 1001 evenly spaced points of each segment.  Required: every environment with a
    sampled contact is blocked; result 0 never has one; result 1 has an oracle contact at t_contact; at most 10 % of class (a) --
    short moves near home, no oracle contact -- blocked; at least 100 of (b) and one of (c) blocked."""
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    n = 1024
    q, tgt, cls = decision_cases(orc, home, cm.geom_names, n)
    venv = _venv(n)
    venv.reset()
    _place(venv, q)
    venv.configure_guard(enabled=False)
    s0 = venv.sim.get_state().copy()
    blocked, result, tc = venv.check_action({"joints": tgt})
    assert (venv.sim.get_state() == s0).all()
    assert set(np.unique(result)) <= {0, 1, 2}
    assert np.array_equal(blocked, result != 0)  # (block_undecided)
    assert ((tc == -1.0) == (result != 1)).all()
    q_to = np.concatenate([tgt, q[:, 7:]], axis=1)
    contact = np.zeros(n, dtype=bool)
    aside = np.zeros(n, dtype=bool)
    for e in range(n):
        contact[e], aside[e] = oracle_samples(orc, q[e], q_to[e])
    keep = ~aside
    print("set aside near the bar:", int(aside.sum()), "| results (free, contact, undecided):", np.bincount(result, minlength=3),
          "| per class blocked:", [int(blocked[cls == c].sum()) for c in range(3)], "sampled contacts:", [int(contact[cls == c].sum()) for c in range(3)])
    assert aside.sum() < 0.01 * n, aside.sum()
    assert not contact[cls == 0].any(), "class (a) must be free of contact for the chosen seed: change the seed"
    assert blocked[keep & contact].all(), np.flatnonzero(keep & contact & ~blocked)
    assert not contact[keep & (result == 0)].any()
    for e in np.flatnonzero(keep & (result == 1)):
        assert orc.hit(q_to[e] if tc[e] == 1.0 else q[e] + tc[e] * (q_to[e] - q[e])), (e, tc[e])
    a = cls == 0
    over = float((blocked[a] & ~contact[a]).mean())
    print("class (a) blocked without a sampled contact:", over)
    assert over <= 0.10, over
    assert blocked[cls == 1].sum() >= 100 and blocked[cls == 2].sum() >= 1
    venv.close()


@pytest.mark.parametrize("scene", ["fr3_empty_world", "fr3_simple_pick_up"])
@pytest.mark.parametrize("relative_to", [None, "last_step", "configured_origin"])
def test_same_bits_as_the_public_query(scene, relative_to):
    """The peek's result and t_contact equal SimRobot.check_motion on (q_now, q_target, the environment's cube) exactly, with
    kinds 7 and 3; q_target from the numpy restatement of the relative action space (tests/test_collision_guard_cpu.py).  One
    earlier step makes CONFIGURED_ORIGIN's last action live."""
    simu, robot, orc, cm, home = _fr3(scene)
    n = 256
    rng = np.random.default_rng(21)
    has_box = scene == "fr3_simple_pick_up"
    venv = _venv(n, scene, relative_to)
    obs, _ = venv.reset()
    origin = obs["joints"].copy()  # RelativeActionSpace.reset: origin := current
    a0 = rng.uniform(-0.2, 0.2, (n, 7)) if relative_to else origin + rng.uniform(-0.05, 0.05, (n, 7))
    venv.step({"joints": a0, "gripper": np.ones(n, dtype=np.float32)})
    _, last = absolute_command(a0, venv.sim.qpos[:, :7], relative_to, origin=origin)
    # where the environments are: near home, above the floor, half folded; hands open; cubes anywhere around the hand
    q, _, _ = decision_cases(orc, home, cm.geom_names, n, seed=22)
    q[n // 3:2 * (n // 3), 1] = rng.uniform(0.6, 1.3, n // 3)
    q[n // 3:2 * (n // 3), 3] = rng.uniform(-1.5, -0.5, n // 3)
    boxes = _boxes(rng, n) if has_box else None
    _place(venv, q, boxes)
    q_now = venv.sim.qpos.copy()
    assert np.array_equal(q_now, q)
    box_now = venv.sim.free_joint_qpos("box_joint").copy() if has_box else None
    if relative_to is None:
        act = q[:, :7] + rng.uniform(-0.6, 0.6, (n, 7))
    else:
        act = rng.uniform(-0.3, 0.3, (n, 7))
    target, _ = absolute_command(act, q_now[:, :7], relative_to, origin=origin, last_action=last)
    q_to = np.concatenate([target, q_now[:, 7:]], axis=1)
    for kinds in (7, 3):
        venv.configure_guard(enabled=False, kinds=kinds, resolution=1e-3)
        blocked, result, tc = venv.check_action(act)
        want_r, want_t = venv.robot.check_motion(q_now, q_to, resolution=1e-3, free_qpos=box_now, kinds=kinds)
        assert np.array_equal(result, want_r), (kinds, np.flatnonzero(result != want_r)[:10])
        assert np.array_equal(tc, want_t), kinds
        print(scene, relative_to, "kinds", kinds, "results:", np.bincount(result, minlength=3))
        assert len(np.unique(result)) >= 2, "the inputs exercise one outcome only"
    venv.close()


def _guarded_oracle_env_class():
    from rcs_env_oracle import JOINTS, OracleEnv

    class GuardedOracleEnv(OracleEnv):
        """OracleEnv with the reference's CollisionGuard between RelativeActionSpace and RobotEnv.step: when `blocked`, the
        absolute command becomes the robot's current joint position (envs/sim.py:202) -- and the env steps on (the backend's
        documented deviation: hold and step, instead of returning the last observation)."""

        def step(self, action, blocked=False):
            if self.max_mov is not None:
                action = self._relative_action(action)
            else:
                action = copy.deepcopy(action)
            if blocked:
                action[JOINTS] = self.sim.get_joint_position()
            if self.has_gripper:
                g = np.clip(np.round(action["gripper"]), 0.0, 1.0)
                if g == 0:
                    self.sim.gripper_grasp()
                else:
                    self.sim.gripper_open()
                self._last_gripper_cmd = g
                del action["gripper"]
            a = np.asarray(action[JOINTS], dtype=np.float64)
            changed = self.prev_action is None or not np.allclose(a, self.prev_action[JOINTS], atol=1e-3, rtol=0)
            if changed:
                self.sim.set_joint_position(a)
            self.prev_action = copy.deepcopy(action)
            s = self.sim.s
            if s.async_control:
                self.sim.step(round(1 / s.frequency / self.timestep))
            else:
                self.sim.step_until_convergence()
            info = {"collision": bool(s.robot_collision), "ik_success": bool(s.ik_success), "is_sim_converged": self.sim.is_converged()}
            truncated = bool(s.robot_collision) or not bool(s.ik_success) or bool(blocked)
            obs, info = self._gripper_obs(self._get_obs(), info)
            return obs, 0, False, truncated, info

    return GuardedOracleEnv


def rollout_actions(n, steps, relative_to, home, seed):
    """[steps, n, 7] actions and the environments' class: 0 stays near home (small seeded moves), 1 is driven into the floor
    (shoulder forward, elbow down) to the end, 2 is driven towards the floor and back up."""
    rng = np.random.default_rng(seed)
    cls = np.arange(n) % 3
    down = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    act = np.zeros((steps, n, 7))
    level = np.zeros(n)  # how many 5-degree steps down the ramp of classes 1 and 2 stands
    walk = np.zeros((n, 7))
    for t in range(steps):
        dirn = np.where(cls == 1, 1.0, np.where(cls == 2, 1.0 if t < 0.6 * steps else -1.0, 0.0))
        small = rng.uniform(-0.02, 0.02, (n, 7)) * (cls == 0)[:, None]
        if relative_to == "last_step":
            act[t] = dirn[:, None] * MAX_MOV * down + small
        else:
            level += dirn
            walk += small
            offset = level[:, None] * MAX_MOV * down + walk
            act[t] = offset if relative_to == "configured_origin" else home + offset
    return act, cls


@pytest.mark.parametrize("async_control", [True, False])
@pytest.mark.parametrize("relative_to", [None, "last_step", "configured_origin"])
def test_step_does_what_the_wrapper_stack_would(relative_to, async_control):
    """64 environments, 60 guarded steps, each environment mirrored by an OracleEnv whose subclass substitutes the oracle's current
    joint position for the absolute command whenever the GPU reported the environment blocked in that step (issue's test 3).
    Ten unguarded steps come first, in both, to open the hands: closed pads touch at a gap of exactly 0, which no certificate
    clears.  info["collision"] is evaluated by step_until_convergence only (Sim::step never runs the collision callbacks), so
    the comparison with the unguarded control run is asserted with async_control off and printed otherwise."""
    from parity_util import rpy_error
    from rcs_amd.mjcf import compile_mjcf
    from rcs_env_oracle import FR3_Q_HOME, JOINTS

    n, steps, warm = 64, 60, 10
    home = np.asarray(FR3_Q_HOME)
    act, cls = rollout_actions(n, steps, relative_to, home, seed=31)
    stay = np.tile(home, (n, 1)) if relative_to is None else np.zeros((n, 7))
    grip = np.ones(n, dtype=np.float32)
    Guarded = _guarded_oracle_env_class()
    cm = compile_mjcf(_venv_scene_path())
    oenvs = [Guarded(cm, control_mode=JOINTS, gripper=True, max_relative_movement=MAX_MOV if relative_to else None,
                     relative_to=relative_to or "last_step", async_control=async_control) for _ in range(n)]

    # LAST_STEP follows its own lagging arm (5 degrees beyond where it IS, a step): from home the floor is more than 60 steps away, so
    # there the floor-bound classes start lowered (free of contact: the oracle's scan in decision_cases' neighbourhood)
    lowered = None
    if relative_to == "last_step":
        lowered = np.tile(home, (n, 1))
        lowered[cls != 0, 1], lowered[cls != 0, 3] = 1.0, -0.6

    def run(guard):
        venv = _venv(n, relative_to=relative_to, async_control=async_control)
        venv.reset()
        for _ in range(warm):
            venv.step({"joints": stay, "gripper": grip})
        if lowered is not None:
            venv.robot.set_joints_hard(lowered)
        if guard:
            venv.configure_guard()
        return venv

    control = run(False)
    for t in range(steps):
        *_, cinfo = control.step({"joints": act[t], "gripper": grip})
    control_collision = cinfo["collision"].copy()
    control_qpos = control.sim.qpos.copy()
    control.close()

    venv = run(True)
    for oe in oenvs:
        oe.reset()
        for _ in range(warm):
            oe.step({"joints": stay[0], "gripper": 1.0})
    if lowered is not None:
        for e, oe in enumerate(oenvs):
            oe.sim.set_joints_hard(lowered[e])
    ever = np.zeros(n, dtype=bool)
    freed = np.zeros(n, dtype=bool)
    physical = np.zeros(n, dtype=bool)
    worst = {"pos": 0.0, "vel": 0.0}
    for t in range(steps):
        obs, rew, term, trunc, info = venv.step({"joints": act[t], "gripper": grip})
        blocked = info["guard_blocked"]
        assert np.array_equal(blocked, (info["guard_result"] == 1) | (info["guard_result"] == 2))
        assert np.array_equal(term, blocked) and not rew.any()
        freed |= ever & ~blocked
        ever |= blocked
        physical |= info["collision"]
        q, v = venv.sim.qpos, venv.sim.qvel
        for e, oe in enumerate(oenvs):
            oo, _, _, otr, oi = oe.step({"joints": act[t, e], "gripper": 1.0}, blocked=bool(blocked[e]))
            dp = max(float(np.abs(obs["joints"][e] - oo["joints"]).max()), float(np.abs(obs["tquat"][e] - oo["tquat"]).max()),
                     float(np.abs(obs["xyzrpy"][e][:3] - oo["xyzrpy"][:3]).max()), rpy_error(obs["xyzrpy"][e][3:], oo["xyzrpy"][3:]),
                     float(np.abs(q[e][:7] - oe.sim.qpos[:7]).max()))
            dv = float(np.abs(v[e][:7] - oe.sim.qvel[:7]).max())
            worst["pos"], worst["vel"] = max(worst["pos"], dp), max(worst["vel"], dv)
            assert dp < 1e-9 and dv < 1e-8, (t, e, dp, dv, bool(blocked[e]))
            for k in ("collision", "ik_success", "is_sim_converged"):
                assert bool(info[k][e]) == bool(oi[k]), (t, e, k)
            assert bool(trunc[e]) == bool(otr), (t, e, "truncated")
            if not async_control:
                assert int(info["substeps"][e]) == int(oe.sim.s.convergence_steps), (t, e, "substeps")
    # what the physics' flag cannot say with async_control on, the oracle's collision pass says in every mode: where the two runs end
    from test_gpu_collision_query import OracleCollider

    orc = OracleCollider(oenvs[0].sim)
    guarded_qpos = venv.sim.qpos.copy()
    control_in_contact = np.array([orc.hit(control_qpos[e, :9]) for e in range(n)])
    guarded_in_contact = np.array([orc.hit(guarded_qpos[e, :9]) for e in range(n)])
    spared = control_in_contact & ~guarded_in_contact
    print(f"final poses in contact (oracle's collision pass): unguarded {int(control_in_contact.sum())}, guarded {int(guarded_in_contact.sum())}, "
          f"in the unguarded run only {int(spared.sum())}")
    # Asserted where the hold can settle (step_until_convergence).  With async_control on and a command that ramps ahead of a lagging
    # arm (absolute and CONFIGURED_ORIGIN actions: measured, the arm trails its command by 0.2 rad and moves at 2.6 rad/s when the
    # segment to the command first meets the floor) the arm overshoots the pose it is told to hold, into the floor, and an environment in
    # contact at the start of its segment stays blocked: 42 guarded final poses in contact against 21 unguarded.  That is the overshoot
    # the issue tells this test to count and not to assert on; the figures are printed for every mode.
    if not async_control:
        assert spared.sum() >= 8, (int(control_in_contact.sum()), int(guarded_in_contact.sum()))
    kept_out = control_collision & ~info["collision"]
    print(f"relative_to={relative_to} async={async_control}: blocked at some step {int(ever.sum())}, never {int((~ever).sum())}, blocked then free "
          f"{int(freed.sum())}; unguarded run ends in collision in {int(control_collision.sum())}, of which the guarded run keeps out {int(kept_out.sum())}; "
          f"guarded environments that still reported a physical collision at some step: {int(physical.sum())}; worst |dpos| {worst['pos']:.2e} |dvel| {worst['vel']:.2e}")
    assert ever.sum() >= 8 and (~ever).sum() >= 8 and freed.sum() >= 1
    if not async_control:
        assert kept_out.sum() >= 8, (int(control_collision.sum()), int(kept_out.sum()))
    venv.close()


def test_fresh_episodes_are_not_blocked():
    """SimEnvCreator()(..., collision_guard=True) at its defaults, stepped straight from reset() with small near-home actions while
    the gripper opens.  After reset the pads of the closed hand touch at a gap of exactly 0, which passes no certificate (the motion
    query reports such segments undecided, asserted here); the guard holds the fingers still over its segment, so it decides those
    pairs by the sample at the segment's start.  Bar: the issue's cap for short moves near home (class (a) of test 1) -- at most
    10 % of the environments blocked, terminated or truncated in any of the first steps."""
    from rcs_amd import sim as S
    from rcs_amd.envs import SimEnvCreator, default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.envs.base import ControlMode

    n, steps = 256, 12
    rng = np.random.default_rng(61)
    for episode in range(2):
        if episode == 0:
            venv = SimEnvCreator()(ControlMode.JOINTS, default_sim_robot_cfg("fr3_empty_world"), collision_guard=True,
                                   gripper_cfg=default_sim_gripper_cfg(), sim_cfg=S.SimConfig(async_control=True, realtime=False, frequency=30),
                                   max_relative_movement=MAX_MOV, n_envs=n)
            assert venv.guard_enabled
        venv.reset()
        q0 = venv.sim.qpos.copy()
        assert np.abs(q0[:, 7:]).max() < 1e-6, "the hand is closed after reset"
        a = rng.uniform(-0.03, 0.03, (n, 7))
        if episode == 0:
            tgt, _ = absolute_command(a, q0[:, :7], "last_step")
            want, _ = venv.robot.check_motion(q0, np.concatenate([tgt, q0[:, 7:]], axis=1))
            assert (want != 0).all(), "the motion query certifies nothing with the pads touching at a gap of 0"
        worst = 0.0
        for t in range(steps):
            obs, rew, term, trunc, info = venv.step({"joints": a, "gripper": np.ones(n, dtype=np.float32)})
            frac = max(float(info["guard_blocked"].mean()), float(term.mean()), float(trunc.mean()))
            worst = max(worst, frac)
            assert frac <= 0.10, (episode, t, frac, np.bincount(info["guard_result"], minlength=3))
            a = rng.uniform(-0.03, 0.03, (n, 7))
        assert venv.sim.qpos[:, 7:].min() > 0.03, "the hands have opened"
        print(f"episode {episode}: worst fraction blocked / terminated / truncated in the first {steps} steps: {worst}")
    venv.close()


def test_open_fingers_resting_past_their_limit_are_still_certified():
    """An open finger rests on its joint limit and the soft limit lets it through by micrometres (up to 44 um measured in a rollout).
    The motion query never certifies a row whose slides have left the stroke its levers were built for; the guard admits 0.5 mm of
    the millimetre of margin those levers carry (csrc/rcs_hip.hip: guard_launch), and nothing beyond it."""
    simu, robot, orc, cm, home = _fr3("fr3_empty_world")
    n = 256
    q, tgt, cls = decision_cases(orc, home, cm.geom_names, 3 * n)
    q, tgt = q[:n].copy(), tgt[:n]  # (class (a): short moves near home)
    venv = _venv(n)
    venv.reset()
    venv.configure_guard(enabled=False)
    frac = {}
    for over in (0.0, 4e-5, 1e-3):
        q[:, 7:] = OPEN + over
        _place(venv, q)
        _, result, _ = venv.check_action(tgt)
        want, _ = venv.robot.check_motion(q, np.concatenate([tgt, q[:, 7:]], axis=1))
        frac[over] = float((result == 0).mean())
        if over == 0.0:
            assert np.array_equal(result, want)
        else:
            assert (want != 0).all(), "the motion query certifies nothing beyond the stroke"
    print("certified free with the fingers past their limit by 0 / 40 um / 1 mm:", frac)
    assert frac[0.0] >= 0.9 and frac[4e-5] >= 0.9 and frac[1e-3] == 0.0
    # 40 um further out moves the finger geoms by 40 um: every environment the guard certifies there is free of contact in the oracle
    q[:, 7:] = OPEN + 4e-5
    _place(venv, q)
    _, result, _ = venv.check_action(tgt)
    q_to = np.concatenate([tgt, q[:, 7:]], axis=1)
    for e in np.flatnonzero(result == 0)[:64]:
        assert not oracle_samples(orc, q[e], q_to[e], samples=201)[0], e
    venv.close()


def _venv_scene_path():
    from rcs_amd import envs

    return envs.default_sim_robot_cfg("fr3_empty_world").mjcf_scene_path


def _rollout(venv, joints, grip, peek_every=0):
    out = []
    for t in range(len(joints)):
        if peek_every and t % peek_every == 0:
            s0 = venv.sim.get_state().copy()
            venv.check_action(joints[t])
            assert (venv.sim.get_state() == s0).all()
        obs, rew, term, trunc, info = venv.step({"joints": joints[t], "gripper": grip[t]})
        out.append((venv.sim.qpos.copy(), venv.sim.qvel.copy(), term.copy(), trunc.copy(), {k: np.asarray(v).copy() for k, v in info.items()}))
    return out


def test_off_means_off():
    """A venv with the guard configured and then disabled, and one whose guard is peeked between steps, reproduce a plain venv's
    100-step rollout bit for bit: qpos, qvel, terminated, truncated and every info key."""
    from parity_util import make_vec_env, synthetic_actions

    joints, grip = synthetic_actions(64, 100, 0)
    runs = []
    for variant in ("plain", "configured then disabled", "disabled, peeked"):
        venv = make_vec_env(64, True)
        if variant != "plain":
            venv.configure_guard()
            venv.configure_guard(enabled=False)
        venv.reset()
        runs.append(_rollout(venv, joints, grip, peek_every=3 if variant == "disabled, peeked" else 0))
        venv.close()
    for other in runs[1:]:
        for (qa, va, ta, ra, ia), (qb, vb, tb, rb, ib) in zip(runs[0], other):
            assert np.array_equal(qa, qb) and np.array_equal(va, vb) and np.array_equal(ta, tb) and np.array_equal(ra, rb)
            assert ia.keys() == ib.keys()
            for k in ia:
                assert np.array_equal(ia[k], ib[k]), k


def test_device_path_equals_host_path():
    """step_dev with the guard equals the host path bit for bit over 20 steps: observations, info rows, substeps, the guard record."""
    from rcs_amd import _lib
    from rcs_env_oracle import FR3_Q_HOME

    n, steps = 64, 20
    act, _ = rollout_actions(n, steps, "last_step", np.asarray(FR3_Q_HOME), seed=41)
    act *= 3.0  # (clamped to 5 degrees a step: the floor classes arrive within the 20 steps from the lowered start below)
    grip = np.ones(n, dtype=np.float32)
    start = np.tile(np.concatenate([FR3_Q_HOME, [OPEN, OPEN]]), (n, 1))
    start[:, 1], start[:, 3] = 0.5, -1.2
    host, dev = _venv(n, relative_to="last_step"), _venv(n, relative_to="last_step")
    for v in (host, dev):
        v.reset()
        _place(v, start)
        v.configure_guard()
    L, h = dev._L, dev.sim._h
    ow = dev.obs_width

    def dalloc(nbytes):
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
        return p

    def down(p, a):
        _lib.check(L.rcsh_dev_download(h, C.c_void_p(a.ctypes.data), p, a.nbytes))
        return a

    d_act, d_grip, d_obs, d_info, d_gw, d_sub = dalloc(n * 7 * 8), dalloc(n * 4), dalloc(n * ow * 8), dalloc(n * 8), dalloc(n * 8), dalloc(n * 4)
    _lib.check(L.rcsh_dev_upload(h, d_grip, C.c_void_p(grip.ctypes.data), grip.nbytes))
    any_blocked = False
    for t in range(steps):
        obs, rew, term, trunc, info = host.step({"joints": act[t], "gripper": grip})
        a = np.ascontiguousarray(act[t])
        _lib.check(L.rcsh_dev_upload(h, d_act, C.c_void_p(a.ctypes.data), a.nbytes))
        dev.step_dev(d_act.value, d_grip.value, d_obs.value, d_info.value, d_gw.value, d_sub.value)
        dobs = down(d_obs, np.zeros((n, ow)))
        dinfo = down(d_info, np.zeros((n, 8), dtype=np.uint8))
        assert np.array_equal(dobs[:, :7], obs["tquat"]) and np.array_equal(dobs[:, 7:14], obs["joints"]) and np.array_equal(dobs[:, 14:20], obs["xyzrpy"])
        assert np.array_equal(dinfo[:, 0].astype(bool), info["collision"]) and np.array_equal(dinfo[:, 4].astype(bool), trunc)
        assert np.array_equal(down(d_sub, np.zeros(n, dtype=np.int32)), info["substeps"])
        assert np.array_equal(dev.sim.qpos, host.sim.qpos) and np.array_equal(dev.sim.qvel, host.sim.qvel)
        b, r, tc = dev.guard_last()
        assert np.array_equal(b, info["guard_blocked"]) and np.array_equal(r, info["guard_result"]) and np.array_equal(tc, info["guard_t_contact"])
        pb, pr, pt = dev.guard_last_dev()
        assert np.array_equal(down(C.c_void_p(pb), np.zeros(n, dtype=np.uint8)).astype(bool), b)
        assert np.array_equal(down(C.c_void_p(pr), np.zeros(n, dtype=np.int32)), r) and np.array_equal(down(C.c_void_p(pt), np.zeros(n)), tc)
        assert np.array_equal(trunc & b, b), "a truncating guard reports its blocked environments truncated"
        any_blocked = any_blocked or b.any()
    assert any_blocked, "no environment was blocked: the comparison shows nothing"
    for p in (d_act, d_grip, d_obs, d_info, d_gw, d_sub):
        _lib.check(L.rcsh_dev_free(h, p))
    host.close(); dev.close()


def test_truncate_on_collision_off_only_reports():
    """truncate_on_collision=False: the blocked environments are held all the same, terminated / truncated stay what they were."""
    from rcs_env_oracle import FR3_Q_HOME

    n = 16
    start = np.tile(np.concatenate([FR3_Q_HOME, [OPEN, OPEN]]), (n, 1))
    start[:, 1], start[:, 3] = 1.0, -0.8  # low above the floor
    a, b = _venv(n), _venv(n)
    for v, trunc_on in ((a, True), (b, False)):
        v.reset()
        _place(v, start)
        v.configure_guard(truncate_on_collision=trunc_on)
    target = start[:, :7].copy()
    target[:, 1] = 1.6
    outs = [v.step({"joints": target, "gripper": np.ones(n, dtype=np.float32)}) for v in (a, b)]
    assert outs[0][4]["guard_blocked"].all() and outs[1][4]["guard_blocked"].all()
    assert outs[0][2].all() and outs[0][3].all()
    assert not outs[1][2].any() and np.array_equal(outs[1][3], ~outs[1][4]["ik_success"] | outs[1][4]["collision"])
    assert np.array_equal(a.sim.qpos, b.sim.qpos)
    a.close(); b.close()


def _pick_env(n):
    from rcs_amd import envs, sim as S
    from rcs_amd.envs.base import ControlMode, RelativeTo
    from rcs_amd.envs.creators import VecPickCubeEnv

    cfg = envs.default_sim_robot_cfg("fr3_simple_pick_up")
    sc = S.SimConfig(async_control=True, realtime=False, frequency=30)
    simu = S.Sim(cfg.mjcf_scene_path, sc, n_envs=n)
    robot = S.SimRobot(simu, None, cfg)
    gripper = S.SimGripper(simu, envs.default_sim_gripper_cfg())
    return VecPickCubeEnv(simu, robot, gripper, ControlMode.JOINTS, MAX_MOV, RelativeTo.LAST_STEP)


def test_task_env_touches_its_cube_by_default():
    """VecPickCubeEnv: with the default kinds (floor | self) closing the fingers on the cube is not blocked; with kinds = 7 moving
    the open hand down onto the cube is."""
    from test_gpu_collision_query import _closing_onto_box

    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    n = 32
    rng = np.random.default_rng(51)
    a, _, boxes = _closing_onto_box(orc, cm, home, rng, n)
    venv = _pick_env(n)
    venv.reset(options={"box_qpos": boxes})
    _place(venv, a, boxes)
    venv.configure_guard()
    assert venv.default_guard_kinds() == 3
    zero = np.zeros((n, 7))
    obs, rew, term, trunc, info = venv.step({"joints": zero, "gripper": np.zeros(n, dtype=np.float32)})  # close on the cube
    assert not info["guard_blocked"].any(), np.bincount(info["guard_result"], minlength=3)
    # the open hand above the cube, moved down onto it: the cube right under the fingertips
    venv2 = _pick_env(n)
    venv2.reset(options={"box_qpos": boxes})
    under = boxes.copy()
    under[:, 2] -= 0.03
    _place(venv2, a, under)
    down_cmd = np.zeros((n, 7))
    down_cmd[:, 1], down_cmd[:, 3] = MAX_MOV, MAX_MOV
    venv2.configure_guard(enabled=False, kinds=3)
    b3, r3, _ = venv2.check_action(down_cmd)
    venv2.configure_guard(kinds=7)
    b7, r7, _ = venv2.check_action(down_cmd)
    print("down onto the cube: blocked with kinds 3:", int(b3.sum()), "with kinds 7:", int(b7.sum()), "of", n)
    assert b7.sum() > b3.sum() and b7.sum() >= n // 2
    obs, rew, term, trunc, info = venv2.step({"joints": down_cmd, "gripper": np.ones(n, dtype=np.float32)})
    assert np.array_equal(info["guard_blocked"], b7) and np.array_equal(term, info["success"] | b7)
    venv.close(); venv2.close()


def test_task_device_path_equals_host_path():
    """step_task_dev with the guard (kinds 7, the open hand over the cube) against the host step, bit for bit over three steps:
    observation, task block, info rows and the guard's record."""
    from rcs_amd import _lib
    from test_gpu_collision_query import _closing_onto_box

    simu, robot, orc, cm, home = _fr3("fr3_simple_pick_up")
    n = 32
    rng = np.random.default_rng(52)
    a, _, boxes = _closing_onto_box(orc, cm, home, rng, n)
    under = boxes.copy()
    under[n // 2:, 2] -= 0.03  # (cubes between the open fingers, half of them lower, under the fingertips: the way down is blocked)
    host, dev = _pick_env(n), _pick_env(n)
    for v in (host, dev):
        v.reset(options={"box_qpos": under})
        _place(v, a, under)
        v.configure_guard(kinds=7)
    L, h = dev._L, dev.sim._h
    ow = dev.obs_width

    def dalloc(nbytes):
        p = C.c_void_p()
        _lib.check(L.rcsh_dev_alloc(h, nbytes, C.byref(p)))
        return p

    def down(p, arr):
        _lib.check(L.rcsh_dev_download(h, C.c_void_p(arr.ctypes.data), p, arr.nbytes))
        return arr

    cmd = np.zeros((n, 7))
    cmd[:, 1], cmd[:, 3] = MAX_MOV, MAX_MOV
    grip = np.ones(n, dtype=np.float32)
    d_act, d_grip, d_obs, d_info, d_gw, d_sub, d_task = (dalloc(n * 7 * 8), dalloc(n * 4), dalloc(n * ow * 8), dalloc(n * 8), dalloc(n * 8),
                                                        dalloc(n * 4), dalloc(n * 9 * 8))
    _lib.check(L.rcsh_dev_upload(h, d_act, C.c_void_p(cmd.ctypes.data), cmd.nbytes))
    _lib.check(L.rcsh_dev_upload(h, d_grip, C.c_void_p(grip.ctypes.data), grip.nbytes))
    seen = np.zeros(n, dtype=bool)
    for t in range(3):
        obs, rew, term, trunc, info = host.step({"joints": cmd, "gripper": grip})
        dev.step_task_dev(d_act.value, d_grip.value, d_obs.value, d_info.value, d_gw.value, d_sub.value, d_task.value)
        dobs, dtask = down(d_obs, np.zeros((n, ow))), down(d_task, np.zeros((n, 9)))
        dinfo = down(d_info, np.zeros((n, 8), dtype=np.uint8))
        assert np.array_equal(dobs[:, :7], obs["tquat"]) and np.array_equal(dobs[:, 7:14], obs["joints"])
        assert np.array_equal(dtask[:, :7], info["box_qpos"]) and np.array_equal(dtask[:, 7], rew)
        assert np.array_equal(dinfo[:, 4].astype(bool), trunc)
        b, r, tc = dev.guard_last()
        assert np.array_equal(b, info["guard_blocked"]) and np.array_equal(r, info["guard_result"]) and np.array_equal(tc, info["guard_t_contact"])
        assert np.array_equal(term, (dtask[:, 8] != 0) | b)
        assert np.array_equal(dev.sim.qpos, host.sim.qpos)
        seen |= b
    assert seen.any(), "no environment was blocked: the comparison shows nothing"
    host.close(); dev.close()


def test_errors_leave_state_and_rollout_untouched():
    from parity_util import make_vec_env, synthetic_actions
    from rcs_amd import _lib, sim as S
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.envs.base import ControlMode

    joints, grip = synthetic_actions(16, 20, 3)
    ref = make_vec_env(16, True)
    ref.reset()
    want = _rollout(ref, joints, grip)
    ref.close()
    venv = make_vec_env(16, True)
    venv.reset()
    s0 = venv.sim.get_state().copy()
    with pytest.raises(ValueError):
        venv.configure_guard(resolution=0.0)
    with pytest.raises(ValueError):
        venv.configure_guard(resolution=-1e-3)
    for kinds in (0, 8, -1):
        with pytest.raises(ValueError):
            venv.configure_guard(kinds=kinds)
    with pytest.raises(RuntimeError):
        venv.check_action(joints[0])  # (no guard was ever configured)
    with pytest.raises(RuntimeError):
        venv.guard_last()
    assert not venv.guard_enabled and (venv.sim.get_state() == s0).all()
    got = _rollout(venv, joints, grip)
    for (qa, va, ta, ra, ia), (qb, vb, tb, rb, ib) in zip(want, got):
        assert np.array_equal(qa, qb) and np.array_equal(va, vb) and ia.keys() == ib.keys()
        assert all(np.array_equal(ia[k], ib[k]) for k in ia)
    venv.close()
    # a Cartesian mode with the guard: refused by configure_guard, by the creator, and by a later rcsh_env_configure
    cart = make_vec_env(4, True, control_mode=ControlMode.CARTESIAN_TRPY, max_relative_movement=0.5)
    cart.reset()
    s0 = cart.sim.get_state().copy()
    with pytest.raises(RuntimeError):
        cart.configure_guard()
    with pytest.raises(RuntimeError):
        cart.configure_guard(enabled=False)
    assert (cart.sim.get_state() == s0).all()
    cart.close()
    from rcs_amd.envs import SimEnvCreator

    with pytest.raises(NotImplementedError, match="collision_guard"):
        SimEnvCreator()(ControlMode.CARTESIAN_TQuat, default_sim_robot_cfg("fr3_empty_world"), collision_guard=True)
    guarded = SimEnvCreator()(ControlMode.JOINTS, default_sim_robot_cfg("fr3_empty_world"), collision_guard=True,
                              gripper_cfg=default_sim_gripper_cfg(), sim_cfg=S.SimConfig(async_control=True), max_relative_movement=MAX_MOV, n_envs=4)
    assert guarded.guard_enabled
    d = _lib.EnvDesc()
    d.control_mode, d.relative_to, d.binary_gripper = 1, 1, 1
    d.max_mov[:] = [0.5, 1.5]
    assert guarded._L.rcsh_env_configure(guarded.sim._h, C.byref(d)) != 0, "a Cartesian mode under an enabled guard must not be accepted silently"
    # a disabled guard does not stop rcsh_env_configure from taking a Cartesian mode: the peek must then refuse (action widths differ)
    guarded.configure_guard(enabled=False)
    assert guarded._L.rcsh_env_configure(guarded.sim._h, C.byref(d)) == 0
    res, tcs, blk = np.zeros(4, dtype=np.int32), np.zeros(4), np.zeros(4, dtype=np.uint8)
    assert guarded._L.rcsh_env_guard_peek(guarded.sim._h, _lib.ptr(np.zeros((4, 7))), _lib.ptr(res), _lib.ptr(tcs), _lib.ptr(blk)) != 0
    d.control_mode, d.max_mov[0], d.max_mov[1] = 0, MAX_MOV, 0.0
    d.joint_low = guarded._low.ctypes.data_as(C.POINTER(C.c_double))
    d.joint_high = guarded._high.ctypes.data_as(C.POINTER(C.c_double))
    assert guarded._L.rcsh_env_configure(guarded.sim._h, C.byref(d)) == 0
    guarded.configure_guard()
    guarded.reset()
    *_, info = guarded.step({"joints": np.zeros((4, 7)), "gripper": np.ones(4, dtype=np.float32)})
    assert "guard_blocked" in info
    guarded.close()
    # a guard before rcsh_env_configure
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
    S.SimRobot(simu, None, cfg)
    g = _lib.GuardDesc()
    g.enabled, g.kinds, g.resolution, g.block_undecided, g.truncate = 1, 3, 1e-3, 1, 1
    s0 = simu.get_state().copy()
    assert simu._L.rcsh_env_configure_guard(simu._h, C.byref(g)) != 0
    assert simu._L.rcsh_env_configure_guard(simu._h, None) != 0
    assert (simu.get_state() == s0).all()


def test_scene_the_query_tables_refuse_is_refused():
    """The derived scene of test_scene_with_an_untested_geom_type_is_refused (a colliding sphere on the hand)."""
    import shutil
    import xml.etree.ElementTree as ET

    from parity_util import SCENE, scratch_dir
    from rcs_amd import envs
    from rcs_amd.envs.base import ControlMode

    path = os.path.join(scratch_dir(), "rcs_amd_fr3_sphere_guard", "scene.xml")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tree = ET.parse(SCENE)
    hand = next(bd for bd in tree.getroot().iter("body") if bd.get("name") == "hand_0")
    ET.SubElement(hand, "geom", {"name": "extra_sphere", "type": "sphere", "size": "0.02", "pos": "0 0 0.05"})
    tree.write(path)
    for extra in ("collision_vertices.npz", "render_hulls.npz"):
        if os.path.exists(os.path.join(os.path.dirname(SCENE), extra)):
            shutil.copy(os.path.join(os.path.dirname(SCENE), extra), os.path.dirname(path))
    cfg = envs.default_sim_robot_cfg("fr3_empty_world")
    cfg.mjcf_scene_path = cfg.kinematic_model_path = path
    try:
        venv = envs.make_vec_env(4, True, robot_cfg=cfg)
    except RuntimeError:
        return  # (refused at creation already)
    venv.reset()
    s0 = venv.sim.get_state().copy()
    with pytest.raises(RuntimeError):
        venv.configure_guard()
    assert not venv.guard_enabled and (venv.sim.get_state() == s0).all()
    with pytest.raises(RuntimeError):
        envs.SimEnvCreator()(ControlMode.JOINTS, cfg, collision_guard=True, gripper_cfg=envs.default_sim_gripper_cfg(),
                             max_relative_movement=MAX_MOV, n_envs=2)
    venv.close()
