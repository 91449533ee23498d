"""CPU checks of the torque / impedance env-step cases (tests/env_torque_cases.py): the numpy wrapper arithmetic the GPU yardstick is
composed from agrees with the oracle's wrapper stack (oracle/rcs_env_oracle.py: OracleEnv._relative_action and the gate of
OracleEnv.step) on the cases' own action sequences; every gate decision keeps its distance from the threshold; the control-mode
enums line up.

The oracle has no torque law, so the state the wrappers see between the actions is synthetic here: after every action the arm has
gone HALF the way from where it was to the commanded target (joint vector or pose).  The GPU tests assert the same margins on the
states the simulation produces.
"""

import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import env_torque_cases as EC  # noqa: E402
import torque_cases as TC  # noqa: E402


class _StubSim:
    """What OracleEnv asks of its simulator in _relative_action and step, without a simulator: the pose / joint getters return the
    synthetic state, the setters record that the gate commanded."""

    class _S:
        async_control, frequency, robot_collision, ik_success, grp_collision = True, 30, False, True, False

    class _NoPose:  # (the observation of a joint-space run: nobody reads it)
        def translation(self):
            return np.zeros(3)

        def rotation_q(self):
            return np.array([0.0, 0.0, 0.0, 1.0])

        def xyzrpy(self):
            return np.zeros(6)

    def __init__(self):
        self.s = self._S()
        self.q = np.zeros(1)
        self.pose = self._NoPose()
        self.commanded = None

    def get_joint_position(self):
        return self.q.copy()

    def get_cartesian_position(self):
        return self.pose

    def set_joint_position(self, a):
        self.commanded = np.asarray(a, dtype=np.float64).copy()

    def set_cartesian_position(self, pose):
        self.commanded = np.concatenate([pose.translation(), pose.rotation_q()])

    def step(self, k):
        pass

    def is_converged(self):
        return True


def _oracle_env(mode, relative_to, max_mov, robot):
    import rcs_env_oracle as R

    env = object.__new__(R.OracleEnv)  # (the constructor builds a simulator; the wrapper logic needs none)
    env.robot = robot
    env.sim = _StubSim()
    env.timestep = 0.002
    env.mode = mode
    env.has_gripper = False
    env.max_mov = max_mov if relative_to is not None else None
    env.relative_to = relative_to if relative_to is not None else R.LAST_STEP
    env.prev_action = None
    env._last_gripper_cmd = None
    env._origin = None
    env._last_action = None
    return env


def _rotdiff(a, b):
    return float(np.abs(TC.rotvec(np.asarray(a)[None], np.asarray(b)[None])).max())


@pytest.mark.parametrize("tag,mask,relative_to", EC.JOINT_RUNS)
def test_joint_wrapper_agrees_with_the_oracle_and_keeps_its_gate_margins(tag, mask, relative_to):
    r = TC.oracle_robot(tag)
    home, low, high = (np.asarray(r[k], dtype=np.float64) for k in ("q_home", "low", "high"))
    actions = EC.joint_actions(home, low, high, relative_to)
    worst, held, clamped = np.inf, 0, 0
    for e in range(EC.N):
        w = EC.Wrapper(EC.JOINTS, relative_to, EC.MAX_JOINT_MOV, low, high)
        env = _oracle_env("joints", relative_to, EC.MAX_JOINT_MOV, r)
        q = home + 0.01 * (e + 1)
        w.reset(q)
        env.sim.q = q.copy()
        if relative_to is not None:
            env._set_origin_to_current()
        for k, a in enumerate(actions):
            out, cmd, margin = w.action(a[e], q)
            env.sim.commanded = None
            env.step({"joints": a[e].copy()})
            assert np.array_equal(env.prev_action["joints"], out), (tag, relative_to, e, k)  # (adds and clamps: bit for bit)
            assert (env.sim.commanded is not None) == cmd, (tag, relative_to, e, k)
            if relative_to is not None:
                assert np.array_equal(env._last_action, w.last) and np.array_equal(env._origin, w.origin)
                clamped += int(np.any(out == low) or np.any(out == high))
            worst = min(worst, margin)
            held += int(not cmd)
            assert margin >= EC.GATE_MARGIN, (tag, relative_to, e, k, margin)
            q = q + 0.5 * (out - q)
            env.sim.q = q.copy()
    print("smallest gate margin", worst, "held", held, "clamped", clamped)
    if relative_to != EC.LAST_STEP:
        assert held >= EC.N  # (the repeated action: the gate holds in every environment)
    if relative_to is not None:
        assert clamped >= EC.N  # (the action towards the nearest joint limit lands on the clamp)


@pytest.mark.parametrize("tag,mode,mask,relative_to", EC.CART_RUNS)
def test_cartesian_wrapper_agrees_with_the_oracle_and_keeps_its_gate_margins(tag, mode, mask, relative_to):
    import rcs_oracle as O
    from rcs_amd.common import Pose

    O.build()
    r = TC.oracle_robot(tag)
    actions = EC.cart_actions(mode)
    # a start pose inside the workspace box, turned a little (any pose will do: the wrappers see nothing else of the robot)
    start = Pose(translation=[0.35, 0.02, 0.45], rpy_vector=[3.0, 0.1, 0.2]) if tag == "fr3" else Pose(translation=[0.2, 0.0, 0.15], rpy_vector=[0.3, 1.2, 0.1])
    worst, held, boxed, limited = np.inf, 0, 0, 0
    for e in range(EC.N):
        w = EC.Wrapper(mode, relative_to, EC.MAX_CART_MOV)
        env = _oracle_env(mode, relative_to, EC.MAX_CART_MOV, r)
        cur = start.as_vec7()
        cur[:3] += 0.01 * e
        w.reset(cur)
        env.sim.pose = O.Pose(translation=cur[:3], quaternion=cur[3:])
        env._set_origin_to_current()
        for k, a in enumerate(actions):
            out, cmd, margin = w.action(a[e], cur)
            env.sim.commanded = None
            env.step({mode: a[e].copy()})
            ref = np.asarray(env.prev_action[mode], dtype=np.float64)
            assert np.abs(out - ref).max() < 1e-12, (tag, mode, relative_to, e, k, out, ref)  # (components, signs included: the gate reads them)
            assert (env.sim.commanded is not None) == cmd, (tag, mode, relative_to, e, k)
            if cmd:
                t7 = w.target7(out)
                assert np.abs(t7[:3] - env.sim.commanded[:3]).max() < 1e-12 and _rotdiff(t7[3:], env.sim.commanded[3:]) < 1e-12
            assert np.abs(w.last.translation() - env._last_action.translation()).max() < 1e-12
            assert _rotdiff(w.last.rotation_q(), env._last_action.rotation_q()) < 1e-12
            worst = min(worst, margin)
            held += int(not cmd)
            boxed += int(out[2] == 0.0)
            limited += int(abs(w.last.total_angle() - EC.MAX_CART_MOV[1]) < 1e-9)
            assert margin >= EC.GATE_MARGIN, (tag, mode, relative_to, e, k, margin)
            # half the way to the target
            tgt = Pose(translation=w.target7(out)[:3], quaternion=w.target7(out)[3:])
            now = Pose(translation=cur[:3], quaternion=cur[3:]).interpolate(tgt, 0.5)
            cur = now.as_vec7()
            env.sim.pose = O.Pose(translation=cur[:3], quaternion=cur[3:])
    print("smallest gate margin", worst, "held", held, "on the box", boxed, "at the rotation limit", limited)
    assert boxed >= EC.N and limited >= EC.N
    if relative_to == EC.CONFIGURED_ORIGIN:
        assert held >= EC.N


def test_torque_cases_have_rows_beyond_ctrlrange():
    for tag in EC.TORQUE_RUNS:
        _, taus = EC.torque_actions(tag)
        assert (np.abs(taus[0][1]) > np.array(TC.RANGES[tag])).sum() == 2


def test_control_mode_enums_line_up():
    """The members that existed keep their values; the new ones map to 3..6 of the C-ABI (fails without the feature)."""
    from rcs_amd import _lib
    from rcs_amd.envs import ControlMode
    from rcs_amd.envs import creators

    assert [m.name for m in ControlMode][:3] == ["JOINTS", "CARTESIAN_TRPY", "CARTESIAN_TQuat"]
    assert [ControlMode.JOINTS.value, ControlMode.CARTESIAN_TRPY.value, ControlMode.CARTESIAN_TQuat.value] == [1, 2, 3]
    assert [creators._MODE[m] for m in (ControlMode.JOINTS, ControlMode.CARTESIAN_TRPY, ControlMode.CARTESIAN_TQuat)] == [0, 1, 2]
    new = (ControlMode.TORQUE, ControlMode.JOINT_IMPEDANCE, ControlMode.CARTESIAN_IMPEDANCE_TRPY, ControlMode.CARTESIAN_IMPEDANCE_TQuat)
    assert [creators._MODE[m] for m in new] == [3, 4, 5, 6]
    assert (_lib.RCSH_MODE_TORQUE, _lib.RCSH_MODE_JOINT_IMPEDANCE, _lib.RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY,
            _lib.RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT) == (3, 4, 5, 6)
    assert (_lib.RCSH_MODE_JOINTS, _lib.RCSH_MODE_CARTESIAN_TRPY, _lib.RCSH_MODE_CARTESIAN_TQUAT) == (0, 1, 2)
    assert [creators._ACTION_KEY[m] for m in new] == ["torque", "joints", "xyzrpy", "tquat"]
    # and the header says the same
    text = open(os.path.join(os.path.dirname(HERE), "include", "rcs_hip.h")).read()
    for name, value in (("RCSH_MODE_TORQUE", 3), ("RCSH_MODE_JOINT_IMPEDANCE", 4), ("RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY", 5),
                        ("RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT", 6)):
        assert f"{name} = {value}" in text
