"""The collision guard's host-side contract (csrc/guard_team.h, rcsh_env_configure_guard): what can be checked without a GPU.

Also home of `absolute_command`, the numpy restatement of RelativeActionSpace.action in JOINTS mode (written from
oracle/rcs_env_oracle.py: OracleEnv._relative_action) that fixes the END of the segment the guard tests; the GPU tests
(tests/test_gpu_collision_guard.py) build their expected segment ends with it."""

import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

GUARD_SYMBOLS = ("rcsh_env_configure_guard", "rcsh_env_guard_peek", "rcsh_env_guard_peek_dev", "rcsh_env_guard_last",
                 "rcsh_env_guard_last_dev")

FR3_LOW = np.array([-2.3093, -1.5133, -2.4937, -2.7478, -2.4800, 0.8521, -2.6895])  # reference include/rcs/Robot.h:36-40
FR3_HIGH = np.array([2.3093, 1.5133, 2.4937, -0.4461, 2.4800, 4.2094, 2.6895])
MAX_MOV = float(np.deg2rad(5))


def absolute_command(action, q_now, relative_to, max_mov=MAX_MOV, origin=None, last_action=None, low=FR3_LOW, high=FR3_HIGH):
    """The absolute joint command RobotEnv.step receives for `action` ([N, dof] or [dof]), and the relative action space's new
    `_last_action` (None for absolute actions).

    relative_to: None (absolute actions: the action IS the command, unclamped), "last_step" (origin = the current joints, the action
    clamped to +-max_mov) or "configured_origin" (origin fixed at reset; the action may move by at most max_mov from the previous
    limited action `last_action`, None before the first step)."""
    a = np.asarray(action, dtype=np.float64)
    if relative_to is None:
        return a.copy(), None
    if relative_to == "last_step":
        origin = np.asarray(q_now, dtype=np.float64)
    fresh = relative_to == "last_step" or last_action is None
    if fresh:
        limited = np.clip(a, -max_mov, max_mov)
    else:
        limited = np.clip(a - last_action, -max_mov, max_mov) + last_action
    return np.clip(np.asarray(origin, dtype=np.float64) + limited, low, high), limited


def test_library_exports_and_declarations():
    from rcs_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "rcs_hip.h")).read()
    for sym in GUARD_SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in _lib.EXPORTS, sym
        assert getattr(L, sym).argtypes is not None, sym
        assert len(re.findall(r"\bint\s+" + sym + r"\s*\(", header)) == 1, sym
    assert re.search(r"#define\s+RCSH_ABI_VERSION\s+2\b", header)
    assert L.rcsh_abi_version() == 2
    # the description struct: the header's fields, in its order, and the ctypes mirror's
    body = re.search(r"typedef struct rcsh_guard_desc \{(.*?)\} rcsh_guard_desc;", header, re.S).group(1)
    fields = re.findall(r"\b(?:int32_t|double)\s+(\w+);", body)
    assert fields == ["enabled", "kinds", "resolution", "block_undecided", "truncate"]
    assert [f for f, _ in _lib.GuardDesc._fields_] == fields


def test_existing_structs_keep_their_layout():
    """Appended functions only: rcsh_env_desc is what it was."""
    import ctypes as C

    from rcs_amd import _lib

    assert [f for f, _ in _lib.EnvDesc._fields_] == ["control_mode", "relative_to", "max_mov", "binary_gripper", "joint_low", "joint_high"]
    assert C.sizeof(_lib.EnvDesc) == 48


def test_creator_no_longer_refuses_the_guard():
    from rcs_amd.envs import creators

    src = inspect.getsource(creators.SimEnvCreator.__call__)
    blanket = re.search(r"if hand_cfg is not None or sim_wrapper is not None([^:]*):\s*\n\s*raise NotImplementedError\(([^\n]*)\)", src)
    assert blanket, "the refusal of hands and sim_wrapper stays"
    assert "collision_guard" not in blanket.group(1) and "collision_guard" not in blanket.group(2)
    assert "configure_guard" in src
    assert inspect.signature(creators.SimEnvCreator.__call__).parameters["collision_guard"].default is False
    sig = inspect.signature(creators.VecSimEnv.configure_guard)
    assert [(k, p.default) for k, p in sig.parameters.items() if k != "self"] == [
        ("enabled", True), ("kinds", None), ("resolution", 1e-3), ("block_undecided", True), ("truncate_on_collision", True)]
    assert hasattr(creators.VecSimEnv, "check_action")


def test_creator_refuses_the_guard_with_a_cartesian_mode_before_building_anything():
    import pytest
    from rcs_amd.envs import creators
    from rcs_amd.envs.base import ControlMode

    with pytest.raises(NotImplementedError, match="collision_guard"):
        creators.SimEnvCreator()(ControlMode.CARTESIAN_TRPY, None, collision_guard=True)


# hand-made cases: (relative_to, q_now, origin, last_action, action) -> (command, new last action)
_Q = np.array([0.0, -0.7, 0.0, -2.3, 0.0, 1.6, 0.8])
HAND_CASES = [
    # absolute: passed through, not even clamped to the joint limits
    (None, _Q, None, None, np.array([0.1, 3.0, 0.0, -2.0, 0.0, 1.5, 0.7]),
     np.array([0.1, 3.0, 0.0, -2.0, 0.0, 1.5, 0.7]), None),
    # last step: +-5 degrees around where the arm is
    ("last_step", _Q, None, None, np.array([0.5, -0.5, 0.01, 0.0, -0.02, 0.2, -0.2]),
     _Q + np.array([MAX_MOV, -MAX_MOV, 0.01, 0.0, -0.02, MAX_MOV, -MAX_MOV]), np.array([MAX_MOV, -MAX_MOV, 0.01, 0.0, -0.02, MAX_MOV, -MAX_MOV])),
    # last step at a joint limit: clamped to it (joint 4 high = -0.4461, joint 6 low = 0.8521)
    ("last_step", np.array([0.0, -0.7, 0.0, -0.45, 0.0, 0.86, 0.8]), None, None, np.array([0, 0, 0, 0.05, 0, -0.05, 0.0]),
     np.array([0.0, -0.7, 0.0, -0.4461, 0.0, 0.8521, 0.8]), np.array([0, 0, 0, 0.05, 0, -0.05, 0.0])),
    # configured origin, first step: as fresh -- the action itself is limited
    ("configured_origin", _Q + 0.3, _Q, None, np.array([0.2, 0.01, 0, 0, 0, 0, -0.3]),
     _Q + np.array([MAX_MOV, 0.01, 0, 0, 0, 0, -MAX_MOV]), np.array([MAX_MOV, 0.01, 0, 0, 0, 0, -MAX_MOV])),
    # configured origin, later: at most 5 degrees from the previous limited action, wherever the arm is now
    ("configured_origin", _Q + 0.3, _Q, np.array([0.05, 0.01, 0, 0, 0, 0, -0.08]), np.array([0.3, 0.0, 0, 0, 0, 0, -0.3]),
     _Q + np.array([0.05 + MAX_MOV, 0.0, 0, 0, 0, 0, -0.08 - MAX_MOV]), np.array([0.05 + MAX_MOV, 0.0, 0, 0, 0, 0, -0.08 - MAX_MOV])),
]


def test_absolute_command_hand_cases():
    for rel, q_now, origin, last, action, want, want_last in HAND_CASES:
        cmd, new_last = absolute_command(action, q_now, rel, origin=origin, last_action=last)
        assert np.allclose(cmd, want, rtol=0, atol=1e-15), (rel, cmd, want)
        if want_last is None:
            assert new_last is None
        else:
            assert np.allclose(new_last, want_last, rtol=0, atol=1e-15), (rel, new_last, want_last)


def test_absolute_command_is_the_oracle_wrappers_arithmetic():
    """Bit for bit what OracleEnv._relative_action computes, over seeded sequences in the two relative modes."""
    import rcs_env_oracle as E

    rng = np.random.default_rng(0)
    for rel, tag in ((E.LAST_STEP, "last_step"), (E.CONFIGURED_ORIGIN, "configured_origin")):
        env = E.OracleEnv.__new__(E.OracleEnv)  # (the wrapper arithmetic alone: no simulation behind it)
        env.mode, env.relative_to, env.max_mov, env.robot = E.JOINTS, rel, MAX_MOV, E.FR3
        q = np.array(E.FR3_Q_HOME)
        env._origin, env._last_action = q.copy(), None
        env._set_origin_to_current = lambda env=env: setattr(env, "_origin", env._q_now.copy())
        origin, last = q.copy(), None
        for _ in range(50):
            q = q + rng.uniform(-0.05, 0.05, 7)
            env._q_now = q
            a = rng.uniform(-0.2, 0.2, 7)
            want = env._relative_action({"joints": a})["joints"]
            cmd, last = absolute_command(a, q, tag, origin=origin, last_action=last)
            assert np.array_equal(cmd, want), tag
            assert np.array_equal(last, env._last_action), tag
    assert np.array_equal(E.FR3_LOW, FR3_LOW) and np.array_equal(E.FR3_HIGH, FR3_HIGH)
