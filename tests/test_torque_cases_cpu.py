"""Torque control without a GPU (tests/torque_cases.py): the torque-actuated scene variants as compiled models and on the oracle, and the
host-side surface of the feature.

* ``mjcf.torque_actuated_scene`` on the FR3, xArm7, arm6 and SO101 scenes: every arm actuator a motor (gainprm (1, 0, 0), biastype
  none, zero biasprm, ctrllimited, ctrlrange = the documented source range, no forcerange); the gripper actuator, nu and the joint and
  body tables identical to the source scene's; an include is expanded (fr3_simple_pick_up); a joint without either range is an error
  that names it.
* On the oracle the motor variant of fr3_empty_world, at rest at home with zero torque, keeps every arm joint's |qacc| over 50 substeps
  within the rest residual of the shipped position-servo scene, measured in the same test; with the fingers started where their
  coupling holds them, within round-off of the forces that cancel, and its drift within what that acceleration allows.
* The held-torque cases of the GPU test: the environment pushed at its limit reaches the limit row within the 40 substeps, the
  clamped case lies beyond ctrlrange on two joints, on the oracle.
* The C-ABI declares the entry points and rcsh_torque_law, the ctypes layer mirrors both, RCSH_ABI_VERSION is still 2, and the env
  factory takes ``torque_actuated``.
"""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "robot-control-stack_amd"), HERE]

import parity_util as P  # noqa: E402
import torque_cases as TC  # noqa: E402

REST_SUBSTEPS = 50


@pytest.mark.parametrize("tag", ["fr3", "xarm7", "arm6", "so101", "fr3_pick"])
def test_variant_turns_the_arm_actuators_into_motors_and_nothing_else(tag):
    from rcs_amd.mjcf import BIAS_NONE, TRN_JOINT, compile_mjcf

    src, var = compile_mjcf(TC.SOURCES[tag]), compile_mjcf(TC.torque_scene(tag))
    A, B = src.arrays, var.arrays
    assert var.nu == src.nu and var.actuator_names == src.actuator_names
    arm = [u for u in range(src.nu) if A["actuator_trntype"][u] == TRN_JOINT]
    assert len(arm) == len(TC.RANGES[tag])
    for k, u in enumerate(arm):
        assert B["actuator_trntype"][u] == TRN_JOINT and B["actuator_trnid"][u] == A["actuator_trnid"][u]
        assert tuple(B["actuator_gainprm"][u]) == (1.0, 0.0, 0.0)
        assert B["actuator_biastype"][u] == BIAS_NONE and not B["actuator_biasprm"][u].any()
        assert B["actuator_ctrllimited"][u] == 1 and not B["actuator_forcelimited"][u]
        assert tuple(B["actuator_ctrlrange"][u]) == (-TC.RANGES[tag][k], TC.RANGES[tag][k])
        assert B["actuator_gear"][u] == A["actuator_gear"][u]
    for u in set(range(src.nu)) - set(arm):  # the gripper's tendon actuator
        for key in A:
            if key.startswith("actuator_"):
                assert np.array_equal(A[key][u], B[key][u]), key
    for key in A:  # everything that is not an actuator: joints, bodies, geoms, tendons, equalities
        if not key.startswith("actuator_"):
            assert np.array_equal(A[key], B[key]), key
    assert (var.nbody, var.njnt, var.nq, var.ngeom, var.neq, var.ntendon) == (src.nbody, src.njnt, src.nq, src.ngeom, src.neq, src.ntendon)
    assert var.jnt_names == src.jnt_names and var.body_names == src.body_names
    assert len(var.free_bodies) == len(src.free_bodies)
    for extra in ("collision_vertices.npz", "render_hulls.npz"):
        from rcs_amd.mjcf import find_data_file

        assert (find_data_file(src.data_dirs, extra) is None) == (not os.path.exists(os.path.join(os.path.dirname(TC.torque_scene(tag)), extra)))


def test_a_joint_without_a_torque_range_is_an_error_that_names_it():
    from rcs_amd.mjcf import MjcfError, torque_actuated_scene

    xml = open(P.ARM6_SCENE).read()
    assert 'forcerange="-28 28"' in xml
    d = os.path.join(P.scratch_dir(), "rcs_amd_arm6_no_range")
    os.makedirs(d, exist_ok=True)
    open(os.path.join(d, "scene.xml"), "w").write(xml.replace(' forcerange="-28 28"', ""))
    with pytest.raises(MjcfError, match="wrist_1"):
        torque_actuated_scene(os.path.join(d, "scene.xml"), os.path.join(d, "torque"))


def _rest_run(scene, fingers=None):
    """50 substeps at home under zero torque (motor scene) or the servos' home command: (max |qacc| of an arm joint, max drift of an
    arm joint, max |qfrc_bias| seen, the oracle).  `fingers`: both finger slides start there instead of where the gripper's reset leaves them."""
    o = TC.make_oracle("fr3", scene)
    home = TC.oracle_robot("fr3")["q_home"]
    if fingers is not None:
        o.s.d.qpos[7] = o.s.d.qpos[8] = fingers
    if scene != P.SCENE:
        TC.oracle_set_torque(o, np.zeros(7))
    acc = drift = bias = 0.0
    for _ in range(REST_SUBSTEPS):
        o.step(1)
        acc = max(acc, float(np.abs(np.array(o.s.d.qacc[:7])).max()))
        drift = max(drift, float(np.abs(o.qpos[:7] - home).max()))
        bias = max(bias, float(np.abs(np.array(o.s.d.qfrc_bias[:9])).max()))
    assert np.isfinite(o.qpos).all() and np.isfinite(o.qvel).all()
    return acc, drift, bias, o


def test_motor_variant_rests_at_home_on_the_oracle():
    """Zero torque, at rest, at home: every body is gravity-compensated, so the arm must stay put.
    (1) As the scenes come out of their resets the bar is what the shipped scene's own servos leave: the largest |qacc| of an arm joint
    over the same substeps.  Both runs begin with the same kick -- the fingers, reset to 0.04 / 0, are snapped together by their
    coupling equality and the hand reacts --, so this bar is that kick's.
    (2) With the fingers started where their coupling and the open command hold them (0.04 / 0.04) nothing is left but the arm's own
    residual: gravity compensation against the bias force, two sums of up to `bias` N m that cancel, solved through a mass matrix whose
    smallest diagonal is the armature.  Bar: 64 roundings of the largest bias force over the smallest armature -- an arm in free fall
    would show g / (a link length), fourteen orders above it.  Its drift over the T = 0.1 s is then at most bar T^2 / 2."""
    servo, _, _, _ = _rest_run(P.SCENE)
    motor, _, _, _ = _rest_run(TC.torque_scene("fr3"))
    print("rest residual |qacc| out of the reset: servo %.3e, motor %.3e" % (servo, motor))
    assert motor <= servo, (motor, servo)
    servo2, _, _, _ = _rest_run(P.SCENE, fingers=0.04)
    motor2, drift2, bias2, o = _rest_run(TC.torque_scene("fr3"), fingers=0.04)
    armature = float(np.asarray(o.cm.arrays["dof_armature"])[:7].min())
    bar = 64 * np.finfo(float).eps * bias2 / armature
    T = REST_SUBSTEPS * float(o.cm.timestep)
    print("rest residual |qacc|, fingers coupled: servo %.3e, motor %.3e (bar %.3e); motor drift %.3e (bar %.3e)" % (servo2, motor2, bar, drift2, 0.5 * bar * T * T))
    assert armature > 0 and bias2 > 1.0
    assert motor2 <= bar and drift2 <= 0.5 * bar * T * T, (motor2, drift2, bar)


@pytest.mark.parametrize("tag", sorted(TC.HELD))
def test_held_cases_clamp_and_reach_a_limit_on_the_oracle(tag):
    q0, tau = TC.held_case(tag)
    lim = np.array(TC.RANGES[tag])
    h = TC.HELD[tag]
    assert (np.abs(tau[0]) < lim).all() and (np.abs(tau[4:]) < lim).all() and not tau[3].any()
    assert (np.abs(tau[1]) > lim).sum() == 2
    o = TC.make_oracle(tag)
    TC.oracle_set_state(o, q0[2], tau[2])
    j = h["limit"]
    margin = float(o.cm.arrays["jnt_margin"][j])
    reached = None
    for k in range(TC.HELD_SUBSTEPS):
        o.step(1)
        if reached is None and o.qpos[j] > h["upper"] - margin:
            reached = k
    assert reached is not None and reached < TC.HELD_SUBSTEPS - 5, reached  # (the row then acts for at least five substeps)
    assert np.isfinite(o.qpos).all()


def test_rotvec_is_the_logarithm_on_the_shorter_arc():
    a = np.array([[0.3, -0.5, 0.8]])
    a /= np.linalg.norm(a)
    for ang in (0.0, 1e-14, 0.3, 3.0):
        q = np.concatenate([np.sin(ang / 2) * a, [[np.cos(ang / 2)]]], axis=1)
        ident = np.array([[0.0, 0.0, 0.0, 1.0]])
        assert np.abs(TC.rotvec(q, ident) - ang * a).max() < 1e-15 + 1e-15 * ang
        assert np.abs(TC.rotvec(-q, ident) - ang * a).max() < 1e-15 + 1e-15 * ang  # (the same rotation)
        assert np.abs(TC.rotvec(q, q)).max() < 4e-16  # (the cross terms of q conj(q) cancel to a rounding of products below 1)


def test_c_abi_declares_torque_control():
    from rcs_amd import _lib
    from rcs_amd import envs as E
    from rcs_amd import sim as S

    text = open(os.path.join(HERE, "..", "include", "rcs_hip.h")).read()
    names = ("rcsh_robot_is_torque_actuated", "rcsh_robot_set_joint_torque", "rcsh_robot_set_joint_torque_dev", "rcsh_torque_configure",
             "rcsh_torque_set_target", "rcsh_torque_set_target_dev", "rcsh_torque_get_target", "rcsh_sim_step_torque", "rcsh_torque_status")
    for name in names:
        assert re.search(r"^int\s+" + name + r"\s*\(rcsh_sim\*", text, re.M), name
        assert name in _lib.EXPORTS
    body = re.search(r"typedef struct rcsh_torque_law \{(.*?)\} rcsh_torque_law;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [re.sub(r"\[.*", "", f.strip()) for stmt in re.findall(r"(?:int32_t|uint32_t|double)\s+([^;]+);", body) for f in stmt.split(",")]
    assert declared == [f for f, _ in _lib.TorqueLaw._fields_]
    assert re.search(r"^#define\s+RCSH_MAX_ARM\s+8\s*$", text, re.M)
    assert C.sizeof(_lib.TorqueLaw) == 4 + 4 + 8 + 7 * 8 + 12 * 8 + 16 * 8 + 8
    assert re.search(r"^#define\s+RCSH_ABI_VERSION\s+2\s*$", text, re.M)  # (entry points were added, none changed)
    assert _lib.load().rcsh_abi_version() == 2
    for fn in (E.make_vec_env,):
        assert inspect.signature(fn).parameters["torque_actuated"].default is False
    for method in ("set_joint_torque", "configure_torque_law", "set_torque_target", "torque_status", "torque_actuated"):
        assert hasattr(S.SimRobot, method), method
    assert hasattr(S.Sim, "step_torque")


def test_factory_routes_through_the_helper():
    from rcs_amd.envs import factory
    from rcs_amd.mjcf import BIAS_NONE, compile_mjcf

    cfg = factory.robot_cfg_for("arm6", torque_actuated=True)
    assert cfg.mjcf_scene_path != factory.robot_cfg_for("arm6").mjcf_scene_path
    m = compile_mjcf(cfg.mjcf_scene_path)
    assert (m.arrays["actuator_biastype"] == BIAS_NONE).all()
