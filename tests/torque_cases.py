"""Cases of the torque-control tests (csrc/torque_team.h): the torque-actuated scene variants, the torque vectors held against the
oracle, and the law of ``Sim.step_torque`` composed in numpy from query outputs the suite already holds to fixtures and to the oracle.

The variants are written by ``rcs_amd.mjcf.torque_actuated_scene`` into this process's scratch directory; nothing here is a copy of a
scene file.  ``RANGES`` is the documented source of every motor's ``ctrlrange``: the old actuator's ``forcerange`` (xArm7, arm6, UR5e,
SO101: their default classes) or the joint's ``actuatorfrcrange`` (FR3: its ``<position>`` servos carry no forcerange).
"""

from __future__ import annotations

import functools
import os

import numpy as np

import parity_util as P

N = 6  # one full wavefront (four teams) and one with two idle teams

SOURCES = {
    "fr3": P.SCENE, "xarm7": P.XARM7_SCENE, "arm6": P.ARM6_SCENE, "so101": P.SO101_SCENE, "ur5e": P.UR5E_SCENE, "fr3_pick": P.PICKUP_SCENE,
}
RANGES = {
    "fr3": [87.0, 87.0, 87.0, 87.0, 12.0, 12.0, 12.0],
    "xarm7": [50.0, 50.0, 30.0, 30.0, 30.0, 20.0, 20.0],
    "arm6": [150.0, 150.0, 150.0, 28.0, 28.0, 28.0],
    "ur5e": [150.0, 150.0, 150.0, 28.0, 28.0, 28.0],
    "so101": [3.0, 3.0, 3.0, 3.0, 3.0],
}
RANGES["fr3_pick"] = RANGES["fr3"]


def torque_scene(tag: str) -> str:
    """Path of the torque-actuated variant of the shipped scene `tag`, written once per process."""
    from rcs_amd.mjcf import torque_actuated_scene

    return torque_actuated_scene(SOURCES[tag], os.path.join(P.scratch_dir(), f"rcs_amd_torque_{tag}"))


def robot_cfg(tag: str):
    """The robot configuration of `tag` on its torque-actuated variant."""
    from rcs_amd import envs as E

    cfg = {"fr3": lambda: E.default_sim_robot_cfg("fr3_empty_world"), "fr3_pick": lambda: E.default_sim_robot_cfg("fr3_simple_pick_up"),
           "xarm7": E.xarm7_sim_robot_cfg, "arm6": E.arm6_sim_robot_cfg, "ur5e": E.ur5e_sim_robot_cfg, "so101": E.so101_sim_robot_cfg}[tag]()
    cfg.mjcf_scene_path = cfg.kinematic_model_path = torque_scene(tag)
    return cfg


def oracle_robot(tag: str) -> dict:
    import rcs_env_oracle as R

    return {"fr3": R.FR3, "xarm7": R.XARM7, "arm6": R.ARM6, "ur5e": R.UR5E, "so101": R.SO101}[tag]


def make_oracle(tag: str, scene: str | None = None):
    """One oracle environment on the torque-actuated variant of `tag` (`scene`: another file of the same robot)."""
    import rcs_oracle as O
    from rcs_amd.mjcf import compile_mjcf

    r = oracle_robot(tag)
    cm = compile_mjcf(scene or torque_scene(tag))
    return O.Sim(cm, r["joints"], r["actuators"], r["site"], r["base"], r["q_home"], None, r["gripper_joint"], r["gripper_actuator"],
                 arm_collision_geoms=r.get("arm_collision_geoms"), gripper_cfg=r.get("gripper_cfg"))


def oracle_set_state(o, qpos, ctrl_arm=None):
    """qpos (all joints) into the oracle, at rest; the arm's torques if given."""
    for i, x in enumerate(qpos):
        o.s.d.qpos[i] = float(x)
        o.s.d.qvel[i] = 0.0
    if ctrl_arm is not None:
        oracle_set_torque(o, ctrl_arm)


def oracle_set_torque(o, tau):
    for i, x in enumerate(tau):
        o.s.d.ctrl[int(o.s.arm_act[i])] = float(x)


# ---- test 1: torque vectors held for 40 substeps.  Per robot: the start configuration of every environment (arm joints; fingers,
# where there are any, mid-stroke) and its torque vector, as fractions of the joints' limits:
#   0 within limits; 1 beyond ctrlrange on two joints (the clamp acts); 2 the `limit` joint started LIMIT_START short of its upper
#   limit and pushed into it at full torque (tests/test_torque_cases_cpu.py checks on the oracle that its limit row is reached within
#   the 40 substeps); 3 all zero; 4, 5 two more within limits, moved off the home pose.
HELD_SUBSTEPS = 40
LIMIT_START = 0.05  # rad
HELD = {
    "fr3": dict(limit=6, upper=3.0159, finger=0.02),
    "xarm7": dict(limit=5, upper=3.14159, finger=None),
    "arm6": dict(limit=2, upper=3.14159, finger=None),
}


@functools.lru_cache(maxsize=None)
def held_case(tag: str):
    """(q0 [N, nl], tau [N, narm]) of the held-torque test; shared: do not modify."""
    r = oracle_robot(tag)
    lim = np.array(RANGES[tag])
    narm = len(lim)
    h = HELD[tag]
    rng = np.random.default_rng(11)
    nl = narm + (2 if h["finger"] is not None else 0)
    q0 = np.zeros((N, nl))
    q0[:, :narm] = r["q_home"]
    if h["finger"] is not None:
        q0[:, narm:] = h["finger"]
    q0[4:, :narm] += rng.uniform(-0.2, 0.2, size=(2, narm))
    q0[2, h["limit"]] = h["upper"] - LIMIT_START
    frac = np.zeros((N, narm))
    frac[0] = rng.uniform(-0.3, 0.3, size=narm)
    frac[1] = rng.uniform(-0.2, 0.2, size=narm)
    frac[1, 0], frac[1, narm - 1] = 1.5, -2.0
    frac[2, h["limit"]] = 1.0
    frac[4:] = rng.uniform(-0.4, 0.4, size=(2, narm))
    tau = frac * lim
    q0.setflags(write=False)
    tau.setflags(write=False)
    return q0, tau


# ---- tests 2 to 5: the law.  Gains on the task acceleration (1 / s^2, 1 / s: a critically damped 10 rad / s) and on the null-space
# torque (N m / rad, N m s / rad).
LAW_SUBSTEPS = 51
TASK_K, TASK_D, JOINT_K, JOINT_D = 100.0, 20.0, 10.0, 2.0
LAW_SETTINGS = {"full": 0x3F, "position": 0x07, "joint": 0}
# a TCP offset that is translated and turned (0.6 rad about an oblique axis): the law's TCP must be the queries'
TCP_OFFSET = np.concatenate([[0.02, -0.01, 0.1034], np.sin(0.3) * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), [np.cos(0.3)]])
# the rotation log away from 0.3 rad: no rotation, below any series threshold, small, and towards the half turn
ARC_ANGLES = (0.0, 1e-14, 1e-6, 0.3, 2.0, 3.0)
# (robot, setting) -> task_mask, tcp_offset, rotation angles of the targets (None: 0.3 rad everywhere).  The three FR3 settings of the
# issue; the offset and the arcs; and the instances the FR3 does not reach: the 7-dof arm with friction rows, the 5-dof arm + gripper.
LAW_RUNS = {
    ("fr3", "full"): dict(mask=0x3F), ("fr3", "position"): dict(mask=0x07), ("fr3", "joint"): dict(mask=0),
    ("fr3", "offset"): dict(mask=0x3F, tcp_offset=TCP_OFFSET), ("fr3", "arc"): dict(mask=0x3F, angles=ARC_ANGLES),
    ("xarm7", "full"): dict(mask=0x3F), ("xarm7", "joint"): dict(mask=0),
    ("so101", "position"): dict(mask=0x07), ("so101", "joint"): dict(mask=0),
}


def quat_mul(a, b):
    """x y z w, rows."""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def rotvec(q_des, q_cur):
    """Rotation vector of R_des R^T on the shorter arc, from the two quaternions (x y z w rows), in the frame both are given in."""
    qd = q_des / np.linalg.norm(q_des, axis=-1, keepdims=True)
    qe = quat_mul(qd, q_cur * np.array([-1.0, -1.0, -1.0, 1.0]))
    sg = np.where(qe[..., 3] < 0.0, -1.0, 1.0)
    nv = np.linalg.norm(qe[..., :3], axis=-1)
    f = np.where(nv > 1e-12, sg * 2.0 * np.arctan2(nv, sg * qe[..., 3]) / np.where(nv > 1e-12, nv, 1.0), 2.0 * sg)
    return f[..., None] * qe[..., :3]


def law_start(tag: str = "fr3", seed: int = 5, angles=None):
    """(q0 [N, nl], pose offsets, q_des [N, narm]): start configurations scattered about home, targets 5 cm and 0.3 rad away."""
    r = oracle_robot(tag)
    narm = len(r["q_home"])
    rng = np.random.default_rng(seed)
    nl = narm + (2 if r["gripper_joint"] else 0)
    q0 = np.zeros((N, nl))
    q0[:, :narm] = r["q_home"] + rng.uniform(-0.15, 0.15, size=(N, narm))
    if nl > narm:
        q0[:, narm:] = 0.015 if tag == "so101" else 0.02
    d = rng.normal(size=(N, 3))
    dp = 0.05 * d / np.linalg.norm(d, axis=1, keepdims=True)
    a = rng.normal(size=(N, 3))
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    half = 0.5 * (np.full(N, 0.3) if angles is None else np.asarray(angles, dtype=np.float64))
    dq = np.concatenate([np.sin(half)[:, None] * a, np.cos(half)[:, None]], axis=1)  # 0.3 rad (or `angles`) about a
    s = rng.choice([-1.0, 1.0], size=(N, narm))
    q_des = q0[:, :narm] + 0.3 * s * (rng.uniform(size=(N, narm)) < 0.4)
    return q0, dp, dq, q_des


def pose_targets(pose0, dp, dq):
    """The start poses [N, 7] moved by dp and turned by dq (base frame)."""
    out = np.array(pose0)
    out[:, :3] += dp
    out[:, 3:] = quat_mul(dq, pose0[:, 3:])
    return out


def compose_torque(venv, mask: int, pose_des, q_des, damping: float = 0.0, tcp_offset=None, compensate_bias: bool = True,
                   task_k=TASK_K, task_d=TASK_D, joint_k=JOINT_K, joint_d=JOINT_D):
    """The law at the environments' present state, from the public queries: (tau [N, narm], status [N]).  Rows of status 1 are NaN."""
    robot = venv.robot
    narm = robot.dof
    q, v = venv.sim.qpos, venv.sim.qvel
    n, nl = q.shape
    d = venv.dynamics(want=("qfrc_bias", "qfrc_gravcomp"))
    null = np.zeros((n, nl))
    null[:, :narm] = joint_k * (q_des - q[:, :narm]) - joint_d * v[:, :narm]
    if compensate_bias:
        null += d["qfrc_bias"]
    if mask == 0:
        return (null - d["qfrc_gravcomp"])[:, :narm], np.zeros(n, dtype=np.int32)
    pose = robot.get_ik().forward(q[:, :narm], tcp_offset)
    tw = venv.opspace(want=("twist",), tcp_offset=tcp_offset, task_mask=mask)["twist"]
    x_err = np.concatenate([pose_des[:, :3] - pose[:, :3], rotvec(pose_des[:, 3:], pose[:, 3:])], axis=1)
    xacc = task_k * x_err - task_d * tw
    o = venv.opspace(xacc=xacc, qfrc_null=null, tcp_offset=tcp_offset, task_mask=mask, damping=damping, want=("qfrc", "status"))
    return (o["qfrc"] - d["qfrc_gravcomp"])[:, :narm], o["status"]
