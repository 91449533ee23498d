"""One-call construction of the batched environments for the shipped scenes.

The reference builds its environments through ``SimEnvCreator()(control_mode, robot_cfg, gripper_cfg=..., ...)``
(python/rcs/envs/creators.py:79-128; examples/fr3/fr3_env_joint_control.py:34-41); this is that call with the
per-robot default configurations filled in, for benchmarks, examples and tests.
"""

from __future__ import annotations

import numpy as np

from .. import sim
from .base import ControlMode, RelativeTo
from .creators import SimEnvCreator
from .utils import (arm6_sim_robot_cfg, default_sim_gripper_cfg, default_sim_robot_cfg, so101_sim_gripper_cfg, so101_sim_robot_cfg,
                    ur5e_sim_robot_cfg, xarm7_pick_sim_gripper_cfg, xarm7_pick_sim_robot_cfg, xarm7_sim_robot_cfg)

# max_relative_movement of the reference's joint-control example (examples/fr3/fr3_env_joint_control.py:38)
MAX_JOINT_MOV = float(np.deg2rad(5))

ROBOTS = ("fr3", "xarm7", "xarm7_box", "xarm7_pick", "arm6", "ur5e", "so101")


def torque_actuated_cfg(cfg: sim.SimRobotConfig) -> sim.SimRobotConfig:
    """A copy of `cfg` with its scene replaced by the torque-actuated variant (mjcf.torque_actuated_scene: the actuators of the
    robot's own joints become `<motor>`s), written to the process's scratch directory."""
    import copy

    from ..mjcf import torque_actuated_scene

    out = copy.copy(cfg)
    src = str(cfg.mjcf_scene_path)
    out.mjcf_scene_path = out.kinematic_model_path = torque_actuated_scene(src[:-4] + ".xml" if src.endswith(".mjb") else src, joints=list(cfg.joints))
    return out


def robot_cfg_for(robot: str, torque_actuated: bool = False) -> sim.SimRobotConfig:
    if torque_actuated:
        return torque_actuated_cfg(robot_cfg_for(robot))
    if robot == "fr3":
        return default_sim_robot_cfg("fr3_empty_world")
    if robot == "xarm7":
        return xarm7_sim_robot_cfg("xarm7_empty_world")
    if robot == "xarm7_box":
        return xarm7_sim_robot_cfg("xarm7_box_world")
    if robot == "xarm7_pick":
        return xarm7_pick_sim_robot_cfg()
    if robot == "arm6":
        return arm6_sim_robot_cfg()
    if robot == "ur5e":
        return ur5e_sim_robot_cfg()
    if robot == "so101":
        return so101_sim_robot_cfg()
    raise ValueError(f"unknown robot {robot!r}: one of {ROBOTS}")


def make_vec_env(n_envs: int, async_control: bool, gripper: bool = True, relative: bool = True, control_mode=None, device: int = 0,
                 max_relative_movement=None, robot: str = "fr3", relative_to: str = "last_step", frequency: int = 30,
                 max_convergence_steps: int = 500, robot_cfg: sim.SimRobotConfig | None = None, resolve_robot_contacts=None,
                 collision_guard: bool = False, torque_actuated: bool = False, torque_law: dict | None = None):
    """`n_envs` environments of one robot type on GPU `device`.  `robot_cfg` overrides the robot's default configuration
    (its scene decides the kernel archetype); only the FR3, SO101 and xarm7_pick scenes carry a gripper.  `collision_guard`: the
    batched collision guard at its defaults (VecSimEnv.configure_guard; joint-space control only).  `torque_actuated`: the scene's
    torque-actuated variant (every arm actuator a `<motor>`: `SimRobot.set_joint_torque`, `Sim.step_torque`).  The env layer drives
    it in the control modes `ControlMode.TORQUE` (action `"torque"`: joint torques; no relative action space, `relative` is ignored),
    `JOINT_IMPEDANCE` (`"joints"`), `CARTESIAN_IMPEDANCE_TRPY` (`"xyzrpy"`) and `CARTESIAN_IMPEDANCE_TQuat` (`"tquat"`), whose actions
    become the targets of the substep-rate law given as `torque_law=dict(...)` (the keyword arguments of
    `SimRobot.configure_torque_law`; SimEnvCreator); these modes need `torque_actuated=True` and `async_control=True`.  In the
    position modes the actions of such an env stay position commands and do not drive it."""
    cfg = sim.SimConfig(async_control=async_control, realtime=False, frequency=frequency, max_convergence_steps=max_convergence_steps)
    mode = control_mode or ControlMode.JOINTS
    if mode == ControlMode.TORQUE:
        relative = False
    if relative and max_relative_movement is None:
        max_relative_movement = MAX_JOINT_MOV
    if not (robot.startswith("fr3") or robot in ("so101", "xarm7_pick")):
        gripper = False
    gripper_cfg = ((so101_sim_gripper_cfg() if robot == "so101" else xarm7_pick_sim_gripper_cfg() if robot == "xarm7_pick" else default_sim_gripper_cfg())
                   if gripper else None)
    rcfg = robot_cfg if robot_cfg is not None else robot_cfg_for(robot)
    if torque_actuated:
        rcfg = torque_actuated_cfg(rcfg)
    return SimEnvCreator()(
        mode, rcfg, collision_guard=collision_guard,
        gripper_cfg=gripper_cfg,
        sim_cfg=cfg, max_relative_movement=max_relative_movement if relative else None,
        relative_to=RelativeTo.LAST_STEP if relative_to == "last_step" else RelativeTo.CONFIGURED_ORIGIN,
        n_envs=n_envs, device=device, resolve_robot_contacts=resolve_robot_contacts, torque_law=torque_law,
    )
