"""``SimEnvCreator`` for N environments (reference python/rcs/envs/creators.py:43-128).

The reference builds one Gymnasium env out of nested wrappers around one MuJoCo
instance.  Here the same constructor arguments produce a :class:`VecSimEnv`:
``reset()`` / ``step(action)`` have the Gymnasium signatures, but every array
carries a leading ``n_envs`` axis and one call is one kernel launch that performs
the wrappers' side effects, the physics substeps and the observation for all
environments (csrc/sim_kernels.h: k_run).
"""

from __future__ import annotations

import ctypes as C
from typing import Any

import numpy as np

from .. import _lib, common, sim
from .base import ControlMode, RelativeTo

_MODE = {ControlMode.JOINTS: _lib.RCSH_MODE_JOINTS, ControlMode.CARTESIAN_TRPY: _lib.RCSH_MODE_CARTESIAN_TRPY,
         ControlMode.CARTESIAN_TQuat: _lib.RCSH_MODE_CARTESIAN_TQUAT, ControlMode.TORQUE: _lib.RCSH_MODE_TORQUE,
         ControlMode.JOINT_IMPEDANCE: _lib.RCSH_MODE_JOINT_IMPEDANCE,
         ControlMode.CARTESIAN_IMPEDANCE_TRPY: _lib.RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY,
         ControlMode.CARTESIAN_IMPEDANCE_TQuat: _lib.RCSH_MODE_CARTESIAN_IMPEDANCE_TQUAT}
_REL = {None: 0, RelativeTo.LAST_STEP: 1, RelativeTo.CONFIGURED_ORIGIN: 2}
_ACTION_KEY = {ControlMode.JOINTS: "joints", ControlMode.CARTESIAN_TRPY: "xyzrpy", ControlMode.CARTESIAN_TQuat: "tquat",
               ControlMode.TORQUE: "torque", ControlMode.JOINT_IMPEDANCE: "joints", ControlMode.CARTESIAN_IMPEDANCE_TRPY: "xyzrpy",
               ControlMode.CARTESIAN_IMPEDANCE_TQuat: "tquat"}
# the torque and impedance modes of torque-actuated robots (csrc/env_torque_team.h)
TORQUE_MODES = (ControlMode.TORQUE, ControlMode.JOINT_IMPEDANCE, ControlMode.CARTESIAN_IMPEDANCE_TRPY, ControlMode.CARTESIAN_IMPEDANCE_TQuat)
_JOINT_ROW_MODES = (ControlMode.JOINTS, ControlMode.TORQUE, ControlMode.JOINT_IMPEDANCE)

DEFAULT_MAX_CART_MOV = 0.5  # reference base.py:366-368
DEFAULT_MAX_CART_ROT = np.deg2rad(90)
DEFAULT_MAX_JOINT_MOV = np.deg2rad(5)


class VecSimEnv:
    """N-environment ``gym.Env`` look-alike returned by :class:`SimEnvCreator`.

    obs dict: ``tquat [N,7]``, ``joints [N,dof]``, ``xyzrpy [N,6]`` (+ ``gripper [N]``);
    info dict: ``collision``, ``ik_success``, ``is_sim_converged`` (+ ``gripper_width``, ``is_grasped``), all ``[N]``;
    ``step`` returns ``(obs, reward [N] = 0, terminated [N] = False, truncated [N], info)``.

    With a collision guard (``SimEnvCreator()(..., collision_guard=True)`` or :meth:`configure_guard`) every step first decides, on
    the device, whether the straight joint-space motion from where each arm is to where its action sends it is proven free of
    contact (csrc/guard_team.h).  A blocked environment is commanded to stay where it is and -- with ``truncate_on_collision`` -- is
    reported ``terminated`` and ``truncated``; ``info`` gains ``guard_blocked``, ``guard_result`` and ``guard_t_contact``.

    With autoreset (:meth:`configure_autoreset`; Gymnasium's ``VectorEnv`` autoreset in its SAME_STEP mode) an environment whose episode
    ends -- ``terminated``, ``truncated``, or a time limit -- is reset on the device inside the same step: the returned ``obs`` rows of
    those environments are the new episode's first observation, ``terminated`` / ``truncated`` / the reward are the terminal step's,
    and ``info`` gains ``autoreset`` (done), ``TimeLimit.truncated``, ``episode`` (``{"r", "l"}``, valid where done) and ``final_obs``
    (the observation dict of the terminal step in the done rows, zeros elsewhere).  A ``CameraSetWrapper``'s ``clear_buffer()`` is
    global to the batch and is NOT called on an autoreset; rate-driven cameras cannot be combined with autoreset.
    """

    def __init__(self, simulation: sim.Sim, robot: sim.SimRobot, gripper: sim.SimGripper | None,
                 control_mode: ControlMode, max_relative_movement, relative_to: RelativeTo, camera_set=None):
        self.camera_set = camera_set  # CameraSetWrapper(env, camera_set, include_depth=True), base.py:585-677
        self.sim = simulation
        self.robot = robot
        self.gripper = gripper
        self.control_mode = control_mode
        self.n_envs = simulation.n_envs
        self.dof = robot.dof
        self._L = simulation._L
        meta = common.sim_robots_meta_config(robot.get_config().robot_type)
        self._low = np.ascontiguousarray(meta.joint_limits[0][: self.dof], dtype=np.float64)
        self._high = np.ascontiguousarray(meta.joint_limits[1][: self.dof], dtype=np.float64)
        rel = 0
        max_mov = [0.0, 0.0]
        if max_relative_movement is not None:
            rel = _REL[relative_to]
            if control_mode in _JOINT_ROW_MODES:
                assert isinstance(max_relative_movement, float), "joint-space max_mov must be a float (rad)"
                max_mov = [float(max_relative_movement), 0.0]
            elif isinstance(max_relative_movement, tuple):
                max_mov = [float(max_relative_movement[0]), float(max_relative_movement[1])]
            else:
                max_mov = [float(max_relative_movement), float(DEFAULT_MAX_CART_ROT)]
        self.max_mov = max_mov
        self.relative_to = relative_to if rel else None
        d = _lib.EnvDesc()
        d.control_mode = _MODE[control_mode]
        d.relative_to = rel
        d.max_mov[:] = max_mov
        d.binary_gripper = 1
        d.joint_low = self._low.ctypes.data_as(C.POINTER(C.c_double))
        d.joint_high = self._high.ctypes.data_as(C.POINTER(C.c_double))
        _lib.check(self._L.rcsh_env_configure(simulation._h, C.byref(d)))
        self.obs_width = self._L.rcsh_env_obs_width(simulation._h)
        self.action_width = self._L.rcsh_env_action_width(simulation._h)
        self.action_key = _ACTION_KEY[control_mode]
        # What an environment gets whose geoms are found in a contact this configuration does not resolve (info["contact_unresolved"],
        # sticky until reset; csrc/check_team.h).  The reference resolves every contact in every mode (mj_step2, sim.cpp:112); the
        # lean kernels of scenes without a free body do not, because the capability costs the contact-free rollout ~15 %.
        #   "resolve": (default, round 5) nothing stays unresolved: the Sim resolves robot contacts environment by environment
        #              (Sim(resolve_robot_contacts=None): mode 7 in scenes without a free body), robot <-> robot included.  A Sim that
        #              was created with resolve_robot_contacts=False is switched to that mode as soon as a step reports a contact
        #              (host-array interface only: the `*_dev` entry points never read the flags back);
        #   "flag":    report only -- with a Sim created with resolve_robot_contacts=False the environment steps on unresolved (the arm
        #              passes through the floor / itself) and the caller decides (mask it, reset it, discard the episode).
        self.on_unresolved_contact = "resolve"
        self.guard_enabled = False
        self.guard_truncates = True
        self.autoreset_enabled = False
        self.autoreset_desc: _lib.AutoresetDesc | None = None  # what the last configure_autoreset passed down (autoreset_draw reads it)

    # ---- collision guard (reference python/rcs/envs/sim.py:156-287: CollisionGuard between RelativeActionSpace and RobotEnv.step)
    def default_guard_kinds(self) -> int:
        """Everything the scene has where there is no free body; floor | self where there is one: a pick-up task must be allowed
        to touch its cube, so guarding against the free body is opt-in (``kinds=7``)."""
        R = sim.SimRobot
        has_free = bool(getattr(self.sim.model, "free_bodies", []))
        return R.COLLISION_FLOOR | R.COLLISION_SELF if has_free else R.COLLISION_ALL

    def configure_guard(self, enabled: bool = True, kinds: int | None = None, resolution: float = 1e-3, block_undecided: bool = True,
                        truncate_on_collision: bool = True) -> None:
        """Configure the batched collision guard (joint-space control modes only; RuntimeError otherwise).

        An action passes only when the straight joint-space motion from the arm's current configuration to the absolute joint
        command the action resolves to is PROVEN free of the selected ``kinds`` of contact (the motion query's lever certificate,
        :meth:`rcs_amd.sim.SimRobot.check_motion`; finger slides and the free body as they are now).  ``guard_result`` 1 (a contact
        was found) blocks; 2 (neither proven nor refuted down to ``resolution``) blocks when ``block_undecided``.  A blocked
        environment's arm is commanded to its current joint position; the relative action space advances on the original action and
        the gripper command applies unchanged.  Two deviations from the reference, on purpose: the decision is kinematic and
        certifying, not a shadow simulation (which the reference marks as not working); and every environment of the batch steps -- a
        blocked one with the hold command, its fresh observation returned -- where the reference returns the previous observation.
        ``truncate_on_collision`` only decides whether blocked environments are reported ``terminated`` and ``truncated``.
        ``enabled=False`` leaves the steps unguarded (:meth:`check_action` still answers)."""
        d = _lib.GuardDesc()
        d.enabled = int(bool(enabled))
        d.kinds = self.default_guard_kinds() if kinds is None else int(kinds)
        d.resolution = float(resolution)
        d.block_undecided = int(bool(block_undecided))
        d.truncate = int(bool(truncate_on_collision))
        _lib.check(self._L.rcsh_env_configure_guard(self.sim._h, C.byref(d)))
        self.guard_enabled = bool(enabled)
        self.guard_truncates = bool(truncate_on_collision)

    def check_action(self, action):
        """The guard's decision for an action batch (``{"joints": [N, dof]}`` or the array), without stepping and without writing any
        state: ``(blocked bool [N], result int32 [N], t_contact [N])``.  Needs :meth:`configure_guard` (``enabled`` or not)."""
        n = self.n_envs
        a = action[self.action_key] if isinstance(action, dict) else action
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, self.action_width)))
        result = np.zeros(n, dtype=np.int32)
        tc = np.zeros(n)
        blocked = np.zeros(n, dtype=np.uint8)
        _lib.check(self._L.rcsh_env_guard_peek(self.sim._h, _lib.ptr(a), _lib.ptr(result), _lib.ptr(tc), _lib.ptr(blocked)))
        return blocked.astype(bool), result, tc

    def guard_last(self):
        """``(blocked, result, t_contact)`` of the most recent guarded step (what ``step`` puts into ``info``; for ``step_dev`` loops)."""
        n = self.n_envs
        result = np.zeros(n, dtype=np.int32)
        tc = np.zeros(n)
        blocked = np.zeros(n, dtype=np.uint8)
        _lib.check(self._L.rcsh_env_guard_last(self.sim._h, _lib.ptr(result), _lib.ptr(tc), _lib.ptr(blocked)))
        return blocked.astype(bool), result, tc

    def guard_last_dev(self) -> tuple[int, int, int]:
        """Device pointers ``(blocked uint8 [N], result int32 [N], t_contact float64 [N])`` of the guarded steps' record: valid for the
        Sim's life, rewritten by every guarded step."""
        r, t, b = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.check(self._L.rcsh_env_guard_last_dev(self.sim._h, C.byref(r), C.byref(t), C.byref(b)))
        return int(b.value), int(r.value), int(t.value)

    # ---- clearance (csrc/clearance_team.h): on demand, not part of step
    def clearance(self, kinds: int | None = None, pair_mask=None, d_max: float = np.inf):
        """Every environment's distance to the nearest obstacle where it is now: its own arm joints and finger slides and -- in a
        scene with a free body, ``kinds`` bit 2 -- the body at its own pose.  Arguments and the returned ``(distance [N], status [N],
        pair [N, 2], witness [N, 6], grad [N, nl])`` as :meth:`rcs_amd.sim.SimRobot.check_clearance` (``kinds`` None: every kind;
        ``pair_mask`` indexed by ``robot.clearance_pairs(kinds)``).  Reads the state, writes none of it."""
        n = self.n_envs
        kinds = sim.SimRobot.COLLISION_ALL if kinds is None else int(kinds)
        mask = None
        if pair_mask is not None:
            mask = np.ascontiguousarray(pair_mask, dtype=np.uint8).reshape(-1)
            count = C.c_int32(0)
            _lib.check(self._L.rcsh_clearance_pairs(self.sim._h, kinds, None, 0, C.byref(count)))
            if mask.shape[0] != count.value:
                raise ValueError(f"pair_mask has {mask.shape[0]} entries, the pair list for kinds={kinds} has {count.value}")
        dist = np.zeros(n)
        status = np.zeros(n, dtype=np.uint8)
        pair = np.full((n, 2), -1, dtype=np.int32)
        wit = np.zeros((n, 6))
        grad = np.zeros((n, int(self.sim.model.nq)))
        _lib.check(self._L.rcsh_env_clearance(self.sim._h, kinds, _lib.ptr(mask), float(d_max), _lib.ptr(dist), _lib.ptr(status),
                                              _lib.ptr(pair), _lib.ptr(wit), _lib.ptr(grad)))
        return dist, status, pair, wit, grad

    def clearance_dev(self, distance_dev: int, status_dev: int = 0, pair_dev: int = 0, witness_dev: int = 0, grad_dev: int = 0,
                      kinds: int | None = None, pair_mask_dev: int = 0, d_max: float = np.inf) -> None:
        """:meth:`clearance` into device buffers (addresses; 0: not wanted -- ``distance_dev`` is required), enqueued on the Sim's
        stream without a synchronisation.  ``pair_mask_dev``: device address of the mask bytes, 0 for every pair."""
        kinds = sim.SimRobot.COLLISION_ALL if kinds is None else int(kinds)
        p = lambda a: C.c_void_p(a) if a else None  # noqa: E731
        _lib.check(self._L.rcsh_env_clearance_dev(self.sim._h, kinds, p(pair_mask_dev), float(d_max), p(distance_dev), p(status_dev),
                                                  p(pair_dev), p(witness_dev), p(grad_dev)))

    # ---- swept clearance (csrc/swept_team.h): on demand, not part of step
    def swept_clearance(self, q_to, tolerance: float = 1e-3, resolution: float = 1e-3, d_max: float = np.inf, kinds: int | None = None,
                        pair_mask=None) -> dict:
        """How close does every environment come to anything on the straight joint-space motion from where it is now to ``q_to``
        [N, nl] (the free body standing still at its own pose)?  Arguments and the returned dict as
        :meth:`rcs_amd.sim.SimRobot.swept_clearance` (``kinds`` None: every kind).  Reads the state, writes none of it."""
        n, nl = self.n_envs, int(self.sim.model.nq)
        kinds = sim.SimRobot.COLLISION_ALL if kinds is None else int(kinds)
        rows = np.ascontiguousarray(np.broadcast_to(np.asarray(q_to, dtype=np.float64), (n, nl)))
        mask = None
        if pair_mask is not None:
            mask = np.ascontiguousarray(pair_mask, dtype=np.uint8).reshape(-1)
            count = C.c_int32(0)
            _lib.check(self._L.rcsh_clearance_pairs(self.sim._h, kinds, None, 0, C.byref(count)))
            if mask.shape[0] != count.value:
                raise ValueError(f"pair_mask has {mask.shape[0]} entries, the pair list for kinds={kinds} has {count.value}")
        arrays, out = self.robot._swept_buffers(n, nl)
        _lib.check(self._L.rcsh_env_swept_clearance(self.sim._h, _lib.ptr(rows), kinds, _lib.ptr(mask), float(d_max), float(tolerance),
                                                    float(resolution), C.byref(out)))
        return arrays

    def swept_clearance_dev(self, q_to_dev: int, out: dict, tolerance: float = 1e-3, resolution: float = 1e-3, d_max: float = np.inf,
                            kinds: int | None = None, pair_mask_dev: int = 0) -> None:
        """:meth:`swept_clearance` into device buffers, enqueued on the Sim's stream without a synchronisation.  ``q_to_dev``: device
        address of the [N, nl] ends; ``out``: device addresses by output name (``distance`` is required; absent or 0: not wanted);
        ``pair_mask_dev``: device address of the mask bytes, 0 for every pair."""
        kinds = sim.SimRobot.COLLISION_ALL if kinds is None else int(kinds)
        o = _lib.SweptOut(**{k: int(v) for k, v in out.items() if v})
        _lib.check(self._L.rcsh_env_swept_clearance_dev(self.sim._h, C.c_void_p(q_to_dev), kinds, C.c_void_p(pair_mask_dev) if pair_mask_dev else None,
                                                        float(d_max), float(tolerance), float(resolution), C.byref(o)))

    # ---- dynamics (csrc/dynamics_team.h): on demand, not part of step
    def dynamics(self, want=None, qacc=None, qfrc=None, tcp_offset=None) -> dict:
        """Every environment's joint-space inertia, bias forces and TCP Jacobian where it is now: its own chain ``qpos`` and ``qvel``.
        ``want``, ``qacc`` / ``qfrc`` ([N, nl], for ``qfrc_inverse`` / ``qacc``), ``tcp_offset`` and the returned dict of arrays as
        :meth:`rcs_amd.sim.SimRobot.dynamics_query`.  Reads the state, writes none of it."""
        n, nl = self.n_envs, int(self.sim.model.nq)
        want = self.robot._dynamics_want(want, qacc, qfrc)
        rows = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, nl)))  # noqa: E731
        a, f = rows(qacc), rows(qfrc)
        arrays, out = self.robot._dynamics_buffers(want, n, nl)
        tcp = sim.DeviceKinematics._tcp(tcp_offset)
        _lib.check(self._L.rcsh_env_dynamics(self.sim._h, _lib.ptr(a), _lib.ptr(f), _lib.ptr(tcp), C.byref(out)))
        return arrays

    def dynamics_derivatives(self, want=None, qacc=None, qfrc=None) -> dict:
        """Every environment's dynamics linearised where it is now: the Jacobians of ``qfrc_inverse`` and ``qacc`` at its own chain
        ``qpos`` and ``qvel``.  ``want``, ``qacc`` / ``qfrc`` ([N, nl]) and the returned dict of arrays [N, nl, nl] as
        :meth:`rcs_amd.sim.SimRobot.dynamics_derivatives`.  Reads the state, writes none of it."""
        n, nl = self.n_envs, int(self.sim.model.nq)
        want = self.robot._dynamics_grad_want(want, qacc, qfrc)
        rows = lambda a: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, nl)))  # noqa: E731
        a, f = rows(qacc), rows(qfrc)
        arrays, out = self.robot._dynamics_grad_buffers(want, n, nl)
        _lib.check(self._L.rcsh_env_dynamics_derivatives(self.sim._h, _lib.ptr(a), _lib.ptr(f), C.byref(out)))
        return arrays

    def opspace(self, xacc=None, qfrc_null=None, tcp_offset=None, task_mask=0x3F, damping=0.0, want=None) -> dict:
        """Every environment's operational-space dynamics where it is now: its own chain ``qpos`` and ``qvel``.  ``xacc`` [N, 6],
        ``qfrc_null`` [N, nl], ``tcp_offset``, ``task_mask``, ``damping``, ``want`` and the returned dict of arrays as
        :meth:`rcs_amd.sim.SimRobot.opspace_query`.  Reads the state, writes none of it."""
        n, nl = self.n_envs, int(self.sim.model.nq)
        want = self.robot._opspace_want(want, xacc)
        rows = lambda a, w: None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n, w)))  # noqa: E731
        x, f = rows(xacc, 6), rows(qfrc_null, nl)
        arrays, out = self.robot._opspace_buffers(want, n, nl)
        opts, _keep = self.robot._opspace_opts(tcp_offset, task_mask, damping)
        _lib.check(self._L.rcsh_env_opspace(self.sim._h, _lib.ptr(x), _lib.ptr(f), C.byref(opts), C.byref(out)))
        return arrays

    def _guard_info(self, i: dict[str, Any]):
        """info["guard_*"] of a guarded step; returns ``blocked`` where it truncates (else None)."""
        if not self.guard_enabled:
            return None
        blocked, result, tc = self.guard_last()
        i["guard_blocked"] = blocked
        i["guard_result"] = result
        i["guard_t_contact"] = tc
        return blocked if self.guard_truncates else None

    # ---- autoreset (csrc/episode_team.h: finished episodes are reset inside the fused step)
    def _autoreset_desc(self, enabled, max_episode_steps, seed, env_offset) -> _lib.AutoresetDesc:
        d = _lib.AutoresetDesc()
        d.enabled = int(bool(enabled))
        d.max_episode_steps = 0 if max_episode_steps is None else int(max_episode_steps)
        d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        d.env_offset = int(env_offset)
        return d

    def _apply_autoreset(self, d: _lib.AutoresetDesc) -> None:
        _lib.check(self._L.rcsh_env_configure_autoreset(self.sim._h, C.byref(d)))
        self.autoreset_enabled = bool(d.enabled)
        self.autoreset_desc = d

    def configure_autoreset(self, enabled: bool = True, max_episode_steps: int | None = None, seed: int = 0, env_offset: int = 0) -> None:
        """Reset finished episodes on the device inside ``step`` / ``step_dev`` (see the class docstring).

        ``max_episode_steps``: Gymnasium's ``TimeLimit`` (an episode is truncated by the step that brings its length to the limit;
        ``None``: no limit).  ``seed`` / ``env_offset`` only matter where the new episode draws something (:class:`VecPickCubeEnv`):
        ``env_offset`` is this env's first environment in a batch sharded over several Sims.  Every call zeroes the episode counters;
        ``enabled=False`` makes the steps run as if autoreset had never been configured.  An explicit :meth:`reset` also begins the
        episodes of the environments it resets again.  Not with rate-driven cameras (RuntimeError)."""
        self._apply_autoreset(self._autoreset_desc(enabled, max_episode_steps, seed, env_offset))

    def autoreset_draw(self, env: int, episode: int) -> np.ndarray:
        """The cube pose the device draws for environment ``env`` at its ``episode``-th autoreset (computed on the host)."""
        if self.autoreset_desc is None:
            raise RuntimeError("call configure_autoreset first")
        q = np.zeros(7)
        _lib.check(self._L.rcsh_autoreset_draw(C.byref(self.autoreset_desc), int(env), int(episode), q.ctypes.data_as(C.POINTER(C.c_double))))
        return q

    _AUTORESET_FIELDS = (("done", np.uint8, ()), ("terminated", np.uint8, ()), ("truncated", np.uint8, ()), ("time_limit", np.uint8, ()),
                         ("final_obs", np.float64, ("obs",)), ("final_info", np.uint8, (8,)), ("final_gripper_width", np.float64, ()),
                         ("final_task", np.float64, (9,)), ("episode_return", np.float64, ()), ("episode_length", np.int32, ()),
                         ("episodes", np.int64, ()), ("elapsed", np.int32, ()), ("running_return", np.float64, ()),
                         ("reset_info", np.uint8, (8,)), ("reset_box_qpos", np.float64, (7,)))

    def autoreset_last(self, fields=None) -> dict[str, np.ndarray]:
        """The record of the most recent step under autoreset as host arrays (``fields``: a subset of its names; default all).
        ``final_*`` and ``reset_*`` rows are meaningful where ``done``."""
        out: dict[str, np.ndarray] = {}
        args = []
        for name, dtype, shape in self._AUTORESET_FIELDS:
            if fields is not None and name not in fields:
                args.append(None)
                continue
            out[name] = np.zeros((self.n_envs, *[self.obs_width if k == "obs" else k for k in shape]), dtype=dtype)
            args.append(_lib.ptr(out[name]))
        _lib.check(self._L.rcsh_env_autoreset_last(self.sim._h, *args))
        return out

    def autoreset_last_dev(self) -> _lib.AutoresetRecord:
        """Device pointers of the record (``.done``, ``.final_obs``, ``.episode_return``, ...: integers), for ``step_dev`` loops: valid
        for the Sim's life, rewritten by every step under autoreset."""
        r = _lib.AutoresetRecord()
        _lib.check(self._L.rcsh_env_autoreset_record_dev(self.sim._h, C.byref(r)))
        return r

    def _obs_dict(self, obs) -> dict[str, Any]:
        d = self.dof
        o: dict[str, Any] = {"tquat": obs[:, 0:7].copy(), "joints": obs[:, 7 : 7 + d].copy(), "xyzrpy": obs[:, 7 + d : 13 + d].copy()}
        if self.gripper is not None:
            o["gripper"] = obs[:, 13 + d].copy()
        return o

    def _autoreset_info(self, i: dict[str, Any], extra=()) -> None:
        """info of a step under autoreset.  The verdict bytes, returns and lengths came with the step's own outputs; the terminal
        observations are fetched only when somebody is done."""
        if not self.autoreset_enabled:
            return
        rec = self.autoreset_last(("done", "time_limit", "episode_return", "episode_length"))
        done = rec["done"].astype(bool)
        i["autoreset"] = done
        i["TimeLimit.truncated"] = rec["time_limit"].astype(bool)
        i["episode"] = {"r": np.where(done, rec["episode_return"], 0.0), "l": np.where(done, rec["episode_length"], 0).astype(np.int32)}
        final = np.zeros((self.n_envs, self.obs_width))
        more = self.autoreset_last(("final_obs", *extra)) if done.any() else {}
        if done.any():
            final[done] = more["final_obs"][done]
        i["final_obs"] = self._obs_dict(final)
        for name in extra:
            a = np.zeros((self.n_envs, 7))
            if done.any():
                a[done] = more[name][done]
            i[name] = a

    def _after_step(self, info) -> None:
        if self.on_unresolved_contact == "resolve" and not self.sim.resolve_robot_contacts and info[:, 7].any():
            self.sim.enable_contact_resolution()

    # ---- host-array interface (Gymnasium-shaped)
    def _unpack(self, obs, info, gw) -> tuple[dict[str, Any], dict[str, Any]]:
        d = self.dof
        o: dict[str, Any] = {"tquat": obs[:, 0:7].copy(), "joints": obs[:, 7 : 7 + d].copy(), "xyzrpy": obs[:, 7 + d : 13 + d].copy()}
        i: dict[str, Any] = {}
        if self.gripper is not None:
            o["gripper"] = obs[:, 13 + d].copy()
        if self.camera_set is not None:
            # CameraSetWrapper.observation (base.py:633-674), include_depth=True: "rgb" always, "depth" next to it
            frameset = self.camera_set.get_latest_frames()
            if frameset is None:
                o["frames"] = {}
                i["camera_available"] = False
            else:
                o["frames"] = {name: {"rgb": {"data": f.camera.color.data, "intrinsics": f.camera.color.intrinsics,
                                              "extrinsics": f.camera.color.extrinsics},
                                      "depth": {"data": f.camera.depth.data, "intrinsics": f.camera.depth.intrinsics,
                                                "extrinsics": f.camera.depth.extrinsics}} for name, f in frameset.frames.items()}
                i["camera_available"] = True
                if frameset.avg_timestamp is not None:
                    i["frame_timestamp"] = frameset.avg_timestamp
        return o, i

    def reset(self, seed: int | None = None, options: dict | None = None, mask=None):
        n = self.n_envs
        obs = np.zeros((n, self.obs_width))
        info = np.zeros((n, 8), dtype=np.uint8)
        gw = np.zeros(n)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        if self.camera_set is not None:
            self.camera_set.clear_buffer()  # CameraSetWrapper.reset
        _lib.check(self._L.rcsh_env_reset(self.sim._h, _lib.ptr(m), _lib.ptr(obs), _lib.ptr(info), _lib.ptr(gw)))
        self.sim._collect_frames()
        o, i = self._unpack(obs, info, gw)
        if self.gripper is not None:  # GripperWrapperSim.observation runs on reset too (envs/sim.py:125-131)
            i["collision"] = info[:, 5].astype(bool)
            i["gripper_width"] = gw
            i["is_grasped"] = info[:, 3].astype(bool)
        return o, i

    def step(self, action: dict[str, Any]):
        n = self.n_envs
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action[self.action_key], dtype=np.float64), (n, self.action_width)))
        g = None
        if self.gripper is not None:
            assert "gripper" in action, "Gripper action not found."
            g = np.ascontiguousarray(np.broadcast_to(np.asarray(action["gripper"], dtype=np.float32), (n,)))
        obs = np.zeros((n, self.obs_width))
        info = np.zeros((n, 8), dtype=np.uint8)
        gw = np.zeros(n)
        sub = np.zeros(n, dtype=np.int32)
        _lib.check(self._L.rcsh_env_step(self.sim._h, _lib.ptr(a), _lib.ptr(g), _lib.ptr(obs), _lib.ptr(info), _lib.ptr(gw), _lib.ptr(sub)))
        self.sim._collect_frames()
        o, i = self._unpack(obs, info, gw)
        i["collision"] = info[:, 0].astype(bool)
        i["ik_success"] = info[:, 1].astype(bool)
        i["is_sim_converged"] = info[:, 2].astype(bool)
        if self.gripper is not None:
            i["gripper_width"] = gw
            i["is_grasped"] = info[:, 3].astype(bool)
        i["substeps"] = sub
        # (no reference counterpart) a contact phase of the environment ran out of contact / link slots since its last reset:
        # its trajectory is no longer what MuJoCo would compute (csrc/contact_team.h: kMaxCon, kMaxActive)
        i["contact_overflow"] = info[:, 6].astype(bool)
        # (no reference counterpart) the environment's geoms were found in a contact this configuration does not resolve, since its
        # last reset (csrc/check_team.h): MuJoCo would have resolved it, so from that step on the trajectory is not MuJoCo's
        i["contact_unresolved"] = info[:, 7].astype(bool)
        if self.control_mode in TORQUE_MODES:
            # (no reference counterpart) the law met a singular task-space matrix, or a non-finite torque, in a substep since the
            # environment's last reset: that substep kept the torque of the one before (SimRobot.torque_status)
            i["torque_singular"] = self.robot.torque_status()
        self._after_step(info)
        truncated = info[:, 4].astype(bool)  # (a truncating guard has set it for the environments it blocked)
        terminated = np.zeros(n, dtype=bool)
        stop = self._guard_info(i)
        if stop is not None:
            terminated |= stop
            truncated |= stop
        self._autoreset_info(i)  # (info row byte 4 -- `truncated` -- carries the time limit already)
        return o, np.zeros(n), terminated, truncated, i

    # ---- device-pointer interface for resident rollouts (pointers are integers / c_void_p)
    def reset_dev(self, obs_ptr, info_ptr=None, gw_ptr=None, mask_ptr=None) -> None:
        _lib.check(self._L.rcsh_env_reset_dev(self.sim._h, C.c_void_p(mask_ptr), C.c_void_p(obs_ptr), C.c_void_p(info_ptr), C.c_void_p(gw_ptr)))

    def step_dev(self, action_ptr, gripper_ptr, obs_ptr, info_ptr=None, gw_ptr=None, substeps_ptr=None) -> None:
        """One resident step.  A configured guard applies here too: its record is at :meth:`guard_last_dev` / :meth:`guard_last`.
        So does autoreset: the rows of done environments in ``obs`` / ``gw`` are the new episode's, the rest of the story is at
        :meth:`autoreset_last_dev` / :meth:`autoreset_last`."""
        _lib.check(self._L.rcsh_env_step_dev(self.sim._h, C.c_void_p(action_ptr), C.c_void_p(gripper_ptr), C.c_void_p(obs_ptr),
                                             C.c_void_p(info_ptr), C.c_void_p(gw_ptr), C.c_void_p(substeps_ptr)))

    def close(self) -> None:
        self.sim.close()


class VecPickCubeEnv(VecSimEnv):
    """``SimTaskEnvCreator()(...)`` of the reference for N environments: the :class:`VecSimEnv` of the pick-up scene
    with ``RandomCubePos`` under the simulation wrapper and ``PickCubeSuccessWrapper`` on top (reference
    python/rcs/envs/sim.py:358-431, creators.py:131-187).

    ``reset`` places each environment's cube (one draw of x, y and -- with ``include_rotation`` -- the quaternion's w per
    environment from numpy's global generator, in the reference's order; or the poses given as
    ``options={"box_qpos": [N, 7]}``); ``step`` returns the wrapper's shaped reward, ``terminated = success`` and
    ``info["success"]``; the cube pose of the step is ``info["box_qpos"]``.
    """

    EE_HOME = np.array([0.34169773, 0.00047028, 0.4309004])  # PickCubeSuccessWrapper.EE_HOME
    SUCCESS_HEIGHT = 0.15 + 0.852
    ISO_CUBE = np.array([0.498, 0.0, 0.226])  # RandomCubePos.reset, robot coordinates

    def __init__(self, *args, include_rotation: bool = True, random_pos_args: dict | None = None, **kwargs):
        super().__init__(*args, **kwargs)
        assert self.gripper is not None, "PickCubeSuccessWrapper reads the gripper observation"
        self.include_rotation = include_rotation
        # RandomObjectPos instead of RandomCubePos (creators.py:160-167): joint_name, init_object_pose, include_position, include_rotation
        self.random_pos_args = random_pos_args
        if random_pos_args is not None:
            self.sim._free_joint(random_pos_args["joint_name"])  # KeyError for an unknown joint, like mjData.joint()
            self.init_object_pose = random_pos_args["init_object_pose"]
        t = _lib.PickTaskDesc()
        t.ee_home[:] = [float(x) for x in self.EE_HOME]
        t.success_height = float(self.SUCCESS_HEIGHT)
        _lib.check(self._L.rcsh_env_configure_pick_task(self.sim._h, C.byref(t)))
        self.task_width = 9

    def configure_autoreset(self, enabled: bool = True, max_episode_steps: int | None = None, seed: int = 0, env_offset: int = 0) -> None:
        """:meth:`VecSimEnv.configure_autoreset` of the task env: ``success`` terminates, the reward is summed into ``info["episode"]
        ["r"]``, and a done environment's cube is placed on the device by the rule :meth:`draw_box_qpos` follows -- RandomCubePos, or
        RandomObjectPos with ``random_pos_args`` -- from a counter-based generator keyed by ``seed``: environment ``env_offset + e``'s
        k-th autoreset draws the same pose whatever the batch size and whoever else finishes (:meth:`autoreset_draw`;
        ``info["reset_box_qpos"]``).  An explicit :meth:`reset` keeps drawing from numpy's global generator."""
        d = self._autoreset_desc(enabled, max_episode_steps, seed, env_offset)
        d.draw_box = 1
        if self.random_pos_args is not None:
            t, q = self.init_object_pose.translation(), self.init_object_pose.rotation_q()  # xyzw
            d.include_position = int(bool(self.random_pos_args.get("include_position", True)))
            d.include_rotation = int(bool(self.random_pos_args.get("include_rotation", False)))
            d.box_pose[:] = [float(t[0]), float(t[1]), float(t[2]), float(q[3]), float(q[0]), float(q[1]), float(q[2])]
            d.rotation_minus = float(q[3])
        else:
            iso = self.robot.to_pose_in_world_coordinates(common.Pose(translation=self.ISO_CUBE, rpy_vector=np.zeros(3))).translation()
            d.include_position = 1
            d.include_rotation = int(bool(self.include_rotation))
            d.box_pose[:] = [float(iso[0]), float(iso[1]), 0.0288 / 2, 0.0, 0.0, 0.0, 1.0]
            d.rotation_minus = 1.0
        self._apply_autoreset(d)

    def draw_box_qpos(self) -> np.ndarray:
        """RandomCubePos.reset's placement (sim.py:371-383) -- or RandomObjectPos.reset's (sim.py:331-354) -- for every
        environment, drawing from numpy's global generator in the reference's order."""
        if self.random_pos_args is not None:
            return random_object_qpos(self.init_object_pose, self.n_envs, self.random_pos_args.get("include_position", True),
                                      self.random_pos_args.get("include_rotation", False))
        iso = self.robot.to_pose_in_world_coordinates(common.Pose(translation=self.ISO_CUBE, rpy_vector=np.zeros(3))).translation()
        q = np.zeros((self.n_envs, 7))
        for e in range(self.n_envs):
            x = iso[0] + np.random.random() * 0.2 - 0.1
            y = iso[1] + np.random.random() * 0.2 - 0.1
            w = 2 * np.random.random() - 1 if self.include_rotation else 0.0
            q[e] = [x, y, 0.0288 / 2, w, 0, 0, 1]
        return q

    def reset(self, seed: int | None = None, options: dict | None = None, mask=None):
        n = self.n_envs
        if options is not None and "RandomObjectPos.init_object_pose" in options and self.random_pos_args is not None:
            assert isinstance(options["RandomObjectPos.init_object_pose"], common.Pose), "RandomObjectPos.init_object_pose must be a rcs.common.Pose"
            self.init_object_pose = options["RandomObjectPos.init_object_pose"]  # sticks for later resets, as in the reference
        box = None if options is None else options.get("box_qpos")
        box = self.draw_box_qpos() if box is None else np.ascontiguousarray(np.broadcast_to(np.asarray(box, dtype=np.float64), (n, 7)))
        obs = np.zeros((n, self.obs_width))
        info = np.zeros((n, 8), dtype=np.uint8)
        gw = np.zeros(n)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        if self.camera_set is not None:
            self.camera_set.clear_buffer()
        _lib.check(self._L.rcsh_env_reset_task(self.sim._h, _lib.ptr(m), _lib.ptr(box), _lib.ptr(obs), _lib.ptr(info), _lib.ptr(gw)))
        self.sim._collect_frames()
        o, i = self._unpack(obs, info, gw)
        i["collision"] = info[:, 5].astype(bool)
        i["gripper_width"] = gw
        i["is_grasped"] = info[:, 3].astype(bool)
        return o, i

    def step(self, action: dict[str, Any]):
        n = self.n_envs
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(action[self.action_key], dtype=np.float64), (n, self.action_width)))
        assert "gripper" in action, "Gripper action not found."
        g = np.ascontiguousarray(np.broadcast_to(np.asarray(action["gripper"], dtype=np.float32), (n,)))
        obs = np.zeros((n, self.obs_width))
        info = np.zeros((n, 8), dtype=np.uint8)
        gw = np.zeros(n)
        sub = np.zeros(n, dtype=np.int32)
        task = np.zeros((n, self.task_width))
        _lib.check(self._L.rcsh_env_step_task(self.sim._h, _lib.ptr(a), _lib.ptr(g), _lib.ptr(obs), _lib.ptr(info), _lib.ptr(gw),
                                              _lib.ptr(sub), _lib.ptr(task)))
        self.sim._collect_frames()
        o, i = self._unpack(obs, info, gw)
        i["collision"] = info[:, 0].astype(bool)
        i["ik_success"] = info[:, 1].astype(bool)
        i["is_sim_converged"] = info[:, 2].astype(bool)
        i["gripper_width"] = gw
        i["is_grasped"] = info[:, 3].astype(bool)
        i["substeps"] = sub
        i["contact_overflow"] = info[:, 6].astype(bool)  # (see VecSimEnv.step)
        i["contact_unresolved"] = info[:, 7].astype(bool)
        i["box_qpos"] = task[:, :7].copy()
        success = task[:, 8] != 0
        i["success"] = success
        terminated, truncated = success.copy(), info[:, 4].astype(bool)
        stop = self._guard_info(i)  # (the task keeps its own reward for a blocked environment)
        if stop is not None:
            terminated |= stop
            truncated |= stop
        self._autoreset_info(i, extra=("reset_box_qpos",))
        return o, task[:, 7].copy(), terminated, truncated, i

    def step_task_dev(self, action_ptr, gripper_ptr, obs_ptr, info_ptr=None, gw_ptr=None, substeps_ptr=None, task_ptr=None) -> None:
        _lib.check(self._L.rcsh_env_step_task_dev(self.sim._h, C.c_void_p(action_ptr), C.c_void_p(gripper_ptr), C.c_void_p(obs_ptr),
                                                  C.c_void_p(info_ptr), C.c_void_p(gw_ptr), C.c_void_p(substeps_ptr), C.c_void_p(task_ptr)))

    def reset_task_dev(self, box_qpos_ptr, obs_ptr, info_ptr=None, gw_ptr=None, mask_ptr=None) -> None:
        _lib.check(self._L.rcsh_env_reset_task_dev(self.sim._h, C.c_void_p(mask_ptr), C.c_void_p(box_qpos_ptr), C.c_void_p(obs_ptr),
                                                   C.c_void_p(info_ptr), C.c_void_p(gw_ptr)))


def random_object_qpos(init_object_pose: common.Pose, n_envs: int, include_position: bool = True, include_rotation: bool = False) -> np.ndarray:
    """RandomObjectPos.reset (reference python/rcs/envs/sim.py:331-354) for n_envs environments: x, y +- 0.1 m around the
    initial pose, z and orientation kept -- with include_rotation the quaternion's w becomes ``2 u - w`` (unnormalised;
    mj_kinematics normalises it).  Draw order per environment: x, y, then w."""
    t, q = init_object_pose.translation(), init_object_pose.rotation_q()  # xyzw
    out = np.zeros((n_envs, 7))
    for e in range(n_envs):
        x = t[0] + np.random.random() * 0.2 - 0.1 if include_position else t[0]
        y = t[1] + np.random.random() * 0.2 - 0.1 if include_position else t[1]
        w = 2 * np.random.random() - q[3] if include_rotation else q[3]
        out[e] = [x, y, t[2], w, q[0], q[1], q[2]]
    return out


class SimEnvCreator:
    """Reference python/rcs/envs/creators.py:43-128 for N environments.  ``collision_guard=True`` returns the env with the batched
    collision guard configured at its defaults (:meth:`VecSimEnv.configure_guard`: a kinematic, certifying guard decided on the
    device, in place of the reference's shadow simulation); it needs a joint-space control mode.

    The torque and impedance modes (``ControlMode.TORQUE``, ``JOINT_IMPEDANCE``, ``CARTESIAN_IMPEDANCE_TRPY`` / ``_TQuat``; no reference
    counterpart) need a torque-actuated scene (``robot_cfg`` from :func:`rcs_amd.envs.factory.torque_actuated_cfg`) and, for the
    impedance modes, ``torque_law=dict(...)``: the keyword arguments of :meth:`rcs_amd.sim.SimRobot.configure_torque_law`, passed on
    before the env is configured.  For the Cartesian modes the law's ``tcp_offset`` defaults to the robot configuration's TCP: the law
    composes the site with the INVERSE of its offset (reference quirk Q7), so the default is ``robot_cfg.tcp_offset.inverse()``.  The
    ``Sim`` is created with ``resolve_robot_contacts=False`` (the fused torque launch resolves no contacts; ``True`` is an error) and
    the env reports unresolved contacts instead of switching modes (``on_unresolved_contact = "flag"``)."""

    def __call__(self, control_mode: ControlMode, robot_cfg: sim.SimRobotConfig, collision_guard: bool = False,
                 gripper_cfg: sim.SimGripperConfig | None = None, sim_cfg: sim.SimConfig | None = None,
                 hand_cfg=None, cameras=None, max_relative_movement: float | tuple[float, float] | None = None,
                 relative_to: RelativeTo = RelativeTo.LAST_STEP, sim_wrapper=None, n_envs: int = 1, device: int = 0,
                 resolve_robot_contacts=None, torque_law: dict | None = None) -> VecSimEnv:
        if hand_cfg is not None or sim_wrapper is not None:
            raise NotImplementedError("hands and sim_wrapper are outside this backend's hot path")
        torque_mode = control_mode in TORQUE_MODES
        if torque_mode:
            if collision_guard:
                raise NotImplementedError("collision_guard guards position commands only: it is not built for the torque and impedance modes")
            if resolve_robot_contacts:
                raise ValueError("resolve_robot_contacts=True with a torque / impedance control mode: the fused torque launch "
                                 "(csrc/env_torque_team.h) resolves no contacts; unresolved contacts are reported in info['contact_unresolved']")
            resolve_robot_contacts = False
        elif torque_law is not None:
            raise ValueError("torque_law configures the torque and impedance control modes only")
        if collision_guard and control_mode != ControlMode.JOINTS:
            raise NotImplementedError("collision_guard guards joint-space actions only (ControlMode.JOINTS): the Cartesian modes' IK runs in a "
                                      "launch of its own, and a guard between it and the stepping launch is not built yet")
        simulation = sim.Sim(robot_cfg.mjcf_scene_path, sim_cfg, n_envs=n_envs, device=device, resolve_robot_contacts=resolve_robot_contacts)
        robot = sim.SimRobot(simulation, None, robot_cfg)
        gripper = sim.SimGripper(simulation, gripper_cfg) if gripper_cfg is not None else None
        camera_set = None
        if cameras is not None:  # creators.py:92-96
            from ..camera import SimCameraSet

            camera_set = SimCameraSet(simulation, cameras, physical_units=True, render_on_demand=True)
        if torque_mode and torque_law is not None:
            law = dict(torque_law)
            if control_mode in (ControlMode.CARTESIAN_IMPEDANCE_TRPY, ControlMode.CARTESIAN_IMPEDANCE_TQuat) and law.get("tcp_offset") is None:
                law["tcp_offset"] = robot_cfg.tcp_offset.inverse()  # (quirk Q7: the law's TCP is site * offset^-1, the env layer's site * tcp_offset)
            robot.configure_torque_law(**law)
        venv = VecSimEnv(simulation, robot, gripper, control_mode, max_relative_movement, relative_to, camera_set=camera_set)
        if torque_mode:
            venv.on_unresolved_contact = "flag"
        if collision_guard:
            venv.configure_guard()
        return venv


class SimTaskEnvCreator:
    """Reference python/rcs/envs/creators.py:131-187: the pick-up task on top of ``SimEnvCreator`` (RandomCubePos +
    PickCubeSuccessWrapper).  ``render_mode`` is accepted for signature compatibility; this backend has no viewer."""

    def __call__(self, robot_cfg: sim.SimRobotConfig, render_mode: str = "rgb_array", control_mode: ControlMode = ControlMode.CARTESIAN_TRPY,
                 delta_actions: bool = True, cameras=None, hand_cfg=None, gripper_cfg: sim.SimGripperConfig | None = None,
                 sim_cfg: sim.SimConfig | None = None, random_pos_args: dict | None = None, n_envs: int = 1, device: int = 0) -> VecPickCubeEnv:
        from .utils import default_sim_gripper_cfg

        if hand_cfg is not None:
            raise NotImplementedError("hands are outside this backend's hot path")
        if random_pos_args is not None:
            missing = [k for k in ("joint_name", "init_object_pose") if k not in random_pos_args]
            if missing:
                raise TypeError(f"RandomObjectPos.__init__() missing required arguments: {missing}")  # partial(RandomObjectPos, **args) would fail here
        if gripper_cfg is None:
            gripper_cfg = default_sim_gripper_cfg()
        simulation = sim.Sim(robot_cfg.mjcf_scene_path, sim_cfg, n_envs=n_envs, device=device)
        robot = sim.SimRobot(simulation, None, robot_cfg)
        gripper = sim.SimGripper(simulation, gripper_cfg)
        camera_set = None
        if cameras:
            from ..camera import SimCameraSet

            camera_set = SimCameraSet(simulation, cameras, physical_units=True, render_on_demand=True)
        return VecPickCubeEnv(simulation, robot, gripper, control_mode,
                              (0.2, float(np.deg2rad(45))) if delta_actions else None, RelativeTo.LAST_STEP, camera_set=camera_set,
                              random_pos_args=random_pos_args)


class FR3SimplePickUpSimEnvCreator:
    """Reference creators.py:190-224 (gym id ``rcs/FR3SimplePickUpSim-v0``): the pick-up scene at 30 Hz async control
    with the reference's TCP offset."""

    def __call__(self, render_mode: str = "rgb_array", control_mode: ControlMode = ControlMode.CARTESIAN_TRPY,
                 resolution: tuple[int, int] | None = None, frame_rate: int = 0, delta_actions: bool = True,
                 cam_list: list[str] | None = None, n_envs: int = 1, device: int = 0) -> VecPickCubeEnv:
        from .utils import default_sim_robot_cfg

        from ..camera import CameraType, SimCameraConfig

        if resolution is None:
            resolution = (256, 256)
        cameras = {cam: SimCameraConfig(identifier=cam, type=CameraType.fixed, resolution_height=resolution[1], resolution_width=resolution[0],
                                        frame_rate=frame_rate) for cam in (cam_list or [])}
        robot_cfg = default_sim_robot_cfg(scene="fr3_simple_pick_up")
        robot_cfg.tcp_offset = common.Pose(translation=np.array([0.0, 0.0, 0.1034]),
                                           rotation=np.array([[0.707, 0.707, 0], [-0.707, 0.707, 0], [0, 0, 1]]))
        sim_cfg = sim.SimConfig()
        sim_cfg.realtime = False
        sim_cfg.async_control = True
        sim_cfg.frequency = 30
        return SimTaskEnvCreator()(robot_cfg, render_mode, control_mode, delta_actions, cameras, sim_cfg=sim_cfg, n_envs=n_envs, device=device)
