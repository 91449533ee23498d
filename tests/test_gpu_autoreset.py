"""Autoreset inside the fused env step (VecSimEnv.configure_autoreset, csrc/episode_team.h) against the same sequence driven by hand.

The yardstick throughout is a second env built the same way on which autoreset is never configured: step_dev / step_task_dev, the
mask computed on the host by the rule (tests/test_autoreset_cpu.py: episode_rule), the cube poses from the numpy restatement of the
placement (draw_pose), rcsh_dev_upload, reset_dev / reset_task_dev -- every step, with an all-zero mask when nobody is done, as the
autoreset enqueues its reset launch every step.  Both sides enqueue the same launches on the same inputs: equality is bit for bit
(compared as bytes, so that a NaN would equal itself)."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_autoreset_cpu import draw_pose, episode_rule  # noqa: E402

pytestmark = pytest.mark.gpu

RECORD_FIELDS = ("done", "terminated", "truncated", "time_limit", "final_obs", "final_info", "final_gripper_width", "final_task",
                 "episode_return", "episode_length", "episodes", "elapsed", "running_return", "reset_info", "reset_box_qpos")


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class DevIO:
    """Device buffers of one env's resident loop, and the loop's calls."""

    def __init__(self, venv):
        from rcs_amd import _lib

        self.v, self.L, self.h, self._lib = venv, venv._L, venv.sim._h, _lib
        n, ow = venv.n_envs, venv.obs_width
        self.task = hasattr(venv, "step_task_dev")
        self.shapes = {"act": ((n, venv.action_width), np.float64), "grip": ((n,), np.float32), "obs": ((n, ow), np.float64),
                       "info": ((n, 8), np.uint8), "gw": ((n,), np.float64), "sub": ((n,), np.int32), "task": ((n, 9), np.float64),
                       "mask": ((n,), np.uint8), "box": ((n, 7), np.float64), "rinfo": ((n, 8), np.uint8)}
        self.p = {}
        for k, (shape, dtype) in self.shapes.items():
            p = C.c_void_p()
            _lib.check(self.L.rcsh_dev_alloc(self.h, max(int(np.prod(shape)) * np.dtype(dtype).itemsize, 8), C.byref(p)))
            self.p[k] = p
            self.up(k, np.zeros(shape, dtype=dtype))

    def up(self, k, a):
        shape, dtype = self.shapes[k]
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=dtype), shape))
        self._lib.check(self.L.rcsh_dev_upload(self.h, self.p[k], C.c_void_p(a.ctypes.data), a.nbytes))

    def down(self, k):
        shape, dtype = self.shapes[k]
        a = np.zeros(shape, dtype=dtype)
        self._lib.check(self.L.rcsh_dev_download(self.h, C.c_void_p(a.ctypes.data), self.p[k], a.nbytes))
        return a

    def step(self, act, grip):
        self.up("act", act)
        self.up("grip", grip)
        p = {k: v.value for k, v in self.p.items()}
        if self.task:
            self.v.step_task_dev(p["act"], p["grip"], p["obs"], p["info"], p["gw"], p["sub"], p["task"])
        else:
            self.v.step_dev(p["act"], p["grip"], p["obs"], p["info"], p["gw"], p["sub"])

    def reset(self, mask, box=None):
        """The manual loop's masked reset: observation and gripper width into the step's buffers, the info rows elsewhere."""
        self.up("mask", mask)
        p = {k: v.value for k, v in self.p.items()}
        if box is not None:
            self.up("box", box)
            self.v.reset_task_dev(p["box"], p["obs"], p["rinfo"], p["gw"], p["mask"])
        else:
            self.v.reset_dev(p["obs"], p["rinfo"], p["gw"], p["mask"])

    def outputs(self):
        keys = ("obs", "info", "gw", "sub") + (("task",) if self.task else ())
        return {k: self.down(k) for k in keys}

    def free(self):
        for p in self.p.values():
            self._lib.check(self.L.rcsh_dev_free(self.h, p))


def down_ptr(venv, ptr, shape, dtype):
    """A host copy of device memory of the env's Sim."""
    from rcs_amd import _lib

    a = np.zeros(shape, dtype=dtype)
    _lib.check(venv._L.rcsh_dev_download(venv.sim._h, C.c_void_p(a.ctypes.data), C.c_void_p(ptr), a.nbytes))
    return a


class Manual:
    """The hand-driven sequence: an env without autoreset, the host rule, the numpy placement."""

    def __init__(self, venv, max_episode_steps, draw=None):
        self.io = DevIO(venv)
        self.v, self.n, self.max = venv, venv.n_envs, int(max_episode_steps or 0)
        self.draw = draw  # None, or dict(seed, box_pose, rotation_minus, include_position, include_rotation, env_offset)
        self.elapsed = np.zeros(self.n, dtype=np.int64)
        self.ret = np.zeros(self.n)
        self.episodes = np.zeros(self.n, dtype=np.int64)

    def explicit_reset(self, mask):
        m = np.asarray(mask, dtype=bool)
        self.elapsed[m] = 0
        self.ret[m] = 0.0

    def step(self, act, grip, between=None):
        """One step and its reset; returns what the autoreset env must show.  `between(out)` runs after the stepping call, before the reset."""
        io = self.io
        io.step(act, grip)
        out = io.outputs()
        if between is not None:
            between(out)
        task = out.get("task")
        success = task[:, 8] != 0 if task is not None else np.zeros(self.n, dtype=bool)
        reward = task[:, 7] if task is not None else np.zeros(self.n)
        done, term, trunc, tl, new_elapsed = episode_rule(out["info"][:, 4], success, self.elapsed, self.max)
        self.ret = self.ret + reward  # (fp64, in step order)
        exp = dict(out)
        exp["info"] = out["info"].copy()
        exp["info"][tl, 4] = 1
        exp.update(done=done, terminated=term, truncated=trunc, time_limit=tl, final_obs=out["obs"].copy(), final_info=exp["info"].copy(),
                   final_gw=out["gw"].copy(), final_task=None if task is None else task.copy(),
                   episode_return=self.ret.copy(), episode_length=(self.elapsed + 1).astype(np.int32))
        box = None
        if self.draw is not None:
            box = np.zeros((self.n, 7))
            for e in np.flatnonzero(done):
                box[e] = draw_pose(self.draw["seed"], int(e), int(self.episodes[e]), self.draw["box_pose"], self.draw["rotation_minus"],
                                   self.draw["include_position"], self.draw["include_rotation"], self.draw["env_offset"])
            exp["reset_box_qpos"] = box
        io.reset(done.astype(np.uint8), box)
        exp["obs"], exp["gw"] = io.down("obs"), io.down("gw")
        exp["reset_info"] = io.down("rinfo")
        self.episodes[done] += 1
        self.elapsed = new_elapsed
        self.ret[done] = 0.0
        exp["elapsed"], exp["running_return"], exp["episodes"] = self.elapsed.astype(np.int32), self.ret.copy(), self.episodes.copy()
        return exp


def check_step(tag, auto_io, auto_env, manual_env, exp, state=True):
    """The autoreset env's outputs, record and state against the manual sequence's."""
    got = auto_io.outputs()
    for k in got:
        assert same(got[k], exp[k]), (tag, k, np.flatnonzero((got[k] != exp[k]).reshape(len(got[k]), -1).any(axis=1)))
    rec = auto_env.autoreset_last()
    assert sorted(rec) == sorted(RECORD_FIELDS)
    done = exp["done"]
    for k in ("done", "terminated", "truncated", "time_limit"):
        assert same(rec[k].astype(bool), exp[k]), (tag, k, rec[k], exp[k])
    for k in ("elapsed", "running_return", "episodes"):
        assert same(rec[k], exp[k]), (tag, k, rec[k], exp[k])
    assert same(rec["final_obs"][done], exp["final_obs"][done]), (tag, "final_obs")
    assert same(rec["final_info"][done], exp["final_info"][done]), (tag, "final_info")
    assert same(rec["final_gripper_width"][done], exp["final_gw"][done]), (tag, "final_gw")
    assert same(rec["episode_return"][done], exp["episode_return"][done]), (tag, "episode_return", rec["episode_return"], exp["episode_return"])
    assert same(rec["episode_length"][done], exp["episode_length"][done]), (tag, "episode_length", rec["episode_length"], exp["episode_length"])
    assert same(rec["reset_info"][done], exp["reset_info"][done]), (tag, "reset_info")
    if exp.get("final_task") is not None:
        assert same(rec["final_task"][done], exp["final_task"][done]), (tag, "final_task")
    if "reset_box_qpos" in exp:
        assert same(rec["reset_box_qpos"][done], exp["reset_box_qpos"][done]), (tag, "reset_box_qpos")
    if state:
        assert same(auto_env.sim.get_state(), manual_env.sim.get_state()), (tag, "state")
    return got, rec


def _pair(n, **kw):
    from parity_util import make_vec_env

    a, m = make_vec_env(n, True, **kw), make_vec_env(n, True, **kw)
    return a, m


# ---- 1. time limit, staggered

def _time_limit_scenario(drive):
    """fr3_empty_world, JOINTS, async, 8 environments, max_episode_steps 3, 10 steps; environments 0..3 reset by hand after the
    first step, so the halves end on different steps.  `drive(t, auto, manual, exp)` does the per-step checks."""
    from parity_util import synthetic_actions

    n, steps = 8, 10
    joints, grip = synthetic_actions(n, steps, 0)
    auto, man = _pair(n)
    for v in (auto, man):
        v.reset()
    auto.configure_autoreset(max_episode_steps=3)
    manual = Manual(man, 3)
    half = np.arange(n) < 4
    ended = []
    for t in range(steps):
        exp = manual.step(joints[t], grip[t])
        drive(t, auto, man, exp, joints[t], grip[t])
        ended.append(exp["done"].copy())
        if t == 0:
            for v in (auto, man):
                v.reset(mask=half)
            manual.explicit_reset(half)
    ended = np.array(ended)
    # the hand-reset half ends on steps 3, 6, 9 (counted from 0), the other half on 2, 5, 8
    assert [np.flatnonzero(ended[:, e]).tolist() for e in (0, 7)] == [[3, 6, 9], [2, 5, 8]]
    auto.close(); man.close()


def test_time_limit_staggered():
    """Outputs, state and record equal the manual sequence after every step; done / time_limit follow the host rule; final_obs is the
    manual env's observation before its reset; elapsed matches the host count.

    episode_length: every episode that ENDS here is ended by the time limit of 3, so every reported length is 3 -- for the half that
    was reset by hand too, whose explicit reset began its episode again (include/rcs_hip.h: an explicit reset zeroes `elapsed`); the
    episode that reset cut short after one step ends without a record.  (The issue's "2 for the half that was reset by hand" cannot
    come out of its own rules -- time limit at elapsed >= 3, explicit resets zero elapsed --; the host count is what is asserted.)"""
    ios = {}

    def drive(t, auto, man, exp, a, g):
        io = ios.setdefault("auto", DevIO(auto))
        io.step(a, g)
        got, rec = check_step(("time limit", t), io, auto, man, exp)
        assert same(rec["time_limit"], rec["done"]) and not rec["terminated"].any()
        assert (rec["episode_length"][exp["done"]] == 3).all()
        assert same(got["info"][:, 4] != 0, exp["truncated"])

    _time_limit_scenario(drive)


# ---- 7. host path equals device path (over test 1's scenario)

def test_host_path_equals_device_path():
    """step() with host arrays gives what step_dev + the record give: outputs, info["episode"], info["final_obs"], info["autoreset"]."""

    def drive(t, auto, man, exp, a, g):
        obs, rew, term, trunc, info = auto.step({"joints": a, "gripper": g})
        d = auto.dof
        assert same(obs["tquat"], exp["obs"][:, :7]) and same(obs["joints"], exp["obs"][:, 7:7 + d]) and same(obs["xyzrpy"], exp["obs"][:, 7 + d:13 + d])
        assert same(obs["gripper"], exp["obs"][:, 13 + d]) and same(info["gripper_width"], exp["gw"]) and same(info["substeps"], exp["sub"])
        assert same(trunc, exp["truncated"]) and same(term, exp["terminated"]) and not rew.any()
        done = exp["done"]
        assert same(info["autoreset"], done) and same(info["TimeLimit.truncated"], exp["time_limit"])
        assert same(info["episode"]["l"][done], exp["episode_length"][done]) and not info["episode"]["l"][~done].any()
        assert same(info["episode"]["r"][done], exp["episode_return"][done])
        fo = exp["final_obs"]
        assert same(info["final_obs"]["tquat"][done], fo[done, :7]) and same(info["final_obs"]["joints"][done], fo[done, 7:7 + d])
        assert same(info["final_obs"]["gripper"][done], fo[done, 13 + d]) and not info["final_obs"]["tquat"][~done].any()
        rec = auto.autoreset_last()
        assert same(rec["done"].astype(bool), info["autoreset"]) and same(rec["elapsed"], exp["elapsed"])
        assert same(rec["final_obs"][done], fo[done]) and same(rec["reset_info"][done], exp["reset_info"][done])
        # the device pointers read the same record
        r = auto.autoreset_last_dev()
        n = auto.n_envs
        assert same(down_ptr(auto, r.done, (n,), np.uint8), rec["done"]) and same(down_ptr(auto, r.episode_length, (n,), np.int32), rec["episode_length"])
        assert same(down_ptr(auto, r.final_obs, (n, auto.obs_width), np.float64), rec["final_obs"])
        assert same(down_ptr(auto, r.episodes, (n,), np.int64), rec["episodes"]) and same(down_ptr(auto, r.running_return, (n,), np.float64), rec["running_return"])
        assert same(auto.sim.get_state(), man.sim.get_state())

    _time_limit_scenario(drive)


def test_null_output_pointers_stand_for_the_staging_slices():
    """A _dev step under autoreset whose obs / info / gripper_width / task pointers are null decides and records as one that passes
    buffers: the record and the state equal the manual sequence's -- over the time-limit scenario with every output null, and in the
    task env through step_dev (no task pointer: `terminated` still comes from the task row)."""
    from parity_util import synthetic_actions
    from rcs_env_oracle import FR3_Q_HOME

    n, steps = 8, 7
    joints, grip = synthetic_actions(n, steps, 1)
    auto, man = _pair(n)
    for v in (auto, man):
        v.reset()
    auto.configure_autoreset(max_episode_steps=3)
    manual, io = Manual(man, 3), DevIO(auto)
    for t in range(steps):
        exp = manual.step(joints[t], grip[t])
        io.up("act", joints[t]); io.up("grip", grip[t])
        auto.step_dev(io.p["act"].value, io.p["grip"].value, None)
        rec = auto.autoreset_last()
        done = exp["done"]
        assert same(rec["done"].astype(bool), done) and same(rec["elapsed"], exp["elapsed"]) and same(rec["final_obs"][done], exp["final_obs"][done])
        assert same(rec["final_info"][done], exp["final_info"][done]) and same(rec["final_gripper_width"][done], exp["final_gw"][done])
        assert same(auto.sim.get_state(), man.sim.get_state()), t
    io.free(); manual.io.free()
    auto.close(); man.close()
    auto, man = _task_env(4), _task_env(4)
    boxes = _first_boxes(auto)
    for v in (auto, man):
        v.reset(options={"box_qpos": boxes})
    auto.configure_autoreset(seed=7)
    manual, io = Manual(man, 0, _draw_args(auto)), DevIO(auto)
    home = np.tile(np.asarray(FR3_Q_HOME, dtype=np.float64), (4, 1))
    lift = np.array([False, False, True, False])
    for t in range(3):
        if t == 1:
            for v in (auto, man):
                q = v.sim.free_joint_qpos("box_joint").copy()
                q[lift, 2] = v.SUCCESS_HEIGHT + 0.1
                v.sim.set_free_joint_qpos("box_joint", q, mask=lift)
        g = np.full(4, 0.0 if t == 1 else 1.0, dtype=np.float32)
        exp = manual.step(home, g)
        io.up("act", home); io.up("grip", g)
        auto.step_dev(io.p["act"].value, io.p["grip"].value, io.p["obs"].value)
        rec = auto.autoreset_last()
        assert same(rec["terminated"].astype(bool), lift if t == 1 else np.zeros(4, dtype=bool)) and same(rec["terminated"].astype(bool), exp["terminated"])
        done = exp["done"]
        assert same(rec["final_task"][done], exp["final_task"][done]) and same(rec["reset_box_qpos"][done], exp["reset_box_qpos"][done])
        assert same(rec["episode_return"][done], exp["episode_return"][done]) and same(io.down("obs"), exp["obs"])
        assert same(auto.sim.get_state(), man.sim.get_state()), t
    io.free(); manual.io.free()
    auto.close(); man.close()


# ---- 2. truncation by the guard

def test_truncation_by_the_guard():
    """Environment 0 is sent an absolute joint command folded into the floor: the guard blocks it, it is done with `truncated` and not
    `time_limit`, its obs row is the reset observation, and the next step's verdict for it is free."""
    from rcs_env_oracle import FR3_Q_HOME

    n = 8
    home = np.asarray(FR3_Q_HOME, dtype=np.float64)
    auto, man = _pair(n, relative=False)
    first = [v.reset()[0] for v in (auto, man)][0]
    for v in (auto, man):
        v.configure_guard()
    auto.configure_autoreset()
    manual, io = Manual(man, 0), DevIO(auto)
    rng = np.random.default_rng(2)
    grip = np.ones(n, dtype=np.float32)
    for t in range(4):
        act = home + rng.uniform(-0.005, 0.005, (n, 7))
        if t == 1:
            act[0, 1], act[0, 3] = 1.6, -0.5  # (folded into the floor, as test_gpu_collision_guard.py's class (b))
        exp = manual.step(act, grip)
        io.step(act, grip)
        got, rec = check_step(("guard", t), io, auto, man, exp)
        blocked, result, _ = auto.guard_last()
        assert same(blocked, man.guard_last()[0])
        assert same(rec["done"].astype(bool), blocked | (got["info"][:, 4] != 0)) and not rec["time_limit"].any() and not rec["terminated"].any()
        if t == 1:
            assert blocked[0] and rec["done"][0] and rec["truncated"][0] and got["info"][0, 4] == 1
            d = auto.dof
            assert same(got["obs"][0, 7:7 + d], first["joints"][0]) and same(got["obs"][0, :7], first["tquat"][0]), "the reset observation"
        if t == 2:
            assert not blocked[0] and result[0] == 0, "the fresh episode's first action is free"
    io.free(); manual.io.free()
    auto.close(); man.close()


# ---- 3. / 4. task env: success, reward, placement; sharding

def _task_env(n):
    from rcs_amd import envs, sim as S
    from rcs_amd.envs.base import ControlMode
    from rcs_amd.envs.creators import SimTaskEnvCreator

    sc = S.SimConfig(async_control=True, realtime=False, frequency=30)
    return SimTaskEnvCreator()(envs.default_sim_robot_cfg("fr3_simple_pick_up"), control_mode=ControlMode.JOINTS, delta_actions=False,
                               sim_cfg=sc, n_envs=n)


def _draw_args(venv):
    d = venv.autoreset_desc
    return dict(seed=int(d.seed), box_pose=list(d.box_pose), rotation_minus=float(d.rotation_minus), include_position=bool(d.include_position),
                include_rotation=bool(d.include_rotation), env_offset=int(d.env_offset))


TASK_STEPS = 6
LIFT_BEFORE = (1, 3)  # the cube of the chosen environments is written above the success height before these steps ...
TASK_GRIP = (1.0, 0.0, 1.0, 0.0, 1.0, 1.0)  # ... in which the gripper is commanded shut: `success` without a scripted pick


def _task_rollout(auto, man, first_boxes, lifted_envs, env_offset, record):
    """Test 3's scenario on a pair of envs; `record` collects per step what the sharding test compares."""
    from rcs_env_oracle import FR3_Q_HOME

    n = auto.n_envs
    home = np.tile(np.asarray(FR3_Q_HOME, dtype=np.float64), (n, 1))
    for v in (auto, man):
        v.reset(options={"box_qpos": first_boxes})
    auto.configure_autoreset(seed=7, env_offset=env_offset)
    draw = _draw_args(auto)
    assert draw["seed"] == 7 and draw["env_offset"] == env_offset and draw["rotation_minus"] == 1.0 and draw["box_pose"][3:] == [0, 0, 0, 1]
    manual, io = Manual(man, 0, draw), DevIO(auto)
    lift = np.zeros(n, dtype=bool)
    lift[list(lifted_envs)] = True
    rewards, successes = [], np.zeros(n, dtype=int)
    for t in range(TASK_STEPS):
        if t in LIFT_BEFORE:
            for v in (auto, man):
                q = v.sim.free_joint_qpos("box_joint").copy()
                q[lift, 2] = v.SUCCESS_HEIGHT + 0.1
                v.sim.set_free_joint_qpos("box_joint", q, mask=lift)
        g = np.full(n, TASK_GRIP[t], dtype=np.float32)
        exp = manual.step(home, g)
        io.step(home, g)
        got, rec = check_step(("task", env_offset, t), io, auto, man, exp)
        rewards.append(exp["task"][:, 7].copy())
        if t in LIFT_BEFORE:
            # confirmed on the manual env: exactly the lifted environments succeed; the caller's task row keeps the terminal step
            assert same(exp["task"][:, 8] != 0, lift), exp["task"][:, 8]
            assert same(rec["terminated"].astype(bool), lift) and same(got["task"][:, 8], lift.astype(np.float64))
            assert same(got["task"][:, 7], exp["task"][:, 7]) and (got["task"][lift, 7] == 1.0).all()  # (the terminal reward)
            for e in np.flatnonzero(lift):
                want = auto.autoreset_draw(int(e), int(successes[e]))
                assert same(rec["reset_box_qpos"][e], want), (e, rec["reset_box_qpos"][e], want)
                assert same(want, draw_pose(7, int(e), int(successes[e]), draw["box_pose"], 1.0, True, draw["include_rotation"], env_offset))
                # the sequential fp64 sum of the rewards the manual env returned over the episode
                total = 0.0
                for r in rewards[-(2 if successes[e] else t + 1):]:
                    total = total + r[e]
                assert rec["episode_return"][e] == total, (e, rec["episode_return"][e], total)
            successes[lift] += 1
            placed = rec["reset_box_qpos"].copy()
        elif t - 1 in LIFT_BEFORE:
            # the cube has settled one step at the drawn x, y
            assert np.abs(got["task"][lift, :2] - placed[lift, :2]).max() <= 1e-6, (got["task"][lift, :2], placed[lift, :2])
            assert not rec["terminated"].any()
        record.append({"out": got, "rec": rec, "state": auto.sim.get_state().copy()})
    io.free(); manual.io.free()


def _first_boxes(venv):
    """The cube poses of the first, explicit reset: the env's own rule on numpy's global generator, seeded."""
    np.random.seed(7)
    return venv.draw_box_qpos()


def test_task_env_success_reward_placement():
    auto, man = _task_env(4), _task_env(4)
    _task_rollout(auto, man, _first_boxes(auto), (1,), 0, [])
    auto.close(); man.close()


def _state_columns(blob, n):
    """The per-environment parts of a state blob: [fields][n] doubles, flags, convergence counts (the tail: escalation words)."""
    tail = 8 * ((n + 63) // 64)
    nf = ((len(blob) - 16 - tail) // n - 8) // 8
    body = blob[16:len(blob) - tail]
    S = body[:8 * nf * n].view(np.float64).reshape(nf, n)
    flags = body[8 * nf * n:8 * nf * n + 4 * n].view(np.uint32)
    conv = body[8 * nf * n + 4 * n:].view(np.int32)
    return S, flags, conv


def test_sharding():
    """Two 4-environment Sims with env_offset 0 and 4 reproduce one 8-environment Sim row for row over the task scenario."""
    whole, shards = [], ([], [])
    auto, man = _task_env(8), _task_env(8)
    boxes = _first_boxes(auto)
    _task_rollout(auto, man, boxes, (1, 6), 0, whole)
    auto.close(); man.close()
    for k, (lifted, rec) in enumerate((((1,), shards[0]), ((2,), shards[1]))):
        auto, man = _task_env(4), _task_env(4)
        _task_rollout(auto, man, boxes[4 * k:4 * k + 4], lifted, 4 * k, rec)
        auto.close(); man.close()
    for t, w in enumerate(whole):
        Sw, fw, cw = _state_columns(w["state"], 8)
        for k in (0, 1):
            s = shards[k][t]
            rows = slice(4 * k, 4 * k + 4)
            for key in w["out"]:
                assert same(w["out"][key][rows], s["out"][key]), (t, k, key)
            done = s["rec"]["done"].astype(bool)
            assert same(w["rec"]["done"][rows], s["rec"]["done"])
            for key in ("episode_return", "episode_length", "reset_box_qpos", "final_obs", "final_task", "reset_info"):
                assert same(w["rec"][key][rows][done], s["rec"][key][done]), (t, k, key)
            for key in ("episodes", "elapsed", "running_return", "terminated", "truncated"):
                assert same(w["rec"][key][rows], s["rec"][key]), (t, k, key)
            Ss, fs, cs = _state_columns(s["state"], 4)
            assert same(Sw[:, rows], Ss) and same(fw[rows], fs) and same(cw[rows], cs), (t, k, "state")
    assert any(w["rec"]["done"][6] for w in whole)


# ---- 5. headline configuration

def test_headline_configuration_with_escalated_environments():
    """fr3_empty_world with contacts resolved environment by environment (the default), 16 environments, max_episode_steps 6: the arms
    start at graded heights above the floor and are driven down 5 degrees a step, so that some rest on the floor -- escalated to the
    contact-resolving kernel -- on the step their time limit ends them.  State, outputs and the now / ever bytes equal the manual
    sequence on every step."""
    from rcs_env_oracle import FR3_Q_HOME

    n, steps = 16, 13
    auto, man = _pair(n)
    start = np.tile(np.concatenate([FR3_Q_HOME, [0.04, 0.04]]), (n, 1))
    start[:, 1] = 0.8 + 0.03 * np.arange(n)
    start[:, 3] = -0.8
    for v in (auto, man):
        v.reset()
        v.robot.set_joints_hard(np.ascontiguousarray(start[:, :7]))
        v.sim.set_qpos(np.ascontiguousarray(start))
    auto.configure_autoreset(max_episode_steps=6)
    manual, io = Manual(man, 6), DevIO(auto)
    act = np.zeros((n, 7))
    act[:, 1] = np.deg2rad(5)
    grip = np.ones(n, dtype=np.float32)
    seen = {"escalated_at_limit": 0}

    for t in range(steps):
        def between(out, t=t):
            if t == 5:
                seen["escalated_at_limit"] = int(man.sim.contact_escalated()[0].sum())
        exp = manual.step(act, grip, between)
        if t == 5:
            assert exp["time_limit"].any()
            if not seen["escalated_at_limit"]:
                pytest.skip("no environment of the manual env is escalated on the step its time limit ends it: the actions show nothing")
        io.step(act, grip)
        check_step(("headline", t), io, auto, man, exp)
        (na, ea), (nm, em) = auto.sim.contact_escalated(), man.sim.contact_escalated()
        assert same(na, nm) and same(ea, em), (t, na, nm, ea, em)
    print("escalated on the step the time limit ended them:", seen["escalated_at_limit"], "of", n)
    io.free(); manual.io.free()
    auto.close(); man.close()


# ---- 6. off means off

def _host_rollout(venv, joints, grip):
    out = []
    for t in range(len(joints)):
        obs, rew, term, trunc, info = venv.step({"joints": joints[t], "gripper": grip[t]})
        flat = {k: np.asarray(v).copy() for k, v in info.items()}
        flat.update({"obs." + k: np.asarray(v).copy() for k, v in obs.items()})
        out.append((venv.sim.get_state().copy(), rew.copy(), term.copy(), trunc.copy(), flat))
    return out


def _assert_same_rollout(want, got):
    for (sa, wa, ta, ra, ia), (sb, wb, tb, rb, ib) in zip(want, got):
        assert same(sa, sb) and same(wa, wb) and same(ta, tb) and same(ra, rb)
        assert ia.keys() == ib.keys()
        for k in ia:
            assert same(ia[k], ib[k]), k


def test_off_means_off():
    """An env with configure_autoreset(enabled=False), and one reconfigured from enabled to disabled, roll out bit-identically to an env
    that never heard of it: 20 steps, outputs and state."""
    from parity_util import make_vec_env, synthetic_actions

    joints, grip = synthetic_actions(16, 20, 0)
    runs = []
    for variant in ("plain", "disabled", "enabled then disabled"):
        venv = make_vec_env(16, True)
        venv.reset()
        if variant == "disabled":
            venv.configure_autoreset(enabled=False, max_episode_steps=3)
        if variant == "enabled then disabled":
            venv.configure_autoreset(max_episode_steps=3)
            venv.configure_autoreset(enabled=False, max_episode_steps=3)
        runs.append(_host_rollout(venv, joints, grip))
        assert "autoreset" not in runs[-1][0][4]
        venv.close()
    _assert_same_rollout(runs[0], runs[1])
    _assert_same_rollout(runs[0], runs[2])


# ---- 8. errors

def test_errors_leave_state_and_rollout_untouched():
    from parity_util import make_vec_env, synthetic_actions
    from rcs_amd import _lib, sim as S
    from rcs_amd.camera import SimCameraConfig, SimCameraSet
    from rcs_amd.envs import ControlMode, RelativeTo, default_sim_gripper_cfg, default_sim_robot_cfg
    from rcs_amd.envs.creators import VecSimEnv
    from test_autoreset_cpu import make_desc

    joints, grip = synthetic_actions(16, 20, 3)
    ref = make_vec_env(16, True)
    ref.reset()
    want = _host_rollout(ref, joints, grip)
    ref.close()
    venv = make_vec_env(16, True)
    venv.reset()
    s0 = venv.sim.get_state().copy()
    L, h = venv._L, venv.sim._h
    with pytest.raises(ValueError):
        venv.configure_autoreset(max_episode_steps=-1)
    with pytest.raises(ValueError):
        venv.configure_autoreset(env_offset=-1)
    with pytest.raises(ValueError):
        venv.configure_autoreset(env_offset=2 ** 32 - 15)  # (env_offset + N > 2^32)
    assert L.rcsh_env_configure_autoreset(h, None) == _lib.RCSH_ERR_ARG
    for k in range(7):
        pose = [0.5, 0.0, 0.0144, 0, 0, 0, 1]
        pose[k] = np.nan
        assert L.rcsh_env_configure_autoreset(h, C.byref(make_desc(box_pose=pose, draw_box=0))) == _lib.RCSH_ERR_ARG
    # draw_box without a configured pick task; the record before any step under autoreset
    assert L.rcsh_env_configure_autoreset(h, C.byref(make_desc(draw_box=1))) == _lib.RCSH_ERR_STATE
    with pytest.raises(RuntimeError):
        venv.autoreset_last()
    with pytest.raises(RuntimeError):
        venv.autoreset_last_dev()
    assert not venv.autoreset_enabled and venv.autoreset_desc is None and same(venv.sim.get_state(), s0)
    venv.configure_autoreset(env_offset=2 ** 32 - 16)  # (the last offset that fits)
    with pytest.raises(RuntimeError):
        venv.autoreset_last()  # (configured, not stepped)
    venv.configure_autoreset(enabled=False)
    assert same(venv.sim.get_state(), s0)
    _assert_same_rollout(want, _host_rollout(venv, joints, grip))
    venv.close()
    # before rcsh_env_configure
    cfg = default_sim_robot_cfg("fr3_empty_world")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=True, frequency=30), n_envs=4)
    robot = S.SimRobot(simu, None, cfg)
    s0 = simu.get_state().copy()
    assert simu._L.rcsh_env_configure_autoreset(simu._h, C.byref(make_desc(draw_box=0))) == _lib.RCSH_ERR_STATE
    assert same(simu.get_state(), s0)
    # a render schedule and autoreset refuse each other
    grip_ = S.SimGripper(simu, default_sim_gripper_cfg())
    cams = {"wrist_0": SimCameraConfig(identifier="wrist_0", frame_rate=30, resolution_width=8, resolution_height=6)}
    cs = SimCameraSet(simu, cams, physical_units=True, render_on_demand=False)
    env = VecSimEnv(simu, robot, grip_, ControlMode.JOINTS, float(np.deg2rad(5)), RelativeTo.LAST_STEP, camera_set=cs)
    env.reset()
    s0 = simu.get_state().copy()
    with pytest.raises(RuntimeError, match="render schedule"):
        env.configure_autoreset()
    assert not env.autoreset_enabled and same(simu.get_state(), s0)
    ids, per = np.zeros(1, dtype=np.int32), np.array([1 / 30.0])
    assert simu._L.rcsh_sim_set_render_schedule(simu._h, None, None, 0, 0) == 0  # (the schedule removed: autoreset may come)
    env.configure_autoreset()
    assert simu._L.rcsh_sim_set_render_schedule(simu._h, _lib.ptr(ids), _lib.ptr(per), 1, 2) == _lib.RCSH_ERR_STATE
    env.configure_autoreset(enabled=False)
    assert simu._L.rcsh_sim_set_render_schedule(simu._h, _lib.ptr(ids), _lib.ptr(per), 1, 2) == 0
    env.close()
