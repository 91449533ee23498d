"""The host-pointer entry points' staging (csrc/rcs_hip.hip: Staging, PinLayout, grow_device / grow_pinned) against the `*_dev` forms
of the same calls, bit for bit.

Two handles are built the same way; one is driven through the host forms, the other through the `_dev` forms with buffers from
rcsh_dev_alloc / upload / download.  n = 5 is a ragged team (4 environments per wavefront) and a ragged 64-lane block of the accessor
kernels, n = 67 two such blocks: the smallest sizes at which a wrong slice offset or width lands in a neighbour's rows."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

SIZES = [5, 67]


class Handle:
    """The C-ABI of one environment batch, with device buffers of its own."""

    def __init__(self, venv):
        from rcs_amd import _lib

        self.venv, self.lib, self.L, self.h, self.n = venv, _lib, venv._L, venv.sim._h, venv.n_envs
        self.ow, self.aw, self.dof = venv.obs_width, venv.action_width, venv.dof
        self.nq = self.L.rcsh_sim_nq(self.h)
        self._bufs = []

    def call(self, name, *args):
        self.lib.check(getattr(self.L, name)(self.h, *[self.lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]))

    def dalloc(self, nbytes):
        p = C.c_void_p()
        self.lib.check(self.L.rcsh_dev_alloc(self.h, max(int(nbytes), 8), C.byref(p)))
        self._bufs.append(p)
        return p

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = self.dalloc(a.nbytes)
        self.lib.check(self.L.rcsh_dev_upload(self.h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def down(self, p, shape, dtype=np.float64):
        a = np.zeros(shape, dtype=dtype)
        self.lib.check(self.L.rcsh_dev_download(self.h, C.c_void_p(a.ctypes.data), p, a.nbytes))
        return a

    def out_host(self, task=False):
        n = self.n
        o = {"obs": np.zeros((n, self.ow)), "info": np.zeros((n, 8), dtype=np.uint8), "gw": np.zeros(n), "sub": np.zeros(n, dtype=np.int32)}
        if task:
            o["task"] = np.zeros((n, 9))
        return o

    def out_dev(self):
        """Device outputs that live as long as the handle: rows a masked `_dev` reset leaves alone keep what the last call wrote."""
        if not hasattr(self, "_out"):
            n = self.n
            self._out = {"obs": self.dalloc(n * self.ow * 8), "info": self.dalloc(n * 8), "gw": self.dalloc(n * 8), "sub": self.dalloc(n * 4),
                         "task": self.dalloc(n * 9 * 8)}
        return self._out

    def fetch(self, keys):
        n, d = self.n, self._out
        shapes = {"obs": ((n, self.ow), np.float64), "info": ((n, 8), np.uint8), "gw": ((n,), np.float64), "sub": ((n,), np.int32),
                  "task": ((n, 9), np.float64)}
        return {k: self.down(d[k], *shapes[k]) for k in keys}

    def close(self):
        for p in self._bufs:
            self.lib.check(self.L.rcsh_dev_free(self.h, p))
        self.venv.close()


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k, np.argwhere(np.asarray(a[k]) != np.asarray(b[k]))[:8].tolist())


def _pair(make):
    return Handle(make()), Handle(make())


def _masks(n):
    part = (np.arange(n) % 3 != 1).astype(np.uint8)  # set and cleared entries, in every 4-team and across the 64-lane block's edge
    return [part, np.ones(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)]


def _step_host(H, act, grip, task=False):
    o = H.out_host(task)
    if task:
        H.call("rcsh_env_step_task", act, grip, o["obs"], o["info"], o["gw"], o["sub"], o["task"])
    else:
        H.call("rcsh_env_step", act, grip, o["obs"], o["info"], o["gw"], o["sub"])
    return o


def _step_dev(D, act, grip, task=False):
    d = D.out_dev()
    a, g = D.up(act), (None if grip is None else D.up(grip))
    if task:
        D.call("rcsh_env_step_task_dev", a, g, d["obs"], d["info"], d["gw"], d["sub"], d["task"])
    else:
        D.call("rcsh_env_step_dev", a, g, d["obs"], d["info"], d["gw"], d["sub"])
    return D.fetch(["obs", "info", "gw", "sub"] + (["task"] if task else []))


def _joint_actions(n, dof, steps, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.05, 0.05, (steps, n, dof)), rng.integers(0, 2, (steps, n)).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_env_reset_with_partial_mask(n):
    """rcsh_env_reset with a mask: the reset launch's rows and the observe pass over the complement (info rows and the inverse mask
    in one call) against rcsh_env_reset_dev.  The `_dev` reset writes the masked rows only; an unmasked environment has not moved since
    the call before, so its row of the `_dev` buffers -- that call's observation of the same state -- is its current observation, and
    its pose and joints are read once more through the accessors."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(n, True))
    o, d = H.out_host(), D.out_dev()
    H.call("rcsh_env_reset", None, o["obs"], o["info"], o["gw"])
    D.call("rcsh_env_reset_dev", None, d["obs"], d["info"], d["gw"])
    keys = ["obs", "info", "gw"]
    _same({k: o[k] for k in keys}, D.fetch(keys), "reset to start")
    acts, grips = _joint_actions(n, H.dof, 2, 1)
    for t in range(2):
        _same(_step_host(H, acts[t], grips[t]), _step_dev(D, acts[t], grips[t]), ("step", t))
    for mask in _masks(n):
        o = H.out_host()
        H.call("rcsh_env_reset", mask, o["obs"], o["info"], o["gw"])
        D.call("rcsh_env_reset_dev", D.up(mask), d["obs"], d["info"], d["gw"])
        got = D.fetch(keys)
        _same({k: o[k] for k in keys}, got, ("masked reset", mask.tolist()[:6]))
        keep = mask == 0
        pose, q = np.zeros((n, 7)), np.zeros((n, D.dof))
        D.call("rcsh_robot_get_cartesian_position", pose)
        D.call("rcsh_robot_get_joint_position", q)
        assert np.array_equal(o["obs"][keep, :7], pose[keep]) and np.array_equal(o["obs"][keep, 7 : 7 + D.dof], q[keep])
        if mask.any() and keep.any():  # (the reset rows did go back to the start, the others did not)
            assert not np.array_equal(o["obs"][mask != 0][0, 7 : 7 + D.dof], o["obs"][keep][0, 7 : 7 + D.dof])
    H.close(), D.close()


@pytest.mark.parametrize("mode", ["joints", "tquat"])
@pytest.mark.parametrize("n", SIZES)
def test_env_step_modes(n, mode):
    """rcsh_env_step in joints mode and in the absolute tquat mode (the widest action, 7 doubles), with a gripper command."""
    from parity_util import make_vec_env
    from rcs_amd.envs import ControlMode

    if mode == "joints":
        H, D = _pair(lambda: make_vec_env(n, True))
    else:
        H, D = _pair(lambda: make_vec_env(n, True, relative=False, control_mode=ControlMode.CARTESIAN_TQuat))
    assert H.aw == (H.dof if mode == "joints" else 7)
    o, d = H.out_host(), D.out_dev()
    H.call("rcsh_env_reset", None, o["obs"], o["info"], o["gw"])
    D.call("rcsh_env_reset_dev", None, d["obs"], d["info"], d["gw"])
    acts, grips = _joint_actions(n, H.dof, 3, 2)
    rng = np.random.default_rng(3)
    cur = o
    for t in range(3):
        if mode == "joints":
            act = acts[t]
        else:  # an absolute target: the current pose, shifted
            act = cur["obs"][:, :7].copy()
            act[:, :3] += rng.uniform(-0.03, 0.03, (n, 3))
        cur = _step_host(H, act, grips[t])
        _same(cur, _step_dev(D, act, grips[t]), (mode, t))
        assert (cur["sub"] > 0).all()  # (substeps were counted and fetched)
    H.close(), D.close()


@pytest.mark.parametrize("n", SIZES)
def test_task_forms_with_partial_mask(n):
    """rcsh_env_reset_task / rcsh_env_step_task on the pick-up scene: box poses in, task rows out, a partial mask."""
    from rcs_amd.envs import FR3SimplePickUpSimEnvCreator

    H, D = _pair(lambda: FR3SimplePickUpSimEnvCreator()(n_envs=n))
    np.random.seed(5)
    rng = np.random.default_rng(6)
    keys = ["obs", "info", "gw"]
    d = D.out_dev()
    for step, mask in enumerate([None, _masks(n)[0]]):
        box = H.venv.draw_box_qpos()
        o = H.out_host()
        H.call("rcsh_env_reset_task", mask, box, o["obs"], o["info"], o["gw"])
        D.call("rcsh_env_reset_task_dev", None if mask is None else D.up(mask), D.up(box), d["obs"], d["info"], d["gw"])
        _same({k: o[k] for k in keys}, D.fetch(keys), ("task reset", step))
        for t in range(2):
            act = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-0.1, 0.1, (n, 3))], axis=1)
            grip = rng.uniform(0, 1, n).astype(np.float32)
            ho = _step_host(H, act, grip, task=True)
            _same(ho, _step_dev(D, act, grip, task=True), ("task step", step, t))
        assert (np.abs(ho["task"][:, :3]).max(axis=1) > 0).all()  # (every environment's task row was written and fetched: its cube is somewhere)
    H.close(), D.close()


@pytest.mark.parametrize("n", SIZES)
def test_ik_and_cartesian_accessors(n):
    """rcsh_ik_inverse with a tcp offset and rcsh_ik_forward on its result (the round trip of test_ik_kernels_match_oracle_and_round_trip,
    2e-4 m); then rcsh_robot_set_cartesian_position with a partial mask, rcsh_robot_get_cartesian_position and rcsh_robot_get_state, on
    two handles that received the same calls."""
    import rcs_oracle as O
    from parity_util import make_vec_env
    from rcs_amd.common import Pose

    A, B = _pair(lambda: make_vec_env(n, True, gripper=False, relative=False))
    tcp = O.franka_hand_tcp_offset()
    tcp7 = np.concatenate([tcp.translation(), tcp.rotation_q()])
    T = Pose(translation=tcp7[:3], quaternion=tcp7[3:])
    rng = np.random.default_rng(0)
    q0 = np.zeros((n, A.dof))
    A.call("rcsh_robot_get_joint_position", q0)
    qt = q0 + rng.uniform(-0.2, 0.2, q0.shape)
    outs = []
    for X in (A, B):
        pose = np.zeros((n, 7))
        X.call("rcsh_ik_forward", qt, tcp7, pose)  # frame * tcp^-1 (reference quirk Q7): inverse() recovers the frame from frame * tcp
        target = np.stack([(Pose(translation=p[:3], quaternion=p[3:]) * T * T).as_vec7() for p in pose])
        q, ok, it = np.zeros((n, X.nq)), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
        X.call("rcsh_ik_inverse", target, q0, tcp7, q, ok, it)
        back = np.zeros((n, 7))
        X.call("rcsh_ik_forward", np.ascontiguousarray(q[:, : X.dof]), tcp7, back)
        assert ok.all() and np.abs(back[:, :3] - pose[:, :3]).max() < 2e-4
        mask = _masks(n)[0]
        goal = pose.copy()
        goal[:, 2] -= 0.02
        X.call("rcsh_robot_set_cartesian_position", goal, mask)
        cart, prev, tgt = np.zeros((n, 7)), np.zeros((n, X.dof)), np.zeros((n, X.dof))
        flags = [np.zeros(n, dtype=np.uint8) for _ in range(4)]
        X.call("rcsh_robot_get_cartesian_position", cart)
        X.call("rcsh_robot_get_state", *flags, prev, tgt)
        assert np.abs(tgt[mask != 0]).max() > 0  # (a commanded environment received a joint target)
        outs.append({"pose": pose, "q": q, "ok": ok, "it": it, "back": back, "cart": cart, "prev": prev, "tgt": tgt,
                     **{"flag%d" % i: f for i, f in enumerate(flags)}})
    _same(outs[0], outs[1], "ik and accessors")
    A.close(), B.close()


def _query_rows(m, nq, dof, home, seed):
    rng = np.random.default_rng(seed)
    rows = np.tile(home, (m, 1)) + np.concatenate([rng.uniform(-0.3, 0.3, (m, dof)), np.zeros((m, nq - dof))], axis=1)
    rows[::2, 1], rows[::2, 3] = 1.7, -0.4  # every other row: the arm folded forward and down
    return np.ascontiguousarray(rows)


def _query_host(H, rows):
    m = len(rows)
    hit, kinds, pair = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint8), np.zeros((m, 2), dtype=np.int32)
    H.call("rcsh_collision_query", rows, None, m, 7, hit, kinds, pair)
    return {"hit": hit, "kinds": kinds, "pair": pair}


def _query_dev(D, rows):
    m = len(rows)
    hit, kinds, pair = D.dalloc(m), D.dalloc(m), D.dalloc(8 * m)
    D.call("rcsh_collision_query_dev", D.up(rows), None, m, 7, hit, kinds, pair)
    D.call("rcsh_sim_synchronize")
    return {"hit": D.down(hit, m, np.uint8), "kinds": D.down(kinds, m, np.uint8), "pair": D.down(pair, (m, 2), np.int32)}


@pytest.mark.parametrize("n", SIZES)
def test_interleaved_calls_leave_nothing_behind(n):
    """No staging content outlives its call: env step, IK, a gripper accessor, a collision query, a guard peek, env step on one handle
    against the two env steps alone on another."""
    from parity_util import make_vec_env

    A, B = _pair(lambda: make_vec_env(n, True))
    acts, grips = _joint_actions(n, A.dof, 2, 4)
    for X in (A, B):
        o = X.out_host()
        X.call("rcsh_env_reset", None, o["obs"], o["info"], o["gw"])
        X.venv.configure_guard(enabled=False)
    home = np.zeros((n, A.nq))
    A.call("rcsh_sim_get_qpos", home)
    first = [_step_host(X, acts[0], grips[0]) for X in (A, B)]
    _same(first[0], first[1], "first step")
    # ... on A alone, between the two steps:
    pose = np.ascontiguousarray(first[0]["obs"][:, :7])
    q, ok, it = np.zeros((n, A.nq)), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
    A.call("rcsh_ik_inverse", pose, np.ascontiguousarray(home[:, : A.dof]), None, q, ok, it)
    lc, mv, lw, col = np.zeros(n), np.zeros(n, dtype=np.uint8), np.zeros(n), np.zeros(n, dtype=np.uint8)
    A.call("rcsh_gripper_get_state", lc, mv, lw, col)
    three = _query_host(A, _query_rows(3, A.nq, A.dof, home[0], 7))
    res, tc, blocked = np.zeros(n, dtype=np.int32), np.zeros(n), np.zeros(n, dtype=np.uint8)
    A.call("rcsh_env_guard_peek", np.ascontiguousarray(acts[1]), res, tc, blocked)
    last = [_step_host(X, acts[1], grips[1]) for X in (A, B)]
    _same(last[0], last[1], "last step")
    A.close(), B.close()


def test_query_staging_grows_and_is_reused():
    """rcsh_collision_query with m = 3, then m = 300 (the staging grows), then m = 3 again (the larger buffer is reused)."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(5, True))
    home = np.zeros((5, H.nq))
    H.call("rcsh_sim_get_qpos", home)
    for m in (3, 300, 3):
        rows = _query_rows(m, H.nq, H.dof, home[0], 10 + m)
        got = _query_host(H, rows)
        _same(got, _query_dev(D, rows), ("collision query", m))
        print("collision query, m =", m, ": rows in contact", int(got["hit"].sum()))
    H.close(), D.close()
