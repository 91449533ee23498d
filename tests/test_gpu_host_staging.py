"""The host-pointer entry points' staging (csrc/rcs_hip.hip: Staging, PinLayout, grow_device / grow_pinned; csrc/host_stage.h and
staged_call for the query family and the render call) against the `*_dev` forms of the same calls, bit for bit.

Two handles are built the same way; one is driven through the host forms, the other through the `_dev` forms with buffers from
rcsh_dev_alloc / upload / download.  n = 5 is a ragged team (4 environments per wavefront) and a ragged 64-lane block of the accessor
kernels, n = 67 two such blocks: the smallest sizes at which a wrong slice offset or width lands in a neighbour's rows."""

import ctypes as C
import math
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


# ---- the query family and the render call: every host form over a grown buffer (staged_call) against its `_dev` form

CLEAR_ORDER = ("distance", "status", "pair", "witness", "grad")
SWEPT_ORDER = ("distance", "lower", "s", "pair", "witness", "grad", "evals", "status")
DYN_ORDER = ("qM", "qfrc_bias", "gravity", "qfrc_gravcomp", "jac", "qfrc_inverse", "qacc")
SENTINEL = 0xA5


def _spec(m, nl):
    """Shape and type of every output array of the query family, by name (clearance, swept clearance and dynamics share names)."""
    f8 = np.float64
    spec = {"distance": ((m,), f8), "lower": ((m,), f8), "s": ((m,), f8), "status": ((m,), np.uint8), "pair": ((m, 2), np.int32),
            "witness": ((m, 6), f8), "grad": ((m, nl), f8), "evals": ((m,), np.int32), "qM": ((m, nl, nl), f8), "jac": ((m, 6, nl), f8)}
    spec.update({k: ((m, nl), f8) for k in ("qfrc_bias", "gravity", "qfrc_gravcomp", "qfrc_inverse", "qacc")})
    spec.update({"result": ((m,), np.int32), "t_contact": ((m,), f8), "blocked": ((m,), np.uint8)})
    return spec


class _Outs:
    """The outputs of one comparison: host arrays for the outputs asked for, device buffers of the same sizes on the other handle, and
    for every output NOT asked for an array filled with a sentinel that stays on this side (the library is handed null for it)."""

    def __init__(self, D, spec, order, want):
        self.D, self.spec, self.want = D, spec, tuple(want)
        self.host = {k: np.zeros(*spec[k]) for k in want}
        self.dev = {k: D.dalloc(self.host[k].nbytes) for k in want}
        self.spare = {k: np.zeros(*spec[k]) for k in order if k not in want}
        for a in self.spare.values():
            a.view(np.uint8)[...] = SENTINEL

    def host_args(self, order):
        return [self.host.get(k) for k in order]

    def dev_args(self, order):
        return [self.dev.get(k) for k in order]

    def struct(self, cls, dev):
        return C.byref(cls(**({k: p.value for k, p in self.dev.items()} if dev else {k: a.ctypes.data for k, a in self.host.items()})))

    def settle(self, what):
        """Every array asked for, bit for bit; every array not asked for, untouched."""
        self.D.call("rcsh_sim_synchronize")
        _same(self.host, {k: self.D.down(self.dev[k], *self.spec[k]) for k in self.want}, what)
        for k, a in self.spare.items():
            assert (a.view(np.uint8) == SENTINEL).all(), (what, k, "a null output was written")
        return self.host


def _dup(D, a):
    return None if a is None else D.up(a)


def _home(H):
    q = np.zeros((H.n, H.nq))
    H.call("rcsh_sim_get_qpos", q)
    return q


def _segments(H, m, seed):
    """m joint-space segments: the rows of _query_rows and ends a few tenths of a radian off on the arm joints."""
    rows = _query_rows(m, H.nq, H.dof, _home(H)[0], seed)
    q_to = rows.copy()
    q_to[:, : H.dof] += np.random.default_rng(seed + 1).uniform(-0.3, 0.3, (m, H.dof))
    return rows, np.ascontiguousarray(q_to)


def _pair_mask(H, kinds):
    mask = np.ones(len(H.venv.robot.clearance_pairs(kinds)), dtype=np.uint8)
    mask[::3] = 0
    return mask


def _motion(H, D, a, b, fq, kinds, what):
    m = len(a)
    o = _Outs(D, _spec(m, H.nq), ("result", "t_contact"), ("result", "t_contact"))
    H.call("rcsh_motion_query", a, b, fq, m, kinds, 1e-2, *o.host_args(("result", "t_contact")))
    D.call("rcsh_motion_query_dev", D.up(a), D.up(b), _dup(D, fq), m, kinds, 1e-2, *o.dev_args(("result", "t_contact")))
    return o.settle(what)


def _clearance(H, D, rows, want, what, mask=None, kinds=3):
    m = len(rows)
    o = _Outs(D, _spec(m, H.nq), CLEAR_ORDER, want)
    H.call("rcsh_clearance_query", rows, None, m, kinds, mask, math.inf, *o.host_args(CLEAR_ORDER))
    D.call("rcsh_clearance_query_dev", D.up(rows), None, m, kinds, _dup(D, mask), math.inf, *o.dev_args(CLEAR_ORDER))
    return o.settle(what)


def _swept(H, D, a, b, want, what, mask=None, kinds=3):
    """a None: the env form, the environments' own rows are the segments' starts."""
    m = len(b)
    o = _Outs(D, _spec(m, H.nq), SWEPT_ORDER, want)
    tail = (kinds, mask, math.inf, 1e-2, 1e-2, o.struct(H.lib.SweptOut, False))
    dtail = (kinds, _dup(D, mask), math.inf, 1e-2, 1e-2, o.struct(D.lib.SweptOut, True))
    if a is None:
        H.call("rcsh_env_swept_clearance", b, *tail)
        D.call("rcsh_env_swept_clearance_dev", D.up(b), *dtail)
    else:
        H.call("rcsh_swept_clearance", a, b, None, m, *tail)
        D.call("rcsh_swept_clearance_dev", D.up(a), D.up(b), None, m, *dtail)
    return o.settle(what)


def _dynamics(H, D, q, qvel, qacc, qfrc, want, what, tcp7=None):
    """q None: the env form."""
    m = H.n if q is None else len(q)
    o = _Outs(D, _spec(m, H.nq), DYN_ORDER, want)
    if q is None:
        H.call("rcsh_env_dynamics", qacc, qfrc, tcp7, o.struct(H.lib.DynamicsOut, False))
        D.call("rcsh_env_dynamics_dev", _dup(D, qacc), _dup(D, qfrc), tcp7, o.struct(D.lib.DynamicsOut, True))
    else:
        H.call("rcsh_dynamics_query", q, qvel, qacc, qfrc, m, tcp7, o.struct(H.lib.DynamicsOut, False))
        D.call("rcsh_dynamics_query_dev", D.up(q), _dup(D, qvel), _dup(D, qacc), _dup(D, qfrc), m, tcp7, o.struct(D.lib.DynamicsOut, True))
    return o.settle(what)


def _peek(H, D, action, what):
    order = ("result", "t_contact", "blocked")
    o = _Outs(D, _spec(H.n, H.nq), order, order)
    H.call("rcsh_env_guard_peek", action, *o.host_args(order))
    D.call("rcsh_env_guard_peek_dev", D.up(action), *o.dev_args(order))
    return o.settle(what)


def _stepped_pair(n):
    """Two environment batches after the same reset and two steps: every environment at a pose of its own."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(n, True))
    acts, grips = _joint_actions(n, H.dof, 2, 21)
    for X in (H, D):
        o = X.out_host()
        X.call("rcsh_env_reset", None, o["obs"], o["info"], o["gw"])
        for t in range(2):
            _step_host(X, acts[t], grips[t])
    return H, D


@pytest.mark.parametrize("scene", ["fr3_empty_world", "fr3_simple_pick_up"])
@pytest.mark.parametrize("m", SIZES)
def test_motion_query(m, scene):
    """rcsh_motion_query: `result` and `t_contact`, without a free body's rows and -- in the pick-up scene -- with them."""
    from parity_util import make_vec_env
    from rcs_amd.envs import FR3SimplePickUpSimEnvCreator

    pick = scene == "fr3_simple_pick_up"
    H, D = _pair((lambda: FR3SimplePickUpSimEnvCreator()(n_envs=5)) if pick else (lambda: make_vec_env(5, True)))
    a, b = _segments(H, m, 30 + m)
    fq = None
    if pick:  # the cube somewhere in front of the robot, at a random attitude
        rng = np.random.default_rng(32)
        quat = rng.normal(size=(m, 4))
        fq = np.ascontiguousarray(np.concatenate([rng.uniform([0.3, -0.2, 0.02], [0.6, 0.2, 0.4], (m, 3)), quat / np.linalg.norm(quat, axis=1, keepdims=True)], axis=1))
    got = _motion(H, D, a, b, fq, 7 if pick else 3, (scene, m))
    assert set(np.unique(got["result"])) - {0}  # (some segment does not end free: the folded rows)
    H.close(), D.close()


@pytest.mark.parametrize("m", SIZES)
def test_clearance_optional_outputs(m):
    """rcsh_clearance_query with all outputs, with `distance` alone, and with `distance` + `grad` under a pair mask."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(5, True))
    rows = _query_rows(m, H.nq, H.dof, _home(H)[0], 40 + m)
    full = _clearance(H, D, rows, CLEAR_ORDER, ("all outputs", m))
    alone = _clearance(H, D, rows, ("distance",), ("distance alone", m))
    assert np.array_equal(alone["distance"], full["distance"])
    masked = _clearance(H, D, rows, ("distance", "grad"), ("distance and grad, masked", m), mask=_pair_mask(H, 3))
    assert np.abs(masked["grad"]).max() > 0
    H.close(), D.close()


@pytest.mark.parametrize("m", SIZES)
def test_swept_clearance_optional_outputs(m):
    """rcsh_swept_clearance with all eight outputs and with `distance` + `lower` + `evals` only."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(5, True))
    a, b = _segments(H, m, 50 + m)
    full = _swept(H, D, a, b, SWEPT_ORDER, ("all outputs", m))
    some = _swept(H, D, a, b, ("distance", "lower", "evals"), ("distance, lower, evals", m))
    for k in some:
        assert np.array_equal(some[k], full[k]), k
    assert (full["evals"] > 0).all()
    H.close(), D.close()


@pytest.mark.parametrize("n", SIZES)
def test_env_swept_clearance(n):
    """rcsh_env_swept_clearance: `q_from` is the environments' own rows, nothing is uploaded for it."""
    H, D = _stepped_pair(n)
    q_to = _home(H)
    q_to[:, : H.dof] += np.random.default_rng(60 + n).uniform(-0.3, 0.3, (n, H.dof))
    got = _swept(H, D, None, q_to, SWEPT_ORDER, ("env form", n), mask=_pair_mask(H, 3))
    assert len({r.tobytes() for r in got["grad"]}) > 1  # (the environments stand at poses of their own)
    H.close(), D.close()


@pytest.mark.parametrize("m", SIZES)
def test_dynamics_optional_outputs(m):
    """rcsh_dynamics_query with all seven outputs, with `jac` alone, and with `qfrc_inverse` alone (which brings `qacc_in` along)."""
    from parity_util import make_vec_env

    H, D = _pair(lambda: make_vec_env(5, True))
    rng = np.random.default_rng(70 + m)
    q = _query_rows(m, H.nq, H.dof, _home(H)[0], 71 + m)
    v, a, f = (np.ascontiguousarray(rng.uniform(-1, 1, q.shape)) for _ in range(3))
    tcp7 = np.array([0.0, 0.01, 0.1, 1.0, 0.0, 0.0, 0.0])
    full = _dynamics(H, D, q, v, a, f, DYN_ORDER, ("all outputs", m), tcp7)
    jac = _dynamics(H, D, q, v, None, None, ("jac",), ("jac alone", m), tcp7)
    inv = _dynamics(H, D, q, v, a, None, ("qfrc_inverse",), ("qfrc_inverse alone", m), tcp7)
    assert np.array_equal(jac["jac"], full["jac"]) and np.array_equal(inv["qfrc_inverse"], full["qfrc_inverse"])
    H.close(), D.close()


@pytest.mark.parametrize("n", SIZES)
def test_env_dynamics(n):
    """rcsh_env_dynamics: the environments' own `qpos` and `qvel`; of the inputs only `qfrc_in` is uploaded."""
    H, D = _stepped_pair(n)
    f = np.ascontiguousarray(np.random.default_rng(80 + n).uniform(-1, 1, (n, H.nq)))
    got = _dynamics(H, D, None, None, None, f, ("qM", "qfrc_bias", "qacc"), ("env form", n))
    assert len({r.tobytes() for r in got["qM"]}) > 1
    H.close(), D.close()


class _SimHandle(Handle):
    """Handle over a bare Sim (no environment layer): what the render calls need."""

    def __init__(self, simu):
        from rcs_amd import _lib

        self.venv, self.lib, self.L, self.h, self.n = simu, _lib, simu._L, simu._h, simu.n_envs
        self._bufs = []


def test_camera_render_outputs():
    """rcsh_camera_render_rgb of an 8 x 6 wrist camera in 5 environments: rgb + both depths + pose, then `depth_mm` alone -- the slice
    whose 2-byte elements lie between the 4-byte depth and the 8-byte pose."""
    from rcs_amd import sim as S
    from rcs_amd.camera import SimCameraConfig, SimCameraSet
    from rcs_amd.envs import default_sim_gripper_cfg, default_sim_robot_cfg

    n, W, Hh = 5, 8, 6
    dq = np.random.default_rng(90).uniform(-0.3, 0.3, (n, 7))
    made = []
    for _ in range(2):
        cfg = default_sim_robot_cfg("fr3_empty_world")
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(max_convergence_steps=40), n_envs=n)
        robot = S.SimRobot(simu, None, cfg)
        S.SimGripper(simu, default_sim_gripper_cfg())
        cs = SimCameraSet(simu, {"wrist_0": SimCameraConfig(identifier="wrist_0", frame_rate=0, resolution_width=W, resolution_height=Hh)}, physical_units=True)
        robot.set_joint_position(robot.get_joint_position() + dq)
        simu.step(25)
        made.append((_SimHandle(simu), cs))
    (H, hc), (D, dc) = made
    cam = hc._ids["wrist_0"]
    assert dc._ids["wrist_0"] == cam
    spec = {"rgb": ((n, Hh, W, 3), np.uint8), "depth_gl": ((n, Hh, W), np.float32), "depth_mm": ((n, Hh, W), np.uint16), "cam_pose": ((n, 12), np.float64)}
    order = ("rgb", "depth_gl", "depth_mm", "cam_pose")
    for want in (order, ("depth_mm",)):
        o = _Outs(D, spec, order, want)
        H.call("rcsh_camera_render_rgb", cam, *o.host_args(order))
        D.call("rcsh_camera_render_rgb_dev", cam, *o.dev_args(order))
        got = o.settle(("render", want))
        assert got["depth_mm"].min() < got["depth_mm"].max()  # (something is in view)
        assert len({got["depth_mm"][e].tobytes() for e in range(n)}) > 1  # (the environments look from poses of their own)
    H.close(), D.close()


def test_query_families_share_one_staging_buffer():
    """Every host form of the query family stages through the handle's one grown buffer.  On ONE handle: a clearance query with m = 300
    (the buffer grows), a dynamics query with m = 3, a guard peek, a swept clearance query with m = 67 and a point query with m = 3, each
    against its `_dev` form on the second handle."""
    H, D = _stepped_pair(5)
    for X in (H, D):
        X.venv.configure_guard(enabled=False)
    home = _home(H)[0]
    rng = np.random.default_rng(100)
    _clearance(H, D, _query_rows(300, H.nq, H.dof, home, 101), CLEAR_ORDER, "clearance, m = 300")
    q = _query_rows(3, H.nq, H.dof, home, 102)
    v, a, f = (np.ascontiguousarray(rng.uniform(-1, 1, q.shape)) for _ in range(3))
    _dynamics(H, D, q, v, a, f, DYN_ORDER, "dynamics, m = 3")
    _peek(H, D, np.ascontiguousarray(rng.uniform(-0.05, 0.05, (H.n, H.dof))), "guard peek")
    _swept(H, D, *_segments(H, 67, 103), SWEPT_ORDER, "swept clearance, m = 67")
    rows = _query_rows(3, H.nq, H.dof, home, 104)
    _same(_query_host(H, rows), _query_dev(D, rows), "point query, m = 3")
    H.close(), D.close()
