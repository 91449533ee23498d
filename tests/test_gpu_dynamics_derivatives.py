"""Batched dynamics derivatives (SimRobot.dynamics_derivatives / VecSimEnv.dynamics_derivatives, csrc/dynamics_grad_team.h): the
Jacobians of inverse and forward dynamics by q and qvel, and M^-1.

* First principles: every sample of tests/golden/dynamics_derivatives.npz (a 60-digit derivation that proves its own precision to
  1e-13), all seven robots, all five outputs, to REL = 1e-10 of tests/test_gpu_dynamics_query.py -- whose outputs these differentiate --
  in the measure max|got - want| / max(1, max|want|).
* Breadth: 64 rows over the whole joint range with inputs of order 1 against central differences (h = 1e-6) of rcsh_dynamics_query's
  qfrc_inverse and qacc.  The differences carry ~2e-10 |f| of round-off (1e-16 |f| / h, two evaluations) and ~2e-13 |f'''| of
  truncation (h^2 / 6); the bar, 1e-6 max(1, max|want|), sits three orders above that.
* Layout, output selection, call forms, identities, errors: as for the dynamics queries.
Worst values measured on an MI355X (profiles/dynamics_derivatives/tests.txt, the output of this file under -s):
    first principles: dqfrc_inverse_dq 3.4e-15, dqfrc_inverse_dqvel 3.1e-15, dqacc_dq 5.1e-15, dqacc_dqvel 1.1e-14, qM_inv 4.4e-15;
    central differences: 1.6e-9, 9.6e-9, 7.6e-9, 4.5e-8, 7.5e-15; qM_inv asymmetry 1.8e-16, |qM_inv qM - I| 3.6e-15."""

import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dynamics_cases as DC  # noqa: E402
import dynamics_derivative_cases as DD  # noqa: E402
import parity_util as P  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-10
FD_H = 1e-6
FD_TOL = 1e-6
OK, ARG, STATE = 0, 1, 5
OUTPUTS = DD.MATRICES
GUARD = 8  # doubles past the end of every device output buffer
SENTINEL = -7.25

_HANDLES = {}


def handle(tag):
    """(simu, robot, cfg) of one robot on a handle with n_envs = 2, built once per module (the queries are independent of n_envs)."""
    if tag not in _HANDLES:
        from rcs_amd import sim as S

        cfg = DD.robot_cfg(tag)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
        _HANDLES[tag] = (simu, S.SimRobot(simu, None, cfg), cfg)
    return _HANDLES[tag]


def _fixture_call(tag, **kw):
    g = DD.stacked(tag)
    _, robot, _ = handle(tag)
    return g, robot.dynamics_derivatives(g["qpos"], qvel=g["qvel"], qacc=g["qacc_in"], qfrc=g["qfrc_in"], **kw)


# ---- 1: first principles
@pytest.mark.parametrize("tag", DD.TAGS)
def test_every_fixture_sample_matches_first_principles(tag):
    g, r = _fixture_call(tag)
    n, nv = g["qpos"].shape
    assert n == len(DD.names(tag)) >= 5 and sorted(r) == sorted(OUTPUTS)
    err = {}
    for k in OUTPUTS:
        assert r[k].shape == (n, nv, nv)
        err[k] = max(DC.rel_err(r[k][i], g[k][i]) for i in range(n))  # per sample: no large sample hides a small one
    print(tag, {k: f"{v:.2e}" for k, v in err.items()})
    assert max(err.values()) < REL, err


# ---- 2: breadth
@pytest.mark.parametrize("tag", ["fr3", "xarm7_pick"])
def test_random_rows_match_central_differences_of_the_dynamics_query(tag):
    from rcs_amd.mjcf import compile_mjcf

    simu, robot, cfg = handle(tag)
    q = DC.random_rows(compile_mjcf(cfg.mjcf_scene_path), 64, seed=21)
    m, nl = q.shape
    assert nl == 9
    rng = np.random.default_rng(22)
    v, a, f = rng.uniform(-1, 1, (m, nl)), rng.uniform(-1, 1, (m, nl)), rng.uniform(-1, 1, (m, nl))
    got = robot.dynamics_derivatives(q, qvel=v, qacc=a, qfrc=f)

    def query(q_, v_):  # parent code: one call for all rows and both outputs
        r = robot.dynamics_query(q_, qvel=v_, qacc=a, qfrc=f, want=("qfrc_inverse", "qacc"))
        return r["qfrc_inverse"], r["qacc"]

    want = {k: np.zeros((m, nl, nl)) for k in ("dqfrc_inverse_dq", "dqfrc_inverse_dqvel", "dqacc_dq", "dqacc_dqvel")}
    for k in range(nl):
        d = np.zeros(nl)
        d[k] = FD_H
        (ip, ap), (im, am) = query(q + d, v), query(q - d, v)
        want["dqfrc_inverse_dq"][:, :, k], want["dqacc_dq"][:, :, k] = (ip - im) / (2 * FD_H), (ap - am) / (2 * FD_H)
        (ip, ap), (im, am) = query(q, v + d), query(q, v - d)
        want["dqfrc_inverse_dqvel"][:, :, k], want["dqacc_dqvel"][:, :, k] = (ip - im) / (2 * FD_H), (ap - am) / (2 * FD_H)
    # d qacc / d qfrc_in: qacc is affine in qfrc_in, so the difference of two calls is M^-1 times the difference of the forces
    zero = robot.dynamics_query(q, qvel=v, qfrc=np.zeros((m, nl)), want=("qacc",))["qacc"]
    want["qM_inv"] = np.zeros((m, nl, nl))
    for k in range(nl):
        unit = np.zeros((m, nl))
        unit[:, k] = 1.0
        want["qM_inv"][:, :, k] = robot.dynamics_query(q, qvel=v, qfrc=unit, want=("qacc",))["qacc"] - zero
    err = {k: max(float(np.abs(got[k][i] - want[k][i]).max() / max(1.0, np.abs(want[k][i]).max())) for i in range(m)) for k in OUTPUTS}
    print(tag, "central differences", {k: f"{x:.2e}" for k, x in err.items()})
    assert max(err.values()) < FD_TOL, err


# ---- device-pointer helpers
class _Dev:
    def __init__(self, simu):
        from rcs_amd import _lib

        self.lib, self.L, self.h, self.ptrs = _lib, simu._L, simu._h, []

    def up(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.lib.check(self.L.rcsh_dev_alloc(self.h, max(int(a.nbytes), 8), C.byref(p)))
        self.ptrs.append(p)
        self.lib.check(self.L.rcsh_dev_upload(self.h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def down(self, p, a):
        self.lib.check(self.L.rcsh_dev_download(self.h, C.c_void_p(a.ctypes.data), p, a.nbytes))
        return a

    def free(self):
        for p in self.ptrs:
            self.lib.check(self.L.rcsh_dev_free(self.h, p))
        self.ptrs = []


def _derivatives_dev(simu, q, qvel, qacc, qfrc, want=OUTPUTS, env=False):
    """rcsh_dynamics_derivatives_dev (env: rcsh_env_dynamics_derivatives_dev) with every output buffer followed by a guard band of GUARD
    doubles.  Returns (outputs, guards intact)."""
    from rcs_amd import _lib

    D = _Dev(simu)
    m, nl = qacc.shape
    bufs = {k: np.full(m * nl * nl + GUARD, SENTINEL) for k in want}
    dev = {k: D.up(b) for k, b in bufs.items()}
    out = _lib.DynamicsGradOut(**{k: p.value for k, p in dev.items()})
    if env:
        _lib.check(D.L.rcsh_env_dynamics_derivatives_dev(D.h, D.up(qacc), D.up(qfrc), C.byref(out)))
    else:
        _lib.check(D.L.rcsh_dynamics_derivatives_dev(D.h, D.up(q), D.up(qvel), D.up(qacc), D.up(qfrc), m, C.byref(out)))
    simu.synchronize()
    res, intact = {}, True
    for k, b in bufs.items():
        D.down(dev[k], b)
        intact = intact and bool(np.all(b[-GUARD:] == SENTINEL))
        res[k] = b[:-GUARD].reshape(m, nl, nl).copy()
    D.free()
    return res, intact


def _rows33(tag="fr3"):
    g = DC.samples(tag)
    idx = np.arange(33) % len(g["qpos"])
    return g["qpos"][idx], g["qvel"][idx], g["qacc_smooth"][idx], g["qfrc_smooth"][idx]


# ---- 3: layout
@pytest.mark.parametrize("tag", ["fr3", "so101"])
def test_team_layout_and_guard_bands(tag):
    simu, _, _ = handle(tag)
    q, v, a, f = _rows33(tag)
    full, intact = _derivatives_dev(simu, q, v, a, f)
    assert intact
    assert all(np.isfinite(x).all() and np.abs(x).max() > 0 for x in full.values())
    for m in (1, 3, 4, 5, 33):
        res, intact = _derivatives_dev(simu, q[:m], v[:m], a[:m], f[:m])
        assert intact, m  # the dead teams of the last wavefront store nothing
        for k in OUTPUTS:
            assert np.array_equal(res[k], full[k][:m]), (m, k)
    # a row's bits do not depend on its position in the batch
    perm = np.random.default_rng(3).permutation(33)
    res, intact = _derivatives_dev(simu, q[perm], v[perm], a[perm], f[perm])
    assert intact
    for k in OUTPUTS:
        assert np.array_equal(res[k], full[k][perm]), k


# ---- 4: output selection
@pytest.mark.parametrize("tag", ["fr3", "so101", "ur5e"])
def test_each_output_alone_equals_the_all_outputs_call(tag):
    g, full = _fixture_call(tag)
    _, robot, _ = handle(tag)
    for k in OUTPUTS:
        one = robot.dynamics_derivatives(g["qpos"], qvel=g["qvel"], qacc=g["qacc_in"] if k == "dqfrc_inverse_dq" else None,
                                         qfrc=g["qfrc_in"] if k in ("dqacc_dq", "dqacc_dqvel") else None, want=(k,))
        assert list(one) == [k]
        assert np.array_equal(one[k], full[k]), (tag, k)
    pair = robot.dynamics_derivatives(g["qpos"], qvel=g["qvel"], qacc=g["qacc_in"], want=("dqfrc_inverse_dq", "dqfrc_inverse_dqvel"))
    assert np.array_equal(pair["dqfrc_inverse_dq"], full["dqfrc_inverse_dq"]) and np.array_equal(pair["dqfrc_inverse_dqvel"], full["dqfrc_inverse_dqvel"])
    # the default asks for what the inputs allow
    assert sorted(robot.dynamics_derivatives(g["qpos"])) == ["dqfrc_inverse_dqvel", "qM_inv"]
    # qvel None means zero
    rest = robot.dynamics_derivatives(g["qpos"], qacc=g["qacc_in"], qfrc=g["qfrc_in"])
    zero = robot.dynamics_derivatives(g["qpos"], qvel=np.zeros_like(g["qpos"]), qacc=g["qacc_in"], qfrc=g["qfrc_in"])
    for k in OUTPUTS:
        assert np.array_equal(rest[k], zero[k]), k


# ---- 5: call forms
def test_dev_equals_host_and_empty_call():
    from rcs_amd import _lib

    simu, robot, _ = handle("fr3")
    q, v, a, f = _rows33()
    host = robot.dynamics_derivatives(q, qvel=v, qacc=a, qfrc=f)
    dev, intact = _derivatives_dev(simu, q, v, a, f)
    assert intact
    for k in OUTPUTS:
        assert np.array_equal(host[k], dev[k]), k
    # m = 0: OK, nothing touched (null pointers everywhere are fine, and filled buffers stay as they are)
    L, h = simu._L, simu._h
    s0 = simu.get_state().copy()
    keep = np.full(81, 3.5)
    out = _lib.DynamicsGradOut(dqfrc_inverse_dqvel=keep.ctypes.data, qM_inv=keep.ctypes.data)
    assert L.rcsh_dynamics_derivatives(h, None, None, None, None, 0, None) == OK
    assert L.rcsh_dynamics_derivatives(h, _lib.ptr(q), None, None, None, 0, C.byref(out)) == OK
    assert L.rcsh_dynamics_derivatives_dev(h, None, None, None, None, 0, None) == OK
    assert np.all(keep == 3.5) and np.array_equal(simu.get_state(), s0)
    assert robot.dynamics_derivatives(np.zeros((0, 9)))["qM_inv"].shape == (0, 9, 9)


def test_env_form_equals_the_row_form_on_the_environments_own_rows():
    n = 33
    venv = P.make_vec_env(n, True)
    venv.reset()
    simu, robot = venv.sim, venv.robot
    joints, grip = P.synthetic_actions(n, 3, 3)
    for t in range(3):
        venv.step({"joints": joints[t], "gripper": grip[t]})
    nl = int(simu.model.nq)
    q, v = simu.qpos[:, :nl].copy(), simu.qvel[:, :nl].copy()
    assert np.abs(v).max() > 1e-3
    _, _, a, f = _rows33()
    s0 = simu.get_state().copy()
    env = venv.dynamics_derivatives(qacc=a, qfrc=f)
    assert np.array_equal(simu.get_state(), s0)  # reads the state, writes none of it
    rows = robot.dynamics_derivatives(q, qvel=v, qacc=a, qfrc=f)
    assert sorted(env) == sorted(OUTPUTS)
    for k in OUTPUTS:
        assert np.array_equal(env[k], rows[k]), k
    some = venv.dynamics_derivatives(want=("qM_inv", "dqfrc_inverse_dqvel"))
    assert sorted(some) == ["dqfrc_inverse_dqvel", "qM_inv"]
    assert np.array_equal(some["qM_inv"], rows["qM_inv"]) and np.array_equal(some["dqfrc_inverse_dqvel"], rows["dqfrc_inverse_dqvel"])
    # the device form writes the same bits
    dev, intact = _derivatives_dev(simu, None, None, a, f, env=True)
    assert intact
    for k in OUTPUTS:
        assert np.array_equal(dev[k], rows[k]), k
    assert np.array_equal(simu.get_state(), s0)
    venv.close()


def test_env_form_in_a_scene_with_a_free_body():
    """fr3_simple_pick_up: the state holds the free body's qpos and qvel behind the chain's; the env form must read the chain's fields.
    Held to the row form at the same rows (bit for bit) and, through it, to central differences of the parent's env-free query."""
    from rcs_amd import envs, sim as S
    from rcs_amd.envs.base import ControlMode, RelativeTo
    from rcs_amd.envs.creators import VecPickCubeEnv

    n = 5
    cfg = envs.default_sim_robot_cfg("fr3_simple_pick_up")
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(async_control=True, realtime=False, frequency=30), n_envs=n)
    robot = S.SimRobot(simu, None, cfg)
    gripper = S.SimGripper(simu, envs.default_sim_gripper_cfg())
    venv = VecPickCubeEnv(simu, robot, gripper, ControlMode.JOINTS, 0.1, RelativeTo.LAST_STEP)
    venv.reset()
    joints, grip = P.synthetic_actions(n, 3, 3)
    for t in range(3):
        venv.step({"joints": joints[t], "gripper": grip[t]})
    nl = int(simu.model.nq)
    assert nl == 9 and simu.model.free_bodies
    q, v = simu.qpos[:, :nl].copy(), simu.qvel[:, :nl].copy()
    assert np.abs(v).max() > 1e-3
    _, _, a, f = (x[:n] for x in _rows33())
    s0 = simu.get_state().copy()
    got = venv.dynamics_derivatives(qacc=a, qfrc=f)
    assert np.array_equal(simu.get_state(), s0)
    rows = robot.dynamics_derivatives(q, qvel=v, qacc=a, qfrc=f)
    for k in OUTPUTS:
        assert got[k].shape == (n, nl, nl) and np.array_equal(got[k], rows[k]), k
    # ... and the rows are the right ones: qM_inv inverts the qM of the environments' own dynamics
    qM = venv.dynamics(want=("qM",))["qM"]
    assert DC.rel_err(np.einsum("eij,ejk->eik", got["qM_inv"], qM), np.broadcast_to(np.eye(nl), (n, nl, nl))) < REL
    # the velocity derivative reads qvel: it differs from the one at rest
    assert np.abs(got["dqfrc_inverse_dqvel"] - robot.dynamics_derivatives(q, want="dqfrc_inverse_dqvel")["dqfrc_inverse_dqvel"]).max() > 1e-6
    venv.close()


# ---- 6: identities on the GPU outputs
@pytest.mark.parametrize("tag", ["fr3", "xarm7_pick", "arm6"])
def test_identities(tag):
    g, r = _fixture_call(tag)
    _, robot, _ = handle(tag)
    n, nv = g["qpos"].shape
    Minv = r["qM_inv"]
    sym = max(float(np.abs(Minv[i] - Minv[i].T).max() / np.abs(Minv[i]).max()) for i in range(n))
    qM = robot.dynamics_query(g["qpos"], want=("qM",))["qM"]
    ident = max(DC.rel_err(Minv[i] @ qM[i], np.eye(nv)) for i in range(n))
    rest = robot.dynamics_derivatives(g["qpos"], want=("dqfrc_inverse_dqvel",))["dqfrc_inverse_dqvel"]
    print(tag, f"qM_inv asymmetry {sym:.2e}  |qM_inv qM - I| {ident:.2e}  |dqfrc_inverse_dqvel| at rest {np.abs(rest).max():.2e}")
    assert sym < 1e-13
    assert ident < REL
    assert np.abs(rest).max() <= 1e-13


# ---- 7: errors
def test_argument_errors_and_the_handle_answers_afterwards():
    from rcs_amd import _lib, sim as S

    simu, robot, cfg = handle("fr3")
    L, h = simu._L, simu._h
    q, v, a, f = (np.ascontiguousarray(x[:4]) for x in _rows33())
    outs = {k: np.full((4, 9, 9), 2.5) for k in OUTPUTS}
    # (the env forms write n_envs = 2 rows)
    s0 = simu.get_state().copy()
    PT = _lib.ptr
    g = DD.stacked("fr3")

    def out(*names):
        return C.byref(_lib.DynamicsGradOut(**{k: outs[k].ctypes.data for k in names}))

    def fails(rc, code, word):
        msg = L.rcsh_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        for k in outs:
            assert np.all(outs[k] == 2.5), k
        assert np.array_equal(simu.get_state(), s0)
        # the handle still answers a correct query
        ok = robot.dynamics_derivatives(g["qpos"][:1], qvel=g["qvel"][:1], want=("qM_inv",))["qM_inv"]
        assert DC.rel_err(ok[0], g["qM_inv"][0]) < REL

    bad = q.copy()
    bad[2, 3] = np.nan
    inf_v = v.copy()
    inf_v[1, 0] = np.inf
    nan_a = a.copy()
    nan_a[0, 8] = np.nan
    inf_f = f.copy()
    inf_f[3, 1] = -np.inf
    D = L.rcsh_dynamics_derivatives
    fails(D(h, PT(q), None, None, None, -1, out("qM_inv")), ARG, "negative")
    fails(D(h, None, None, None, None, 4, out("qM_inv")), ARG, "null")
    fails(D(h, PT(q), None, None, None, 4, None), ARG, "null")
    fails(D(h, PT(q), None, None, PT(f), 4, out("dqfrc_inverse_dq")), ARG, "qacc_in")
    fails(D(h, PT(q), None, PT(a), None, 4, out("dqacc_dq")), ARG, "qfrc_in")
    fails(D(h, PT(q), None, PT(a), None, 4, out("dqacc_dqvel")), ARG, "qfrc_in")
    fails(D(h, PT(bad), None, None, None, 4, out("qM_inv")), ARG, "non-finite")
    fails(D(h, PT(q), PT(inf_v), None, None, 4, out("qM_inv")), ARG, "non-finite")
    fails(D(h, PT(q), None, PT(nan_a), None, 4, out("dqfrc_inverse_dq")), ARG, "non-finite")
    fails(D(h, PT(q), None, None, PT(inf_f), 4, out("dqacc_dq")), ARG, "non-finite")
    fails(L.rcsh_dynamics_derivatives_dev(h, None, None, None, None, 4, out("qM_inv")), ARG, "null")
    fails(L.rcsh_dynamics_derivatives_dev(h, PT(q), None, None, None, -2, out("qM_inv")), ARG, "negative")
    fails(L.rcsh_dynamics_derivatives_dev(h, PT(q), None, None, None, 4, None), ARG, "null")
    fails(L.rcsh_env_dynamics_derivatives(h, None, None, out("dqacc_dq")), ARG, "qfrc_in")
    fails(L.rcsh_env_dynamics_derivatives(h, None, None, out("dqfrc_inverse_dq")), ARG, "qacc_in")
    fails(L.rcsh_env_dynamics_derivatives(h, None, None, None), ARG, "null")
    fails(L.rcsh_env_dynamics_derivatives_dev(h, None, None, out("dqacc_dqvel")), ARG, "qfrc_in")
    # no robot attached
    bare = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    rc = bare._L.rcsh_dynamics_derivatives(bare._h, PT(q), None, None, None, 4, out("qM_inv"))
    assert rc == STATE and "no robot" in L.rcsh_last_error().decode()
    rc = bare._L.rcsh_env_dynamics_derivatives(bare._h, None, None, out("qM_inv"))
    assert rc == STATE and "no robot" in L.rcsh_last_error().decode()
    bare.close()
    # the Python layer raises, and the handle answers a valid call afterwards
    with pytest.raises(ValueError):
        robot.dynamics_derivatives(bad)
    with pytest.raises(ValueError):
        robot.dynamics_derivatives(q, want=("dqacc_dq",))
    with pytest.raises(ValueError):
        robot.dynamics_derivatives(q, want=("qM",))
    r = robot.dynamics_derivatives(g["qpos"], qvel=g["qvel"], qacc=g["qacc_in"], qfrc=g["qfrc_in"])
    assert max(DC.rel_err(r[k], g[k]) for k in OUTPUTS) < REL
