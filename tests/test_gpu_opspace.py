"""Batched operational-space dynamics of the TCP (SimRobot.opspace_query / VecSimEnv.opspace, csrc/opspace_team.h): twist, jdot_qvel,
lambda_inv, lambda, jbar, op_bias, null_proj, qfrc and status.

* First principles: every sample of tests/golden/opspace.npz (a 60-digit derivation that proves its own precision to 1e-13), all seven
  robots, every output, per sample in the measure max|got - want| / max(1, max|want|).  twist, jdot_qvel and lambda_inv are held to
  REL = 1e-10; lambda, jbar, op_bias, null_proj and qfrc to max(1e-10, 1e-13 cond(A)), cond(A) from the fixture: a backward-stable
  6 x 6 solve and an A that is itself good to about 1e-15 relative give an error of about 1e-15 cond(A); the factor 1e-13 leaves two
  orders.  The status of every sample is exact.
* Against the parent's code: 64 rows over the whole joint range with inputs of order 1 against dynamics_query and
  dynamics_derivatives -- twist = jac qvel, lambda_inv = jac qM_inv jac^T, jdot_qvel against central differences (h = 1e-6, bar 1e-6
  as in the derivative tests) of jac along q +- h qvel, and the loop closed: the qacc that dynamics_query returns for the qfrc of this
  query satisfies jac qacc + jdot_qvel = xacc_des to max(1e-9, 1e-12 cond), cond from numpy on the parent's matrices.
* Shapes and layout, status, errors: as for the sibling queries.
Worst values measured on an MI355X (profiles/opspace/tests.txt, the output of this file under -s):
    first principles: twist 1.1e-15, jdot_qvel 1.9e-15, lambda_inv 4.2e-15, lambda 2.3e-13, jbar 2.2e-13, op_bias 2.1e-13,
    null_proj 3.4e-13, qfrc 2.0e-13 (the last five at ur5e, cond(A) up to 2.8e5, bar 2.8e-8);
    parent's code: twist 3.1e-16, lambda_inv 8.4e-15, jdot_qvel against central differences 5.3e-10, the closed loop at 1.6e-4 of its
    bar with no row left out (worst cond 1.3e5)."""

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
import opspace_cases as OC  # noqa: E402
import parity_util as P  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-10
COND_REL = 1e-13
FD_H = 1e-6
FD_TOL = 1e-6
OK, ARG, STATE = 0, 1, 5
DOUBLES = OC.OUTPUTS
OUTPUTS = DOUBLES + ("status",)
GUARD = 8  # doubles past the end of every device output buffer
SENTINEL = -7.25
STATUS_SENTINEL = -77

_HANDLES = {}


def handle(tag):
    """(simu, robot, cfg) of one robot on a handle with n_envs = 2, built once per module (the queries are independent of n_envs)."""
    if tag not in _HANDLES:
        from rcs_amd import sim as S

        cfg = OC.robot_cfg(tag)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
        _HANDLES[tag] = (simu, S.SimRobot(simu, None, cfg), cfg)
    return _HANDLES[tag]


def _query(robot, a, opts, **kw):
    return robot.opspace_query(a["qpos"], qvel=a["qvel"], xacc=a["xacc_des"], qfrc_null=a["qfrc_null"], **opts, **kw)


def _bar(k, cond):
    return REL if k in OC.ALWAYS else max(REL, COND_REL * cond)


def _shape(k, m, nl):
    return {"twist": (m, 6), "jdot_qvel": (m, 6), "lambda_inv": (m, 6, 6), "lambda": (m, 6, 6), "jbar": (m, nl, 6), "op_bias": (m, 6),
            "null_proj": (m, nl, nl), "qfrc": (m, nl), "status": (m,)}[k]


def _same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- 1: first principles
@pytest.mark.parametrize("tag", OC.TAGS)
def test_every_fixture_sample_matches_first_principles(tag):
    _, robot, _ = handle(tag)
    worst = {k: 0.0 for k in DOUBLES}
    seen = 0
    for opts, names, a in OC.calls(tag):
        r = _query(robot, a, opts)
        n, nv = a["qpos"].shape
        assert sorted(r) == sorted(OUTPUTS)
        assert r["status"].dtype == np.int32 and np.array_equal(r["status"], a["status"]), (tag, names, r["status"])
        for k in DOUBLES:
            assert r[k].shape == _shape(k, n, nv)
        for i, name in enumerate(names):
            seen += 1
            for k in DOUBLES:
                if a["status"][i] == 1 and k in OC.FAMILY:
                    assert np.isnan(r[k][i]).all() and np.isnan(a[k][i]).all(), (tag, name, k)
                    continue
                err = DC.rel_err(r[k][i], a[k][i])  # per sample: no large sample hides a small one
                worst[k] = max(worst[k], err)
                assert err < _bar(k, float(a["cond"][i])), (tag, name, k, err, float(a["cond"][i]))
    assert seen == len(OC.names(tag)) >= 6
    print(tag, "first principles", {k: f"{v:.2e}" for k, v in worst.items()})


# ---- 2: against the parent's code
@pytest.mark.parametrize("tag", ["fr3", "xarm7_pick"])
def test_random_rows_against_the_dynamics_queries(tag):
    from rcs_amd.mjcf import compile_mjcf

    simu, robot, cfg = handle(tag)
    q = DC.random_rows(compile_mjcf(cfg.mjcf_scene_path), 64, seed=31)
    m, nl = q.shape
    assert nl == 9
    rng = np.random.default_rng(32)
    v, xacc, tau0 = rng.uniform(-1, 1, (m, nl)), rng.uniform(-1, 1, (m, 6)), rng.uniform(-1, 1, (m, nl))
    got = robot.opspace_query(q, qvel=v, xacc=xacc, qfrc_null=tau0)
    jac = robot.dynamics_query(q, qvel=v, want=("jac",))["jac"]
    Minv = robot.dynamics_derivatives(q, want=("qM_inv",))["qM_inv"]
    per_row = lambda a, b: max(DC.rel_err(a[i], b[i]) for i in range(m))  # noqa: E731
    A = np.einsum("eri,eij,ecj->erc", jac, Minv, jac)
    err = {"twist": per_row(got["twist"], np.einsum("eri,ei->er", jac, v)), "lambda_inv": per_row(got["lambda_inv"], A)}
    jp = robot.dynamics_query(q + FD_H * v, want=("jac",))["jac"]
    jm = robot.dynamics_query(q - FD_H * v, want=("jac",))["jac"]
    err["jdot_qvel"] = per_row(got["jdot_qvel"], np.einsum("eri,ei->er", jp - jm, v) / (2 * FD_H))
    # closing the loop: the forward dynamics under this query's qfrc accelerate the TCP as asked
    cond = np.linalg.cond(A)
    keep = (cond <= 1e8) & (got["status"] == 0)
    assert np.all(got["status"][cond <= 1e8] == 0) and (~keep).sum() <= 8, (cond.max(), got["status"])
    qacc = robot.dynamics_query(q[keep], qvel=v[keep], qfrc=got["qfrc"][keep], want=("qacc",))["qacc"]
    xa = np.einsum("eri,ei->er", jac[keep], qacc) + got["jdot_qvel"][keep]
    loop = [DC.rel_err(xa[i], xacc[keep][i]) / max(1e-9, 1e-12 * cond[keep][i]) for i in range(int(keep.sum()))]
    print(tag, "parent's code", {k: f"{x:.2e}" for k, x in err.items()}, f"closed loop: worst error / bar {max(loop):.2e} over {int(keep.sum())} rows,",
          f"worst cond {cond[keep].max():.2e}")
    assert err["twist"] < REL and err["lambda_inv"] < REL, err
    assert err["jdot_qvel"] < FD_TOL, err
    assert max(loop) < 1.0, max(loop)


# ---- device-pointer helpers
class _Dev:
    def __init__(self, simu):
        from rcs_amd import _lib

        self.lib, self.L, self.h, self.ptrs = _lib, simu._L, simu._h, []

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        self.lib.check(self.L.rcsh_dev_alloc(self.h, max(int(a.nbytes), 8), C.byref(p)))
        self.ptrs.append(p)
        if a.nbytes:
            self.lib.check(self.L.rcsh_dev_upload(self.h, p, C.c_void_p(a.ctypes.data), a.nbytes))
        return p

    def down(self, p, a):
        self.lib.check(self.L.rcsh_dev_download(self.h, C.c_void_p(a.ctypes.data), p, a.nbytes))
        return a

    def free(self):
        for p in self.ptrs:
            self.lib.check(self.L.rcsh_dev_free(self.h, p))
        self.ptrs = []


def _opspace_dev(simu, q, qvel, xacc, tau0, m, nl, opts=None, want=OUTPUTS, env=False):
    """rcsh_opspace_query_dev (env: rcsh_env_opspace_dev) with every output buffer followed by a guard band of GUARD doubles.
    Returns (outputs, guards intact)."""
    from rcs_amd import _lib
    from rcs_amd import sim as S

    D = _Dev(simu)
    bufs = {}
    for k in want:
        size = int(np.prod(_shape(k, m, nl)))
        bufs[k] = np.full(size + 2 * GUARD, STATUS_SENTINEL, dtype=np.int32) if k == "status" else np.full(size + GUARD, SENTINEL)
    dev = {k: D.up(b) for k, b in bufs.items()}
    out = _lib.OpspaceOut(**{k: p.value for k, p in dev.items()})
    o, _keep = S.SimRobot._opspace_opts(**(opts or {"tcp_offset": None, "task_mask": 0x3F, "damping": 0.0}))
    if env:
        _lib.check(D.L.rcsh_env_opspace_dev(D.h, D.up(xacc), D.up(tau0), C.byref(o), C.byref(out)))
    else:
        _lib.check(D.L.rcsh_opspace_query_dev(D.h, D.up(q), D.up(qvel), D.up(xacc), D.up(tau0), m, C.byref(o), C.byref(out)))
    simu.synchronize()
    res, intact = {}, True
    for k, b in bufs.items():
        D.down(dev[k], b)
        size = int(np.prod(_shape(k, m, nl)))
        intact = intact and bool(np.all(b[size:] == (STATUS_SENTINEL if k == "status" else SENTINEL)))
        res[k] = b[:size].reshape(_shape(k, m, nl)).copy()
    D.free()
    return res, intact


def _rows(n, tag="fr3"):
    g = DC.samples(tag)
    idx = np.arange(n) % len(g["qpos"])
    rng = np.random.default_rng(41)
    return g["qpos"][idx], g["qvel"][idx], rng.uniform(-1, 1, (n, 6)), rng.uniform(-1, 1, (n, g["nv"]))


# ---- 3: shapes and layout
@pytest.mark.parametrize("tag", ["fr3", "so101"])
def test_shapes_guard_bands_and_call_forms(tag):
    simu, robot, _ = handle(tag)
    q, v, x, f = _rows(67, tag)
    nl = q.shape[1]
    opts = {"tcp_offset": None, "task_mask": 0x07 if tag == "so101" else 0x3F, "damping": 0.0}
    full, intact = _opspace_dev(simu, q, v, x, f, 67, nl, opts)
    assert intact
    assert not full["status"].any() and all(np.isfinite(full[k]).all() and np.abs(full[k]).max() > 0 for k in DOUBLES)
    for m in (0, 1, 5):
        res, intact = _opspace_dev(simu, q[:m], v[:m], x[:m], f[:m], m, nl, opts)
        assert intact, m  # the dead teams of the last wavefront store nothing
        for k in OUTPUTS:
            assert _same(res[k], full[k][:m]), (m, k)
    # the host form writes the same bits
    host = robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=f, **opts)
    for k in OUTPUTS:
        assert _same(host[k], full[k]), k
    assert robot.opspace_query(np.zeros((0, nl)), **opts)["null_proj"].shape == (0, nl, nl)
    # any subset of the outputs equals the full call
    for want in [(k,) for k in OUTPUTS] + [("twist", "jdot_qvel"), ("lambda_inv", "status"), ("jbar", "qfrc"), ("op_bias", "null_proj", "status")]:
        one = robot.opspace_query(q, qvel=v, xacc=x if "qfrc" in want else None, qfrc_null=f if "qfrc" in want else None, want=want, **opts)
        assert sorted(one) == sorted(want)
        for k in want:
            assert _same(one[k], full[k]), (want, k)
    # the default asks for what the inputs allow; qvel None and qfrc_null None mean zero
    rest = robot.opspace_query(q, **opts)
    assert sorted(rest) == sorted(k for k in OUTPUTS if k != "qfrc") and not rest["twist"].any() and not rest["jdot_qvel"].any()
    a = robot.opspace_query(q, qvel=v, xacc=x, want=("qfrc",), **opts)["qfrc"]
    b = robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=np.zeros_like(f), want=("qfrc",), **opts)["qfrc"]
    assert _same(a, b)


def test_env_form_equals_the_row_form_on_the_environments_own_rows():
    n = 5
    venv = P.make_vec_env(n, True)
    venv.reset()
    simu, robot = venv.sim, venv.robot
    joints, grip = P.synthetic_actions(n, 3, 3)
    for t in range(3):
        venv.step({"joints": joints[t], "gripper": grip[t]})
    nl = int(simu.model.nq)
    q, v = simu.qpos[:, :nl].copy(), simu.qvel[:, :nl].copy()
    assert np.abs(v).max() > 1e-3
    _, _, x, f = _rows(n)
    tcp = DC.franka_tcp7()
    s0 = simu.get_state().copy()
    env = venv.opspace(xacc=x, qfrc_null=f, tcp_offset=tcp, damping=1e-4)
    assert np.array_equal(simu.get_state(), s0)  # reads the state, writes none of it
    rows = robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=f, tcp_offset=tcp, damping=1e-4)
    assert sorted(env) == sorted(OUTPUTS)
    for k in OUTPUTS:
        assert _same(env[k], rows[k]), k
    some = venv.opspace(want=("lambda", "twist"), tcp_offset=tcp, damping=1e-4)
    assert sorted(some) == ["lambda", "twist"] and _same(some["lambda"], rows["lambda"]) and _same(some["twist"], rows["twist"])
    assert np.abs(rows["twist"]).max() > 1e-4
    # the device form writes the same bits
    dev, intact = _opspace_dev(simu, None, None, x, f, n, nl, {"tcp_offset": tcp, "task_mask": 0x3F, "damping": 1e-4}, env=True)
    assert intact
    for k in OUTPUTS:
        assert _same(dev[k], rows[k]), k
    assert np.array_equal(simu.get_state(), s0)
    venv.close()


def test_a_singular_row_leaves_its_wavefronts_regular_rows_alone():
    _, robot, _ = handle("ur5e")
    sing = OC.sample("ur5e", "0s")
    q, v, x, f = _rows(3, "ur5e")
    with_row = [np.insert(a, 2, sing[k], axis=0) for a, k in ((q, "qpos"), (v, "qvel"), (x, "xacc_des"), (f, "qfrc_null"))]
    alone = robot.opspace_query(q, qvel=v, xacc=x, qfrc_null=f)
    mixed = robot.opspace_query(with_row[0], qvel=with_row[1], xacc=with_row[2], qfrc_null=with_row[3])
    assert mixed["status"].tolist() == [0, 0, 1, 0] and not alone["status"].any()
    for k in OUTPUTS:
        assert _same(np.delete(mixed[k], 2, axis=0), alone[k]), k
    assert all(np.isnan(mixed[k][2]).all() for k in OC.FAMILY) and all(np.isfinite(mixed[k][2]).all() for k in OC.ALWAYS)


# ---- 4: status
def test_status_of_the_rank_deficient_and_singular_samples():
    _, so101, _ = handle("so101")
    for opts, names, a in OC.calls("so101"):
        r = _query(so101, a, opts)
        if opts["task_mask"] == 0x3F:
            assert names == ("0f",) and r["status"].tolist() == [1]  # five arm joints cannot span six task rows
            for k in DOUBLES:
                assert np.isnan(r[k]).all() == (k in OC.FAMILY) and np.isnan(r[k]).any() == (k in OC.FAMILY), k
            for k in OC.ALWAYS:
                assert DC.rel_err(r[k][0], a[k][0]) < REL, k
        else:
            assert opts["task_mask"] == 0x07 and not r["status"].any() and all(np.isfinite(r[k]).all() for k in DOUBLES)
            assert not r["lambda"][:, 3:, :].any() and not r["lambda"][:, :, 3:].any() and not r["jbar"][:, :, 3:].any()
    _, ur5e, _ = handle("ur5e")
    seen = set()
    for opts, names, a in OC.calls("ur5e"):
        for tagged in ("0s", "0d"):
            if tagged not in names:
                continue
            seen.add(tagged)
            i = names.index(tagged)
            r = _query(ur5e, a, opts)
            assert r["status"][i] == a["status"][i] == (1 if tagged == "0s" else 0)
            assert opts["damping"] == (0.0 if tagged == "0s" else 1e-3)
            for k in DOUBLES:
                if tagged == "0s" and k in OC.FAMILY:
                    assert np.isnan(r[k][i]).all(), k
                else:
                    assert DC.rel_err(r[k][i], a[k][i]) < _bar(k, float(a["cond"][i])), (tagged, k)
    assert seen == {"0s", "0d"}


# ---- 5: errors
def test_argument_errors_and_the_handle_answers_afterwards():
    from rcs_amd import _lib, sim as S

    simu, robot, cfg = handle("fr3")
    L, h = simu._L, simu._h
    q, v, x, f = (np.ascontiguousarray(a) for a in _rows(4))
    outs = {k: np.full(_shape(k, 4, 9), 7, dtype=np.int32) if k == "status" else np.full(_shape(k, 4, 9), 2.5) for k in OUTPUTS}
    # (the env forms write n_envs = 2 rows)
    s0 = simu.get_state().copy()
    PT = _lib.ptr
    (fopts, _, g), = [c for c in OC.calls("fr3") if c[0]["task_mask"] == 0x3F and c[0]["tcp_offset"] is None]

    def out(*names):
        return C.byref(_lib.OpspaceOut(**{k: outs[k].ctypes.data for k in names}))

    keep = []

    def opts(mask=0x3F, damping=0.0, tcp=None):
        keep.append(None if tcp is None else np.ascontiguousarray(tcp, dtype=np.float64))
        return C.byref(_lib.OpspaceOpts(tcp_offset7=None if tcp is None else keep[-1].ctypes.data, task_mask=mask, damping=damping))

    def fails(rc, code, word):
        msg = L.rcsh_last_error().decode()
        assert rc == code and word in msg, (rc, msg)
        for k in outs:
            assert np.all(outs[k] == (7 if k == "status" else 2.5)), k
        assert np.array_equal(simu.get_state(), s0)
        # the handle still answers a correct query
        ok = robot.opspace_query(g["qpos"][:1], qvel=g["qvel"][:1], want=("lambda_inv",))["lambda_inv"]
        assert DC.rel_err(ok[0], g["lambda_inv"][0]) < REL

    def bad(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    Q, QD, E, ED = L.rcsh_opspace_query, L.rcsh_opspace_query_dev, L.rcsh_env_opspace, L.rcsh_env_opspace_dev
    fails(Q(h, PT(q), None, None, None, -1, None, out("twist")), ARG, "negative")
    fails(Q(h, None, None, None, None, 4, None, out("twist")), ARG, "null")
    fails(Q(h, PT(q), None, None, None, 4, None, None), ARG, "null")
    fails(Q(h, PT(q), None, None, PT(f), 4, None, out("qfrc")), ARG, "xacc_des")
    fails(Q(h, PT(q), None, None, None, 4, opts(mask=0), out("twist")), ARG, "task_mask")
    fails(Q(h, PT(q), None, None, None, 4, opts(mask=0x40), out("twist")), ARG, "task_mask")
    fails(Q(h, PT(q), None, None, None, 4, opts(damping=-1e-3), out("lambda")), ARG, "damping")
    fails(Q(h, PT(q), None, None, None, 4, opts(damping=float("nan")), out("lambda")), ARG, "damping")
    fails(Q(h, PT(q), None, None, None, 4, opts(damping=float("inf")), out("lambda")), ARG, "damping")
    fails(Q(h, PT(q), None, None, None, 4, opts(tcp=[0, 0, 0.1, 0, 0, 0, 0]), out("twist")), ARG, "zero norm")
    fails(Q(h, PT(q), None, None, None, 4, opts(tcp=[0, np.nan, 0.1, 0, 0, 0, 1]), out("twist")), ARG, "non-finite")
    fails(Q(h, PT(bad(q, (2, 3), np.nan)), None, None, None, 4, None, out("twist")), ARG, "non-finite")
    fails(Q(h, PT(q), PT(bad(v, (1, 0), np.inf)), None, None, 4, None, out("twist")), ARG, "non-finite")
    fails(Q(h, PT(q), None, PT(bad(x, (0, 5), np.nan)), None, 4, None, out("qfrc")), ARG, "non-finite")
    fails(Q(h, PT(q), None, PT(x), PT(bad(f, (3, 8), -np.inf)), 4, None, out("qfrc")), ARG, "non-finite")
    fails(QD(h, None, None, None, None, 4, None, out("twist")), ARG, "null")
    fails(QD(h, PT(q), None, None, None, -2, None, out("twist")), ARG, "negative")
    fails(QD(h, PT(q), None, None, None, 4, None, None), ARG, "null")
    fails(QD(h, PT(q), None, None, None, 4, None, out("qfrc")), ARG, "xacc_des")
    fails(QD(h, PT(q), None, None, None, 4, opts(mask=0x80), out("twist")), ARG, "task_mask")
    fails(QD(h, PT(q), None, None, None, 4, opts(damping=-1.0), out("twist")), ARG, "damping")
    fails(QD(h, PT(q), None, None, None, 4, opts(tcp=[0, 0, 0, 0, 0, 0, 0]), out("twist")), ARG, "zero norm")
    fails(E(h, None, None, None, None), ARG, "null")
    fails(E(h, None, None, None, out("qfrc")), ARG, "xacc_des")
    fails(E(h, None, None, opts(mask=0), out("twist")), ARG, "task_mask")
    fails(E(h, None, None, opts(damping=-1.0), out("twist")), ARG, "damping")
    fails(E(h, PT(bad(x[:2], (1, 1), np.nan)), None, None, out("qfrc")), ARG, "non-finite")
    fails(ED(h, None, None, None, None), ARG, "null")
    fails(ED(h, None, None, None, out("qfrc")), ARG, "xacc_des")
    fails(ED(h, None, None, opts(mask=0x40), out("twist")), ARG, "task_mask")
    fails(ED(h, None, None, opts(tcp=[0, 0, 0, 0, 0, 0, 0]), out("twist")), ARG, "zero norm")
    # M = 0 does nothing, whatever else is null
    assert Q(h, None, None, None, None, 0, None, None) == OK and QD(h, None, None, None, None, 0, None, None) == OK
    assert Q(h, PT(q), None, PT(x), None, 0, None, out(*OUTPUTS)) == OK
    fails(Q(h, PT(q), None, None, None, -1, None, None), ARG, "negative")  # (checks the buffers once more)
    # no robot attached
    bare = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    for rc in (bare._L.rcsh_opspace_query(bare._h, PT(q), None, None, None, 4, None, out("twist")),
               bare._L.rcsh_opspace_query_dev(bare._h, PT(q), None, None, None, 4, None, out("twist")),
               bare._L.rcsh_env_opspace(bare._h, None, None, None, out("twist")), bare._L.rcsh_env_opspace_dev(bare._h, None, None, None, out("twist"))):
        assert rc == STATE and "no robot" in L.rcsh_last_error().decode()
    bare.close()
    assert all(np.all(outs[k] == (7 if k == "status" else 2.5)) for k in outs)
    # the Python layer raises, and the handle answers a valid call afterwards
    with pytest.raises(ValueError):
        robot.opspace_query(bad(q, (0, 0), np.nan))
    with pytest.raises(ValueError):
        robot.opspace_query(q, want=("qfrc",))
    with pytest.raises(ValueError):
        robot.opspace_query(q, task_mask=0)
    with pytest.raises(ValueError):
        robot.opspace_query(q, damping=-1.0)
    with pytest.raises(ValueError):
        robot.opspace_query(q, want=("jac",))
    r = _query(robot, g, fopts)
    assert max(DC.rel_err(r[k][0], g[k][0]) for k in DOUBLES) < max(REL, COND_REL * float(g["cond"][0]))
