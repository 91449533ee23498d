"""Batched dynamics queries (SimRobot.dynamics_query / VecSimEnv.dynamics, csrc/dynamics_team.h): the joint-space inertia, the bias
forces, the gravity-compensation force, inverse and forward dynamics of the chain and the TCP Jacobian, held DIRECTLY to the
first-principles vectors of tests/golden/*_dynamics.json (the substep tests see them only through the state after a whole step) and to
the Jacobian tests/dynamics_cases.py composes from the oracle's kinematics.

The bar is REL = 1e-10 of tests/test_dynamics_golden.py, max|got - golden| / max(1, max|golden|) per vector, no sample left out (the
oracle measures 4e-13 on the same vectors).  Worst values measured on an MI355X, over every robot of tests 1 and 2:
    qM 1.6e-15, qfrc_bias 8.1e-16, gravity 7.9e-16, coriolis 7.6e-15, qfrc_gravcomp 6.9e-16, qfrc_inverse 9.9e-15, qacc 4.7e-15;
    partly compensated FR3 against the oracle: qM 2.0e-15, qfrc_bias 7.4e-16, qfrc_gravcomp 8.3e-16; jac 1.6e-15 (test 3);
    pick-up scene against orc_step1: qM 1.7e-15, qfrc_bias 1.4e-15.

Row counts are not multiples of 4 on purpose: dead teams sit in the last wavefront."""

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
import parity_util as P  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-10
OK, ARG, STATE = 0, 1, 5
OUTPUTS = ("qM", "qfrc_bias", "gravity", "qfrc_gravcomp", "jac", "qfrc_inverse", "qacc")
GUARD = 8  # doubles past the end of every device output buffer


def _scene_and_cfg(tag):
    from rcs_amd import envs as E

    if tag in ("fr3", "fr3_arm", "xarm7"):
        cfg = E.xarm7_sim_robot_cfg() if tag == "xarm7" else E.default_sim_robot_cfg("fr3_empty_world")
        path = {"fr3": lambda: P.SCENE, "fr3_arm": P.fr3_arm_only_scene, "xarm7": P.xarm7_frictionless_scene}[tag]()
        cfg.mjcf_scene_path = cfg.kinematic_model_path = path
        return cfg
    return {"ur5e": E.ur5e_sim_robot_cfg, "arm6": E.arm6_sim_robot_cfg, "so101": E.so101_sim_robot_cfg, "xarm7_pick": E.xarm7_pick_sim_robot_cfg}[tag]()


_HANDLES = {}


def handle(tag):
    """(simu, robot, cfg) of one robot on a handle with n_envs = 2, built once per module (the queries are independent of n_envs)."""
    if tag not in _HANDLES:
        from rcs_amd import sim as S

        cfg = _scene_and_cfg(tag)
        simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=2)
        _HANDLES[tag] = (simu, S.SimRobot(simu, None, cfg), cfg)
    return _HANDLES[tag]


def _all_outputs(tag):
    """Every output of one call on all golden samples: rows qpos, qvel; qacc_in = qacc_smooth; qfrc_in = qfrc_smooth + qfrc_bias."""
    g = DC.samples(tag)
    _, robot, _ = handle(tag)
    return g, robot.dynamics_query(g["qpos"], qvel=g["qvel"], qacc=g["qacc_smooth"], qfrc=g["qfrc_smooth"] + g["qfrc_bias"])


def _golden_errors(tag):
    g, r = _all_outputs(tag)
    nv = g["nv"]
    assert r["qM"].shape == (len(g["qpos"]), nv, nv) and r["jac"].shape == (len(g["qpos"]), 6, nv)
    err = {"qM": DC.rel_err(r["qM"], g["qM"]), "qfrc_bias": DC.rel_err(r["qfrc_bias"], g["qfrc_bias"]),
           "gravity": DC.rel_err(r["gravity"], g["gravity"]), "coriolis": DC.rel_err(r["qfrc_bias"] - r["gravity"], g["coriolis"]),
           "qfrc_gravcomp": DC.rel_err(r["qfrc_gravcomp"], g["qfrc_gravcomp"]),
           "qfrc_inverse": DC.rel_err(r["qfrc_inverse"], g["qfrc_smooth"] + g["qfrc_bias"]),
           "qacc": DC.rel_err(r["qacc"], g["qacc_smooth"])}
    print(tag, {k: f"{v:.2e}" for k, v in err.items()})
    assert np.array_equal(r["qM"], np.swapaxes(r["qM"], 1, 2))  # mirrored on the way out
    return err


# ---- 1
@pytest.mark.parametrize("tag", DC.REFERENCE_TAGS)
def test_reference_robots_match_first_principles(tag):
    assert len(DC.samples(tag)["qpos"]) == 32
    err = _golden_errors(tag)
    assert max(err.values()) < REL, err


# ---- 2
@pytest.mark.parametrize("tag", DC.AUTHORED_TAGS)
def test_authored_scenes_match_first_principles(tag):
    """Topo<6, false> (ur5e, arm6), Topo<5, true> (so101) and the general gravity-compensation path (ur5e, arm6, so101: no body is
    compensated, so the path must return zeros where the shortcut would return gravity); xarm7_pick as shipped, with its dry friction:
    nothing returned depends on it."""
    g = DC.samples(tag)
    assert len(g["qpos"]) == 16
    if tag != "xarm7_pick":
        assert np.abs(g["qfrc_gravcomp"] - g["gravity"]).max() > 0.1
    err = _golden_errors(tag)
    assert max(err.values()) < REL, err


def _fr3_partial_gravcomp_scene() -> str:
    """The FR3 scene with gravcomp 0.5 on link 3 and 0.25 on the hand (welded to link 7 next to the fully compensated flange and camera:
    the compensated centre of that link is then not its centre of mass), written to a temporary file."""
    import shutil

    path = os.path.join(P.scratch_dir(), "rcs_amd_fr3_partial_gravcomp", "scene.xml")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        xml = open(P.SCENE).read()
        for old, new in (('<body name="fr3_link3_0" pos="0 -0.316 0" quat="1 1 0 0" gravcomp="1">', '<body name="fr3_link3_0" pos="0 -0.316 0" quat="1 1 0 0" gravcomp="0.5">'),
                         ('<body name="hand_0" pos="0 0 0.107" quat="0.9238795 0 0 -0.3826834" gravcomp="1">', '<body name="hand_0" pos="0 0 0.107" quat="0.9238795 0 0 -0.3826834" gravcomp="0.25">')):
            assert old in xml, old
            xml = xml.replace(old, new)
        open(path, "w").write(xml)
        for extra in ("collision_vertices.npz", "render_hulls.npz"):
            shutil.copy(os.path.join(os.path.dirname(P.SCENE), extra), os.path.dirname(path))
    return path


def test_partial_gravity_compensation_matches_the_oracle():
    """The general gravity-compensation path with numbers in it: no golden vector has a partly compensated robot, so the reference
    is the oracle's orc_step1 on the same scene, itself within 4e-13 of the golden vectors on the shipped scenes: REL stands."""
    import rcs_oracle as O
    from rcs_amd import envs as E, sim as S
    from rcs_amd.mjcf import compile_mjcf

    cfg = E.default_sim_robot_cfg("fr3_empty_world")
    cfg.mjcf_scene_path = cfg.kinematic_model_path = _fr3_partial_gravcomp_scene()
    simu = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    robot = S.SimRobot(simu, None, cfg)
    g = DC.samples("fr3")
    q, v = g["qpos"][:16], g["qvel"][:16]
    got = robot.dynamics_query(q, qvel=v, want=("qM", "qfrc_bias", "gravity", "qfrc_gravcomp"))
    m = O.make_model(compile_mjcf(cfg.mjcf_scene_path), False)
    L = O.lib()
    want = {"qM": [], "qfrc_bias": [], "qfrc_gravcomp": []}
    for r in range(len(q)):
        d = O.OrcData()
        L.orc_reset_data(C.byref(m), C.byref(d))
        for i in range(9):
            d.qpos[i], d.qvel[i] = q[r, i], v[r, i]
        L.orc_step1(C.byref(m), C.byref(d))
        want["qM"].append(np.array(d.qM[:]).reshape(O.MAXV, O.MAXV)[:9, :9])
        want["qfrc_bias"].append(d.qfrc_bias[:9])
        want["qfrc_gravcomp"].append(d.qfrc_gravcomp[:9])
    err = {k: DC.rel_err(got[k], np.array(x)) for k, x in want.items()}
    print("partial gravcomp", {k: f"{x:.2e}" for k, x in err.items()})
    gc = np.array(want["qfrc_gravcomp"])
    assert np.abs(gc - got["gravity"]).max() > 0.1 and np.abs(gc).max() > 1.0  # neither the shortcut's answer nor zero
    assert max(err.values()) < REL, err
    simu.close()


# ---- 3
@pytest.mark.parametrize("tag", ["fr3", "xarm7"])
@pytest.mark.parametrize("with_offset", [True, False])
def test_jacobian_matches_the_oracle_composition(tag, with_offset):
    from rcs_amd.mjcf import compile_mjcf

    simu, robot, cfg = handle(tag)
    cm = compile_mjcf(cfg.mjcf_scene_path)
    truth = DC.TcpJacobian(cm, cfg.attachment_site)
    q = DC.random_rows(cm, 33, seed=5)
    tcp7 = DC.franka_tcp7() if with_offset else None
    want = np.array([truth.jacobian(row, tcp7) for row in q])
    got = robot.dynamics_query(q, tcp_offset=tcp7, want=("jac",))["jac"]
    err = float(np.abs(got - want).max())
    print(tag, with_offset, f"jac {err:.2e}")
    assert err < REL * max(1.0, float(np.abs(want).max())), err
    assert np.all(got[:, :, ~truth.above] == 0.0)  # the finger columns are exactly zero
    if tag == "fr3":
        assert (~truth.above).sum() == 2
    # DeviceKinematics.jacobian is the same call
    from rcs_amd import sim as S

    assert np.array_equal(S.DeviceKinematics(simu, robot.dof).jacobian(q, tcp7), got)
    assert np.array_equal(S.DeviceKinematics(simu, robot.dof).jacobian(q[:, : robot.dof], tcp7), got)


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


def _shapes(m, nl):
    return {k: (m, nl, nl) if k == "qM" else (m, 6, nl) if k == "jac" else (m, nl) for k in OUTPUTS}


def _query_dev(simu, q, qvel, qacc, qfrc, tcp7=None, want=OUTPUTS):
    """rcsh_dynamics_query_dev with every output buffer followed by a guard band of GUARD doubles.  Returns (outputs, guards intact)."""
    from rcs_amd import _lib

    D = _Dev(simu)
    m, nl = q.shape
    sentinel = -7.25
    bufs = {k: np.full(int(np.prod(s)) + GUARD, sentinel) for k, s in _shapes(m, nl).items() if k in want}
    dev = {k: D.up(b) for k, b in bufs.items()}
    out = _lib.DynamicsOut(**{k: p.value for k, p in dev.items()})
    tcp = None if tcp7 is None else np.ascontiguousarray(tcp7, dtype=np.float64)
    _lib.check(D.L.rcsh_dynamics_query_dev(D.h, D.up(q), D.up(qvel), D.up(qacc), D.up(qfrc), m, _lib.ptr(tcp), C.byref(out)))
    simu.synchronize()
    res, intact = {}, True
    for k, b in bufs.items():
        D.down(dev[k], b)
        intact = intact and bool(np.all(b[-GUARD:] == sentinel))
        res[k] = b[:-GUARD].reshape(_shapes(m, nl)[k]).copy()
    D.free()
    return res, intact


def _rows33(tag="fr3"):
    g = DC.samples(tag)
    idx = np.arange(33) % len(g["qpos"])
    return g["qpos"][idx], g["qvel"][idx], g["qacc_smooth"][idx], (g["qfrc_smooth"] + g["qfrc_bias"])[idx]


# ---- 4
def test_team_layout_and_guard_bands():
    simu, robot, _ = handle("fr3")
    assert simu.n_envs == 2
    q, v, a, f = _rows33()
    tcp7 = DC.franka_tcp7()
    full, intact = _query_dev(simu, q, v, a, f, tcp7)
    assert intact
    assert all(np.isfinite(x).all() for x in full.values())
    for m in (1, 3, 4, 5, 33):
        res, intact = _query_dev(simu, q[:m], v[:m], a[:m], f[:m], tcp7)
        assert intact, m  # the dead teams of the last wavefront store nothing
        for k in OUTPUTS:
            assert np.array_equal(res[k], full[k][:m]), (m, k)


# ---- 5
def test_each_output_alone_equals_the_all_outputs_call():
    for tag in ("fr3", "so101"):
        g, full = _all_outputs(tag)
        _, robot, _ = handle(tag)
        for k in OUTPUTS:
            one = robot.dynamics_query(g["qpos"], qvel=g["qvel"], qacc=g["qacc_smooth"] if k == "qfrc_inverse" else None,
                                       qfrc=g["qfrc_smooth"] + g["qfrc_bias"] if k == "qacc" else None, want=(k,))
            assert list(one) == [k]
            assert np.array_equal(one[k], full[k]), (tag, k)
        pair = robot.dynamics_query(g["qpos"], qvel=g["qvel"], want=("qM", "qfrc_bias"))
        assert np.array_equal(pair["qM"], full["qM"]) and np.array_equal(pair["qfrc_bias"], full["qfrc_bias"])
    # qvel None means zero: the bias is then the gravity term
    g = DC.samples("fr3")
    _, robot, _ = handle("fr3")
    rest = robot.dynamics_query(g["qpos"], want=("qfrc_bias", "gravity"))
    zero = robot.dynamics_query(g["qpos"], qvel=np.zeros_like(g["qpos"]), want=("qfrc_bias", "gravity"))
    assert np.array_equal(rest["qfrc_bias"], zero["qfrc_bias"]) and np.array_equal(rest["gravity"], zero["gravity"])
    assert DC.rel_err(rest["qfrc_bias"], g["gravity"]) < REL


# ---- 6
def test_dev_equals_host_and_empty_call():
    from rcs_amd import _lib

    simu, robot, _ = handle("fr3")
    q, v, a, f = _rows33()
    tcp7 = DC.franka_tcp7()
    host = robot.dynamics_query(q, qvel=v, qacc=a, qfrc=f, tcp_offset=tcp7)
    dev, intact = _query_dev(simu, q, v, a, f, tcp7)
    assert intact
    for k in OUTPUTS:
        assert np.array_equal(host[k], dev[k]), k
    # m = 0: OK, nothing touched (null pointers everywhere are fine, and filled buffers stay as they are)
    L, h = simu._L, simu._h
    s0 = simu.get_state().copy()
    keep = np.full(9, 3.5)
    out = _lib.DynamicsOut(qM=keep.ctypes.data, qfrc_bias=keep.ctypes.data)
    assert L.rcsh_dynamics_query(h, None, None, None, None, 0, None, None) == OK
    assert L.rcsh_dynamics_query(h, _lib.ptr(q), None, None, None, 0, None, C.byref(out)) == OK
    assert L.rcsh_dynamics_query_dev(h, None, None, None, None, 0, None, None) == OK
    assert np.all(keep == 3.5) and np.array_equal(simu.get_state(), s0)
    assert robot.dynamics_query(np.zeros((0, 9)))["qM"].shape == (0, 9, 9)


# ---- 7
def test_env_form_equals_the_query_on_the_same_rows():
    n = 33
    venv = P.make_vec_env(n, True)
    venv.reset()
    simu, robot = venv.sim, venv.robot
    q, v, a, f = _rows33()
    simu.set_qpos(q)
    simu.set_qvel(v)
    s0 = simu.get_state().copy()
    tcp7 = DC.franka_tcp7()
    env = venv.dynamics(qacc=a, qfrc=f, tcp_offset=tcp7)
    assert np.array_equal(simu.get_state(), s0)  # reads the state, writes none of it
    rows = robot.dynamics_query(q, qvel=v, qacc=a, qfrc=f, tcp_offset=tcp7)
    assert sorted(env) == sorted(OUTPUTS)
    for k in OUTPUTS:
        assert np.array_equal(env[k], rows[k]), k
    some = venv.dynamics(want=("qM", "qfrc_bias"))
    assert sorted(some) == ["qM", "qfrc_bias"] and np.array_equal(some["qM"], rows["qM"]) and np.array_equal(some["qfrc_bias"], rows["qfrc_bias"])
    # the device form writes the same bits
    from rcs_amd import _lib

    D = _Dev(simu)
    buf = np.full(n * 9 + GUARD, -7.25)
    p = D.up(buf)
    _lib.check(simu._L.rcsh_env_dynamics_dev(simu._h, None, None, None, C.byref(_lib.DynamicsOut(qfrc_bias=p.value))))
    simu.synchronize()
    D.down(p, buf)
    D.free()
    assert np.array_equal(buf[:-GUARD].reshape(n, 9), rows["qfrc_bias"]) and np.all(buf[-GUARD:] == -7.25)
    assert np.array_equal(simu.get_state(), s0)
    venv.close()


def test_env_form_in_a_scene_with_a_free_body():
    """fr3_simple_pick_up: MuJoCo's nq is nl + 7; the query covers the chain's nl dofs, whose block of M the free body does not couple
    to.  Held to the oracle's orc_step1 (qM[:nl, :nl], qfrc_bias[:nl]) at the environments' own states."""
    import rcs_oracle as O
    from rcs_amd import envs, sim as S
    from rcs_amd.envs.base import ControlMode, RelativeTo
    from rcs_amd.envs.creators import VecPickCubeEnv
    from rcs_amd.mjcf import compile_mjcf

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
    s0 = simu.get_state().copy()
    got = venv.dynamics(want=("qM", "qfrc_bias"))
    assert np.array_equal(simu.get_state(), s0)
    assert got["qM"].shape == (n, nl, nl) and got["qfrc_bias"].shape == (n, nl)
    m = O.make_model(compile_mjcf(cfg.mjcf_scene_path), False)
    L = O.lib()
    worst = {"qM": 0.0, "qfrc_bias": 0.0}
    for e in range(n):
        d = O.OrcData()
        L.orc_reset_data(C.byref(m), C.byref(d))
        for i in range(nl):
            d.qpos[i], d.qvel[i] = q[e, i], v[e, i]
        L.orc_step1(C.byref(m), C.byref(d))
        qM = np.array(d.qM[:]).reshape(O.MAXV, O.MAXV)[:nl, :nl]
        worst["qM"] = max(worst["qM"], DC.rel_err(got["qM"][e], qM))
        worst["qfrc_bias"] = max(worst["qfrc_bias"], DC.rel_err(got["qfrc_bias"][e], d.qfrc_bias[:nl]))
    print("pick-up", {k: f"{x:.2e}" for k, x in worst.items()})
    assert max(worst.values()) < REL, worst
    venv.close()


# ---- 8
def test_argument_errors_and_the_handle_answers_afterwards():
    from rcs_amd import _lib, sim as S

    simu, robot, cfg = handle("fr3")
    L, h = simu._L, simu._h
    q, v, a, f = (np.ascontiguousarray(x[:4]) for x in _rows33())
    outs = {k: np.full(s, 2.5) for k, s in _shapes(4, 9).items()}
    keep = {k: o.copy() for k, o in outs.items()}
    s0 = simu.get_state().copy()
    PT = _lib.ptr

    def out(*names):
        return C.byref(_lib.DynamicsOut(**{k: outs[k].ctypes.data for k in names}))

    def fails(rc, code, word):
        msg = L.rcsh_last_error().decode()
        assert rc == code and word in msg, (rc, msg)

    bad = q.copy()
    bad[2, 3] = np.nan
    inf_v = v.copy()
    inf_v[1, 0] = np.inf
    zero_quat = np.array([0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 0.0])
    fails(L.rcsh_dynamics_query(h, PT(q), None, None, None, -1, None, out("qM")), ARG, "negative")
    fails(L.rcsh_dynamics_query(h, None, None, None, None, 4, None, out("qM")), ARG, "null")
    fails(L.rcsh_dynamics_query(h, PT(q), None, None, None, 4, None, None), ARG, "null")
    fails(L.rcsh_dynamics_query(h, PT(q), None, None, PT(f), 4, None, out("qfrc_inverse")), ARG, "qacc_in")
    fails(L.rcsh_dynamics_query(h, PT(q), None, PT(a), None, 4, None, out("qacc")), ARG, "qfrc_in")
    fails(L.rcsh_dynamics_query(h, PT(bad), None, None, None, 4, None, out("qM")), ARG, "non-finite")
    fails(L.rcsh_dynamics_query(h, PT(q), PT(inf_v), None, None, 4, None, out("qM")), ARG, "non-finite")
    fails(L.rcsh_dynamics_query(h, PT(q), None, None, None, 4, PT(zero_quat), out("jac")), ARG, "zero norm")
    fails(L.rcsh_dynamics_query_dev(h, None, None, None, None, 4, None, out("qM")), ARG, "null")
    fails(L.rcsh_dynamics_query_dev(h, PT(q), None, None, None, -2, None, out("qM")), ARG, "negative")
    fails(L.rcsh_env_dynamics(h, None, None, None, out("qacc")), ARG, "qfrc_in")
    fails(L.rcsh_env_dynamics(h, None, None, PT(zero_quat), out("jac")), ARG, "zero norm")
    fails(L.rcsh_env_dynamics_dev(h, None, None, None, out("qfrc_inverse")), ARG, "qacc_in")
    for k in outs:
        assert np.array_equal(outs[k], keep[k]), k
    assert np.array_equal(simu.get_state(), s0)
    # no robot attached
    bare = S.Sim(cfg.mjcf_scene_path, S.SimConfig(), n_envs=1)
    fails(bare._L.rcsh_dynamics_query(bare._h, PT(q), None, None, None, 4, None, out("qM")), STATE, "no robot")
    fails(bare._L.rcsh_env_dynamics(bare._h, None, None, None, out("qM")), STATE, "no robot")
    bare.close()
    # the Python layer raises, and the handle answers a valid call afterwards
    with pytest.raises(ValueError):
        robot.dynamics_query(bad)
    with pytest.raises(ValueError):
        robot.dynamics_query(q, want=("qacc",))
    with pytest.raises(ValueError):
        robot.dynamics_query(q, want=("mass",))
    g = DC.samples("fr3")
    assert DC.rel_err(robot.dynamics_query(g["qpos"], want=("qM",))["qM"], g["qM"]) < REL
