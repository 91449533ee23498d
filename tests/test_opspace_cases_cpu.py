"""The ground truth of the operational-space queries (tests/golden/opspace.npz, tests/opspace_cases.py) checked without a GPU, and the
host-side surface of the feature.

* Against a second source that shares no formulation with the fixture: the oracle's kinematics (dynamics_cases.TcpJacobian), the golden
  qM and qfrc_bias of the robots' samples (the oracle's orc_step1 where a sample's configuration is not a golden one) and float64
  numpy; jdot_qvel against Richardson-extrapolated central differences (steps 2e-5 and 1e-5) of that Jacobian along qvel.  To 1e-6 in
  dynamics_cases.rel_err; for the lambda family the bar is multiplied by max(1, cond(A) / 1e4) -- float64 numpy loses cond(A) ulps.
* The fixture's own identities, to 1e-12 max(1, cond(A)): lambda lambda_inv = I_sel; J jbar = I_sel, J Minv null_proj = 0,
  null_proj^2 = null_proj and J Minv (qfrc - b) + jdot_qvel = xacc_des on the selected rows (the four hold without damping: with it
  J jbar = I_sel - damping lambda); jdot_qvel = 0 and twist = 0 at rest.
* The caps: self_agreement <= 1e-13; every status-0 sample has cond(A) <= 1e6 and relative pivot >= 1e-6, every status-1 sample a
  relative pivot <= 1e-30; at least four full-mask status-0 samples per robot with six or more arm joints; the file under 400 KB.
* The C-ABI declares the four entry points and both structs, RCSH_ABI_VERSION is still 2, the ctypes layer lists them with the same
  fields, and the Python layer refuses unknown output names before the library is called.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "robot-control-stack_amd"), HERE]

import dynamics_cases as DC  # noqa: E402
import dynamics_derivative_cases as DD  # noqa: E402
import opspace_cases as OC  # noqa: E402

SECOND_SOURCE_TOL = 1e-6
H = 2e-5
IDENTITY_TOL = 1e-12
ARM_JOINTS = {"fr3": 7, "fr3_arm": 7, "xarm7": 7, "ur5e": 6, "arm6": 6, "so101": 5, "xarm7_pick": 7}


class _SecondSource:
    """J from the oracle's kinematics; qM and qfrc_bias from the golden samples, or from the oracle's orc_step1 off them."""

    def __init__(self, tag):
        import rcs_oracle as O
        from rcs_amd.mjcf import compile_mjcf

        cfg = OC.robot_cfg(tag)
        cm = compile_mjcf(cfg.mjcf_scene_path)
        self.jac = DC.TcpJacobian(cm, site=cfg.attachment_site)
        self.golden = DC.samples(tag)
        self.O, self.L = O, O.lib()
        self.model = O.make_model(cm, False)

    def dynamics(self, name, q, v):
        idx = int(name.rstrip("rtmfsd"))
        g = self.golden
        if np.array_equal(q, g["qpos"][idx]):
            if np.array_equal(v, g["qvel"][idx]):
                return g["qM"][idx], g["qfrc_bias"][idx]
            if not v.any():
                return g["qM"][idx], g["gravity"][idx]  # at rest the bias is the gravity term
        d = self.O.OrcData()
        self.L.orc_reset_data(C.byref(self.model), C.byref(d))
        nv = len(q)
        for i in range(nv):
            d.qpos[i], d.qvel[i] = float(q[i]), float(v[i])
        self.L.orc_step1(C.byref(self.model), C.byref(d))
        return np.array(d.qM[:]).reshape(self.O.MAXV, self.O.MAXV)[:nv, :nv].copy(), np.array(d.qfrc_bias[:nv])


def _second_source(src, name, s):
    q, v = s["qpos"], s["qvel"]
    sel = OC.selection(int(s["task_mask"]))
    J = src.jac.jacobian(q, s["tcp_offset"]) * sel[:, None]
    jd = DD.richardson(lambda x: (src.jac.jacobian(q + x[0] * v, s["tcp_offset"]) * sel[:, None]) @ v, np.zeros(1), H)[:, 0]
    M, b = src.dynamics(name, q, v)
    Minv = np.linalg.inv(M)
    A = J @ Minv @ J.T + float(s["damping"]) * np.diag(sel)
    out = {"twist": J @ v, "jdot_qvel": jd, "lambda_inv": A}
    if int(s["status"]) == 0:
        on = sel > 0
        lam = np.zeros((6, 6))
        lam[np.ix_(on, on)] = np.linalg.inv(A[np.ix_(on, on)])
        jbar = Minv @ J.T @ lam
        ob = jbar.T @ b - lam @ jd
        null = np.eye(len(q)) - J.T @ jbar.T
        out.update({"lambda": lam, "jbar": jbar, "op_bias": ob, "null_proj": null, "qfrc": J.T @ (lam @ s["xacc_des"] + ob) + null @ s["qfrc_null"]})
    return out


@pytest.mark.parametrize("tag", OC.TAGS)
def test_fixture_matches_the_oracles_kinematics_and_the_golden_dynamics(tag):
    src = _SecondSource(tag)
    worst = {k: 0.0 for k in OC.OUTPUTS}
    for name in OC.names(tag):
        s = OC.sample(tag, name)
        want = _second_source(src, name, s)
        scale = max(1.0, float(s["cond"]) / 1e4)
        for k, x in want.items():
            err = DC.rel_err(x, s[k])
            bar = SECOND_SOURCE_TOL * (scale if k in OC.FAMILY else 1.0)
            worst[k] = max(worst[k], err / bar)
            assert err < bar, (tag, name, k, err, bar)
        if int(s["status"]) == 1:
            assert all(np.isnan(s[k]).all() for k in OC.FAMILY)
    print(tag, "error / bar", {k: f"{x:.2e}" for k, x in worst.items()})


@pytest.mark.parametrize("tag", OC.TAGS)
def test_fixture_identities(tag):
    g = DC.samples(tag)
    for name in OC.names(tag):
        s = OC.sample(tag, name)
        nv = g["nv"]
        sel = OC.selection(int(s["task_mask"]))
        Isel = np.diag(sel)
        J, Minv = s["jac"], s["qM_inv"]
        assert J.shape == (6, nv) and Minv.shape == (nv, nv) and not J[sel == 0].any()
        assert DC.rel_err(J @ s["qvel"], s["twist"]) < IDENTITY_TOL
        assert DC.rel_err(J @ Minv @ J.T + float(s["damping"]) * Isel, s["lambda_inv"]) < IDENTITY_TOL
        assert not s["twist"][sel == 0].any() and not s["jdot_qvel"][sel == 0].any()
        if name.endswith("r"):
            assert not s["qvel"].any() and not s["twist"].any() and not s["jdot_qvel"].any()
        if int(s["status"]) == 1:
            continue
        tol = IDENTITY_TOL * max(1.0, float(s["cond"]))
        assert DC.rel_err(s["lambda"] @ s["lambda_inv"], Isel) < tol
        assert DC.rel_err(s["jbar"], Minv @ J.T @ s["lambda"]) < tol
        if float(s["damping"]) == 0.0:
            idx = int(name.rstrip("rtmfsd"))
            assert np.array_equal(s["qpos"], g["qpos"][idx])
            b = g["gravity"][idx] if name.endswith("r") else g["qfrc_bias"][idx]
            assert DC.rel_err(J @ s["jbar"], Isel) < tol
            assert DC.rel_err(J @ Minv @ s["null_proj"], np.zeros((6, nv))) < tol
            assert DC.rel_err(s["null_proj"] @ s["null_proj"], s["null_proj"]) < tol
            assert DC.rel_err(sel * (J @ Minv @ (s["qfrc"] - b) + s["jdot_qvel"]), sel * s["xacc_des"]) < tol
    assert any(n.endswith("r") for n in OC.names(tag))


def test_fixture_precision_and_caps():
    assert OC.self_agreement() <= 1e-13
    assert os.path.getsize(OC.FIXTURE) < 400 * 1024
    for tag in OC.TAGS:
        full = 0
        for name in OC.names(tag):
            s = OC.sample(tag, name)
            if int(s["status"]) == 0:
                assert float(s["cond"]) <= OC.COND_CAP and float(s["rel_pivot"]) >= OC.PIVOT_CAP, (tag, name)
                full += int(s["task_mask"]) == 0x3F
            else:
                assert float(s["rel_pivot"]) <= OC.SINGULAR_CAP, (tag, name)
        if ARM_JOINTS[tag] >= 6:
            assert full >= 4, (tag, full)
    # the samples the feature's description names
    assert OC.sample("so101", "0f")["status"] == 1 and int(OC.sample("so101", "0f")["task_mask"]) == 0x3F
    assert all(int(OC.sample("so101", n)["task_mask"]) == 0x07 and OC.sample("so101", n)["status"] == 0 for n in OC.names("so101") if n != "0f")
    sing, damped = OC.sample("ur5e", "0s"), OC.sample("ur5e", "0d")
    assert sing["qpos"][4] == 0.0 and sing["status"] == 1 and np.array_equal(sing["qpos"], damped["qpos"])
    assert damped["status"] == 0 and float(damped["damping"]) == 1e-3
    assert int(OC.sample("fr3", "1m")["task_mask"]) == 0x07
    for tag in ("fr3", "xarm7_pick"):
        assert OC.sample(tag, "1t")["tcp_offset"].shape == (7,)


def test_c_abi_declares_the_operational_space_queries():
    from rcs_amd import _lib
    from rcs_amd import sim as S

    text = open(os.path.join(HERE, "..", "include", "rcs_hip.h")).read()
    for name in ("rcsh_opspace_query", "rcsh_opspace_query_dev", "rcsh_env_opspace", "rcsh_env_opspace_dev"):
        assert re.search(r"^int\s+" + name + r"\s*\(rcsh_sim\*", text, re.M), name
        assert name in _lib.EXPORTS
    body = re.search(r"typedef struct rcsh_opspace_out \{(.*?)\} rcsh_opspace_out;", text, re.S).group(1)
    fields = re.findall(r"\b(?:double|int32_t)\*\s+(\w+);", body)
    assert tuple(fields) == OC.OUTPUTS + ("status",) == S.SimRobot.OPSPACE_OUTPUTS
    assert [f for f, _ in _lib.OpspaceOut._fields_] == fields
    assert re.search(r"\bint32_t\*\s+status;", body)
    body = re.search(r"typedef struct rcsh_opspace_opts \{(.*?)\} rcsh_opspace_opts;", text, re.S).group(1)
    declared = re.findall(r"^\s*(?:const double\*|uint32_t|double)\s+(\w+);", body, re.M)
    assert declared == ["tcp_offset7", "task_mask", "damping"] == [f for f, _ in _lib.OpspaceOpts._fields_]
    assert [t for _, t in _lib.OpspaceOpts._fields_] == [C.c_void_p, C.c_uint32, C.c_double]
    assert re.search(r"^#define\s+RCSH_OPSPACE_REL_PIVOT\s+1e-10\b", text, re.M)
    assert re.search(r"^#define\s+RCSH_ABI_VERSION\s+2\s*$", text, re.M)


def test_want_is_validated_before_the_library_is_called():
    from rcs_amd import sim as S

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached: {name}")

    robot = S.SimRobot.__new__(S.SimRobot)  # no handle, no library: only the validation runs
    robot._L = robot.sim = NoLibrary()
    with pytest.raises(ValueError, match="unknown operational-space output"):
        robot.opspace_query(np.zeros((1, 9)), want=("lambda", "Lambda"))
    with pytest.raises(ValueError, match="unknown operational-space output"):
        robot.opspace_query(np.zeros((1, 9)), want="jac")
    everything = S.SimRobot.OPSPACE_OUTPUTS
    assert robot._opspace_want(None, None) == tuple(k for k in everything if k != "qfrc")
    assert robot._opspace_want(None, np.zeros(6)) == everything
    assert robot._opspace_want("status", None) == ("status",)
