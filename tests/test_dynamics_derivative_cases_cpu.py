"""The ground truth of the dynamics derivatives (tests/golden/dynamics_derivatives.npz, tests/dynamics_derivative_cases.py) checked
without a GPU, and the host-side surface of the feature.

* Against a second source that shares no formulation with the fixture: Richardson-extrapolated central differences (steps 2e-5 and
  1e-5) of the oracle's orc_step1 (qM, qfrc_bias) at the same states, to 1e-6 in dynamics_cases.rel_err.  Double-precision differences
  at h ~ 1e-5 carry round-off ~1e-16 |f| / h ~ 1e-9 and, extrapolated, truncation ~h^4: room to spare, while a missing term shows at
  order 1.
* The fixture's own identities: qM_inv qM = I (1e-12, qM from the robots' golden samples), dqacc_dq = -qM_inv dqfrc_inverse_dq taken
  at the solved acceleration, dqacc_dqvel = -qM_inv dqfrc_inverse_dqvel, and dqfrc_inverse_dqvel = 0 on the samples at rest.
* The C-ABI declares the four entry points and the struct, RCSH_ABI_VERSION is still 2, the ctypes layer lists them, and the Python
  layer refuses unknown output names before the library is called.
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

FD_TOL = 1e-6
H = 2e-5
IDENTITY_TOL = 1e-12


class _Oracle:
    """qM and qfrc_bias of one robot from the oracle's orc_step1."""

    def __init__(self, tag):
        import rcs_oracle as O
        from rcs_amd.mjcf import compile_mjcf

        self.O, self.L = O, O.lib()
        self.model = O.make_model(compile_mjcf(DD.robot_cfg(tag).mjcf_scene_path), False)

    def __call__(self, q, v):
        d = self.O.OrcData()
        self.L.orc_reset_data(C.byref(self.model), C.byref(d))
        nv = len(q)
        for i in range(nv):
            d.qpos[i], d.qvel[i] = float(q[i]), float(v[i])
        self.L.orc_step1(C.byref(self.model), C.byref(d))
        return np.array(d.qM[:]).reshape(self.O.MAXV, self.O.MAXV)[:nv, :nv].copy(), np.array(d.qfrc_bias[:nv])


@pytest.mark.parametrize("tag", DD.TAGS)
def test_fixture_matches_differences_of_the_oracle(tag):
    orc = _Oracle(tag)
    worst = {k: 0.0 for k in DD.MATRICES}
    assert len(DD.names(tag)) >= 4
    for name in DD.names(tag):
        s = DD.sample(tag, name)
        q, v, a, f = (s[k] for k in DD.INPUTS)

        def inverse(q_, v_):
            M, b = orc(q_, v_)
            return M @ a + b

        def forward(q_, v_):
            M, b = orc(q_, v_)
            return np.linalg.solve(M, f - b)

        got = {"dqfrc_inverse_dq": DD.richardson(lambda x: inverse(x, v), q, H), "dqfrc_inverse_dqvel": DD.richardson(lambda x: inverse(q, x), v, H),
               "dqacc_dq": DD.richardson(lambda x: forward(x, v), q, H), "dqacc_dqvel": DD.richardson(lambda x: forward(q, x), v, H),
               "qM_inv": np.linalg.inv(orc(q, v)[0])}
        for k in DD.MATRICES:
            worst[k] = max(worst[k], DC.rel_err(got[k], s[k]))
    print(tag, {k: f"{x:.2e}" for k, x in worst.items()})
    assert max(worst.values()) < FD_TOL, worst


def test_fixture_precision_is_proven_by_the_tool():
    assert DD.self_agreement() <= 1e-13
    assert os.path.getsize(DD.FIXTURE) < 400 * 1024


@pytest.mark.parametrize("tag", DD.TAGS)
def test_fixture_identities(tag):
    g = DC.samples(tag)
    for name in DD.names(tag):
        s = DD.sample(tag, name)
        idx = int(name.rstrip("r"))
        nv = g["nv"]
        assert all(s[k].shape == (nv, nv) for k in DD.MATRICES)
        assert np.array_equal(s["qpos"], g["qpos"][idx]) and np.array_equal(s["qacc_in"], g["qacc_smooth"][idx])
        assert np.array_equal(s["qfrc_in"], g["qfrc_smooth"][idx])
        assert DC.rel_err(s["qM_inv"] @ g["qM"][idx], np.eye(nv)) < IDENTITY_TOL
        assert DC.rel_err(s["qM_inv"], s["qM_inv"].T) < IDENTITY_TOL
        assert DC.rel_err(-s["qM_inv"] @ s["dqfrc_inverse_dq_at_qacc"], s["dqacc_dq"]) < IDENTITY_TOL
        assert DC.rel_err(-s["qM_inv"] @ s["dqfrc_inverse_dqvel"], s["dqacc_dqvel"]) < IDENTITY_TOL
        if name.endswith("r"):
            assert not s["qvel"].any()
            assert np.abs(s["dqfrc_inverse_dqvel"]).max() == 0.0 and np.abs(s["dqacc_dqvel"]).max() == 0.0
            # at rest qfrc_bias is the gravity term: qacc = qM_inv (qfrc_in - gravity)
            assert DC.rel_err(s["qM_inv"] @ (s["qfrc_in"] - g["gravity"][idx]), s["qacc"]) < IDENTITY_TOL
        else:
            assert np.array_equal(s["qvel"], g["qvel"][idx])
            assert DC.rel_err(s["qM_inv"] @ (s["qfrc_in"] - g["qfrc_bias"][idx]), s["qacc"]) < IDENTITY_TOL
    assert any(n.endswith("r") for n in DD.names(tag))


def test_central_differences_of_a_known_function():
    f = lambda x: np.array([x[0] * x[1], np.sin(x[1]), x[0] ** 3])  # noqa: E731
    x = np.array([0.7, -0.4])
    want = np.array([[x[1], x[0]], [0.0, np.cos(x[1])], [3 * x[0] ** 2, 0.0]])
    assert np.abs(DD.central_differences(f, x, 1e-5) - want).max() < 1e-9
    assert np.abs(DD.richardson(f, x, 1e-3) - want).max() < 1e-11


def test_c_abi_declares_the_dynamics_derivatives():
    from rcs_amd import _lib

    text = open(os.path.join(HERE, "..", "include", "rcs_hip.h")).read()
    for name in ("rcsh_dynamics_derivatives", "rcsh_dynamics_derivatives_dev", "rcsh_env_dynamics_derivatives", "rcsh_env_dynamics_derivatives_dev"):
        assert re.search(r"^int\s+" + name + r"\s*\(rcsh_sim\*", text, re.M), name
        assert name in _lib.EXPORTS
    body = re.search(r"typedef struct rcsh_dynamics_grad_out \{(.*?)\} rcsh_dynamics_grad_out;", text, re.S).group(1)
    fields = re.findall(r"\bdouble\*\s+(\w+);", body)
    assert fields == list(DD.MATRICES)
    assert [f for f, _ in _lib.DynamicsGradOut._fields_] == fields
    assert re.search(r"^#define\s+RCSH_ABI_VERSION\s+2\s*$", text, re.M)


def test_want_is_validated_before_the_library_is_called():
    from rcs_amd import sim as S

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached: {name}")

    robot = S.SimRobot.__new__(S.SimRobot)  # no handle, no library: only the validation runs
    robot._L = robot.sim = NoLibrary()
    assert S.SimRobot.DYNAMICS_DERIVATIVES == DD.MATRICES
    with pytest.raises(ValueError, match="unknown dynamics derivative"):
        robot._dynamics_grad_want(("dqacc_dq", "dqM_dq"), None, None)
    with pytest.raises(ValueError, match="unknown dynamics derivative"):
        robot._dynamics_grad_want("qM", None, None)
    a = np.zeros(9)
    assert robot._dynamics_grad_want(None, None, None) == ("dqfrc_inverse_dqvel", "qM_inv")
    assert robot._dynamics_grad_want(None, a, None) == ("dqfrc_inverse_dq", "dqfrc_inverse_dqvel", "qM_inv")
    assert robot._dynamics_grad_want(None, a, a) == DD.MATRICES
    assert robot._dynamics_grad_want("qM_inv", None, None) == ("qM_inv",)
