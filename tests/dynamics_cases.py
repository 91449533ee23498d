"""Ground truth for the dynamics queries (csrc/dynamics_team.h), independent of the library under test: numpy and the oracle only.

* the first-principles vectors of tests/golden/*_dynamics.json (tools/derive_fr3_dynamics.py: a 40-digit Lagrangian derivation), as
  arrays over the samples;
* the geometric Jacobian of the TCP, composed from the oracle's kinematics (orc_kinematics -> xaxis, xanchor, site_xpos, site_xmat) as
  tests/clearance_cases.py reads them: per hinge above the site axis x (point - anchor) and the axis, per slide the axis and zero,
  expressed in the frame of the chain's root body (the change of frame of ik_to_root_frame in oracle/rcs_pose_ik.c).  The TCP is the
  pose the oracle's ik_forward returns, site * offset^-1 (reference quirk Q7), the offset composed here in numpy.
"""

from __future__ import annotations

import ctypes as C
import functools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [os.path.join(ROOT, "oracle")]

REFERENCE_TAGS = ("fr3", "fr3_arm", "xarm7")
AUTHORED_TAGS = ("ur5e", "arm6", "so101", "xarm7_pick")
VECTORS = ("qpos", "qvel", "qM", "qfrc_bias", "coriolis", "gravity", "qfrc_gravcomp", "qfrc_passive", "qfrc_actuator", "qfrc_smooth",
           "qacc_smooth")


@functools.lru_cache(maxsize=None)
def samples(tag: str) -> dict:
    """The golden samples of one robot as arrays [n_samples, ...] (keys: VECTORS), plus "nv"."""
    if tag in REFERENCE_TAGS:
        g = json.load(open(os.path.join(HERE, "golden", f"{tag}_dynamics.json")))
    else:
        g = json.load(open(os.path.join(HERE, "golden", "authored_scene_dynamics.json")))["models"][tag]
    out = {k: np.array([s[k] for s in g["samples"]], dtype=np.float64) for k in VECTORS}
    out["nv"] = int(g["nv"])
    return out


def rel_err(got, want) -> float:
    """max|got - want| / max(1, max|want|): the measure of tests/test_dynamics_golden.py."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def quat_to_mat(q):
    """x y z w -> rotation matrix."""
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def franka_tcp7() -> np.ndarray:
    """The Franka hand's TCP offset as x y z qx qy qz qw (the oracle's own constant)."""
    import rcs_oracle as O

    p = O.franka_hand_tcp_offset()
    return np.concatenate([p.translation(), p.rotation_q()])


class TcpJacobian:
    """The TCP's geometric Jacobian of one compiled scene (rcs_amd.mjcf.Model), from the oracle's kinematics."""

    def __init__(self, cm, site: str = "attachment_site"):
        import rcs_oracle as O

        self.O, self.L = O, O.lib()
        self.model = O.make_model(cm, False)
        self.data = O.OrcData()
        A = cm.arrays
        self.nq = int(cm.njnt)
        self.site = cm.name2id("site", site)
        assert self.site >= 0, site
        self.parent = np.asarray(A["body_parentid"], dtype=np.int64)
        self.jbody = np.asarray(A["jnt_bodyid"], dtype=np.int64)
        self.jtype = np.asarray(A["jnt_type"], dtype=np.int64)
        self.site_body = int(np.asarray(A["site_bodyid"], dtype=np.int64)[self.site])
        chain, b = set(), self.site_body
        while b > 0:
            chain.add(b)
            b = int(self.parent[b])
        self.above = np.array([int(self.jbody[j]) in chain for j in range(self.nq)])
        root = self.site_body
        while root > 0 and self.parent[root] > 0:
            root = int(self.parent[root])
        self.root = root

    def jacobian(self, q, tcp7=None) -> np.ndarray:
        """[6, nq] at the configuration q [nq]: rows 0-2 d(position)/dq, rows 3-5 angular velocity per unit joint rate, root-body
        frame.  tcp7: x y z qx qy qz qw (None: the site itself)."""
        d = self.data
        for i, x in enumerate(np.asarray(q, dtype=np.float64)[: self.nq]):
            d.qpos[i] = float(x)
        self.L.orc_kinematics(C.byref(self.model), C.byref(d))
        sp = np.array(list(d.site_xpos[self.site]))
        sR = np.array(list(d.site_xmat[self.site])).reshape(3, 3)
        point = sp
        if tcp7 is not None:
            t = np.asarray(tcp7, dtype=np.float64)
            qn = t[3:] / np.linalg.norm(t[3:])
            point = sp + sR @ (-quat_to_mat(qn).T @ t[:3])  # the origin of site * offset^-1
        Rb = np.array(list(d.xmat[self.root])).reshape(3, 3) if self.root > 0 else np.eye(3)
        J = np.zeros((6, self.nq))
        for j in range(self.nq):
            if not self.above[j]:
                continue
            ax = np.array(list(d.xaxis[j]))
            if self.jtype[j] == 3:
                lin, ang = np.cross(ax, point - np.array(list(d.xanchor[j]))), ax
            else:
                lin, ang = ax, np.zeros(3)
            J[:3, j] = Rb.T @ lin
            J[3:, j] = Rb.T @ ang
        return J


def random_rows(cm, n: int, seed: int) -> np.ndarray:
    """n configurations drawn uniformly within the joint ranges of the compiled scene (unlimited joints: +-pi)."""
    A = cm.arrays
    nq = int(cm.njnt)
    rng = np.random.default_rng(seed)
    rg = np.asarray(A["jnt_range"], dtype=np.float64).reshape(-1, 2)[:nq]
    limited = np.asarray(A["jnt_limited"], dtype=np.int64)[:nq] != 0
    lo = np.where(limited, rg[:, 0], -np.pi)
    hi = np.where(limited, rg[:, 1], np.pi)
    return lo + (hi - lo) * rng.uniform(0.0, 1.0, size=(n, nq))
