"""Ground truth for the operational-space queries (csrc/opspace_team.h), independent of the library under test.

tests/golden/opspace.npz (tools/derive_opspace.py: the 60-digit Lagrangian derivation of tools/derive_fr3_dynamics.py, the TCP's
Jacobian and acceleration by differences of its forward kinematics, every sample evaluated at two step sizes that agree to
`self_agreement`): per robot the samples named in `names(tag)`, each with its inputs, its options (task_mask, damping, tcp_offset), the
eight outputs, the expected status, cond(A) in the 2-norm and the smallest relative pivot of A's L D L^T.
"""

from __future__ import annotations

import functools
import os

import numpy as np

from dynamics_derivative_cases import TAGS, robot_cfg  # noqa: F401  (the same seven robots and scenes)

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "opspace.npz")
INPUTS = ("qpos", "qvel", "xacc_des", "qfrc_null")
ALWAYS = ("twist", "jdot_qvel", "lambda_inv")  # defined whatever the status
FAMILY = ("lambda", "jbar", "op_bias", "null_proj", "qfrc")  # NaN in a status-1 row
OUTPUTS = ALWAYS + FAMILY
EXTRAS = ("jac", "qM_inv")  # the masked Jacobian [6, nv] and the chain's M^-1 [nv, nv] the outputs were formed from
RECORDS = ("status", "cond", "rel_pivot", "task_mask", "damping")
COND_CAP, PIVOT_CAP, SINGULAR_CAP = 1e6, 1e-6, 1e-30


@functools.lru_cache(maxsize=None)
def _npz() -> dict:
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def self_agreement() -> float:
    """The worst disagreement between the tool's two step sizes, in the measure of dynamics_cases.rel_err."""
    return float(_npz()["self_agreement"])


def names(tag: str) -> tuple:
    """The samples of one robot: the index into the robot's golden samples, then a letter for a variant ("r": at rest, "t": with a
    tcp_offset, "m": task_mask 0x07, "f": so101 with the full mask, "s" / "d": the UR5e wrist singularity without and with damping)."""
    found = {k.split("/")[1] for k in _npz() if k.startswith(tag + "/")}
    return tuple(sorted(found, key=lambda n: (n[-1].isalpha(), n[-1] if n[-1].isalpha() else "", int(n.rstrip("rtmfsd")))))


def sample(tag: str, name: str) -> dict:
    """Inputs, OUTPUTS, EXTRAS and RECORDS of one sample; "tcp_offset" is x y z qx qy qz qw or None (the site itself)."""
    z = _npz()
    out = {k: z[f"{tag}/{name}/{k}"] for k in INPUTS + OUTPUTS + EXTRAS + RECORDS}
    out["tcp_offset"] = z.get(f"{tag}/{name}/tcp_offset")
    return out


@functools.lru_cache(maxsize=None)
def calls(tag: str) -> tuple:
    """The samples of one robot grouped by what one call shares -- (task_mask, damping, tcp_offset) --: a tuple of
    (options dict, names, stacked arrays: inputs [n, ...], OUTPUTS [n, ...], status / cond / rel_pivot [n]).  Shared: do not modify."""
    groups = {}
    for n in names(tag):
        s = sample(tag, n)
        key = (int(s["task_mask"]), float(s["damping"]), None if s["tcp_offset"] is None else tuple(s["tcp_offset"]))
        groups.setdefault(key, []).append((n, s))
    out = []
    for (mask, damping, tcp), members in groups.items():
        arrays = {k: np.stack([s[k] for _, s in members]) for k in INPUTS + OUTPUTS + EXTRAS + ("status", "cond", "rel_pivot")}
        for a in arrays.values():
            a.setflags(write=False)
        opts = {"task_mask": mask, "damping": damping, "tcp_offset": None if tcp is None else np.array(tcp)}
        out.append((opts, tuple(n for n, _ in members), arrays))
    return tuple(out)


def selection(mask: int) -> np.ndarray:
    """I_sel as a [6] vector of zeros and ones."""
    return np.array([(mask >> r) & 1 for r in range(6)], dtype=np.float64)
