"""Ground truth for the dynamics derivatives (csrc/dynamics_grad_team.h), independent of the library under test.

* tests/golden/dynamics_derivatives.npz (tools/derive_dynamics_derivatives.py: the 60-digit Lagrangian derivation of
  tools/derive_fr3_dynamics.py differentiated once more, every matrix evaluated at two step sizes that agree to `self_agreement`):
  per robot the golden samples named in `names(tag)`, each with its inputs and the five matrices;
* central differences in numpy, for a second opinion from any function of the state.
"""

from __future__ import annotations

import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "dynamics_derivatives.npz")
TAGS = ("fr3", "fr3_arm", "xarm7", "ur5e", "arm6", "so101", "xarm7_pick")
INPUTS = ("qpos", "qvel", "qacc_in", "qfrc_in")
MATRICES = ("dqfrc_inverse_dq", "dqfrc_inverse_dqvel", "dqacc_dq", "dqacc_dqvel", "qM_inv")
EXTRAS = ("qacc", "dqfrc_inverse_dq_at_qacc")  # the solved acceleration qM_inv (qfrc_in - qfrc_bias) and dqfrc_inverse_dq taken there


@functools.lru_cache(maxsize=None)
def _npz() -> dict:
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def self_agreement() -> float:
    """The worst disagreement between the tool's two step sizes, in the measure of dynamics_cases.rel_err."""
    return float(_npz()["self_agreement"])


def names(tag: str) -> tuple:
    """The samples of one robot: the index into the robot's golden samples, with a trailing "r" where the sample was evaluated at
    rest (qvel = 0)."""
    found = {k.split("/")[1] for k in _npz() if k.startswith(tag + "/")}
    return tuple(sorted(found, key=lambda n: (n.endswith("r"), int(n.rstrip("r")))))


def sample(tag: str, name: str) -> dict:
    """Inputs (INPUTS, [nv]), matrices (MATRICES, [nv, nv]) and EXTRAS of one sample."""
    z = _npz()
    return {k: z[f"{tag}/{name}/{k}"] for k in INPUTS + MATRICES + EXTRAS}


@functools.lru_cache(maxsize=None)
def stacked(tag: str) -> dict:
    """Every sample of one robot, stacked in the order of names(tag): inputs [n, nv], matrices [n, nv, nv].  Shared: do not modify."""
    rows = [sample(tag, n) for n in names(tag)]
    out = {k: np.stack([r[k] for r in rows]) for k in INPUTS + MATRICES + EXTRAS}
    for a in out.values():
        a.setflags(write=False)
    return out


def robot_cfg(tag: str):
    """The robot configuration (scene path in ``mjcf_scene_path``) the fixture's robot `tag` is simulated with: the scenes of
    tests/test_gpu_dynamics_query.py."""
    import parity_util as P
    from rcs_amd import envs as E

    if tag in ("fr3", "fr3_arm", "xarm7"):
        cfg = E.xarm7_sim_robot_cfg() if tag == "xarm7" else E.default_sim_robot_cfg("fr3_empty_world")
        path = {"fr3": lambda: P.SCENE, "fr3_arm": P.fr3_arm_only_scene, "xarm7": P.xarm7_frictionless_scene}[tag]()
        cfg.mjcf_scene_path = cfg.kinematic_model_path = path
        return cfg
    return {"ur5e": E.ur5e_sim_robot_cfg, "arm6": E.arm6_sim_robot_cfg, "so101": E.so101_sim_robot_cfg, "xarm7_pick": E.xarm7_pick_sim_robot_cfg}[tag]()


def central_differences(f, x, h: float) -> np.ndarray:
    """d f / d x by central differences of step h: f maps [n] to an array of any shape S; returns S + [n], the last axis the variable."""
    x = np.asarray(x, dtype=np.float64)
    cols = []
    for k in range(x.size):
        d = np.zeros_like(x)
        d[k] = h
        cols.append((np.asarray(f(x + d), dtype=np.float64) - np.asarray(f(x - d), dtype=np.float64)) / (2.0 * h))
    return np.stack(cols, axis=-1)


def richardson(f, x, h: float) -> np.ndarray:
    """Central differences extrapolated once (steps h and h / 2): the h^2 term cancels, the error is O(h^4) plus round-off."""
    return (4.0 * central_differences(f, x, h / 2) - central_differences(f, x, h)) / 3.0
