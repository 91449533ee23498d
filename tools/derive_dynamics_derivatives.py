"""First-principles derivatives of the chain dynamics -> tests/golden/dynamics_derivatives.npz.

Ground truth for rcsh_dynamics_derivatives (csrc/dynamics_grad_team.h), independent of the library and of the oracle: the Lagrangian
derivation of tools/derive_fr3_dynamics.py (`Chain`, used as it stands), differentiated once more in mpmath.

For a golden sample (qpos, qvel) with qacc_in = the sample's qacc_smooth and qfrc_in = its qfrc_smooth:

  * dqfrc_inverse_dq [i][l] = d( M(q) qacc_in + bias(q, qvel) )_i / dq_l : central differences, step H, of Chain.mass_matrix and
    Chain.bias (which are nested central differences themselves: steps 1e-14 and h);
  * dqfrc_inverse_dqvel [i][l] = d bias_i / d qvel_l from the Christoffel symbols of M(q), no further differencing:
    sum_k (dM_il/dq_k - 1/2 dM_lk/dq_i) v_k + sum_j (dM_ij/dq_l - 1/2 dM_jl/dq_i) v_j;
  * qM_inv = M(q)^-1;  qacc = qM_inv (qfrc_in - bias);
  * dqacc_dq = -qM_inv (dM/dq_l qacc + d bias/dq_l),  dqacc_dqvel = -qM_inv dqfrc_inverse_dqvel;
  * beside them qacc and the bracket above (dqfrc_inverse_dq taken at qacc, "dqfrc_inverse_dq_at_qacc"), so that a reader of the file
    can check the last identity without differentiating anything.

Precision.  At DPS digits the round-off of M is 10^(14 - DPS), of dM/dq 10^(14 - DPS) / h, of the outer difference that over H; the
truncation is h^2 and H^2 times third derivatives.  The tool does not take this on trust: every matrix is evaluated TWICE, with
(H, h) = (1e-9, 1e-10) and (2e-9, 2e-10) -- four times the truncation error -- and the tool fails unless all agree to 1e-13 in the
measure max|a - b| / max(1, max|b|) (tests/dynamics_cases.rel_err).  The worst disagreement is printed and stored ("self_agreement").

Samples: the first four golden samples of each of the seven robots (even indices: velocities of order 1, odd: gentle), and sample 0 of
every robot once more at rest (qvel = 0, name "<index>r"), where the velocity derivative must vanish.

    python tools/derive_dynamics_derivatives.py        (about five minutes on 6 cores; DERIVE_JOBS sets the number of processes)
"""
import json
import multiprocessing
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import derive_fr3_dynamics as D  # noqa: E402
from derive_fr3_dynamics import Chain, mpf  # noqa: E402

DPS = 60
STEPS = ((mp.mpf(10) ** -9, mp.mpf(10) ** -10), (2 * mp.mpf(10) ** -9, 2 * mp.mpf(10) ** -10))  # (H outer, h inside Chain.bias)
AGREE = 1e-13
INDICES = (0, 1, 2, 3)
REFERENCE = {"fr3": ("fr3", ()), "fr3_arm": ("fr3", ("hand_0",)), "xarm7": ("xarm7", ())}
AUTHORED = {"ur5e": "ur5e_empty_world", "arm6": "arm6_empty_world", "so101": "so101_empty_world", "xarm7_pick": "xarm7_pick_world"}
TAGS = tuple(REFERENCE) + tuple(AUTHORED)
MATRICES = ("dqfrc_inverse_dq", "dqfrc_inverse_dqvel", "dqacc_dq", "dqacc_dqvel", "qM_inv")
EXTRAS = ("qacc", "dqfrc_inverse_dq_at_qacc")  # the solved acceleration and dqfrc_inverse_dq taken there: dqacc_dq = -qM_inv times it
GOLDEN = os.path.join(D.ROOT, "tests", "golden")


def load(tag):
    """(Chain, golden samples) of one robot: the model loading of derive_fr3_dynamics.main / main_authored."""
    if tag in REFERENCE:
        key, drop = REFERENCE[tag]
        chain = Chain(json.load(open(D.MODELS))[key], drop)
        samples = json.load(open(os.path.join(GOLDEN, f"{tag}_dynamics.json")))["samples"]
    else:
        from make_reference_model_fixture import read_robot

        chain = Chain(read_robot(os.path.join(D.ROOT, "robot-control-stack_amd", "rcs_amd", "scenes", AUTHORED[tag], "scene.xml")))
        samples = json.load(open(os.path.join(GOLDEN, "authored_scene_dynamics.json")))["models"][tag]["samples"]
    return chain, samples


def shifted(q, k, h):
    qp, qm = list(q), list(q)
    qp[k] += h
    qm[k] -= h
    return qp, qm


def derivatives(chain, q, v, a_in, f_in, H, h):
    nv = chain.nv
    vec = lambda x: mp.matrix(list(x))  # noqa: E731
    M = chain.mass_matrix(q)
    Minv = mp.inverse(M)
    bias = chain.bias(q, v, h)[0]
    qacc = Minv * (vec(f_in) - bias)
    # first derivatives of M at q: the Christoffel form of d bias / d qvel
    dM = []
    for k in range(nv):
        qp, qm = shifted(q, k, h)
        dM.append((chain.mass_matrix(qp) - chain.mass_matrix(qm)) / (2 * h))
    dbdv = mp.zeros(nv, nv)
    for i in range(nv):
        for l in range(nv):
            dbdv[i, l] = sum((dM[k][i, l] - dM[i][l, k] / 2) * v[k] + (dM[l][i, k] - dM[i][k, l] / 2) * v[k] for k in range(nv))
    # outer differences in q of M and of the bias
    did, dfd = mp.zeros(nv, nv), mp.zeros(nv, nv)
    for l in range(nv):
        qp, qm = shifted(q, l, H)
        dMl = (chain.mass_matrix(qp) - chain.mass_matrix(qm)) / (2 * H)
        dbl = (chain.bias(qp, v, h)[0] - chain.bias(qm, v, h)[0]) / (2 * H)
        ci, cf = dMl * vec(a_in) + dbl, dMl * qacc + dbl
        for i in range(nv):
            did[i, l], dfd[i, l] = ci[i], cf[i]
    out = {"dqfrc_inverse_dq": did, "dqfrc_inverse_dqvel": dbdv, "dqacc_dq": -(Minv * dfd), "dqacc_dqvel": -(Minv * dbdv), "qM_inv": Minv,
           "dqfrc_inverse_dq_at_qacc": dfd}
    res = {k: np.array([[float(m[i, j]) for j in range(nv)] for i in range(nv)]) for k, m in out.items()}
    res["qacc"] = np.array([float(x) for x in qacc])
    return res


_LOADED = {}


def job(args):
    tag, name, step = args
    mp.mp.dps = DPS
    if tag not in _LOADED:
        _LOADED[tag] = load(tag)
    chain, samples = _LOADED[tag]
    s = samples[int(name.rstrip("r"))]
    qvel = [0.0] * chain.nv if name.endswith("r") else s["qvel"]
    inputs = {"qpos": s["qpos"], "qvel": qvel, "qacc_in": s["qacc_smooth"], "qfrc_in": s["qfrc_smooth"]}
    H, h = STEPS[step]
    res = derivatives(chain, *[[mpf(x) for x in inputs[k]] for k in ("qpos", "qvel", "qacc_in", "qfrc_in")], H, h)
    return tag, name, step, inputs, res


def rel_err(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def main():
    names = [str(i) for i in INDICES] + ["0r"]
    only = [a for a in sys.argv[1:] if a in TAGS]
    jobs = [(tag, name, step) for tag in (only or TAGS) for name in names for step in range(len(STEPS))]
    jobs.sort(key=lambda j: -{"fr3": 9, "xarm7_pick": 9}.get(j[0], 7))  # the 9-dof chains first: they take longest
    done = {}
    with multiprocessing.Pool(min(len(jobs), int(os.environ.get("DERIVE_JOBS", "8")))) as pool:
        for tag, name, step, inputs, res in pool.imap_unordered(job, jobs):
            done[(tag, name, step)] = (inputs, res)
            print("done", tag, name, "step", step, flush=True)
    out, worst = {}, {k: 0.0 for k in MATRICES + EXTRAS}
    for tag in (only or TAGS):
        for name in names:
            (inputs, fine), (_, coarse) = done[(tag, name, 0)], done[(tag, name, 1)]
            for k, x in inputs.items():
                out[f"{tag}/{name}/{k}"] = np.asarray(x, dtype=np.float64)
            for k in MATRICES + EXTRAS:
                worst[k] = max(worst[k], rel_err(coarse[k], fine[k]))
                out[f"{tag}/{name}/{k}"] = fine[k]
    for k in MATRICES + EXTRAS:
        print(f"self-agreement {k:22s} {worst[k]:.3e}")
    agreement = max(worst.values())
    print(f"worst disagreement between the two step sizes: {agreement:.3e} (bar {AGREE:g})")
    assert agreement <= AGREE, agreement
    if only:
        return
    out["self_agreement"] = np.array(agreement)
    out["self_agreement_by_output"] = np.array([worst[k] for k in MATRICES + EXTRAS])
    path = os.path.join(GOLDEN, "dynamics_derivatives.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
