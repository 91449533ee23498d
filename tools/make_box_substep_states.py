"""Harvest tests/golden/box_substep_states.json: states of the free box that take the substep's rare branches.

Replays the inputs of tests/parity_util.py: run_free_box_parity (seed 3 with 32 environments over 300 substeps, seed 9 with 5 over
150) on the CPU oracle substep by substep and records the state BEFORE every substep whose noslip pass ran 1, 3 or 5 sweeps or whose
Newton solve took >= 9 iterations.  A device handle's state writes do not write the warm start, so a recorded state is kept only if it
still takes its rare branch from a zero warm start on a fresh oracle, and only if the oracle's own spread on it
(tests/box_cases.py: spread) is within 1/100 of the bars.  About a dozen are kept, at least one per rare value.

    python tools/make_box_substep_states.py            # rewrites the golden file, prints what it found
"""

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("robot-control-stack_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import box_cases as B  # noqa: E402

SCENE = "fr3_simple_pick_up"
PER_VALUE = 3


def rollout_inputs(n_envs, seed):
    """The draws of run_free_box_parity(kick=True), in its order."""
    rng = np.random.default_rng(seed)
    qb = np.zeros((n_envs, 7))
    qb[:, 0] = 0.45 + rng.uniform(-0.1, 0.1, n_envs)
    qb[:, 1] = rng.uniform(-0.1, 0.1, n_envs)
    qb[:, 2] = rng.uniform(0.0144, 0.06, n_envs)
    qb[:, 3:] = rng.normal(size=(n_envs, 4)) * np.array([1.0, 0.15, 0.15, 1.0])
    qb[: n_envs // 4, 3:] = np.array([2 * rng.uniform(size=n_envs // 4) - 1, 0 * qb[: n_envs // 4, 0], 0 * qb[: n_envs // 4, 0], 1 + 0 * qb[: n_envs // 4, 0]]).T
    vb = np.zeros((n_envs, 6))
    vb[:, :3] = rng.uniform(-0.5, 0.5, (n_envs, 3))
    vb[:, 3:] = rng.uniform(-3, 3, (n_envs, 3))
    return qb, vb


def rare(rec):
    if rec["ncon"] and rec["noslip"] in (1, 3, 5):
        return f"noslip{rec['noslip']}"
    if rec["newton"] >= 9:
        return "newton9"
    return None


def main():
    orc = B.oracle(SCENE)
    found, counts = [], {}
    for n_envs, substeps, seed in ((32, 300, 3), (5, 150, 9)):
        qb, vb = rollout_inputs(n_envs, seed)
        for e in range(n_envs):
            orc.place(qb[e], vb[e])
            for k in range(substeps):
                pre = (orc.o.box_qpos, orc.o.box_qvel)
                tag = rare(orc.substep())
                if tag:
                    counts[tag] = counts.get(tag, 0) + 1
                    found.append(dict(rare=tag, seed=seed, env=e, substep=k, qpos=pre[0], qvel=pre[1]))
    print("rare substeps in the rollouts:", counts, "of", len(found))
    kept = {}
    for f in found:
        orc.place(f["qpos"], f["qvel"])
        if rare(orc.substep()) != f["rare"]:
            continue  # (took the branch only with the rollout's warm start)
        case = dict(name="", qpos=f["qpos"], qvel=f["qvel"])
        sp = B.spread(SCENE, case)
        if not (sp["same_branches"] and max(sp["ulp_vel"], sp["path_vel"]) <= B.SPREAD_VEL and max(sp["ulp_pose"], sp["path_pose"]) <= B.SPREAD_POSE):
            print("dropped (spread):", f["rare"], f["seed"], f["env"], f["substep"], sp)
            continue
        kept.setdefault(f["rare"], []).append(f)
    print("reproduce from a zero warm start within the spread cap:", {k: len(v) for k, v in kept.items()})
    states = []
    for tag in ("noslip1", "noslip3", "noslip5", "newton9"):
        rows = kept.get(tag, [])
        assert rows, f"no state left for {tag}"
        pick = [rows[i] for i in sorted({round(j * (len(rows) - 1) / max(PER_VALUE - 1, 1)) for j in range(PER_VALUE)})]
        for i, f in enumerate(pick):
            expect = {}
            for scene in B.SCENES:
                o2 = B.oracle(scene)
                o2.place(f["qpos"], f["qvel"])
                r = o2.substep()
                expect[scene] = dict(ncon=r["ncon"], zones=list(r["zones"]), newton=r["newton"], noslip=r["noslip"])
            states.append(dict(name=f"{tag}-{'abc'[i]}", rare=tag, seed=f["seed"], env=f["env"], substep=f["substep"],
                               qpos=[float(x).hex() for x in f["qpos"]], qvel=[float(x).hex() for x in f["qvel"]], expect=expect))
    doc = dict(source="tools/make_box_substep_states.py: pre-substep states of run_free_box_parity's rollouts on the CPU oracle (hex floats)", states=states)
    with open(B.GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    for s in states:
        print(s["name"], s["seed"], s["env"], s["substep"], s["expect"])


if __name__ == "__main__":
    main()
