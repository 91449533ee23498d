#!/usr/bin/env python
"""Writes tests/golden/swept_clearance_cases.json: the rows of the swept clearance tests with their ground truth.

Everything here runs on the CPU and shares nothing with the library under test (tests/swept_clearance_cases.py: the numpy GJK over the
oracle's frames, the oracle's collision pass, the host table builders' pair list and levers).  Rows are chosen by a directed search, as
tools/make_certificate_cases.py chooses its cases: candidates of a family are classified by their dense truth, grazes and contact
entries are bisected onto their targets.  Minutes to run (a configuration's truth costs ~14 ms); the work is spread over processes."""
import json
import math
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import swept_clearance_cases as SC  # noqa: E402

GRID = np.linspace(0.0, 1.0, SC.N_DENSE)
_CTX = {}


def ctx(scene, kinds):
    """(ground-truth scene, oracle collider, tables, pairs, mask, selected pairs, home, dof) per process."""
    key = (scene, kinds)
    if key not in _CTX:
        if "tables" not in _CTX:
            _CTX["tables"] = SC.host_tables()
        cm, sc, orc, home, dof = SC.cpu_scene(scene)
        T = SC.Tables(cm, _CTX["tables"][scene])
        pairs = T.pairs(kinds)
        mask = SC.finger_mask(cm, pairs, dof)
        _CTX[key] = (sc, orc, T, pairs, mask, SC.selected_pairs(pairs, mask), home, dof, cm)
    return _CTX[key]


def sweep(row, n):
    """clearance and the attaining pair (index into the selected pairs) at n uniform samples"""
    sc, orc, T, pairs, mask, sub, *_ = ctx(row["scene"], row["kinds"])
    d, who = np.empty(n), np.empty(n, dtype=int)
    for k, s in enumerate(np.linspace(0.0, 1.0, n)):
        d[k], who[k], _ = SC.truth_at(sc, SC.config(row, float(s)), row["box"], sub)
    return d, who


def oracle_hit(row, s):
    sc, orc, T, pairs, mask, sub, *_ = ctx(row["scene"], row["kinds"])
    p, _ = orc.pairs(SC.config(row, s), row["box"])
    sel = {frozenset(x) for x in sub}
    depth = 0.0
    for k in range(3):
        if row["kinds"] >> k & 1:
            for pr, dp in p[k].items():
                if frozenset(pr) in sel:
                    depth = max(depth, dp)
    return depth


def finish(row):
    """The row's record: dense truth, L_p, the premise's worst step, s_enter for contact rows, must_converge.  None: rejected."""
    sc, orc, T, pairs, mask, sub, home, dof, cm = ctx(row["scene"], row["kinds"])
    L_all = T.lipschitz(row["kinds"], row["q_from"], row["q_to"])
    L = L_all[mask.astype(bool)]
    per = np.full((SC.N_DENSE, len(sub)), np.inf)
    d = np.empty(SC.N_DENSE)
    who = np.empty(SC.N_DENSE, dtype=int)
    for k, s in enumerate(GRID):
        d[k], who[k], per[k] = SC.truth_at(sc, SC.config(row, float(s)), row["box"], sub)
    contact = "contact" in row["classes"]
    if SC.leaves_stroke(cm, row["q_from"], row["q_to"]) != ("stroke" in row["classes"]):
        return None
    rec = dict(row)
    rec["L"] = [float(x) for x in L_all]
    if contact:
        hits = np.array([oracle_hit(row, float(s)) for s in GRID])
        first = int(np.argmax(hits > 1e-9))
        if not hits[first] > 1e-9 or first == 0 or (hits[first:] <= 0.0).any():
            return None
        lo, hi = float(GRID[first - 1]), float(GRID[first])
        if (hits[:first] > 0.0).any() or (d[:first] <= 1e-6).any():
            return None
        while hi - lo > 1e-7:
            m = 0.5 * (lo + hi)
            if oracle_hit(row, m) > 1e-9:
                hi = m
            else:
                lo = m
        rec["s_enter"] = [lo, hi]
        if not oracle_hit(row, min(1.0, hi + 1.0 / 64)) > 1e-4:
            return None
        d_before = d[:first]
        rec["d_dense"], rec["s_dense"] = float(d_before.min()), float(GRID[int(np.argmin(d_before))])
        rec["must_converge"] = False
    else:
        if (np.abs(d) < 1e-6).any() or (d <= 0).any():
            return None
        k = int(np.argmin(d))
        rec["d_dense"], rec["s_dense"] = float(d[k]), float(GRID[k])
        rec["pair_dense"] = [int(x) for x in sub[who[k]]]
        rec["s_enter"] = None
    # the premise: a pair's distance moves by at most L_p per unit of s
    both = np.isfinite(per[1:]) & np.isfinite(per[:-1]) & (per[1:] > 0) & (per[:-1] > 0)
    with np.errstate(invalid="ignore"):
        step = np.where(both, np.abs(per[1:] - per[:-1]), 0.0) - L[None, :] / (SC.N_DENSE - 1)
    if contact:
        step = step[: max(first - 1, 0)]
    rec["premise_excess"] = float(step.max()) if step.size else 0.0
    if not contact:
        stroke = "stroke" in row["classes"]
        if stroke:
            rec["must_converge"] = False
            rec["restated_evals"] = 0
        else:
            values = lambda s, best: SC.pair_values(sc, SC.config(row, s), row["box"], sub, min(best, row["d_max"] or math.inf) + 0.05)  # noqa: E731
            best, s_best, lower, evals, ok = SC.bracket(values, L, 1e-3, row["d_max"] or math.inf, budget=SC.SWEPT_BUDGET // 4)
            rec["must_converge"] = bool(ok and evals <= SC.SWEPT_BUDGET // 4)
            rec["restated_evals"] = int(evals)
            if not lower <= rec["d_dense"] + 1e-9:
                raise AssertionError(("the restated bracket's lower bound is above the dense truth", row, lower, rec["d_dense"]))
    return rec


def classify(row, d, who):
    """classes a free row falls into by its (coarse or dense) truth"""
    out = []
    k = int(np.argmin(d))
    n = len(d)
    if 0.02 * n < k < 0.98 * n and d[k] < min(d[0], d[-1]) - 1e-4:
        out.append("interior")
    elif k == 0 and d[-1] > d[0] + 1e-4:
        out.append("end0")
    elif k == n - 1 and d[0] > d[-1] + 1e-4:
        out.append("end1")
    mins = [i for i in range(1, n - 1) if d[i] < d[i - 1] and d[i] <= d[i + 1]]
    for i in mins:
        for j in mins:
            if i < j and who[i] != who[j] and abs(d[i] - d[j]) < 5e-3 and max(d[i], d[j]) < d[k] + 5e-3:
                if "two_minima" not in out:
                    out.append("two_minima")
    return out


def base_row(scene, kinds, qa, qb, box=None, d_max=None, classes=()):
    return dict(scene=scene, kinds=kinds, q_from=[float(x) for x in qa], q_to=[float(x) for x in qb], box=None if box is None else [float(x) for x in box],
                d_max=d_max, classes=list(classes))


def graze(scene, kinds, base, sweep_dir, approach, target, lo, hi):
    """The there-and-back segment base + a approach -+ sweep_dir whose smallest clearance is `target`: bisection on a in [lo (free), hi]."""
    def f(a):
        row = base_row(scene, kinds, base + a * approach - sweep_dir, base + a * approach + sweep_dir)
        d, who = sweep(row, 33)
        return float(d.min()), row
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        v, row = f(mid)
        if 0.5 * target < v < 1.6 * target:
            # (refine the minimum: the coarse sweep may have missed it)
            d, who = sweep(row, 129)
            if 2.2e-4 < d.min() < 1.9e-3 and 2 < int(np.argmin(d)) < 126:
                return row
            v = float(d.min())
        if v > target:
            lo = mid
        else:
            hi = mid
    return None


def candidates():
    """rows before their truth: (row, wanted classes or None for "whatever it turns out to be")"""
    rng = np.random.default_rng(20)
    out = []
    # ---- fr3_empty_world, kinds 3
    cm, sc, orc, home, dof = SC.cpu_scene("fr3_empty_world")
    full = lambda a, f=0.04: np.concatenate([a, [f, f]])  # noqa: E731
    lo, hi = cm.jnt_range[:dof, 0], cm.jnt_range[:dof, 1]
    def arm(scale=0.5):
        return np.clip(home + rng.uniform(-1, 1, dof) * scale * (hi - lo) / 2, lo + 0.05, hi - 0.05)
    for _ in range(40):  # random segments: interior / end minima, two minima
        a = arm()
        b = np.clip(a + rng.uniform(-0.8, 0.8, dof), lo, hi)
        out.append((base_row("fr3_empty_world", 3, full(a, rng.uniform(0, 0.04)), full(b, rng.uniform(0, 0.04))), None))
    for _ in range(4):
        a = full(arm(), rng.uniform(0, 0.04))
        out.append((base_row("fr3_empty_world", 3, a, a, classes=["zero"]), ["zero"]))
    for f0, f1 in ((0.0, 0.04), (0.04, 0.005), (0.01, 0.03), (0.035, 0.0)):
        a = arm(0.4)
        out.append((base_row("fr3_empty_world", 3, full(a, f0), full(a, f1), classes=["fingers_only"]), ["fingers_only"]))
    for k in range(6):
        a = arm(0.6)
        b = a.copy()
        j = 6 if k % 2 == 0 else 5
        b[j] = np.clip(a[j] + rng.choice([-1, 1]) * rng.uniform(0.8, 1.6), lo[j], hi[j])
        out.append((base_row("fr3_empty_world", 3, full(a), full(b), classes=["wrist_only"]), ["wrist_only"]))
    for _ in range(12):  # far from everything: the floor alone (kinds 1) and a d_max of 5 cm
        a = np.clip(home + rng.uniform(-0.3, 0.3, dof), lo, hi)
        b = np.clip(a + rng.uniform(-0.3, 0.3, dof), lo, hi)
        out.append((base_row("fr3_empty_world", 1, full(a), full(b), d_max=0.05, classes=["beyond"]), ["beyond"]))
    for f0, f1 in ((0.02, 0.05), (0.03, 0.06), (0.0, 0.045), (0.045, 0.01)):
        a = arm(0.3)
        b = np.clip(a + rng.uniform(-0.2, 0.2, dof), lo, hi)
        out.append((base_row("fr3_empty_world", 3, full(a, f0), full(b, f1), classes=["stroke"]), ["stroke"]))
    # ---- fr3_simple_pick_up, kinds 4 and 7: a cube near the hand
    cm2, sc2, orc2, home2, dof2 = SC.cpu_scene("fr3_simple_pick_up")
    from test_gpu_clearance import _boxes_near_hand
    for k in range(70):
        a = np.concatenate([home2 + rng.uniform(-0.3, 0.3, dof2), [rng.uniform(0, 0.04)] * 2])
        b = a.copy()
        b[:dof2] += rng.uniform(-0.4, 0.4, dof2)
        mid = (0.5 * (a + b))[None, :]
        box = _boxes_near_hand(orc2, cm2, mid, rng, 0.22)[0]
        out.append((base_row("fr3_simple_pick_up", 4 if k % 2 else 7, a, b, box=box), None))
    # ---- xarm7_pick_world, kinds 3
    cm3, sc3, orc3, home3, dof3 = SC.cpu_scene("xarm7_pick_world")
    lo3, hi3 = cm3.jnt_range[:dof3, 0], cm3.jnt_range[:dof3, 1]
    nl3 = int(cm3.nq)
    for _ in range(20):
        a = np.clip(home3 + rng.uniform(-0.6, 0.6, dof3), lo3, hi3)
        b = np.clip(a + rng.uniform(-0.6, 0.6, dof3), lo3, hi3)
        f = rng.uniform(0.0, 0.04)
        out.append((base_row("xarm7_pick_world", 3, np.concatenate([a, [f] * (nl3 - dof3)]), np.concatenate([b, [f] * (nl3 - dof3)])), None))
    return out


def directed():
    """grazes and contact entries of fr3_empty_world: scans against the oracle, then bisection"""
    cm, sc, orc, home, dof = SC.cpu_scene("fr3_empty_world")
    base = np.concatenate([home, [0.04, 0.04]])
    e = lambda j: np.eye(len(base))[j]  # noqa: E731
    rows = []
    # the arm towards the floor: shoulder forward (joint 2), the elbow (joint 4) swings the hand through its lowest point
    for q4, sw in ((-0.6, 0.25), (-0.9, 0.3), (-0.4, 0.2), (-1.2, 0.3)):
        b = base.copy()
        b[3] = q4
        rows.append((dict(graze=("fr3_empty_world", 3, b, sw * e(5), e(1), (3e-4, 8e-4, 1.5e-3), 0.0, 1.76 - b[1])), ["graze_floor"]))
    # the hand folded back against links 1 and 2: joint 4 folds it in, a wrist joint swings it past them
    for q2, q6 in ((0.0, 1.5), (0.0, 1.2), (0.0, 1.8), (0.3, 1.5), (-0.3, 1.5), (0.0, 1.0), (0.2, 1.3), (-0.2, 1.7)):
        b = base.copy()
        b[1], b[3], b[5] = q2, -2.7, q6
        for sw in (0.3 * e(5), 0.3 * e(4), 0.4 * e(6)):
            rows.append((dict(graze=("fr3_empty_world", 3, b, sw, -e(3), (4e-4, 1e-3), 0.0, 0.37)), ["graze_link"]))
    # contact rows: from a free configuration straight into a penetration
    for q2 in (1.3, 1.4, 1.5, 1.6, 1.7, 1.75):
        a, b = base.copy(), base.copy()
        a[1], a[3] = 0.4, -0.5
        b[1], b[3] = q2, -0.3
        rows.append((base_row("fr3_empty_world", 3, a, b, classes=["contact"]), ["contact"]))
    for q2, q6 in ((0.0, 1.5), (0.0, 1.2), (0.0, 1.8), (0.3, 1.5), (-0.3, 1.5), (0.0, 1.0)):
        a, b = base.copy(), base.copy()
        a[1], a[3], a[5] = q2, -2.6, q6
        b[1], b[3], b[5] = q2, -3.07, q6 + 0.1
        rows.append((base_row("fr3_empty_world", 3, a, b, classes=["contact"]), ["contact"]))
    return rows


def work(item):
    row, wanted = item
    try:
        if "graze" in row:
            scene, kinds, b, sw, ap, targets, lo, hi = row["graze"]
            row = None
            for target in targets:
                row = graze(scene, kinds, b, sw, ap, target, lo, hi)
                if row is not None:
                    break
            if row is None:
                return None
            row["classes"] = list(wanted)
        if wanted is None or wanted == ["beyond"] or wanted == ["wrist_only"] or wanted == ["fingers_only"]:
            d, who = sweep(row, 33)
            if (d < 2e-4).any():
                return None
            if wanted == ["beyond"] and d.min() < 0.06:
                return None
        rec = finish(row)
        if rec is None:
            return None
        if "contact" not in rec["classes"]:
            sc, orc, T, pairs, mask, sub, *_ = ctx(row["scene"], row["kinds"])
            d, who = sweep(row, 65)
            extra = classify(row, d, who) if "zero" not in rec["classes"] and "beyond" not in rec["classes"] else []
            L = np.asarray(rec["L"])[mask.astype(bool)]
            if rec.get("pair_dense") and "beyond" not in rec["classes"]:
                i = sub.index(tuple(rec["pair_dense"]))
                if L[i] == 0.0 and "zero" not in rec["classes"]:
                    extra.append("rigid_pair")
            rec["classes"] = sorted(set(rec["classes"]) | set(extra))
        return rec
    except AssertionError:
        raise
    except Exception as exc:  # a candidate the truth cannot handle is no row
        print("rejected:", repr(exc), file=sys.stderr)
        return None


def main():
    want = {"fr3_empty_world": 48, "fr3_simple_pick_up": 16, "xarm7_pick_world": 8}
    items = directed() + candidates()
    with mp.Pool(min(8, os.cpu_count() or 1)) as pool:
        recs = [r for r in pool.map(work, items, chunksize=1) if r is not None]
    # keep every directed or special row, then fill each scene with the random ones, those of the rarest classes first
    count = {c: 0 for c in SC.CLASSES}
    rows = []
    special = [r for r in recs if set(r["classes"]) & {"zero", "fingers_only", "wrist_only", "beyond", "stroke", "graze_floor", "graze_link", "contact",
                                                       "two_minima", "rigid_pair"}]
    rest = [r for r in recs if r not in special]
    per_scene = {s: 0 for s in want}
    cap = {"beyond": 4, "contact": 8, "zero": 3, "stroke": 3, "fingers_only": 4, "wrist_only": 5, "graze_floor": 3, "graze_link": 3}
    for r in special + rest:
        s = r["scene"]
        if per_scene[s] >= want[s]:
            continue
        over = [c for c in r["classes"] if c in cap and count[c] >= cap[c]]
        if over and not any(count[c] < 3 for c in r["classes"]):
            continue
        rows.append(r)
        per_scene[s] += 1
        for c in r["classes"]:
            count[c] += 1
    T = SC.host_tables()
    scenes = {}
    for s in want:
        cm, sc, orc, home, dof = SC.cpu_scene(s)
        tb = SC.Tables(cm, T[s])
        scenes[s] = {str(k): {"pairs": tb.pairs(k), "mask": [int(x) for x in SC.finger_mask(cm, tb.pairs(k), dof)]} for k in (1, 3, 4, 7)}
    out = {"n_dense": SC.N_DENSE, "scenes": scenes, "rows": rows, "class_counts": count}
    os.makedirs(os.path.dirname(SC.FIXTURE), exist_ok=True)
    with open(SC.FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(json.dumps(count), per_scene, "must_converge:", sum(bool(r["must_converge"]) for r in rows), "bytes:", os.path.getsize(SC.FIXTURE))


if __name__ == "__main__":
    main()
