"""The swept clearance fixture (tests/golden/swept_clearance_cases.json, tools/make_swept_clearance_fixture.py) proven on the CPU: its
dense truth and contact entries are recomputed on a subset, its classes are populated, and the premise the kernel rests on -- a pair's
distance changes by at most L_p per unit of the segment's parameter -- holds on every row.  Nothing of the library is loaded."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import swept_clearance_cases as SC  # noqa: E402


@pytest.fixture(scope="module")
def F():
    return SC.load_fixture()


@pytest.fixture(scope="module")
def tables():
    return SC.host_tables()


def _sub(F, r):
    rec = F["scenes"][r["scene"]][str(r["kinds"])]
    return [tuple(p) for p, m in zip(rec["pairs"], rec["mask"]) if m]


def test_class_sizes(F):
    count = {c: 0 for c in SC.CLASSES}
    for r in F["rows"]:
        for c in r["classes"]:
            count[c] += 1
    assert all(v >= 3 for v in count.values()), count
    assert sum(bool(r["must_converge"]) for r in F["rows"]) >= 24
    per_scene = {s: sum(r["scene"] == s for r in F["rows"]) for s in SC.SCENES}
    assert per_scene["fr3_empty_world"] >= 40 and per_scene["fr3_simple_pick_up"] >= 12 and per_scene["xarm7_pick_world"] >= 6, per_scene
    assert len(F["rows"]) <= 80
    for r in F["rows"]:
        assert SC.leaves_stroke(SC.cpu_scene(r["scene"])[0], r["q_from"], r["q_to"]) == ("stroke" in r["classes"])
        if "contact" not in r["classes"]:
            assert abs(r["d_dense"]) >= 1e-6 and r["d_dense"] > 0  # (no row of the GPU test is skipped for being on the bar)
        if "beyond" in r["classes"]:
            assert r["d_max"] == 0.05 and r["d_dense"] > 0.05
        if "zero" in r["classes"]:
            assert r["q_from"] == r["q_to"]
        if "graze_floor" in r["classes"] or "graze_link" in r["classes"]:
            assert 2e-4 <= r["d_dense"] <= 2e-3 and 0.0 < r["s_dense"] < 1.0


def test_pairs_masks_and_lipschitz_constants(F, tables):
    """the lists and L_p of the fixture are what the host builders give today"""
    for name, per in F["scenes"].items():
        cm, sc, orc, home, dof = SC.cpu_scene(name)
        T = SC.Tables(cm, tables[name])
        for kinds, rec in per.items():
            assert [tuple(p) for p in rec["pairs"]] == T.pairs(int(kinds))
            assert rec["mask"] == [int(x) for x in SC.finger_mask(cm, T.pairs(int(kinds)), dof)]
    for r in F["rows"]:
        cm = SC.cpu_scene(r["scene"])[0]
        L = SC.Tables(cm, tables[r["scene"]]).lipschitz(r["kinds"], r["q_from"], r["q_to"])
        assert np.array_equal(L, np.array(r["L"]))
        if "zero" in r["classes"]:
            assert not L.any()
        if "fingers_only" in r["classes"] or "wrist_only" in r["classes"]:
            moved = np.flatnonzero(np.array(r["q_from"]) != np.array(r["q_to"]))
            dof = SC.cpu_scene(r["scene"])[4]
            assert len(moved) and ((moved >= dof).all() if "fingers_only" in r["classes"] else (len(moved) == 1 and moved[0] in (dof - 1, dof - 2)))
        if "rigid_pair" in r["classes"]:
            sub = _sub(F, r)
            Ls = L[np.array(F["scenes"][r["scene"]][str(r["kinds"])]["mask"], dtype=bool)]
            assert Ls[sub.index(tuple(r["pair_dense"]))] == 0.0 and L.any()


def test_premise_on_every_row(F):
    """|d_p(s_k+1) - d_p(s_k)| <= L_p / 256 + 1e-9 for every pair with finite truth at both samples: recorded by the generator for
    every row, recomputed here on a stretch of three rows"""
    for r in F["rows"]:
        assert r["premise_excess"] <= 1e-9, (r["classes"], r["premise_excess"])
    n = F["n_dense"]
    for r in [x for x in F["rows"] if "interior" in x["classes"]][:3]:
        sc = SC.cpu_scene(r["scene"])[1]
        sub = _sub(F, r)
        L = np.array(r["L"])[np.array(F["scenes"][r["scene"]][str(r["kinds"])]["mask"], dtype=bool)]
        k0 = int(round(r["s_dense"] * (n - 1)))
        ks = range(max(k0 - 4, 0), min(k0 + 5, n))
        per = np.array([SC.truth_at(sc, SC.config(r, k / (n - 1)), r["box"], sub)[2] for k in ks])
        both = np.isfinite(per[1:]) & np.isfinite(per[:-1])
        assert both.any()
        with np.errstate(invalid="ignore"):
            step = np.where(both, np.abs(per[1:] - per[:-1]), 0.0) - L[None, :] / (n - 1)
        assert step.max() <= 1e-9


def test_spot_checks(F):
    """d_dense recomputed around its sample on a subset; every contact row's entry bracket against the oracle's predicate"""
    n = F["n_dense"]
    picked = [r for r in F["rows"] if "contact" not in r["classes"]][::9]
    assert len(picked) >= 6
    for r in picked:
        sc = SC.cpu_scene(r["scene"])[1]
        sub = _sub(F, r)
        k0 = int(round(r["s_dense"] * (n - 1)))
        assert abs(k0 / (n - 1) - r["s_dense"]) < 1e-12
        d = {k: SC.truth_at(sc, SC.config(r, k / (n - 1)), r["box"], sub)[0] for k in (0, max(k0 - 1, 0), k0, min(k0 + 1, n - 1), n - 1)}
        assert abs(d[k0] - r["d_dense"]) <= 1e-12, (d[k0], r["d_dense"])
        assert min(d.values()) >= d[k0] - 1e-12
    import make_swept_clearance_fixture as M  # (tools/: the oracle's predicate over the selected pairs)

    for r in [x for x in F["rows"] if "contact" in x["classes"]]:
        lo, hi = r["s_enter"]
        assert 0.0 < lo < hi <= 1.0 and hi - lo <= 1e-7
        row = dict(r, q_from=np.array(r["q_from"]), q_to=np.array(r["q_to"]))
        assert not M.oracle_hit(row, lo) > 1e-9 and M.oracle_hit(row, hi) > 1e-9
        assert M.oracle_hit(row, min(1.0, hi + 1.0 / 64)) > 1e-4 and M.oracle_hit(row, 1.0) > 0.0
        assert not r["must_converge"]


def test_bracket_restated_on_a_row(F):
    """the numpy bracket that decides must_converge, rerun on one cheap row: the same count, a bound under the dense truth"""
    r = min((x for x in F["rows"] if x["must_converge"] and x["scene"] == "fr3_empty_world"), key=lambda x: x["restated_evals"])
    sc = SC.cpu_scene(r["scene"])[1]
    sub = _sub(F, r)
    L = np.array(r["L"])[np.array(F["scenes"][r["scene"]][str(r["kinds"])]["mask"], dtype=bool)]
    d_max = r["d_max"] or math.inf
    values = lambda s, best: SC.pair_values(sc, SC.config(r, s), r["box"], sub, min(best, d_max) + 0.05)  # noqa: E731
    best, s_best, lower, evals, ok = SC.bracket(values, L, 1e-3, d_max, budget=SC.SWEPT_BUDGET // 4)
    assert ok and evals == r["restated_evals"] and evals <= SC.SWEPT_BUDGET // 4
    assert lower <= r["d_dense"] + 1e-9 and best - lower <= 1e-3
