"""Batched swept clearance (SimRobot.swept_clearance / VecSimEnv.swept_clearance, csrc/swept_team.h) against a ground truth that shares
nothing with the library: the rows and dense truth of tests/golden/swept_clearance_cases.json (tools/make_swept_clearance_fixture.py),
the numpy GJK over the oracle's frames at the reported configuration, and the oracle's collision pass for the rows in contact.

Every bound of the bracket tests follows from the query's definitions: no measured tolerance is involved.  Each test prints its worst
figures before it asserts (profiles/swept_clearance/tests.txt is this output)."""

import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "robot-control-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import swept_clearance_cases as SC  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9
BAND = 1e-7  # test_in_contact's bar for the oracle's depth
BRACKETED, BEYOND, CONTACT, OPEN = 0, 1, 2, 3
RES = 1e-4
OUTPUTS = ("distance", "lower", "s", "pair", "witness", "grad", "evals", "status")


def scene(name):
    from test_gpu_clearance import scene as _scene

    return _scene(name)  # (simu, robot, oracle collider, compiled scene, home, ground-truth scene), built once per session


@pytest.fixture(scope="module")
def fx():
    F = SC.load_fixture()
    for r in F["rows"]:
        r["q_from"], r["q_to"] = np.array(r["q_from"]), np.array(r["q_to"])
        r["box"] = None if r["box"] is None else np.array(r["box"])
        r["d_max"] = math.inf if r["d_max"] is None else float(r["d_max"])
    # the pair lists the truth was made with are the library's
    for name, per in F["scenes"].items():
        robot = scene(name)[1]
        for kinds, rec in per.items():
            if int(kinds) & 4 and scene(name)[5].box_size is None:
                continue
            assert [tuple(p) for p in rec["pairs"]] == [(int(a), int(b)) for a, b in robot.clearance_pairs(int(kinds))], (name, kinds)
            assert np.array_equal(np.array(rec["mask"], dtype=np.uint8), robot.clearance_mask(int(kinds))), (name, kinds)
    return F


def groups(rows):
    """rows that share one call: {(scene, kinds, d_max): [row indices]}"""
    out = {}
    for i, r in enumerate(rows):
        out.setdefault((r["scene"], r["kinds"], r["d_max"]), []).append(i)
    return out


def run(F, tolerance, resolution=RES, rows=None, mask_of=None):
    """the query on the fixture's rows (or a subset), one call per group; a list of per-row dicts in the rows' order"""
    rows = F["rows"] if rows is None else rows
    out = [None] * len(rows)
    for (name, kinds, d_max), idx in groups(rows).items():
        robot = scene(name)[1]
        mask = np.array(F["scenes"][name][str(kinds)]["mask"], dtype=np.uint8) if mask_of is None else mask_of(name, kinds)
        a, b = np.array([rows[i]["q_from"] for i in idx]), np.array([rows[i]["q_to"] for i in idx])
        boxes = np.array([rows[i]["box"] for i in idx]) if rows[idx[0]]["box"] is not None else None
        res = robot.swept_clearance(a, b, tolerance=tolerance, resolution=resolution, d_max=d_max, free_qpos=boxes, kinds=kinds, pair_mask=mask)
        for k, i in enumerate(idx):
            out[i] = {key: res[key][k] for key in res}
    return out


@pytest.fixture(scope="module")
def answers(fx):
    return {tol: run(fx, tol) for tol in (1e-3, 1e-4)}


def sub_pairs(F, r):
    rec = F["scenes"][r["scene"]][str(r["kinds"])]
    return [tuple(p) for p, m in zip(rec["pairs"], rec["mask"]) if m]


def check_bracket(r, a, tolerance, d_true):
    assert a["lower"] <= d_true + TOL, (r["classes"], a, d_true)
    assert a["lower"] <= a["distance"]
    if a["status"] == BRACKETED:
        assert a["distance"] <= d_true + tolerance + TOL, (r["classes"], a, d_true)
    assert (a["status"] == BRACKETED) == (a["distance"] - a["lower"] <= tolerance), (r["classes"], a)


# ---- 1 (and 11: the xarm7_pick_world rows are rows of the fixture)
@pytest.mark.parametrize("tolerance", [1e-3, 1e-4])
def test_bracket(fx, answers, tolerance):
    hist, width, compared = np.zeros(4, dtype=int), 0.0, 0
    evals = []
    for r, a in zip(fx["rows"], answers[tolerance]):
        hist[a["status"]] += 1
        evals.append(int(a["evals"]))
        if "contact" in r["classes"] or "beyond" in r["classes"] or "stroke" in r["classes"]:
            continue
        assert a["status"] in (BRACKETED, OPEN), (r["classes"], a)
        compared += 1
        width = max(width, a["distance"] - a["lower"])
    print(f"test_bracket tol={tolerance}: status histogram {hist.tolist()}, worst bracket width {width:.3e}, evals mean {np.mean(evals):.1f} max {max(evals)}, rows {compared}")
    for r, a in zip(fx["rows"], answers[tolerance]):
        if "contact" in r["classes"] or "beyond" in r["classes"]:
            continue
        if "stroke" in r["classes"]:
            assert a["status"] == OPEN and a["lower"] == -math.inf, a
            continue
        check_bracket(r, a, tolerance, r["d_dense"])
        if tolerance == 1e-3 and r["must_converge"]:
            assert a["status"] == BRACKETED, (r["classes"], r["restated_evals"], a)
        assert a["evals"] <= SC.SWEPT_BUDGET
    assert compared >= 50


# ---- 2
@pytest.mark.parametrize("tolerance", [1e-3, 1e-4])
def test_attained_value(fx, answers, tolerance):
    worst = dict(distance=0.0, witness=0.0, grad=0.0)
    seen = 0
    fails = []
    for r, a in zip(fx["rows"], answers[tolerance]):
        if a["status"] in (BEYOND, CONTACT) or a["s"] < 0:
            continue
        sc = scene(r["scene"])[5]
        sub = sub_pairs(fx, r)
        assert 0.0 <= a["s"] <= 1.0
        q = SC.config(r, float(a["s"]))
        t, i, dd = SC.truth_at(sc, q, r["box"], sub)
        fr = sc.frames(q, r["box"])
        g0, g1 = int(a["pair"][0]), int(a["pair"][1])
        assert (g0, g1) in sub, (r["classes"], g0, g1)
        e_d = max(abs(a["distance"] - t), abs(sc.pair_distance(fr, g0, g1)[0] - t))
        wa, wb = a["witness"][:3], a["witness"][3:]
        e_w = max(sc.witness_error(fr, g0, wa), sc.witness_error(fr, g1, wb))
        radii = sum(sc.radius[g] for g in (g0, g1) if g != sc.plane_geom)
        e_w = max(e_w, abs(np.linalg.norm(wb - wa) - radii - a["distance"]))
        n = (wb - wa) / np.linalg.norm(wb - wa)
        g = sc.gradient(fr, g0, g1, wa, wb, n)
        e_g = np.abs(g - a["grad"]).max() / max(1.0, np.abs(g).max())
        worst = dict(distance=max(worst["distance"], e_d), witness=max(worst["witness"], e_w), grad=max(worst["grad"], e_g))
        seen += 1
        if not (e_d <= TOL and e_w <= TOL and e_g <= TOL):
            fails.append((r["classes"], a, t, e_d, e_w, e_g))
        if "zero" in r["classes"]:
            assert a["s"] == 0.0
    print(f"test_attained_value tol={tolerance}: rows {seen}, worst |distance - truth| {worst['distance']:.3e}, witness {worst['witness']:.3e}, grad {worst['grad']:.3e}")
    assert not fails, fails[:3]
    assert seen >= 50


# ---- 3
def test_contact_rows(fx, answers):
    seen = 0
    for tolerance in (1e-3, 1e-4):
        for r, a in zip(fx["rows"], answers[tolerance]):
            if "contact" not in r["classes"]:
                continue
            orc = scene(r["scene"])[2]
            maxtravel = float(np.abs(r["q_to"] - r["q_from"]).max())
            lo, hi = r["s_enter"]
            print(f"test_contact_rows tol={tolerance}: s {a['s']:.9f} s_enter [{lo:.9f}, {hi:.9f}] distance {a['distance']:.3e} evals {a['evals']}")
            assert a["status"] == CONTACT, a
            assert a["lower"] == -math.inf
            assert lo - 1e-7 <= a["s"] <= hi + RES / maxtravel + 1e-7, (a["s"], lo, hi, RES / maxtravel)
            p, near = orc.pairs(SC.config(r, float(a["s"])), r["box"])
            hits = {frozenset(k): v for kk in range(3) if r["kinds"] >> kk & 1 for k, v in p[kk].items()}
            assert frozenset(int(x) for x in a["pair"]) in hits, (a["pair"], hits)
            assert abs(-a["distance"] - max(hits.values())) <= BAND, (a["distance"], hits)
            assert a["evals"] <= SC.SWEPT_BUDGET + SC.SWEPT_CONTACT_BUDGET
            seen += 1
    assert seen >= 6


# ---- 4
def test_consistent_with_the_motion_query(fx, answers):
    rows = fx["rows"]
    counts = np.zeros((4, 3), dtype=int)
    for (name, kinds, d_max), idx in groups(rows).items():
        if d_max != math.inf:
            continue
        robot = scene(name)[1]
        a, b = np.array([rows[i]["q_from"] for i in idx]), np.array([rows[i]["q_to"] for i in idx])
        boxes = np.array([rows[i]["box"] for i in idx]) if rows[idx[0]]["box"] is not None else None
        # (the motion query has no mask: the swept query is asked with every pair, as the motion query tests them)
        res, tc = robot.check_motion(a, b, resolution=RES, free_qpos=boxes, kinds=kinds)
        sw = robot.swept_clearance(a, b, tolerance=1e-3, resolution=RES, free_qpos=boxes, kinds=kinds)
        for k in range(len(idx)):
            counts[sw["status"][k], res[k]] += 1
            if sw["status"][k] == CONTACT:
                assert res[k] != 0, (rows[idx[k]]["classes"], res[k], tc[k], {key: sw[key][k] for key in sw})
            if sw["lower"][k] > 0:
                assert res[k] != 1, (rows[idx[k]]["classes"], res[k], tc[k])
            if res[k] == 0:
                assert sw["status"][k] != CONTACT
    print("test_consistent_with_the_motion_query: swept status x motion result\n", counts)
    assert counts[CONTACT].sum() >= 3 and counts[:, 0].sum() >= 3


# ---- 5
def test_d_max(fx, answers):
    seen = 0
    for r, a in zip(fx["rows"], answers[1e-3]):
        if "beyond" not in r["classes"]:
            continue
        assert r["d_dense"] > r["d_max"] + TOL
        assert a["status"] == BEYOND and a["distance"] == r["d_max"] and a["lower"] == r["d_max"] and a["s"] == -1.0, a
        assert tuple(a["pair"]) == (-1, -1) and not a["witness"].any() and not a["grad"].any()
        seen += 1
    assert seen >= 3
    # rows on either side of a d_max taken from their own truth; within 1e-9 of it a row may fall either way
    rows = [r for r in fx["rows"] if r["scene"] == "fr3_empty_world" and r["kinds"] == 3 and not set(r["classes"]) & {"contact", "stroke"}]
    d_max = float(np.median([r["d_dense"] for r in rows]))
    cut = [dict(r, d_max=d_max) for r in rows]
    below = above = 0
    for r, a in zip(cut, run(fx, 1e-3, rows=cut)):
        if abs(r["d_dense"] - d_max) <= TOL:
            continue
        assert a["lower"] <= min(r["d_dense"], d_max) + TOL
        if r["d_dense"] > d_max:
            # (the dense samples are not the whole segment: the truth may dip under d_max between them, never the bound over it)
            assert a["status"] in (BEYOND, BRACKETED, OPEN)
            above += a["status"] == BEYOND
        else:
            assert a["status"] in (BRACKETED, OPEN) and a["distance"] < d_max, a
            check_bracket(r, a, 1e-3, r["d_dense"])
            below += 1
    assert below >= 5 and above >= 5, (below, above)


# ---- 6
def test_pair_mask(fx, answers):
    rows = [r for r, a in zip(fx["rows"], answers[1e-3]) if r["scene"] == "fr3_empty_world" and r["kinds"] == 3 and a["status"] == BRACKETED
            and set(r["classes"]) & {"interior", "end0", "end1"}][:4]
    assert len(rows) == 4
    base = [a for r, a in zip(fx["rows"], answers[1e-3]) if any(r is x for x in rows)]
    simu, robot, orc, cm, home, sc = scene("fr3_empty_world")
    rec = fx["scenes"]["fr3_empty_world"]["3"]
    pairs = [tuple(p) for p in rec["pairs"]]
    for r, a0 in zip(rows, base):
        win = (int(a0["pair"][0]), int(a0["pair"][1]))
        mask = np.array(rec["mask"], dtype=np.uint8)
        mask[pairs.index(win)] = 0
        sub = SC.selected_pairs(pairs, mask)
        d65 = min(SC.truth_at(sc, SC.config(r, float(s)), None, sub)[0] for s in np.linspace(0, 1, 65))
        a = run(fx, 1e-3, rows=[r], mask_of=lambda n, k: mask)[0]
        print(f"test_pair_mask: winner {win} masked: distance {a0['distance']:.6f} -> {a['distance']:.6f}, truth over 65 samples {d65:.6f}, status {a['status']}")
        assert tuple(a["pair"]) != win
        check_bracket(r, a, 1e-3, d65)
        assert a["distance"] >= a0["distance"] - 1e-3 - TOL


def _same(x, y):
    return all(np.array_equal(x[k], y[k]) for k in OUTPUTS)


def _call(robot, rows, F, **kw):
    r0 = rows[0]
    mask = np.array(F["scenes"][r0["scene"]][str(r0["kinds"])]["mask"], dtype=np.uint8)
    return robot.swept_clearance(np.array([r["q_from"] for r in rows]), np.array([r["q_to"] for r in rows]), tolerance=1e-3, resolution=RES, kinds=r0["kinds"],
                                 pair_mask=mask, **kw)


# ---- 7
def test_own_inputs_only(fx):
    from test_gpu_clearance import _Dev

    rows = [r for r in fx["rows"] if r["scene"] == "fr3_empty_world" and r["kinds"] == 3 and r["d_max"] == math.inf]
    simu, robot = scene("fr3_empty_world")[:2]
    ref = _call(robot, rows, fx)
    m = len(rows)
    perm = np.random.default_rng(5).permutation(m)
    got = _call(robot, [rows[i] for i in perm], fx)
    for k in OUTPUTS:
        assert np.array_equal(got[k], ref[k][perm]), k
    for i in (0, m // 2, m - 1):
        one = _call(robot, [rows[i]], fx)
        for k in OUTPUTS:
            assert np.array_equal(one[k][0], ref[k][i]), (k, i)
    five = _call(robot, rows[3:8], fx)
    for k in OUTPUTS:
        assert np.array_equal(five[k], ref[k][3:8]), k
    rng = np.random.default_rng(6)
    pad = []
    for _ in range(67 - m):
        a = np.concatenate([rng.uniform(-1.5, 1.5, 7), [0.02, 0.02]])
        pad.append(dict(rows[0], q_from=a, q_to=a + rng.uniform(-0.5, 0.5, 9) * np.array([1] * 7 + [0, 0])))
    where = np.sort(rng.choice(67, m, replace=False))
    mixed = [None] * 67
    for i, w in enumerate(where):
        mixed[w] = rows[i]
    it = iter(pad)
    mixed = [x if x is not None else next(it) for x in mixed]
    big = _call(robot, mixed, fx)
    for k in OUTPUTS:
        assert np.array_equal(big[k][where], ref[k]), k
    # the _dev form: the same bits
    D = _Dev(simu)
    a, b = np.array([r["q_from"] for r in rows]), np.array([r["q_to"] for r in rows])
    mask = np.array(fx["scenes"]["fr3_empty_world"]["3"]["mask"], dtype=np.uint8)
    arrays, _ = robot._swept_buffers(m, a.shape[1])
    dev = {k: D.alloc(v.nbytes) for k, v in arrays.items()}
    out = D.lib.SweptOut(**{k: p.value for k, p in dev.items()})
    D.lib.check(D.L.rcsh_swept_clearance_dev(D.h, D.up(a), D.up(b), None, m, 3, D.up(mask), math.inf, 1e-3, RES, C.byref(out)))
    simu.synchronize()
    for k, v in arrays.items():
        D.down(dev[k], v)
        assert np.array_equal(v, ref[k]), k
    D.free()


# ---- 8
def test_zero_length_rows(fx, answers):
    seen = 0
    for r, a in zip(fx["rows"], answers[1e-3]):
        if "zero" not in r["classes"]:
            continue
        robot = scene(r["scene"])[1]
        mask = np.array(fx["scenes"][r["scene"]][str(r["kinds"])]["mask"], dtype=np.uint8)
        d, st, pr, w, g = robot.check_clearance(r["q_from"][None, :], kinds=r["kinds"], pair_mask=mask)
        assert a["s"] == 0.0 and a["status"] == BRACKETED and a["lower"] == a["distance"]
        assert abs(a["distance"] - d[0]) <= TOL and tuple(a["pair"]) == tuple(pr[0])
        assert np.abs(a["witness"] - w[0]).max() <= TOL and np.abs(a["grad"] - g[0]).max() <= TOL
        seen += 1
    assert seen >= 3


# ---- 9
def test_budget(fx):
    rows = [r for r in fx["rows"] if r["scene"] == "fr3_empty_world" and r["kinds"] == 3 and "interior" in r["classes"]][:4]
    assert len(rows) == 4
    for r, a in zip(rows, run(fx, 1e-12, resolution=1e-9, rows=rows)):
        print(f"test_budget: evals {a['evals']} status {a['status']} width {a['distance'] - a['lower']:.3e}")
        assert a["evals"] <= SC.SWEPT_BUDGET + SC.SWEPT_CONTACT_BUDGET
        assert a["status"] == OPEN
        check_bracket(r, a, 1e-12, r["d_dense"])
    stroke = [r for r in fx["rows"] if "stroke" in r["classes"]]
    assert len(stroke) >= 3
    for r, a in zip(stroke, run(fx, 1e-12, resolution=1e-9, rows=stroke)):
        assert a["status"] == OPEN and a["lower"] == -math.inf and a["evals"] <= SC.SWEPT_BUDGET + SC.SWEPT_CONTACT_BUDGET


# ---- 10
@pytest.mark.parametrize("task", [False, True])
def test_env_form(task):
    from parity_util import make_vec_env, synthetic_actions
    from test_gpu_clearance import _pick_env

    n = 6
    venv = _pick_env(n) if task else make_vec_env(n, True)
    venv.reset()
    joints, grip = synthetic_actions(n, 4, 3)
    for t in range(4):
        venv.step({"joints": joints[t], "gripper": grip[t]})
    simu, robot = venv.sim, venv.robot
    nl = int(simu.model.nq)
    rows = simu.qpos[:, :nl].copy()
    fq = simu.free_joint_qpos(simu.model.free_bodies[0]["joint_name"]) if task else None
    q_to = rows + np.random.default_rng(8).uniform(-0.3, 0.3, rows.shape) * np.array([1.0] * robot.dof + [0.0] * (nl - robot.dof))
    s0 = simu.get_state().copy()
    for kinds in (7, 3):
        a = venv.swept_clearance(q_to, kinds=kinds, resolution=RES)
        b = robot.swept_clearance(rows, q_to, free_qpos=fq, kinds=kinds, resolution=RES)
        assert _same(a, b), kinds
        assert (a["status"] != BEYOND).all()
    mask = robot.clearance_mask(7)
    assert _same(venv.swept_clearance(q_to, pair_mask=mask, d_max=0.3, tolerance=1e-4), robot.swept_clearance(rows, q_to, free_qpos=fq, pair_mask=mask, d_max=0.3, tolerance=1e-4))
    assert np.array_equal(simu.get_state(), s0)
    venv.close()


def test_rollout_bit_identical_with_swept_queries_between_steps():
    from parity_util import make_vec_env, synthetic_actions
    from test_gpu_clearance import _Dev

    runs = []
    steps = 50
    for with_queries in (False, True):
        venv = make_vec_env(16, True)
        robot = venv.robot
        nl = int(venv.sim.model.nq)
        joints, grip = synthetic_actions(16, steps, 0)
        venv.reset()
        rng = np.random.default_rng(6)
        out = []
        D = _Dev(venv.sim)
        arrays, _ = robot._swept_buffers(16, nl)
        dev = {k: D.alloc(v.nbytes) for k, v in arrays.items()}
        for t in range(steps):
            if with_queries:
                q = np.concatenate([rng.uniform(-1, 1, (10, 7)), np.full((10, 2), 0.02)], axis=1)
                robot.swept_clearance(q, q + 0.2, tolerance=1e-2)
                q_to = venv.sim.qpos[:, :nl] + 0.1
                venv.swept_clearance(q_to, tolerance=1e-2)
                venv.swept_clearance_dev(D.up(q_to).value, {k: p.value for k, p in dev.items()}, tolerance=1e-2)
            obs, rew, term, trunc, info = venv.step({"joints": joints[t], "gripper": grip[t]})
            out.append((venv.sim.qpos.copy(), venv.sim.qvel.copy(), {k: np.asarray(v).copy() for k, v in info.items()}))
        venv.sim.synchronize()
        D.free()
        runs.append(out)
        venv.close()
    for (qa, va, ia), (qb, vb, ib) in zip(*runs):
        assert np.array_equal(qa, qb) and np.array_equal(va, vb)
        for k in ia:
            assert np.array_equal(ia[k], ib[k]), k


# ---- 11
def test_robot_without_geoms():
    from parity_util import make_vec_env

    venv = make_vec_env(5, True, robot="ur5e")
    nl = int(venv.sim.model.nq)
    a = venv.robot.swept_clearance(np.zeros((5, nl)), np.full((5, nl), 0.3), d_max=0.25)
    assert (a["status"] == BEYOND).all() and (a["distance"] == 0.25).all() and (a["lower"] == 0.25).all() and (a["s"] == -1).all()
    assert (a["pair"] == -1).all() and not a["witness"].any() and not a["grad"].any() and not a["evals"].any()
    b = venv.swept_clearance(np.full((5, nl), 0.3))
    assert (b["status"] == BEYOND).all() and np.isinf(b["distance"]).all()
    venv.close()


# ---- 12
def test_errors_leave_outputs_and_state_untouched():
    from rcs_amd import _lib

    simu, robot, orc, cm, home, sc = scene("fr3_empty_world")
    L, h = simu._L, simu._h
    s0 = simu.get_state().copy()
    q = np.tile(np.concatenate([home, [0.02, 0.02]]), (4, 1))
    q2 = q + 0.1
    bad = q.copy()
    bad[2, 3] = np.nan
    box = np.tile([0.5, 0, 0.5, 1, 0, 0, 0.0], (4, 1))
    P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    inf = float("inf")
    arrays, out = robot._swept_buffers(4, 9)
    for v in arrays.values():
        v[...] = 7
    keep = {k: v.copy() for k, v in arrays.items()}
    O = C.byref(out)
    nodist = _lib.SweptOut(**{k: v.ctypes.data for k, v in arrays.items() if k != "distance"})
    ARG = 1
    f = L.rcsh_swept_clearance
    assert f(h, P(q), P(q2), None, -1, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, P(q), P(q2), None, 4, 8, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, None, P(q2), None, 4, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, P(q), None, None, 4, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, P(q), P(q2), None, 4, 3, None, inf, 1e-3, 1e-3, None) == ARG
    assert f(h, P(q), P(q2), None, 4, 3, None, inf, 1e-3, 1e-3, C.byref(nodist)) == ARG
    assert f(h, P(q), P(q2), P(box), 4, 3, None, inf, 1e-3, 1e-3, O) == ARG  # (no free body in this scene)
    assert f(h, P(bad), P(q2), None, 4, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, P(q), P(bad), None, 4, 3, None, inf, 1e-3, 1e-3, O) == ARG
    for d_max in (0.0, float("nan"), -1.0):
        assert f(h, P(q), P(q2), None, 4, 3, None, d_max, 1e-3, 1e-3, O) == ARG
    for x in (0.0, -1e-3, inf, float("nan")):
        assert f(h, P(q), P(q2), None, 4, 3, None, inf, x, 1e-3, O) == ARG
        assert f(h, P(q), P(q2), None, 4, 3, None, inf, 1e-3, x, O) == ARG
        assert L.rcsh_env_swept_clearance(h, P(q[:2]), 3, None, inf, x, 1e-3, O) == ARG
        assert L.rcsh_env_swept_clearance(h, P(q[:2]), 3, None, inf, 1e-3, x, O) == ARG
    assert L.rcsh_swept_clearance_dev(h, None, None, None, 4, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert L.rcsh_env_swept_clearance(h, P(q[:2]), 8, None, inf, 1e-3, 1e-3, O) == ARG
    assert L.rcsh_env_swept_clearance(h, None, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert L.rcsh_env_swept_clearance(h, P(bad[1:3]), 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert L.rcsh_env_swept_clearance_dev(h, None, 3, None, inf, 1e-3, 1e-3, O) == ARG
    assert f(h, None, None, None, 0, 3, None, inf, 1e-3, 1e-3, None) == 0  # m = 0 does nothing
    for k, v in arrays.items():
        assert np.array_equal(v, keep[k]), k
    assert np.array_equal(simu.get_state(), s0)
    with pytest.raises(ValueError):
        robot.swept_clearance(bad, q2)
    with pytest.raises(ValueError):
        robot.swept_clearance(q, q2, tolerance=0.0)
    with pytest.raises(ValueError):
        robot.swept_clearance(q, q2[:3])
    with pytest.raises(ValueError):
        robot.swept_clearance(q, q2, kinds=3, pair_mask=np.ones(3, dtype=np.uint8))
    # only `distance` is required
    d = np.zeros(4)
    only = _lib.SweptOut(distance=d.ctypes.data)
    assert f(h, P(q), P(q2), None, 4, 3, None, inf, 1e-3, 1e-3, C.byref(only)) == 0
    assert np.array_equal(d, robot.swept_clearance(q, q2, kinds=3)["distance"])
    assert robot.swept_clearance(np.zeros((0, 9)), np.zeros((0, 9)))["distance"].shape == (0,)
