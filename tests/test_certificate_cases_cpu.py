"""The rows of tests/golden/certificate_cases.json on the CPU oracle: the precondition of tests/test_gpu_certificate_cases.py.

The GPU test asserts that a launch in which the oracle saw a penetration was sent to the contact-resolving kernel, and that the kernels
match the resolving oracle to 1e-9 after it.  That says something about the lean launch's certificate (csrc/check_team.h) only if every
row really is a contact that begins and ends inside the launch it names, is as deep as its family says, leaves the resolving and the
non-resolving oracle far enough apart for parity to see a certificate that passed, and is reproducible (a twin nudged by 1e-13 rad stays
within 1e-10).  All of it is asserted here, for every row: the table holds only rows that pass, none is skipped or excluded."""

import numpy as np
import pytest

import certificate_cases as CC

ROWS = CC.characters()
GRAZE = [r for r in ROWS if r["family"] != "quiet"]


def _ids(rows):
    return [r["name"] for r in rows]


@pytest.mark.parametrize("row", GRAZE, ids=_ids(GRAZE))
def test_graze_is_where_and_what_the_table_says(row):
    rep = CC.oracle_run()[row["name"]]
    lo, hi = CC.depth_range(row)
    print(f"\n{row['name']}: pen per launch {rep['pen'].tolist()}, substeps {list(zip(rep['first'].tolist(), rep['last'].tolist()))}")
    assert len(row["ramp"]) == CC.LAUNCHES[row["form"]] and row["start"][7:] == [CC.OPEN, CC.OPEN]
    assert row["graze"] and np.flatnonzero(rep["pen"] > 0.0).tolist() == row["graze"]
    for t in range(CC.launches(row)):
        assert rep["ends"][t] == (0, 0) and rep["begins"][t] == (0, 0), (t, rep["begins"][t], rep["ends"][t])
        if t in row["graze"]:
            assert lo <= rep["pen"][t] <= hi, (t, rep["pen"][t])
            assert rep["pen"][t] > CC.SEEN, "deep enough for the GPU test to demand an escalation"
            depth, kind, names = rep["deepest"][t]
            assert kind == row["kind"] and depth == rep["pen"][t]
            assert 0 <= rep["first"][t] <= rep["last"][t] < rep["steps"][t]
        else:
            assert rep["pen"][t] == 0.0, (t, rep["pen"][t])
    t0 = row["graze"][0]
    assert rep["deepest"][t0][2] == (row["lowest"] if row["kind"] == "floor" else row["pair"])
    assert all(rep["converged"])


@pytest.mark.parametrize("row", GRAZE, ids=_ids(GRAZE))
def test_unresolved_oracle_parts_from_the_resolving_one(row):
    """Deep families: >= 1e-6 rad in some joint at the end of every graze launch -- 1000 x the parity bar, which is what gives the GPU
    test's parity assertion its teeth.  (Shallow rows: reported; there the escalation bits are the assertion.)"""
    rep = CC.oracle_run()[row["name"]]
    lean = CC.replay(row, resolve=False)
    gaps = [float(np.abs(lean["qpos"][t][:7] - rep["qpos"][t][:7]).max()) for t in row["graze"]]
    print(f"\n{row['name']}: resolved - unresolved after the graze launches {gaps}")
    if CC.depth_range(row) is CC.DEEP:
        assert min(gaps) >= CC.RESOLVED_GAP, gaps


@pytest.mark.parametrize("row", ROWS, ids=_ids(ROWS))
def test_twin_stays_within_1e_10(row):
    rep = CC.oracle_run()[row["name"]]
    twin = CC.replay(row, nudge=CC.TWIN_NUDGE)
    dq = float(np.abs(twin["qpos"] - rep["qpos"]).max())
    print(f"\n{row['name']}: twins' largest distance {dq:.2e}")
    assert dq <= CC.TWIN_SPLIT and np.array_equal(twin["steps"], rep["steps"])


STEPPED = [r for r in GRAZE if r["form"] != "env"]  # (the env rows take no part in the state-write variants)


@pytest.mark.parametrize("row", STEPPED, ids=_ids(STEPPED))
def test_hard_start_after_a_rest_is_the_same_script(row):
    """The state-write variants of the GPU test rest at a quiet pose first and then write the start state: on the oracle that is the same
    trajectory bit for bit under asynchronous control.  Under synchronous control the callbacks that decide convergence run by the clock,
    which the rest has moved: the call takes another number of substeps (the GPU test replays the rest on the oracle too) -- and still
    holds the graze."""
    quiet = CC.quiet_rows(row["form"])[0]
    rep, rested = CC.oracle_run()[row["name"]], CC.replay(row, rest=(CC.REST_LAUNCHES, np.asarray(quiet["start"])))
    if row["form"] == "converge":
        print(f"\n{row['name']}: substeps {rep['steps'].tolist()} / after the rest {rested['steps'].tolist()}, pen {rested['pen'].tolist()}")
        assert np.flatnonzero(rested["pen"] > CC.SEEN).tolist() == row["graze"] and all(e == (0, 0) for e in rested["ends"])
        return
    assert np.array_equal(rep["qpos"], rested["qpos"]) and np.array_equal(rep["qvel"], rested["qvel"]) and np.array_equal(rep["pen"], rested["pen"])


def test_quiet_characters_stay_a_centimetre_from_everything():
    """In every launch form they are neighbours in: no collision pass sees a penetration, and the GJK reference of
    tests/clearance_cases.py puts every geom pair and the floor at >= 1 cm at the end of every launch (every pair but link 0 / link 1,
    which are a millimetre apart in every pose: certificate_cases.ALWAYS_NEAR)."""
    import clearance_cases as K

    scene = K.Scene(CC.compiled_model())
    pairs = CC.clearance_pairs(scene)
    assert len([r for r in ROWS if r["family"] == "quiet"]) == 4
    for form in CC.SUBSTEPS:
        quiet = CC.quiet_rows(form)
        assert len(quiet) == 4
        for row in quiet:
            rep = CC.replay(row)
            worst = min(float(scene.distances(scene.frames(q), pairs).min()) for q in rep["qpos"])
            print(f"{row['name']} as {form}: clearance {worst:.4f} m, substeps {rep['steps'].tolist()}")
            assert rep["pen"].max() == 0.0 and worst >= CC.QUIET_CLEARANCE and all(rep["converged"])


def _family(name):
    return [r for r in ROWS if r["family"] == name]


def test_families_and_coverage():
    assert {r["family"] for r in ROWS} == set(CC.FAMILIES)
    floor = _family("floor-deep")
    lowest = {r["lowest"] for r in floor}
    print("\nfloor-deep lowest links:", sorted(lowest))
    assert len(floor) >= 6 and all(r["kind"] == "floor" and r["form"] == "step17" for r in floor)
    assert any("hand" in n for n in lowest) and any("finger" in n for n in lowest) and any(k in n for n in lowest for k in ("link5", "link6", "link7"))
    assert len(lowest) >= 3

    # characters whose graze is in launch 0, begun with the velocity of a sweep under way: the launch an environment begins on the lean
    # launch whatever the certificate made of the launches before (tools/make_certificate_cases.py: from_its_graze_launch)
    first = [r for r in floor + _family("self-deep") if r["graze"] == [0] and r["vel"] is not None and np.abs(r["vel"][:7]).max() > 0.1]
    assert sum(r["kind"] == "floor" for r in first) >= 2 and sum(r["kind"] == "self" for r in first) >= 2, [r["name"] for r in first]

    cm = CC.compiled_model()
    types = {n: int(cm.arrays["geom_type"][g]) for g, n in enumerate(cm.geom_names)}
    own = _family("self-deep")
    pairs = {tuple(r["pair"]) for r in own}
    print("self-deep pairs:", sorted(pairs))
    assert len(own) >= 6 and len(pairs) >= 3 and all(r["kind"] == "self" and r["form"] == "step17" for r in own)
    assert any(types[a] == 7 and types[b] == 7 for a, b in pairs), "a hull-hull pair: it reaches the narrow phase"
    assert any(6 in (types[a], types[b]) for a, b in pairs), "a pair with a box geom"

    shallow = _family("shallow")
    assert sum(r["kind"] == "floor" for r in shallow) >= 3 and sum(r["kind"] == "self" for r in shallow) >= 3
    for r in shallow:  # a fraction of a degree a launch
        assert np.abs(np.diff([r["start"][r["joint"]]] + r["ramp"])).max() < np.deg2rad(0.5), r["name"]

    carried = _family("carried-slack")
    assert len(carried) >= 4 and {r["quiet_before"] for r in carried} >= {1, 3, 8}
    for r in carried:
        assert r["graze"][0] >= r["quiet_before"], r["name"]
    # the ones that rest on their start pose and graze in their first moving launch: the GPU test asserts that they begin it on the lean launch
    held = [r for r in carried if r["name"].startswith("held")]
    assert {r["quiet_before"] for r in held if r.get("lean")} >= {1, 3, 8} and all(r["graze"] == [r["quiet_before"]] for r in held)
    assert all(r.get("lean") for r in held if r["kind"] == "floor")
    for r in held:
        assert all(r["ramp"][t] == r["start"][r["joint"]] for t in range(r["quiet_before"])), r["name"]

    back = _family("there-and-back")
    assert {r["kind"] for r in back} >= {"floor", "self"}
    for r in back:
        assert len(r["graze"]) == 2 and r["graze"][1] - r["graze"][0] >= 5, (r["name"], r["graze"])
    assert {r["kind"] for r in back if r.get("returns")} >= {"floor", "self"}  # (nine launches at rest between the grazes: GPU test)

    long_ = _family("long-launch")
    assert len(long_) >= 2 and {r["form"] for r in long_} >= {"step48", "step100"}
    for r in long_:
        rep, k, t = CC.oracle_run()[r["name"]], CC.SUBSTEPS[r["form"]], r["graze"][0]
        assert k // 4 <= rep["first"][t] <= rep["last"][t] < 3 * k // 4, (r["name"], rep["first"][t], rep["last"][t])

    conv = _family("convergence-pieces")
    inside = straddle = 0
    assert {r["form"] for r in conv} == {"converge", "env"}
    for r in conv:
        rep, t = CC.oracle_run()[r["name"]], r["graze"][0]
        a, b = int(rep["first"][t]), int(rep["last"][t])
        assert [a, b] == r["substeps"] and rep["steps"].tolist() == r["steps"] and rep["steps"].max() <= 500 and all(rep["converged"])
        print(f"{r['name']}: penetrating substeps {a} .. {b} of {rep['steps'][t]}")
        if r["form"] == "env":  # (through the env layer: relative actions of at most 5 degrees; both kinds are asserted there)
            assert np.abs(CC.actions(r)).max() <= np.deg2rad(5) and r.get("lean")
            inside += a // CC.PIECE == b // CC.PIECE
            straddle += a // CC.PIECE < b // CC.PIECE
    assert inside >= 1 and straddle >= 1
    assert len(ROWS) <= 56 and len({tuple(r["start"]) for r in ROWS}) == len(ROWS)


def test_a_call_of_500_substeps_converged_and_did_not_run_out():
    """Some convergence rows take exactly 500 substeps, which is also the cap: the convergence callbacks run by the clock, and 500 substeps
    are one second of it.  With the cap at 2000 the call takes the same 500 and reports convergence."""
    rows = [r for r in _family("convergence-pieces") if r["form"] == "converge" and max(r["steps"]) == 500]
    for r in rows:
        o = CC.make_oracle("converge")
        o.s.max_convergence_steps = 2000
        CC.place(o, *CC.start_state(r))
        for t, tgt in enumerate(CC.targets(r)):
            o.set_joint_position(tgt)
            o.step_until_convergence()
            assert int(o.s.convergence_steps) == r["steps"][t] and o.is_converged(), (r["name"], t, int(o.s.convergence_steps))


def test_arrangements_hold_every_character_at_every_team_position():
    for form in CC.SUBSTEPS:
        graze = [r["name"] for r in CC.by_form(form) if r["family"] != "quiet"]
        table = CC.arrangements(form)
        assert [r["name"] for r in table["once"]][:len(graze)] == graze and len(table["once"]) == len(graze) + 4
        for p in range(4):
            arr = [r for name in sorted(table) if name.startswith(f"team{p}") for r in table[name]]
            assert len(arr) == 4 * len(graze) and all(len(table[name]) <= 128 for name in table if name.startswith("team"))
            for i, name in enumerate(graze):
                team = arr[4 * i:4 * i + 4]
                assert team[p]["name"] == name and all(r["family"] == "quiet" for k, r in enumerate(team) if k != p)
        assert [r["name"] for r in table["packed"]] == graze
        assert len(table["ragged"]) % 4 == 3 and {r["name"] for r in table["ragged"]} >= set(graze)
