"""The table of tests/box_cases.py on the CPU oracle: the precondition of tests/test_gpu_box_substep.py.

The GPU test holds the kernel's box substep to the oracle at 1e-10 (velocity) and 1e-12 (pose).  That says something only if every case
takes the branches it was designed for -- contact count, cone zones, Newton iterations, noslip sweeps -- if the table as a whole covers
the collider and the solver (every face down, every contact count, every zone, the rare sweep counts), and if the oracle itself is that
reproducible on the case: moved by one ulp in every input, or sent down another solver path, its result stays within 1/100 of the bars.
All of it is asserted here, case by case and for both scenes; a case that fails the spread assertion has to move off its knife edge, the
bars do not widen.  Flight has no branch at all: there the oracle is held to a 50-digit restatement of the update.
Run with -s for the measured figures (profiles/box_substep/tests.txt is that output)."""

import numpy as np
import pytest

import box_cases as B

CASES = B.cases()
PAIRS = [(s, c) for s in B.SCENES for c in CASES]
FLIGHT = [(s, c) for s, c in PAIRS if c["flight"]]


def _id(p):
    return f"{p[0]}-{p[1]['name']}"


def _case(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("scene", B.SCENES)
def test_cube_constants_are_the_solid_box_formulas(scene):
    """Half extents as the table assumes; the compiler's mass and inertia against the solid-box formulas on the scene file's numbers."""
    fb = B.compiled(scene).free_bodies[0]
    m, inertia = B.solid_box_constants(scene)
    assert np.array_equal(fb["size"], B.SIZE) and float(B.compiled(scene).timestep) == B.H and fb["plane_z"] == 0.0
    assert abs(fb["mass"] - float(m)) <= 4e-16 * float(m)
    assert np.abs(np.asarray(fb["inertia"]) - [float(x) for x in inertia]).max() <= 4e-16 * float(max(inertia))
    assert len(CASES) <= 48 and len({c["name"] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_case_takes_the_branches_it_claims(pair):
    scene, case = pair
    rec = B.reference(scene)[case["name"]]
    b = rec["branch"]
    got = (b["ncon"], b["zones"], b["newton"], b["noslip"])
    print(f"\n{scene} {case['name']}: contacts {got[0]} zones {got[1]} newton {got[2]} noslip {got[3]}; down {B.down_axis(case['qpos'])}")
    assert got == B.expected(scene, case)
    # the box's block stands alone in all 25 substeps: no robot geom touches it, the robot's rows are solved apart
    assert all(r["coupled"] == 0 and not r["robot_touches_box"] for r in rec["records"])
    assert abs(case["qpos"][0] - B.X0) < 0.2 and abs(case["qpos"][1] - B.Y0) < 0.2
    if case["cls"] == "harvested":
        tag = case["rare"]
        if scene == "fr3_simple_pick_up":
            assert (b["newton"] >= 9) if tag == "newton9" else (b["noslip"] == int(tag[-1]) and b["ncon"] > 0)
        else:
            assert b["noslip"] == 0


@pytest.mark.parametrize("scene", B.SCENES)
def test_designed_classes_are_what_they_say(scene):
    ref = B.reference(scene)
    sweeps = 2 if scene == "fr3_simple_pick_up" else 0
    by = lambda cls: [(c, ref[c["name"]]["branch"]) for c in CASES if c["cls"] == cls]  # noqa: E731
    rest, twist = by("face-rest"), by("face-twist")
    # a face at rest: four sticking contacts, one Newton step from the unconstrained acceleration; all six faces
    assert [B.down_axis(c["qpos"]) for c, _ in rest] == ["+x", "-x", "+y", "-y", "+z", "-z"] == [B.down_axis(c["qpos"]) for c, _ in twist]
    assert all(b["ncon"] == 4 and b["zones"] == (2, 2, 2, 2) and b["newton"] == 1 and b["noslip"] == sweeps for _, b in rest)
    assert all(b["ncon"] == 4 and 4 <= b["newton"] <= 6 and 2 not in b["zones"] for _, b in twist)
    assert {z for _, b in twist for z in b["zones"]} == {0, 1}
    # each face is another set of four corners in the walk from contact slots to corners
    lowest = {B.down_axis(c["qpos"]): tuple(np.argsort(B.corner_heights(c["qpos"][3:]))[:4].tolist()) for c, _ in rest}
    assert {k: tuple(sorted(v)) for k, v in lowest.items()} == {"+x": (1, 3, 5, 7), "-x": (0, 2, 4, 6), "+y": (2, 3, 6, 7), "-y": (0, 1, 4, 5),
                                                                  "+z": (4, 5, 6, 7), "-z": (0, 1, 2, 3)}
    assert [b["ncon"] for _, b in by("edge")] == [2] * 4 and [b["ncon"] for _, b in by("corner")] == [1] * 4
    pairs = [tuple(sorted(np.argsort(B.corner_heights(c["qpos"][3:]))[:2].tolist())) for c, _ in by("edge")]
    assert pairs == [(3, 7), (4, 6), (2, 3), (1, 3)]
    assert [int(np.argmin(B.corner_heights(c["qpos"][3:]))) for c, _ in by("corner")] == [7, 2, 1, 4]
    assert ref["three-contacts"]["branch"]["ncon"] == 3 and ref["three-contacts"]["branch"]["zones"] == (2, 1, 2)
    # the centre under the floor; and all eight corners under it: there the upper four are left out by `ld > 0` alone
    assert _case("centre-below")["qpos"][2] < 0 and ref["centre-below"]["branch"]["ncon"] == 4
    c = _case("buried")
    assert (c["qpos"][2] + B.corner_heights(c["qpos"][3:]) < 0).all() and ref["buried"]["branch"]["ncon"] == 4
    assert ref["deep-tilted-sink"]["branch"]["zones"] == (1, 2, 0, 0) and ref["deep-tilted-sink"]["branch"]["newton"] == 7
    # leaving: all four contacts separate; in flight from the next substep on
    recs = ref["leaving"]["records"]
    assert recs[0]["zones"] == (0, 0, 0, 0) and recs[0]["noslip"] == (1 if sweeps else 0) and all(r["ncon"] == 0 for r in recs[1:10])
    assert ref["unnormalised"]["branch"]["ncon"] == 4 and 1 in ref["unnormalised"]["branch"]["zones"]
    assert abs(np.linalg.norm(_case("unnormalised")["qpos"][3:]) - 3.0) < 1e-15
    assert all(r["ncon"] == 0 for cse in CASES if cse["flight"] for r in ref[cse["name"]]["records"])


def test_table_covers_the_collider_and_the_solver():
    ref = B.reference("fr3_simple_pick_up")
    first = [ref[c["name"]]["branch"] for c in CASES]
    assert {b["ncon"] for b in first} == {0, 1, 2, 3, 4}
    assert {z for b in first for z in b["zones"]} == {0, 1, 2}
    assert {B.down_axis(c["qpos"]) for c, b in zip(CASES, first) if b["ncon"] == 4} == {"+x", "-x", "+y", "-y", "+z", "-z"}
    assert {b["noslip"] for b in first} == {0, 1, 2, 3, 5}
    assert max(b["newton"] for b in first) >= 9
    harvested = [c for c in CASES if c["cls"] == "harvested"]
    assert 10 <= len(harvested) <= 14 and {c["rare"] for c in harvested} == {"noslip1", "noslip3", "noslip5", "newton9"}
    # the other scene: the same table, nothing dropped, no sweep anywhere
    other = B.reference("xarm7_box_world")
    assert set(other) == set(ref) and {r["noslip"] for rec in other.values() for r in rec["records"]} == {0}
    assert {rec["branch"]["ncon"] for rec in other.values()} == {0, 1, 2, 3, 4} and {z for rec in other.values() for z in rec["branch"]["zones"]} == {0, 1, 2}


WORST = {}


@pytest.mark.parametrize("pair", PAIRS, ids=_id)
def test_oracle_spread_is_a_hundredth_of_the_bars(pair):
    """One-ulp moves of every input (6 draws) and the warm start scaled by 1.001 / 0.99 / 0, after 1 and 3 substeps.  The exact touch is
    measured but not asserted: one ulp decides whether it is a contact at all (test_exact_touch_is_a_knife_edge)."""
    scene, case = pair
    sp = B.spread(scene, case)
    print(f"\n{scene} {case['name']}: ulp vel {sp['ulp_vel']:.2e} pose {sp['ulp_pose']:.2e}; path vel {sp['path_vel']:.2e} pose {sp['path_pose']:.2e}; same branches {sp['same_branches']}")
    if case["touch"]:
        assert sp["ulp_vel"] > 1e-3, "the knife edge is gone: this case no longer pins the predicate"
        assert sp["path_vel"] <= B.SPREAD_VEL and sp["path_pose"] <= B.SPREAD_POSE
        return
    w = WORST.setdefault((scene, case["cls"]), {"ulp_vel": 0.0, "ulp_pose": 0.0, "path_vel": 0.0, "path_pose": 0.0})
    for k in w:
        w[k] = max(w[k], sp[k])
    assert sp["same_branches"]
    assert max(sp["ulp_vel"], sp["path_vel"]) <= B.SPREAD_VEL and max(sp["ulp_pose"], sp["path_pose"]) <= B.SPREAD_POSE, sp


def test_oracle_spread_summary():
    """(prints the worst spread per case class measured by the test above, when it ran in this session)"""
    for (scene, cls), w in sorted(WORST.items()):
        print(f"\nworst spread {scene} {cls}: " + ", ".join(f"{k} {v:.2e}" for k, v in w.items()), end="")
    print()
    for w in WORST.values():
        assert max(w["ulp_vel"], w["path_vel"]) <= B.SPREAD_VEL and max(w["ulp_pose"], w["path_pose"]) <= B.SPREAD_POSE


def test_exact_touch_is_a_knife_edge():
    """z equal to the z half extent with the identity quaternion: dist + ld is exactly 0 and counts as contact (`<=`).  One ulp higher it
    is flight, and the velocity after the substep differs by ~2e-2: the GPU test's 1e-10 pins the predicate."""
    case = _case("exact-touch")
    assert case["qpos"][2] == B.SIZE[2] and case["qpos"][2] + B.corner_heights(case["qpos"][3:]).min() == 0.0
    orc = B.oracle("fr3_simple_pick_up")
    orc.place(case["qpos"], case["qvel"])
    on = orc.substep()
    v_on = orc.o.box_qvel
    above = case["qpos"].copy()
    above[2] = np.nextafter(above[2], 1.0)
    orc.place(above, case["qvel"])
    off = orc.substep()
    dv = float(np.abs(orc.o.box_qvel - v_on).max())
    print(f"\nexact touch: contacts {on['ncon']} / one ulp higher {off['ncon']}, velocity apart by {dv:.3e}")
    assert on["ncon"] == 4 and off["ncon"] == 0 and dv > 1e-2


@pytest.mark.parametrize("pair", FLIGHT, ids=_id)
def test_flight_matches_the_mpmath_restatement(pair):
    """v' = v + h (g, -I^-1 (w x I w)), p' = p + h v', q' = normalise(q) * exp(h w' / 2) at 50 digits, mass and inertia by the solid-box
    formulas.  The oracle's distance from it is the baseline of the kernel's flight bar (box_cases.FLIGHT_BAR)."""
    scene, case = pair
    ref, mp = B.reference(scene)[case["name"]], B.flight_reference(scene, case["name"])
    for k in (1, 25):
        dq, dv = float(np.abs(ref[k][0] - mp[k][0]).max()), float(np.abs(ref[k][1] - mp[k][1]).max())
        print(f"\n{scene} {case['name']}: oracle - mpmath after {k} substeps: pose {dq:.2e} velocity {dv:.2e}", end="")
        assert max(dq, dv) <= B.ORACLE_FLIGHT_BAR[k]
    print()


@pytest.mark.parametrize("scene", B.SCENES)
def test_flight_branches(scene):
    ref = B.reference(scene)
    q0 = B.FLIGHT_Q / np.linalg.norm(B.FLIGHT_Q)
    # below kMin the quaternion is not turned at all (it is only normalised); at 1e-14 it goes through the integration (by 1e-17 rad a
    # substep, which no double shows: the case is there for the branch, the mpmath test holds its numbers)
    assert np.abs(ref["flight-spin-1e-16"][25][0][3:] - q0).max() <= 2.3e-16 and np.array_equal(ref["flight-spin-1e-16"][25][0][3:], ref["flight-still"][25][0][3:])
    assert np.abs(ref["flight-spin-1e-14"][25][0][3:] - q0).max() <= 1e-15
    # the zero quaternion and (1e-16, 0, 0, 0) both become the identity before anything else: the same flight, bit for bit
    a, b = ref["flight-zero-quat"], ref["flight-tiny-quat"]
    assert all(np.array_equal(a[k][0], b[k][0]) and np.array_equal(a[k][1], b[k][1]) for k in B.CHECKPOINTS)
    spin = B.flight_reference(scene, "flight-zero-quat")[1][1][3:]
    expect = B.quat(spin, B.H * np.linalg.norm(spin))  # identity * exp(h w' / 2)
    assert np.abs(a[1][0][3:] - expect).max() < 1e-15
    # the gyroscopic term alone: about no principal axis the body-frame spin changes without any torque
    assert np.abs(ref["flight-spin"][1][1][3:] - B.SPIN[3:]).min() > 1e-4
