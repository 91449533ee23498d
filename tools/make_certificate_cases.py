"""Writes tests/golden/certificate_cases.json: contacts that begin and end inside one launch, found on the CPU oracle by a directed search
(tests/certificate_cases.py describes the rows; tests/test_certificate_cases_cpu.py is what admits them).

A candidate is a pose, a joint that is ramped through it at a chosen speed (the sweep) and a joint that decides how deep the sweep's
lowest point goes (the depth joint).  The search moves the depth joint until the sweep first touches (bisection on "some collision pass
saw a penetration"), then a little further until the deepest penetration is the wanted one (bisection on pen_seen), and keeps the
candidate if the penetrating substeps lie inside the wanted launch(es) with both ends clear, the resolving and the non-resolving oracle
part, and a twin nudged by 1e-13 rad does not.  Candidates are drawn from a seeded generator until every family has its rows; the
families are tasks that run side by side, each with a random stream of its own, so a task can be run again alone (--only, --merge).
Three tasks are made from rows the others wrote (launch0, env-inside, env-straddle): they run after them, one by one, on the table --out.

    python tools/make_certificate_cases.py [--seed 0] [--only task,task] [--merge] [--out tests/golden/certificate_cases.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("robot-control-stack_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import certificate_cases as CC  # noqa: E402
from rcs_env_oracle import FR3_HIGH, FR3_LOW  # noqa: E402

LOW = np.array([-2.3093, -1.5133, -2.4937, -2.7478 - 0.3, -2.4800, 0.5, -2.6895])   # (the folded poses pass FR3's soft limits, as
HIGH = np.array([2.3093, 1.7, 2.4937, -0.4461, 2.4800, 4.2094, 2.6895])              #  parity_util.run_self_contact_parity's do)


def row_of(name, family, kind, form, start, joint, ramp, vel=None):
    start9 = [float(x) for x in start[:7]] + [CC.OPEN, CC.OPEN]
    ramp = list(ramp)
    assert len(ramp) <= CC.LAUNCHES[form], (name, len(ramp))
    ramp += [ramp[-1]] * (CC.LAUNCHES[form] - len(ramp))
    return {"name": name, "family": family, "kind": kind, "form": form, "start": start9, "vel": vel, "target0": start9[:7], "joint": int(joint),
            "ramp": [float(x) for x in ramp], "graze": []}


def ramp_of(a, rate, pre, sweep, hold, back=None):
    """Targets of the swept joint: `pre` launches at a slow approach (a tenth of the rate), `sweep` launches at `rate` rad a launch, `hold`
    launches at rest; `back`: then the same sweep backwards and a hold."""
    r, x = [], a
    for _ in range(pre):
        x += 0.1 * rate
        r.append(x)
    for _ in range(sweep):
        x += rate
        r.append(x)
    r += [x] * hold
    if back:
        for _ in range(sweep):
            x -= rate
            r.append(x)
        r += [x] * back
    return r


def pens(row, h_joint, h, **kw):
    row = dict(row)
    row["start"] = list(row["start"]); row["target0"] = list(row["target0"])
    row["start"][h_joint] = row["target0"][h_joint] = float(h)
    return row, CC.replay(row, **kw)


def shifted(row, delta):
    """The row with its sweep `delta` further along: the lowest point comes earlier in the script."""
    row = dict(row)
    row["start"] = list(row["start"]); row["target0"] = list(row["target0"])
    row["start"][row["joint"]] += delta
    row["target0"][row["joint"]] += delta
    row["ramp"] = [x + delta for x in row["ramp"]]
    return row


def first_touch(row, h_joint, lo, hi, rounds):
    for _ in range(rounds):
        mid = 0.5 * (lo + hi)
        if pens(row, h_joint, mid)[1]["pen"].max() > 0.0:
            hi = mid
        else:
            lo = mid
    return lo, hi


def search(row, h_joint, h0, h1, want, n_graze=1, log=None, aim=None):
    """Move the depth joint from h0 (clear) towards h1 until the deepest penetration of the script lies in `want`; None: no such pose."""
    def peak(h):
        return float(pens(row, h_joint, h)[1]["pen"].max())

    if peak(h0) > 0.0:
        return None
    lo, hi = h0, None
    for s in np.linspace(0.0, 1.0, 31)[1:]:
        h = h0 + s * (h1 - h0)
        if peak(h) > 0.0:
            hi = h
            break
        lo = h
    if hi is None:
        return None
    lo, hi = first_touch(row, h_joint, lo, hi, 22)
    # (1e-8 rad past the first touch: a sweep that touches where it stops, or in the wrong number of launches, is given up here)
    rep = pens(row, h_joint, hi)[1]
    graze = np.flatnonzero(rep["pen"] > 0.0)
    if (n_graze == 1 and len(graze) != 1) or rep["ends"][-1] != (0, 0):  # (a sweep there and back: its second touch comes a little deeper)
        return None
    k = CC.SUBSTEPS[row["form"]]
    if k is not None and n_graze == 1:
        # the touch to the middle of its launch: the sweep is moved along by what the arm travels in the substeps between
        t = int(graze[0])
        q_before = rep["qpos"][t - 1][row["joint"]] if t else row["start"][row["joint"]]
        travel = rep["qpos"][t][row["joint"]] - q_before
        off = 0.5 * (rep["first"][t] + rep["last"][t]) - 0.5 * (k - 1)
        if abs(off) > 0.15 * k:
            row = shifted(row, travel * off / k)
            if pens(row, h_joint, lo - 0.003 * np.sign(h1 - h0))[1]["pen"].max() > 0.0 or not peak(hi + 0.003 * np.sign(h1 - h0)) > 0.0:
                return None
            lo, hi = first_touch(row, h_joint, lo - 0.003 * np.sign(h1 - h0), hi + 0.003 * np.sign(h1 - h0), 20)
    touch = hi
    target = float(np.sqrt(want[0] * want[1])) if aim is None else aim
    lo, hi = touch, touch + 0.02 * np.sign(h1 - h0)
    if peak(hi) < target:
        return None
    for _ in range(26):
        mid = 0.5 * (lo + hi)
        if peak(mid) > target:
            hi = mid
        else:
            lo = mid
    out, rep = pens(row, h_joint, hi)
    out["graze"] = [int(t) for t in np.flatnonzero(rep["pen"] > 0.0)]
    if len(out["graze"]) != n_graze:
        return None
    return (out, rep) if admit(out, rep, log) else None


def admit(row, rep, log=None):
    """The conditions tests/test_certificate_cases_cpu.py asserts, on a candidate."""
    lo, hi = CC.depth_range(row)
    say = (lambda *a: print("   reject", row["name"], *a, file=log, flush=True)) if log else (lambda *a: None)
    for t in row["graze"]:
        if not lo <= rep["pen"][t] <= hi:
            return say("depth", rep["pen"][t])
        if rep["ends"][t] != (0, 0) or rep["begins"][t] != (0, 0):
            return say("ends", rep["begins"][t], rep["ends"][t])
        if rep["deepest"][t][1] != row["kind"]:
            return say("kind", rep["deepest"][t])
    if any(e != (0, 0) for e in rep["ends"]) or not all(rep["converged"]):
        return say("an end in contact, or a call that did not converge")
    t0 = row["graze"][0]
    if row["family"] in CC.DEEP_FAMILIES and not row.get("shallow"):
        lean = CC.replay(row, resolve=False)
        if np.abs(lean["qpos"][t0][:7] - rep["qpos"][t0][:7]).max() < CC.RESOLVED_GAP:
            return say("the unresolved oracle stays within", np.abs(lean["qpos"][t0] - rep["qpos"][t0]).max())
    twin = CC.replay(row, nudge=CC.TWIN_NUDGE)
    if np.abs(twin["qpos"] - rep["qpos"]).max() > CC.TWIN_SPLIT or (twin["steps"] != rep["steps"]).any():
        return say("twins part", np.abs(twin["qpos"] - rep["qpos"]).max())
    kind, names = rep["deepest"][t0][1], rep["deepest"][t0][2]
    row["lowest" if kind == "floor" else "pair"] = names
    row["depth"] = [float(rep["pen"][t]) for t in row["graze"]]
    if row["form"] in ("converge", "env"):
        row["substeps"] = [int(rep["first"][t0]), int(rep["last"][t0])]
        row["steps"] = [int(s) for s in rep["steps"]]
    return True


def draw_floor(rng):
    q = np.array([rng.uniform(-1, 1), rng.uniform(0.5, 1.3), rng.uniform(-0.6, 0.6), rng.uniform(-2.2, -0.5), rng.uniform(-1.5, 1.5),
                  rng.uniform(0.9, 3.6), rng.uniform(-2.0, 2.0)])
    return q, int(rng.choice([6, 6, 4, 5, 2])), 1, 0.2, 1.7


def draw_floor_wrist_up(rng):
    """The wrist bent back so far that the hand points upwards: links 5 to 7 are the lowest."""
    q = np.array([rng.uniform(-1, 1), rng.uniform(0.5, 1.3), rng.uniform(-0.6, 0.6), rng.uniform(-1.3, -0.45), rng.uniform(-1.5, 1.5),
                  rng.uniform(2.5, 3.7), rng.uniform(-2.0, 2.0)])
    return q, int(rng.choice([4, 5, 2])), 1, 0.2, 1.7


def draw_near_a_known_graze(rng):
    """A 5 degree sweep holds a lowest point far less often than a 40 degree one: the env calls are drawn around the pose at which a floor
    character of the table (written by the tasks before this one) is deepest -- the middle of its graze launch -- and jittered."""
    if not hasattr(draw_near_a_known_graze, "poses"):
        with open(from_its_graze_launch.table) as f:
            table = [r for r in json.load(f)["characters"] if r["family"] == "floor-deep" and r["vel"] is None]
        draw_near_a_known_graze.poses = []
        for r in table:
            rep, t = CC.replay(r), r["graze"][0]
            q = 0.5 * (rep["qpos"][t - 1][:7] + rep["qpos"][t][:7])
            if FR3_LOW[1] < q[1] < FR3_HIGH[1] - 0.06:
                draw_near_a_known_graze.poses.append((q, r["joint"]))
    q, j = draw_near_a_known_graze.poses[int(rng.integers(len(draw_near_a_known_graze.poses)))]
    q = q.copy()
    q[j] += rng.uniform(-0.03, 0.03)
    q[[0, 2, 4]] += rng.uniform(-0.02, 0.02, 3)
    return q, j, 1, q[1] - 0.06, min(q[1] + 0.06, FR3_HIGH[1] - 0.001)


def draw_self(rng):
    q = np.array([rng.uniform(-1, 1), rng.uniform(-1.78, 0.2), rng.uniform(-0.3, 0.3), -2.45, rng.uniform(-0.9, 0.9), rng.uniform(0.55, 1.6),
                  rng.uniform(-2.0, 2.0)])
    return q, int(rng.choice([6, 6, 4, 5])), 3, -2.45, -3.04


def candidates(rng, kind, family, form, want, count, accept, log, rate=(0.03, 0.09), pre=0, sweep=8, hold=2, back=None, n_graze=1, tries=4000, tag=None, draw=None, script=None, h_end=None, aim=None):
    rows = []
    for i in range(tries):
        if len(rows) >= count:
            break
        q, j, hj, h0, h1 = (draw if draw else draw_floor if kind == "floor" else draw_self)(rng)
        r = float(rng.uniform(*rate)) * (1 if rng.uniform() < 0.5 else -1)
        span = r * (sweep + 0.1 * pre)
        a = float(np.clip(q[j] - 0.5 * span, LOW[j] + abs(span) + 0.01, HIGH[j] - abs(span) - 0.01))  # (the drawn pose: the middle of the sweep)
        q[j] = a
        if h_end is not None:
            h1 = h_end
        row = row_of(f"{tag or family}-{kind}-{len(rows)}", family, kind, form, q, j, script(a, r) if script else ramp_of(a, r, pre, sweep, hold, back))
        if want is CC.SHALLOW and family != "shallow":
            row["shallow"] = True
        if pre:
            row["quiet_before"] = pre
        got = search(row, hj, h0, h1, want, n_graze, log, aim)
        if got and accept(got[0], got[1]):
            rows.append(got[0])
            print(f"  {got[0]['name']}: try {i}, joint {j}, graze {got[0]['graze']}, depth {got[0]['depth']}, {got[0].get('lowest') or got[0].get('pair')}"
                  + (f", substeps {got[0]['substeps']} of {got[0]['steps']}" if form in ("converge", "env") else ""), file=log, flush=True)
    if len(rows) < count:
        print(f"  !! {family} {kind}: {len(rows)} of {count} after {tries} tries", file=log, flush=True)
    return rows


class Coverage:
    """Accepts candidates so that the names (lowest links / geom pairs) the family must cover are met before it is filled with repeats."""

    def __init__(self, classes, per_class=2):
        self.classes, self.per, self.seen = classes, per_class, {}

    def __call__(self, row, rep):
        names = row.get("lowest") or row.get("pair")
        c = next((k for k, f in self.classes.items() if f(names)), None)
        if c is None or self.seen.get(c, 0) >= self.per:
            return False
        self.seen[c] = self.seen.get(c, 0) + 1
        return True


def quiet_rows(rng, log):
    """Four characters near home that stay a centimetre from everything: clearance from the GJK reference of tests/clearance_cases.py."""
    import clearance_cases as K
    from rcs_env_oracle import FR3_Q_HOME

    scene = K.Scene(CC.compiled_model())
    pairs = CC.clearance_pairs(scene)
    rows = []
    for _ in range(200):
        if len(rows) == 4:
            break
        q = np.asarray(FR3_Q_HOME) + rng.uniform(-0.25, 0.25, 7)
        j = int(rng.integers(0, 7))
        rate = float(rng.uniform(0.01, 0.04)) * (1 if rng.uniform() < 0.5 else -1)
        row = row_of(f"quiet-{len(rows)}", "quiet", "quiet", "step17", q, j, ramp_of(q[j], rate, 0, 6, 12))
        worst = np.inf
        for form in CC.SUBSTEPS:
            rep = CC.replay(CC.quiet_rows(form, [row])[0])
            if rep["pen"].max() > 0.0 or not all(rep["converged"]):
                worst = -1.0
                break
            for qp in rep["qpos"]:
                worst = min(worst, float(scene.distances(scene.frames(qp), pairs).min()))
        print(f"  {row['name']}: clearance over its launches' ends, every form: {worst:.4f} m", file=log, flush=True)
        if worst >= 1.5 * CC.QUIET_CLEARANCE:
            row["clearance"] = worst
            rows.append(row)
    return rows


def from_its_graze_launch(rng, log):
    """Characters that begin where a deep character's graze launch begins, with the velocity it has there: the graze is in launch 0, which
    an environment begins on the lean launch whatever the launches before would have made of it.  (A sweep nears its lowest point along a
    tangent, so the launch BEFORE a graze ends nearer to the contact than it travelled, cannot be certified and sends the environment to
    the contact-resolving launch a launch early: of the swept characters only these have their graze launch itself decided by the lean
    launch's certificate.)  Made from the rows the table already holds."""
    with open(from_its_graze_launch.table) as f:
        table = json.load(f)["characters"]
    rows = []
    for name in ("floor-deep-floor-0", "floor-deep-floor-2", "floor-deep-link-floor-0", "self-deep-self-0", "self-deep-self-2", "self-deep-box-self-0"):
        src = next(r for r in table if r["name"] == name)
        t = src["graze"][0]
        rep = CC.replay(src)
        row = dict(src, name=name + "-launch0", start=[float(x) for x in rep["qpos"][t - 1]], vel=[float(x) for x in rep["qvel"][t - 1]], graze=[])
        row["start"][7:] = [CC.OPEN, CC.OPEN]  # (the slides of the open gripper rest at 0.04 less 7e-8: the table's starts are all alike)
        row["ramp"] = src["ramp"][t:] + [src["ramp"][-1]] * t
        row["from"] = name
        rep = CC.replay(row)
        row["graze"] = [int(k) for k in np.flatnonzero(rep["pen"] > 0.0)]
        ok = row["graze"] == [0] and admit(row, rep, log)
        print(f"  {row['name']}: graze {row['graze']}, depth {rep['pen'][0]}, admitted {bool(ok)}", file=log, flush=True)
        if ok:
            rows.append(row)
    return rows


from_its_graze_launch.table = CC.TABLE  # (main: the table being written)


def tasks():
    """(family task name, function of (rng, log) -> rows), in the table's order."""
    def is_link(names, *which):
        return any(w in names for w in which)

    def floor_deep(rng, log):
        cov = Coverage({"hand": lambda n: is_link(n, "hand"), "finger": lambda n: is_link(n, "finger")})
        return candidates(rng, "floor", "floor-deep", "step17", CC.DEEP, 4, cov, log)

    def floor_deep_links(rng, log):
        cov = Coverage({"link": lambda n: is_link(n, "link5", "link6", "link7")})
        return candidates(rng, "floor", "floor-deep", "step17", CC.DEEP, 1, cov, log, tag="floor-deep-link", draw=draw_floor_wrist_up)

    def floor_deep_more(rng, log):
        return candidates(rng, "floor", "floor-deep", "step17", CC.DEEP, 1, lambda *a: True, log, tag="floor-deep-more")

    def self_deep_box(rng, log):
        return candidates(rng, "self", "self-deep", "step17", CC.DEEP, 1, lambda row, rep: any("pad" in n for n in row["pair"]), log, tag="self-deep-box")

    def self_deep(rng, log):
        seen = {}

        def pairs(row, rep):
            key = tuple(row["pair"])
            if seen.get(key, 0) >= 2:
                return False
            seen[key] = seen.get(key, 0) + 1
            return True

        return candidates(rng, "self", "self-deep", "step17", CC.DEEP, 7, pairs, log)

    def shallow(kind):
        return lambda rng, log: candidates(rng, kind, "shallow", "step17", CC.SHALLOW, 3, lambda *a: True, log, rate=(0.002, 0.008), sweep=10)

    def carried(k, pre, kind, want):
        return lambda rng, log: candidates(rng, kind, "carried-slack", "step17", want, 1, lambda row, rep: row["graze"][0] > pre, log, pre=pre, sweep=8, hold=1, tag=f"carried{k}")

    def held(k, n, kind):
        """Carried slack: n launches at rest on the start pose, whose certificates pass and write and charge the slack record, then one
        large step of the target: the first moving launch is the graze launch, and the environment begins it on the lean launch."""
        def script(a, r):
            return [a] * n + [a + 12.0 * r] * (CC.LAUNCHES["step17"] - n)

        def accept(row, rep):
            row["quiet_before"] = n
            return row["graze"] == [n]

        return lambda rng, log: candidates(rng, kind, "carried-slack", "step17", CC.SHALLOW, 1, accept, log, script=script, sweep=12, tag=f"held{k}")

    def there_and_back(kind):
        return lambda rng, log: candidates(rng, kind, "there-and-back", "step17", CC.DEEP, 1, lambda row, rep: row["graze"][1] - row["graze"][0] >= 5, log,
                                           sweep=5, hold=5, back=2, n_graze=2)

    def there_and_back_long(kind):
        # (three launches through the lowest point, nine at rest beyond it -- long enough for the environment to go back to the lean
        # launch --, three launches back)
        return lambda rng, log: candidates(rng, kind, "there-and-back", "step17", CC.DEEP, 1, lambda row, rep: row["graze"][1] - row["graze"][0] >= 9, log,
                                           sweep=3, hold=9, back=2, n_graze=2, tag="there-and-back-long")

    def env_call(rng, log, accept, tag, tries):
        # (one relative action of at most 5 degrees from rest; the depth joint stays inside the env's joint limits)
        return candidates(rng, "floor", "convergence-pieces", "env", CC.DEEP, 1, accept, log, rate=(0.06, 0.087), sweep=1, hold=1, tag=tag, tries=tries, aim=4e-5, draw=draw_near_a_known_graze)  # (a 5 degree sweep is too short to be clear at both ends of a deeper graze)

    def middle(row, rep):
        t, k = row["graze"][0], CC.SUBSTEPS[row["form"]]
        return rep["first"][t] >= k // 4 and rep["last"][t] < 3 * k // 4

    def inside(row, rep):
        a, b = row["substeps"]
        return a // CC.PIECE == b // CC.PIECE and a % CC.PIECE >= 4 and b % CC.PIECE <= CC.PIECE - 5

    def straddles(row, rep):
        a, b = row["substeps"]
        return a // CC.PIECE + 1 == b // CC.PIECE

    t = [("floor-deep", floor_deep), ("floor-deep-link", floor_deep_links), ("floor-deep-more", floor_deep_more), ("self-deep", self_deep), ("self-deep-box", self_deep_box), ("shallow-floor", shallow("floor")), ("shallow-self", shallow("self"))]
    t += [(f"carried{k}", carried(k, *a)) for k, a in enumerate(((1, "floor", CC.DEEP), (3, "self", CC.DEEP), (8, "floor", CC.SHALLOW), (8, "self", CC.DEEP), (3, "floor", CC.DEEP)))]
    t += [("there-and-back-floor", there_and_back("floor")), ("there-and-back-self", there_and_back("self"))]
    t += [("long48", lambda rng, log: candidates(rng, "floor", "long-launch", "step48", CC.DEEP, 1, middle, log, rate=(0.1, 0.25), sweep=3, hold=2)),
          ("long100", lambda rng, log: candidates(rng, "self", "long-launch", "step100", CC.DEEP, 1, middle, log, rate=(0.2, 0.5), sweep=3, hold=2)),
          ("inside", lambda rng, log: candidates(rng, "floor", "convergence-pieces", "converge", CC.DEEP, 1, inside, log, rate=(0.3, 0.9), sweep=1, hold=1, tag="inside")),
          ("straddle", lambda rng, log: candidates(rng, "floor", "convergence-pieces", "converge", CC.DEEP, 1, straddles, log, rate=(0.3, 0.9), sweep=1, hold=1, tag="straddle", tries=20000)),
          ("quiet", quiet_rows), ("launch0", from_its_graze_launch)]
    t += [(f"held{k}", held(k, n, kind)) for k, (n, kind) in enumerate(((1, "floor"), (3, "floor"), (8, "floor"), (3, "self")))]
    # (the same for a self character was tried with three seeds: the folded arm never left the contact-resolving launch in the rest)
    t += [("there-and-back-long-floor", there_and_back_long("floor"))]
    t += [("env-inside", lambda rng, log: env_call(rng, log, inside, "env-inside", 4000)), ("env-straddle", lambda rng, log: env_call(rng, log, straddles, "env-straddle", 20000))]
    return t


# The random stream of every task, fixed when the table's rows were found: a task added later takes a key of its own choosing and leaves the
# others' streams -- and the rows they find -- alone.
STREAM = {"floor-deep": 0, "floor-deep-link": 1, "self-deep": 2, "self-deep-box": 3, "shallow-floor": 3, "shallow-self": 4, "carried0": 5, "carried1": 6,
          "carried2": 7, "carried3": 8, "carried4": 9, "there-and-back-floor": 10, "there-and-back-self": 11, "long48": 12, "long100": 13, "inside": 14,
          "straddle": 16, "quiet": 17, "floor-deep-more": 18, "launch0": 19, "held0": 20, "held1": 21, "held2": 22, "held3": 23,
          "there-and-back-long-floor": 24, "there-and-back-long-self": 25, "env-inside": 26, "env-straddle": 27}  # (two tasks share key 3: harmless, they draw differently)


def run_task(args):
    seed, index = args
    name, fn = tasks()[index]
    t0 = time.time()
    rows = fn(np.random.default_rng([seed, STREAM[name]]), sys.stdout)
    for r in rows:
        # what the GPU test asserts of the escalation bits BEFORE a graze launch: a graze in the first launch after the hard start, or after
        # launches at rest on the start pose, begins on the lean launch; a long rest between two grazes takes the environment back to it
        # (held: the floor ones -- a link's height is an exact number, while a hull pair at rest within microns of touching is not proven
        # apart by the certificate's single-precision narrow phase and is on the contact-resolving launch while it rests: reported, not asserted)
        if r["graze"] and (r["graze"][0] == 0 or (name.startswith("held") and r["kind"] == "floor")):
            r["lean"] = True
        if r["family"] == "there-and-back":
            r["returns"] = True
    for r in rows:  # (a table may be merged from the runs of several seeds: a row says which one found it)
        r["seed"] = seed
        if seed:
            r["name"] += f"-s{seed}"
    print(f"{name}: {len(rows)} rows in {time.time() - t0:.0f} s", flush=True)
    return rows


def main():
    import concurrent.futures as F

    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=CC.TABLE)
    ap.add_argument("--only", default="", help="comma-separated task names (default: all)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--merge", action="store_true", help="keep the rows the table already has (but those found again), in the families' order")
    args = ap.parse_args()
    todo = [i for i, (name, _) in enumerate(tasks()) if not args.only or name in args.only.split(",")]
    # tasks made from rows of the table run when the others have written theirs
    last = [i for i in todo if tasks()[i][0] in ("launch0", "env-inside", "env-straddle")]
    todo = [i for i in todo if i not in last]
    from_its_graze_launch.table = args.out
    parts = {}
    kept = []
    if args.merge and os.path.exists(args.out):
        with open(args.out) as f:
            kept = json.load(f)["characters"]
    with F.ProcessPoolExecutor(args.jobs) as pool:
        futures = {pool.submit(run_task, (args.seed, i)): i for i in todo}
        for fu in F.as_completed(futures):  # (the table is rewritten as the tasks finish, in the tasks' order)
            parts[futures[fu]] = fu.result()
            rows = [r for i in sorted(parts) for r in parts[i]]
            rows = sorted([r for r in kept if r["name"] not in {x["name"] for x in rows}] + rows, key=lambda r: CC.FAMILIES.index(r["family"]))
            with open(args.out, "w") as f:
                f.write('{"seed": %d, "characters": [\n' % args.seed)
                f.write(",\n".join(json.dumps(r) for r in rows))
                f.write("\n]}\n")
    for i in last:
        parts[i] = run_task((args.seed, i))
        rows = [r for k in sorted(parts) for r in parts[k]]
        rows = sorted([r for r in kept if r["name"] not in {x["name"] for x in rows}] + rows, key=lambda r: CC.FAMILIES.index(r["family"]))
        with open(args.out, "w") as f:
            f.write('{"seed": %d, "characters": [\n' % args.seed)
            f.write(",\n".join(json.dumps(r) for r in rows))
            f.write("\n]}\n")
    print(f"{len(rows)} rows -> {args.out}")


if __name__ == "__main__":
    main()
