"""Contacts that begin AND end inside one launch, for the lean launch's end-of-launch certificate (csrc/check_team.h, fed by chk_dend /
chk_psum / chk_q0 in csrc/sim_kernels.h), built from the oracle alone.

With the robot's contacts resolved environment by environment, a launch runs lean (no collision pass in its substeps) because the
certificate proves afterwards that no substep of it can have been in contact.  A certificate that passes a launch it should not have
passed crashes nothing and flags nothing: the arm is stepped through the floor or through itself.  A contact that persists is caught
by looking at the position the launch ends on; the certificate exists for the graze -- a few substeps of penetration in the middle of
a launch whose two ends are clear.  The rows of tests/golden/certificate_cases.json (written by tools/make_certificate_cases.py, a
directed search on the oracle) are such grazes, made on purpose.

A CHARACTER is a start state and a script, in fr3_empty_world with the gripper commanded open (shut fingers pressed together are the
one regime in which the oracle does not reproduce itself):
  * `start`  nine numbers, the arm's joints and the two finger slides (0.04: open), hard-set; `vel` nine velocities or null;
  * `target0`, `joint`, `ramp`  the absolute joint target of launch t (SimRobot.set_joint_position before the launch) is `target0` with
     entry `joint` replaced by ramp[t]: a ramp drives one joint at a chosen speed through the pose at which a geom is nearest to the
     floor or to another geom, and the other joints decide how deep that pose is;
  * `form`   "step17" / "step48" / "step100": Sim.step(k) launches under asynchronous control; "converge": step_until_convergence under
     synchronous control (cap 500, cut into pieces of 48 substeps by the kernels' launcher); "env": the same through the env layer -- the
     fused env step, JOINTS relative to the last step, where `ramp` gives the relative action of call t as ramp[t] - ramp[t - 1];
  * `graze`  the launches in which the resolving oracle sees a penetration; every other launch of the script is quiet (pen_seen == 0);
  * `family`, `kind` ("floor" / "self" / "quiet"), `lowest` (the link of the deepest floor contact) or `pair` (the geom pair of the deepest
     self contact), `substeps` (convergence family: first and last penetrating substep of the graze call), `quiet_before` (carried slack),
     `from` (the character whose graze launch this one begins at, with its velocity: the graze is then in launch 0).

tests/test_certificate_cases_cpu.py replays every row on the oracle and asserts what the row claims; tests/test_gpu_certificate_cases.py
holds the kernels to the rows.  replay() is the one replay both use.
"""

from __future__ import annotations

import functools
import json
import os

import numpy as np

OPEN = 0.04                      # finger slides of the open gripper
PIECE = 48                       # substeps of one piece of step_until_convergence (the kernels' launcher)
DEEP = (3e-5, 5e-4)              # m, deepest penetration of a graze launch: the deep families
SHALLOW = (1e-8, 1e-5)           # ... the shallow family
SEEN = 1e-8                      # 10 x kCheckTouch (csrc/check_team.h): deeper than this, the launch must have been escalated
RESOLVED_GAP = 1e-6              # rad: the resolving and the non-resolving oracle differ by at least this after a deep graze launch
from parity_util import MANY_CONTACT_SPLIT as TWIN_SPLIT, MANY_CONTACT_TWIN_NUDGE as TWIN_NUDGE  # noqa: E402  (1e-10; 1e-13 rad on qpos[3])
QUIET_CLEARANCE = 0.01           # m: what the quiet characters keep from everything
SUBSTEPS = {"step17": 17, "step48": 48, "step100": 100, "converge": None, "env": None}
LAUNCHES = {"step17": 18, "step48": 6, "step100": 6, "converge": 4, "env": 4}  # every script of a form has this many launches (a batch steps together)
REST_LAUNCHES = 3                # launches a batch rests at quiet poses before the state-write variants write the start states
FAMILIES = ("floor-deep", "self-deep", "shallow", "carried-slack", "there-and-back", "long-launch", "convergence-pieces", "quiet")
DEEP_FAMILIES = ("floor-deep", "self-deep", "carried-slack", "there-and-back", "long-launch", "convergence-pieces")
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "certificate_cases.json")
ARM = [f"fr3_joint{i}_0" for i in range(1, 8)]


@functools.lru_cache(maxsize=None)
def characters():
    """The rows of the table, in its order."""
    with open(TABLE) as f:
        rows = json.load(f)["characters"]
    assert len({r["name"] for r in rows}) == len(rows)
    return tuple(rows)


def by_form(form, rows=None):
    return [r for r in (characters() if rows is None else rows) if r["form"] == form]


def depth_range(row):
    """The range the deepest penetration of a graze launch must lie in (a shallow row of another family says so by `shallow`)."""
    return SHALLOW if row["family"] == "shallow" or row.get("shallow") else DEEP


def launches(row):
    return len(row["ramp"])


def targets(row):
    """[launches, 7]: the absolute joint target of every launch."""
    t = np.tile(np.asarray(row["target0"], dtype=np.float64), (launches(row), 1))
    t[:, row["joint"]] = row["ramp"]
    return t


def start_state(row):
    """(qpos [9], qvel [9])"""
    vel = row.get("vel")
    return np.asarray(row["start"], dtype=np.float64), np.zeros(9) if vel is None else np.asarray(vel, dtype=np.float64)


@functools.lru_cache(maxsize=None)
def compiled_model():
    from rcs_amd.envs import default_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf

    return compile_mjcf(default_sim_robot_cfg("fr3_empty_world").mjcf_scene_path)


def make_oracle(form, resolve=3):
    """One oracle environment the way the kernels' Sim + SimRobot + SimGripper stand after their first substep at home."""
    import rcs_oracle as O
    from rcs_env_oracle import FR3_Q_HOME

    o = O.Sim(compiled_model(), ARM, ARM, "attachment_site_0", "base_0", FR3_Q_HOME, None, "finger_joint1_0", "actuator8_0", resolve_contacts=resolve)
    o.s.async_control = int(form != "converge")
    o.reset(); o.robot_reset(); o.gripper_reset(); o.step(1)
    return o


def place(o, qpos9, qvel9, nudge=0.0):
    """What set_joints_hard + set_qpos + set_qvel do to an environment of the kernels'."""
    o.set_joints_hard(qpos9[:7])
    for k in range(9):
        o.s.d.qpos[k] = float(qpos9[k])
        o.s.d.qvel[k] = float(qvel9[k])
    o.s.d.qpos[3] += nudge


def static_contacts(o, touch=1e-9):
    from parity_util import oracle_contacts_at_current_qpos

    return oracle_contacts_at_current_qpos(o, touch)


def _deepest(o):
    """(depth, kind, names) of the deepest entry of the oracle's last collision pass: the link of a floor contact, the geom pair of a self
    contact.  (0.0, None, None): nothing penetrates."""
    cm, d = compiled_model(), o.s.d
    best = (0.0, None, None)
    for i in range(d.ncon):
        c = d.contact[i]
        if -c.dist > best[0] and (c.body[0] <= 0 or c.body[1] <= 0):
            g = c.geom[1] if c.body[0] <= 0 else c.geom[0]
            best = (-c.dist, "floor", cm.body_names[int(cm.arrays["geom_bodyid"][g])])
    for i in range(d.nself):
        if d.self_depth[i] > best[0]:
            ga, gb = sorted((int(d.self_geom[i][0]), int(d.self_geom[i][1])))
            best = (float(d.self_depth[i]), "self", [cm.geom_names[ga], cm.geom_names[gb]])
    return best


def actions(row):
    """[launches, 7]: the relative joint actions of an "env" row -- the swept joint's step from one entry of `ramp` to the next."""
    a = np.zeros((launches(row), 7))
    a[:, row["joint"]] = np.diff([row["start"][row["joint"]]] + list(row["ramp"]))
    return a


def make_oracle_env(resolve=3):
    """One oracle environment of the env layer: JOINTS relative to the last step (+-5 degrees), synchronous control."""
    import rcs_oracle as O
    from parity_util import make_oracle_envs

    saved = O.DEFAULT_RESOLVE_CONTACTS
    try:
        O.DEFAULT_RESOLVE_CONTACTS = resolve
        oe = make_oracle_envs(1, False)[0]
    finally:
        O.DEFAULT_RESOLVE_CONTACTS = saved
    assert oe.sim.model.resolve_contacts == (resolve or 0)
    return oe


def _replay_env(row, resolve, nudge):
    """replay() of an "env" row: RobotEnv.step of the oracle's env layer per call.  A second instance takes the call whole and says how many
    substeps it took; the first one's step_until_convergence is then that many single substeps, looked at one by one."""
    q0, v0 = start_state(row)
    oe, om = make_oracle_env(resolve), make_oracle_env(resolve)
    for x in (oe, om):
        x.reset()
        place(x.sim, q0, v0, nudge)
    o = oe.sim
    out = {k: [] for k in ("pen", "ends", "begins", "qpos", "qvel", "steps", "first", "last", "deepest", "converged", "truncated")}
    seen = {}

    def substeps():
        pen, first, last, deepest = 0.0, -1, -1, (0.0, None, None)
        for s in range(seen["k"]):
            o.s.d.pen_seen = 0.0
            o.step(1)
            p = float(o.s.d.pen_seen)
            if p > 0.0:
                first, last = (s if first < 0 else first), s
                dp = _deepest(o)
                if dp[0] > deepest[0]:
                    deepest = dp
            pen = max(pen, p)
        seen.update(pen=pen, first=first, last=last, deepest=deepest)

    o.step_until_convergence = substeps
    for act in actions(row):
        out["begins"].append(static_contacts(o))
        _, _, _, trunc, _ = om.step({"joints": act, "gripper": 1.0})
        seen["k"] = int(om.sim.s.convergence_steps)
        oe.step({"joints": act, "gripper": 1.0})
        assert np.array_equal(np.asarray(om.sim.qpos), np.asarray(o.qpos)), "the counting instance took another path"
        out["converged"].append(bool(om.sim.s.converged)); out["truncated"].append(bool(trunc))
        out["pen"].append(seen["pen"]); out["first"].append(seen["first"]); out["last"].append(seen["last"]); out["deepest"].append(seen["deepest"])
        out["steps"].append(seen["k"])
        out["ends"].append(static_contacts(o))
        out["qpos"].append(np.array(o.qpos)[:9]); out["qvel"].append(np.array(o.qvel)[:9])
    for k in ("pen", "qpos", "qvel", "steps", "first", "last"):
        out[k] = np.asarray(out[k])
    return out


def replay(row, resolve=3, nudge=0.0, rest=None):
    """The row on the oracle, a substep at a time.  Per launch: `pen` (the deepest penetration any collision pass of the launch saw),
    `ends` (contacts at the position the launch ends on: (ncon, nself)), `begins` (the same before it), `qpos`, `qvel` [9], `steps` (the
    substeps of the launch), `first` / `last` (the first and last substep whose collision pass saw a penetration, -1: none), `deepest`
    (kind and names of the deepest contact).  `rest`: (launches, qpos9) -- rest there first, with the pose as the target, then hard-set
    the row's start (the GPU test's state-write variants)."""
    form = row["form"]
    if form == "env":
        assert rest is None
        return _replay_env(row, resolve, nudge)
    o = make_oracle(form, resolve)
    q0, v0 = start_state(row)
    if rest is not None:
        place(o, rest[1], np.zeros(9))
        o.set_joint_position(rest[1][:7])
        for _ in range(rest[0]):
            o.step_until_convergence() if form == "converge" else o.step(SUBSTEPS[form])
    place(o, q0, v0, nudge)
    mirror = None
    if form == "converge":  # the counting instance: it decides how many substeps a call takes, `o` is stepped that many one at a time
        mirror = make_oracle(form, resolve)
        if rest is not None:
            place(mirror, rest[1], np.zeros(9))
            mirror.set_joint_position(rest[1][:7])
            for _ in range(rest[0]):
                mirror.step_until_convergence()
        place(mirror, q0, v0, nudge)
    out = {k: [] for k in ("pen", "ends", "begins", "qpos", "qvel", "steps", "first", "last", "deepest", "converged")}
    for tgt in targets(row):
        out["begins"].append(static_contacts(o))
        o.set_joint_position(tgt)
        if mirror is not None:
            mirror.set_joint_position(tgt)
            mirror.step_until_convergence()
            k = int(mirror.s.convergence_steps)
            out["converged"].append(bool(mirror.s.converged))
        else:
            k = SUBSTEPS[form]
            out["converged"].append(True)
        pen, first, last, deepest = 0.0, -1, -1, (0.0, None, None)
        for s in range(k):
            o.s.d.pen_seen = 0.0
            o.step(1)
            p = float(o.s.d.pen_seen)
            if p > 0.0:
                first, last = (s if first < 0 else first), s
                dp = _deepest(o)
                if dp[0] > deepest[0]:
                    deepest = dp
            pen = max(pen, p)
        if mirror is not None:
            assert np.array_equal(np.asarray(mirror.qpos), np.asarray(o.qpos)), "the counting instance took another path"
        out["pen"].append(pen); out["first"].append(first); out["last"].append(last); out["deepest"].append(deepest); out["steps"].append(k)
        out["ends"].append(static_contacts(o))
        out["qpos"].append(np.array(o.qpos)[:9]); out["qvel"].append(np.array(o.qvel)[:9])
    for k in ("pen", "qpos", "qvel", "steps", "first", "last"):
        out[k] = np.asarray(out[k])
    return out


@functools.lru_cache(maxsize=None)
def oracle_run():
    """name -> replay(row) on the resolving oracle, once for all the tests."""
    return {r["name"]: replay(r) for r in characters()}


# Link 0 and link 1 are 1 mm apart in EVERY pose (joint 1 turns link 1 about the axis the two hulls share; link 0 is welded to the world, so
# MuJoCo's parent-child filter does not drop the pair): "a centimetre from everything" cannot include it.
ALWAYS_NEAR = ("fr3_link0_collision_0", "fr3_link1_collision_0")


def clearance_pairs(scene):
    """The geom pairs (and floor, geom) pairs a quiet character keeps its distance from: every pair MuJoCo's filter admits but ALWAYS_NEAR,
    and the floor against every geom of a moving body.  `scene`: a tests/clearance_cases.py Scene."""
    names = compiled_model().geom_names
    pairs = [(a, b) for a, b in scene.admitted_pairs() if {names[a], names[b]} != set(ALWAYS_NEAR)]
    return pairs + [(scene.plane_geom, g) for g in range(scene.ngeom)
                    if g != scene.plane_geom and len(scene.local_points[g]) and scene.weld[scene.gbody[g]] != 0]


# ------------------------------------------------------------------------------------------------------------------- arrangements
def quiet_rows(form, rows=None):
    """The quiet characters as neighbours of a batch of `form`: their scripts are Sim.step(17) scripts, their ramps move a few degrees a
    launch and stop, which every launch form steps without coming near anything (tests/test_certificate_cases_cpu.py replays them in
    every form)."""
    return [dict(r, form=form, ramp=r["ramp"][:LAUNCHES[form]]) for r in (characters() if rows is None else rows) if r["family"] == "quiet"]


def arrangements(form, rows=None):
    """name -> list of rows, one per environment, for the graze characters of one launch form:
      * "once"     every character once, the quiet ones last: the batch every other arrangement is compared with, bit for bit;
      * "team<p>"  every graze character at position p of a wavefront's four teams, with three quiet neighbours (more than 32 graze
                   characters: in batches "team<p>a", "team<p>b" of at most 32 wavefronts);
      * "packed"   graze characters four to a wavefront, no quiet neighbour;
      * "ragged"   a batch whose size is no multiple of 4: the graze characters in reverse order, then quiet ones up to n % 4 == 3."""
    graze = [r for r in by_form(form, rows) if r["family"] != "quiet"]
    quiet = quiet_rows(form, rows)
    assert len(quiet) == 4
    t = {"once": graze + quiet}
    chunks = [graze[i:i + 32] for i in range(0, len(graze), 32)]  # (at most 128 environments a batch)
    for p in range(4):
        for c, chunk in enumerate(chunks):
            arr = []
            for i, r in enumerate(chunk):
                team = [quiet[(i + k) % 4] for k in range(3)]
                team.insert(p, r)
                arr += team
            t[f"team{p}" + ("" if len(chunks) == 1 else "abcd"[c])] = arr
    t["packed"] = list(graze)
    rag = graze[::-1]
    k = 0
    while len(rag) % 4 != 3:
        rag.append(quiet[k % 4])
        k += 1
    t["ragged"] = rag
    return t
