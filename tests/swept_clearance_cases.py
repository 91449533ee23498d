"""Ground truth for the swept clearance query (csrc/swept_team.h), independent of the library under test.

* distances: clearance_cases.Scene, the numpy GJK over the oracle's frames;
* the pair list and the levers: the stand-alone host program test_collision_tables_cpu.py drives (tests/host/collision_tables_main.cpp
  with csrc/model.cpp: `query_pairs`, `chk_ent`, `link_lever` with `lev_geom`), run on the CPU;
* the per-pair Lipschitz constants L_p of a segment: the lever sums restated in numpy (reach of the two geoms over the joints between
  their links, rounded up as the kernel rounds);
* the bracket restated in numpy: exact truth at every sample, the Piyavskii-Shubert bound, bisection of the piece of the smallest
  bound (`bracket`).

tools/make_swept_clearance_fixture.py writes tests/golden/swept_clearance_cases.json with it; the CPU test proves the fixture, the GPU
test holds the kernel against it."""

import json
import math
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "robot-control-stack_amd")
CSRC = os.path.join(PKG, "csrc")
for p in (PKG, os.path.join(ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import clearance_cases as CC  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "swept_clearance_cases.json")
SCENES = ("fr3_empty_world", "fr3_simple_pick_up", "xarm7_pick_world")
N_DENSE = 257
SWEPT_BUDGET = 2048          # kSweptBudget (csrc/swept_team.h)
SWEPT_CONTACT_BUDGET = 256   # kSweptContactBudget
CLASSES = ("interior", "end0", "end1", "zero", "fingers_only", "wrist_only", "rigid_pair", "two_minima", "beyond", "stroke",
           "graze_floor", "graze_link", "contact")


def load_fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def scene_xml(scene):
    return os.path.join(PKG, "rcs_amd", "scenes", scene, "scene.xml")


def host_tables(scenes=SCENES):
    """{scene: the host program's JSON}: model.cpp's table builders run on the CPU, as test_collision_tables_cpu.py runs them."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no host C++ compiler"
    out = {}
    with tempfile.TemporaryDirectory() as d:
        obj = os.path.join(d, "model.o")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-c", os.path.join(CSRC, "model.cpp"), "-o", obj])
        for scene in scenes:
            sd = os.path.join(d, scene)
            os.mkdir(sd)
            inc = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "export_model_c.py"), scene_xml(scene)], text=True)
            with open(os.path.join(sd, "model.inc"), "w") as f:
                f.write(inc)
            prog = os.path.join(sd, "collision_tables")
            subprocess.check_call([cxx, "-std=c++17", "-O1", f"-I{sd}", f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "collision_tables_main.cpp"),
                                   obj, "-o", prog])
            out[scene] = json.loads(subprocess.check_output([prog], text=True))
    return out


class Tables:
    """What the kernel's per-pair constants are made of, from the host program's JSON of one scene."""

    def __init__(self, cm, J):
        self.J = J
        self.nl = int(J["nl"])
        self.geom_ids = [int(g["geom_id"]) for g in J["geoms"]]      # table index -> mjModel geom id
        self.glink = [int(g["link"]) for g in J["geoms"]]             # table index -> link (-1: welded to the world)
        self.index = {g: i for i, g in enumerate(self.geom_ids)}
        lev = np.asarray(J["link_lever"], dtype=np.float64)
        self.lev_geom = lev[int(J["lev_geom"]):].reshape(12, 32)      # [joint][table geom]
        self.ent = [(int(a), int(b), int(c) - 1) for a, b, c, _ in J["chk_ent"]]
        self.plane_geom, self.box_geom = int(J["plane_geom"]), int(J["box_geom"])
        # ancestors-or-self of every link, as joint bits: joint j is link j (one joint per body)
        A = cm.arrays
        jbody = [int(b) for b in np.asarray(A["jnt_bodyid"])[: self.nl]]
        parent = np.asarray(A["body_parentid"])
        of_body = {b: j for j, b in enumerate(jbody)}
        self.anc = {-1: 0}
        for j, b in enumerate(jbody):
            m = 0
            while b > 0:
                if b in of_body:
                    m |= 1 << of_body[b]
                b = int(parent[b])
            self.anc[j] = m

    def pairs(self, kinds):
        # (the list of a kinds mask is its kinds' lists in order: floor, self, free body -- the program prints the single kinds)
        return [(int(a), int(b)) for k in (1, 2, 4) if kinds & k for a, b in self.J["query_pairs"][str(k)]["ids"]]

    def reach(self, g, l, c, trav):
        if l < 0:
            return 0.0
        jm = self.anc[l] & ~self.anc[c]
        return float(sum(np.float32(self.lev_geom[j, g]) * trav[j] for j in range(self.nl) if jm >> j & 1))

    def lipschitz(self, kinds, q_from, q_to):
        """L_p of every pair of the list for `kinds`, in the list's order, for the segment q_from -> q_to."""
        trav = np.abs(np.asarray(q_to, dtype=np.float64) - np.asarray(q_from, dtype=np.float64))
        up = lambda r: 0.0 if r == 0.0 else r * 1.000001 + 1e-12  # noqa: E731
        self_i = 0
        out = []
        for a, b in self.pairs(kinds):
            if a == self.plane_geom:
                g = self.index[b]
                out.append(up(self.reach(g, self.glink[g], -1, trav)))
            elif self.box_geom in (a, b):
                g = self.index[b if a == self.box_geom else a]
                out.append(up(self.reach(g, self.glink[g], -1, trav)))
            else:
                g0, g1, c = self.ent[self_i]
                self_i += 1
                assert {self.geom_ids[g0], self.geom_ids[g1]} == {a, b}
                out.append(up(self.reach(g0, self.glink[g0], c, trav) + self.reach(g1, self.glink[g1], c, trav)))
        return np.array(out)


def finger_mask(cm, pairs, dof):
    """SimRobot.clearance_mask's default, restated: 0 for the pairs of two gripper-finger geoms."""
    arr = cm.arrays
    bodies = {int(b) for b in np.asarray(arr["jnt_bodyid"])[dof:]}
    fingers = {g for g, b in enumerate(np.asarray(arr["geom_bodyid"])) if int(b) in bodies}
    return np.array([0 if (a in fingers and b in fingers) else 1 for a, b in pairs], dtype=np.uint8)


def leaves_stroke(cm, q_from, q_to):
    """Does a slide leave qpos0 -+ the stroke its levers were built for (the larger distance of qpos0 from its range's ends)?"""
    A = cm.arrays
    nl = int(cm.nq)
    for j in range(nl):
        if int(np.asarray(A["jnt_type"])[j]) != 2:
            continue
        q0 = float(np.asarray(A["qpos0"])[j])
        stroke = max(abs(float(cm.jnt_range[j, 0]) - q0), abs(float(cm.jnt_range[j, 1]) - q0))
        if any(not (q0 - stroke <= float(q[j]) <= q0 + stroke) for q in (q_from, q_to)):
            return True
    return False


_SCENES = {}


def cpu_scene(name):
    """(compiled scene, ground-truth scene, oracle collider, home, arm dof) of a scene, on the CPU alone."""
    if name in _SCENES:
        return _SCENES[name]
    import rcs_oracle as O
    from rcs_amd.envs import default_sim_robot_cfg, xarm7_pick_sim_robot_cfg
    from rcs_amd.mjcf import compile_mjcf
    from rcs_env_oracle import FR3_Q_HOME, XARM7_PICK
    from test_gpu_collision_query import OracleCollider

    if name == "xarm7_pick_world":
        cfg = xarm7_pick_sim_robot_cfg()
        cm = compile_mjcf(cfg.mjcf_scene_path)
        R = XARM7_PICK
        tcp = O.Pose(translation=np.array([0.0, 0.0, 0.1034]))
        osim = O.Sim(cm, R["joints"], R["actuators"], R["site"], R["base"], R["q_home"], tcp, R["gripper_joint"], R["gripper_actuator"],
                     arm_collision_geoms=[], gripper_cfg=R["gripper_cfg"])
        home = np.asarray(R["q_home"], dtype=np.float64)
    else:
        cfg = default_sim_robot_cfg(name)
        cm = compile_mjcf(cfg.mjcf_scene_path)
        arm = [f"fr3_joint{i}_0" for i in range(1, 8)]
        osim = O.Sim(cm, arm, arm, "attachment_site_0", "base_0", FR3_Q_HOME, None, "finger_joint1_0", "actuator8_0")
        home = np.asarray(FR3_Q_HOME, dtype=np.float64)
    _SCENES[name] = (cm, CC.Scene(cm), OracleCollider(osim), home, len(home))
    return _SCENES[name]


def config(row, s):
    a, b = np.asarray(row["q_from"], dtype=np.float64), np.asarray(row["q_to"], dtype=np.float64)
    return b.copy() if s == 1.0 else a + s * (b - a)


def selected_pairs(pairs, mask):
    return [p for p, m in zip(pairs, mask) if m]


def truth_at(sc, q, box, sub):
    """(clearance, index into `sub` of the pair that attains it, per-pair distances with inf where pruned) at one configuration."""
    fr = sc.frames(q, box)
    dd = sc.distances(fr, sub)
    if not len(dd):
        return math.inf, -1, dd
    i = int(np.argmin(dd))
    return float(dd[i]), i, dd


def pair_values(sc, q, box, sub, below):
    """A LOWER BOUND of every pair's distance at q: exact where the bounding spheres' bound is under `below`, that bound elsewhere."""
    fr = sc.frames(q, box)
    out = np.empty(len(sub))
    for i, (a, b) in enumerate(sub):
        lb = sc.lower_bound(fr, a, b)
        out[i] = sc.pair_distance(fr, a, b)[0] if lb < below else lb
    return out


def bracket(values_at, L, tolerance, d_max=math.inf, budget=SWEPT_BUDGET):
    """The bracket restated: values_at(s, best) -> per-pair lower bounds (exact near `best`); bisect the piece of the smallest bound
    until every piece's bound is >= min(best - tolerance, d_max).  Returns (best, s_best, lower, evals, converged)."""
    L = np.asarray(L, dtype=np.float64)
    v0, v1 = values_at(0.0, math.inf), values_at(1.0, math.inf)
    evals = 2
    best, s_best = (float(v0.min()), 0.0) if v0.min() <= v1.min() else (float(v1.min()), 1.0)
    bound = lambda a, va, b, vb: float((0.5 * (va + vb - (b - a) * L)).min())  # noqa: E731
    pieces = [(bound(0.0, v0, 1.0, v1), 0.0, v0, 1.0, v1)]
    while True:
        pieces.sort(key=lambda p: p[0])
        lo = pieces[0][0]
        if lo >= min(best - tolerance, d_max):
            return best, s_best, min(best, lo), evals, True
        if evals >= budget:
            return best, s_best, min(best, lo), evals, False
        _, a, va, b, vb = pieces.pop(0)
        m = 0.5 * (a + b)
        vm = values_at(m, best)
        evals += 1
        if vm.min() < best:
            best, s_best = float(vm.min()), m
        pieces.append((bound(a, va, m, vm), a, va, m, vm))
        pieces.append((bound(m, vm, b, vb), m, vm, b, vb))
