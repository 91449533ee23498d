"""Ground truth for the clearance queries (csrc/clearance_team.h), independent of the library under test: numpy and the oracle only.

* world frames of every geom from the oracle's kinematics (orc_kinematics -> xpos / xmat, with geom_pos / geom_quat of the compiled
  scene), joint anchors and axes from xanchor / xaxis;
* shapes as point sets plus a radius: hull vertices, the 8 corners of a box, the two ends of a capsule's segment;
* a GJK over point sets whose sub-simplex step is exhaustive (every sub-simplex is solved, the nearest admissible projection wins);
  it returns the distance, the witnesses and the separating-plane LOWER bound, so every answer carries its own error bar
  (distance - lower: the duality gap);
* MuJoCo's geom-pair filter, restated from the rule in oracle/rcs_contact.c list_pairs.
"""

import ctypes as C
import itertools
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

PLANE, CAPSULE, BOX, MESH = 0, 3, 6, 7


# ---- small vector algebra on tuples (python floats: faster than numpy at this size)
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _project(pts):
    """Weights of the origin's projection onto the affine hull of 1..4 points, or None where the points are degenerate."""
    a = pts[0]
    if len(pts) == 1:
        return (1.0,)
    w = (-a[0], -a[1], -a[2])
    if len(pts) == 2:
        d = _sub(pts[1], a)
        dd = _dot(d, d)
        if not dd > 0.0:
            return None
        t = _dot(w, d) / dd
        return (1.0 - t, t)
    e1, e2 = _sub(pts[1], a), _sub(pts[2], a)
    if len(pts) == 3:
        n = _cross(e1, e2)
        nn = _dot(n, n)
        if not nn > 1e-20 * _dot(e1, e1) * _dot(e2, e2):
            return None
        s = _dot(_cross(w, e2), n) / nn
        t = _dot(_cross(e1, w), n) / nn
        return (1.0 - s - t, s, t)
    e3 = _sub(pts[3], a)
    c23 = _cross(e2, e3)
    det = _dot(e1, c23)
    if not det * det > 1e-24 * _dot(e1, e1) * _dot(e2, e2) * _dot(e3, e3):
        return None
    s, t, u = _dot(w, c23) / det, _dot(w, _cross(e3, e1)) / det, _dot(w, _cross(e1, e2)) / det
    return (1.0 - s - t - u, s, t, u)


def nearest_on_simplex(pts):
    """The point of the simplex (1..4 points, tuples) nearest the origin, by exhaustion: weights per point."""
    best, best_w = math.inf, None
    n = len(pts)
    for k in range(1, n + 1):
        for idx in itertools.combinations(range(n), k):
            lam = _project([pts[i] for i in idx])
            if lam is None or min(lam) < 0.0:
                continue
            p = [sum(l * pts[i][c] for l, i in zip(lam, idx)) for c in range(3)]
            n2 = _dot(p, p) if k < 4 else 0.0
            if n2 < best:
                best = n2
                best_w = [0.0] * n
                for l, i in zip(lam, idx):
                    best_w[i] = l
    return best_w


def gjk(P, Q, max_iter=200, band=1e-15):
    """Distance of the convex hulls of the point sets P [n, 3] and Q [m, 3].  Returns (distance, wa, wb, lower): the witnesses on
    the two hulls and the largest separating-plane bound seen (lower <= true distance <= distance)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    Q = np.asarray(Q, dtype=np.float64).reshape(-1, 3)
    x = tuple(P.mean(0) - Q.mean(0))
    if not _dot(x, x) > 0.0:
        x = (1.0, 0.0, 0.0)
    simplex = []  # (v, i, j): v = P[i] - Q[j]
    lower = 0.0
    wa, wb = P.mean(0), Q.mean(0)
    dist = math.inf
    for _ in range(max_iter):
        nx = math.sqrt(_dot(x, x))
        if simplex and nx <= band:
            return 0.0, wa, wb, 0.0
        xd = np.array(x)
        i, j = int(np.argmin(P @ xd)), int(np.argmax(Q @ xd))
        v = tuple(P[i] - Q[j])
        lower = max(lower, _dot(v, x) / nx)
        if simplex:
            if dist - lower <= band * max(1.0, dist) or any(s[1] == i and s[2] == j for s in simplex):
                break
        simplex.append((v, i, j))
        lam = nearest_on_simplex([s[0] for s in simplex])
        keep = [(s, l) for s, l in zip(simplex, lam) if l > 0.0]
        tot = sum(l for _, l in keep)
        nxt = tuple(sum(l / tot * s[0][c] for s, l in keep) for c in range(3))
        nd = math.sqrt(_dot(nxt, nxt))
        if not nd < dist:
            break
        simplex = [s for s, _ in keep]
        x, dist = nxt, nd
        wa = sum(l / tot * P[s[1]] for s, l in keep)
        wb = sum(l / tot * Q[s[2]] for s, l in keep)
        if len(simplex) == 4:
            return 0.0, wa, wb, 0.0
    return dist, wa, wb, min(lower, dist)


# ---- closed forms used to place a witness on its geom
def point_box_distance(p, R, c, size):
    """Signed distance of a world point from the surface of a box (negative inside)."""
    loc = R.T @ (np.asarray(p) - c)
    d = np.abs(loc) - np.asarray(size)
    out = np.linalg.norm(np.maximum(d, 0.0))
    return out if out > 0.0 else float(d.max())


def point_capsule_distance(p, R, c, radius, half):
    loc = R.T @ (np.asarray(p) - c)
    z = min(max(loc[2], -half), half)
    return float(np.linalg.norm(loc - np.array([0.0, 0.0, z])) - radius)


def quat_to_mat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


_CORNERS = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)


class Frames:
    """One configuration: world frames, point sets and radii of every geom (index ngeom: the free box, if the scene has one)."""

    def __init__(self, scene, R, p, xanchor, xaxis):
        self.scene, self.R, self.p, self.xanchor, self.xaxis = scene, R, p, xanchor, xaxis
        self._pts = {}

    def points(self, g):
        if g not in self._pts:
            self._pts[g] = self.scene.local_points[g] @ self.R[g].T + self.p[g]
        return self._pts[g]

    def sphere(self, g):
        pts = self.points(g)
        c = pts.mean(0)
        return c, float(np.linalg.norm(pts - c, axis=1).max()) + self.scene.radius[g]


class Scene:
    def __init__(self, cm):
        import rcs_oracle as O

        self.cm, self.O, self.L = cm, O, O.lib()
        self.model = O.make_model(cm)
        self.data = O.OrcData()
        A = cm.arrays
        self.ngeom = int(cm.ngeom)
        self.nq = int(cm.nq)
        self.gtype = np.asarray(A["geom_type"], dtype=np.int64)[: self.ngeom]
        self.gbody = np.asarray(A["geom_bodyid"], dtype=np.int64)[: self.ngeom]
        self.gpos = np.asarray(A["geom_pos"], dtype=np.float64).reshape(-1, 3)
        self.gquat = np.asarray(A["geom_quat"], dtype=np.float64).reshape(-1, 4)
        self.gsize = np.asarray(A["geom_size"], dtype=np.float64).reshape(-1, 3)
        self.parent = np.asarray(A["body_parentid"], dtype=np.int64)
        self.weld = np.asarray(A["body_weldid"], dtype=np.int64)
        self.contype = np.asarray(A["geom_contype"], dtype=np.int64)
        self.conaff = np.asarray(A["geom_conaffinity"], dtype=np.int64)
        self.jbody = np.asarray(A["jnt_bodyid"], dtype=np.int64)
        self.jtype = np.asarray(A["jnt_type"], dtype=np.int64)
        vadr, vnum = np.asarray(A["geom_vertadr"], dtype=np.int64), np.asarray(A["geom_vertnum"], dtype=np.int64)
        verts = np.asarray(A["mesh_vert"], dtype=np.float64).reshape(-1, 3)
        self.local_points, self.radius = [], []
        for g in range(self.ngeom):
            t = self.gtype[g]
            if t == MESH:
                self.local_points.append(verts[vadr[g]: vadr[g] + vnum[g]].copy())
                self.radius.append(0.0)
            elif t == BOX:
                self.local_points.append(_CORNERS * self.gsize[g])
                self.radius.append(0.0)
            elif t == CAPSULE:
                self.local_points.append(np.array([[0.0, 0.0, -self.gsize[g][1]], [0.0, 0.0, self.gsize[g][1]]]))
                self.radius.append(float(self.gsize[g][0]))
            else:
                self.local_points.append(np.zeros((0, 3)))
                self.radius.append(0.0)
        free = getattr(cm, "free_bodies", [])
        self.box_size = np.asarray(free[0]["size"], dtype=np.float64) if free else None
        if free:
            self.local_points.append(_CORNERS * self.box_size)
            self.radius.append(0.0)
        self.plane_geom = next((g for g in range(self.ngeom) if self.gtype[g] == PLANE), -1)

    def type_of(self, g):
        return BOX if g == self.ngeom else int(self.gtype[g])

    def size_of(self, g):
        return self.box_size if g == self.ngeom else self.gsize[g]

    def frames(self, q, box=None):
        d = self.data
        for i, x in enumerate(np.asarray(q, dtype=np.float64)[: self.nq]):
            d.qpos[i] = float(x)
        self.L.orc_kinematics(C.byref(self.model), C.byref(d))
        nb = int(self.model.nbody)
        xpos = np.array([list(d.xpos[b]) for b in range(nb)])
        xmat = np.array([list(d.xmat[b]) for b in range(nb)]).reshape(nb, 3, 3)
        R, p = [], []
        for g in range(self.ngeom):
            b = self.gbody[g]
            R.append(xmat[b] @ quat_to_mat(self.gquat[g]))
            p.append(xpos[b] + xmat[b] @ self.gpos[g])
        if self.box_size is not None:
            bq = np.array([0, 0, 0, 1.0, 0, 0, 0]) if box is None else np.asarray(box, dtype=np.float64)
            qn = np.linalg.norm(bq[3:])
            R.append(quat_to_mat(bq[3:] / qn) if qn >= 1e-15 else np.eye(3))
            p.append(bq[:3].copy())
        xanchor = np.array([list(d.xanchor[j]) for j in range(self.nq)])
        xaxis = np.array([list(d.xaxis[j]) for j in range(self.nq)])
        return Frames(self, R, p, xanchor, xaxis)

    # ---- MuJoCo's pair filter (oracle/rcs_contact.c list_pairs): different weld bodies, the contype / conaffinity masks, no
    # parent-child pair unless one side is welded to the world; a pair is ordered by geom type, then by id
    def admitted_pairs(self):
        out = []
        # (a mesh geom without collision vertices has no shape: the oracle's collision pass skips it)
        skip = [self.gtype[g] == PLANE or (self.gtype[g] == MESH and len(self.local_points[g]) == 0) for g in range(self.ngeom)]
        for g1 in range(self.ngeom):
            if skip[g1]:
                continue
            for g2 in range(g1 + 1, self.ngeom):
                if skip[g2]:
                    continue
                w1, w2 = self.weld[self.gbody[g1]], self.weld[self.gbody[g2]]
                if w1 == w2:
                    continue
                if not ((self.contype[g1] & self.conaff[g2]) or (self.contype[g2] & self.conaff[g1])):
                    continue
                pw1, pw2 = self.weld[self.parent[w1]], self.weld[self.parent[w2]]
                if w1 and w2 and (w1 == pw2 or w2 == pw1):
                    continue
                out.append((g2, g1) if self.gtype[g1] > self.gtype[g2] else (g1, g2))
        return out

    # ---- distances
    def pair_distance(self, fr, g0, g1):
        """(distance, wa, wb, gap) of two geoms: the radii are taken off the distance, the witnesses are points of the point sets'
        hulls (a capsule's: of its core segment).  A plane is the first geom."""
        if g0 == self.plane_geom:
            n, c = fr.R[g0][:, 2], fr.p[g0]
            pts = fr.points(g1)
            h = (pts - c) @ n
            i = int(np.argmin(h))
            return float(h[i] - self.radius[g1]), pts[i] - h[i] * n, pts[i], 0.0
        dist, wa, wb, lower = gjk(fr.points(g0), fr.points(g1))
        return dist - self.radius[g0] - self.radius[g1], wa, wb, dist - lower

    def lower_bound(self, fr, g0, g1):
        if g0 == self.plane_geom:
            return -math.inf
        (c0, r0), (c1, r1) = fr.sphere(g0), fr.sphere(g1)
        return float(np.linalg.norm(c0 - c1)) - r0 - r1

    def distances(self, fr, pairs, cutoff_slack=1e-6):
        """Per-pair distance (inf where a bounding-sphere bound already exceeds the best by more than cutoff_slack), best first."""
        lbs = [self.lower_bound(fr, a, b) for a, b in pairs]
        out = np.full(len(pairs), np.inf)
        best = math.inf
        for i in sorted(range(len(pairs)), key=lambda k: lbs[k]):
            if lbs[i] > best + cutoff_slack:
                break
            out[i] = self.pair_distance(fr, *pairs[i])[0]
            best = min(best, out[i])
        return out

    def witness_error(self, fr, g, w):
        """How far a world point is from where a witness on geom g belongs: the surface of a box or a hull, the plane, the core
        segment of a capsule."""
        t = self.type_of(g)
        if t == PLANE:
            return abs(float((np.asarray(w) - fr.p[g]) @ fr.R[g][:, 2]))
        if t == BOX:
            return abs(point_box_distance(w, fr.R[g], fr.p[g], self.size_of(g)))
        if t == CAPSULE:
            return abs(point_capsule_distance(w, fr.R[g], fr.p[g], 0.0, self.gsize[g][1]))
        return gjk(np.asarray(w).reshape(1, 3), fr.points(g))[0]

    def moves(self, j, g):
        """Does joint j move geom g (is the joint's body an ancestor-or-self of the geom's)?"""
        if g >= self.ngeom or g == self.plane_geom:
            return False
        b = int(self.gbody[g])
        while b > 0:
            if b == int(self.jbody[j]):
                return True
            b = int(self.parent[b])
        return False

    def gradient(self, fr, g0, g1, wa, wb, n):
        """d(distance)/dq with the witnesses held fixed on their geoms: n . (v_b - v_a) per joint."""
        out = np.zeros(self.nq)
        for j in range(self.nq):
            va = vb = np.zeros(3)
            hinge = self.jtype[j] == 3
            if self.moves(j, g0):
                va = np.cross(fr.xaxis[j], np.asarray(wa) - fr.xanchor[j]) if hinge else fr.xaxis[j]
            if self.moves(j, g1):
                vb = np.cross(fr.xaxis[j], np.asarray(wb) - fr.xanchor[j]) if hinge else fr.xaxis[j]
            out[j] = float(np.asarray(n) @ (vb - va))
        return out
