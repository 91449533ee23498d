// clearance_team.h -- clearance queries on configurations the caller supplies (rcsh_clearance_query / rcsh_env_clearance).
//
// The collision queries of query_team.h answer yes or no.  These kernels answer with a number and a direction, for M configurations at
// once: the smallest distance between the geoms of any selected pair, the pair that attains it, the two closest points (the
// witnesses; a capsule's is the point of its core segment, its surface point a radius further along the line between them) and d(distance)/dq with the witnesses held fixed on their geoms.  In contact the number is minus the penetration depth of
// the deepest pair -- the depth the narrow phase of the contact pass computes (MPR; the box-box collider for two boxes; the lowest
// point against the floor).  The pairs are the point query's: the floor pairs, the check's table, the free body's pairs.
//
// One row per TEAM of 16 lanes (team.h), four per wavefront, as k_collision_query.  Per row:
//  1. link frames, world boxes and the free body's frame as query_config computes them (query_box_frame and, for an environment's own
//     row, query_env_row are query_team.h's; the frames, the broad levels and the narrow phase's setup are this kernel's own text: calling
//     query_config's made this kernel slower than it was);
//  2. LOWER BOUNDS of every selected pair's distance, a lane per pair (t + 16 j) and geom (t + 16 u): bounding spheres, then the
//     oriented boxes' face separation (as query_config has them).  A pair the boxes do not prove apart is bounded by -inf: it may penetrate.  A pair the caller's
//     mask leaves out is bounded by +inf.  Floor pairs are exact at this level, with their witness;
//  3. best first: the team takes the pending pair of the smallest bound (ties: the lowest key) and computes its exact distance on its
//     16 lanes (gjk_distance), until the smallest pending bound is no smaller than the best value found or than d_max;
//  4. the gradient of the winner: lane j < NL computes joint j's component.
#pragma once
#include "query_team.h"

namespace rcsh {

constexpr int kClearApart = 0, kClearBeyond = 1, kClearContact = 2, kClearOpen = 3;  // the status byte of a row
// gjk_distance: support queries a pair may spend.  Hulls, boxes and capsule cores are polytopes: the iteration ends after finitely many
// steps, in practice 4 to 12; the cap is only ever met where round-off keeps the simplex from settling (status kClearOpen).
constexpr int kGjkCap = 64;
constexpr double kGjkBand = 1e-10;  // stop: |x| minus the proven lower bound at most this

struct ClearArgs {
  QueryArgs Q;               // tables, kinds, the pair set's bits, m, q0, free_qpos (the outputs of the collision queries are unused)
  const uint8_t* pair_mask;  // [count], in the list's order for Q.kinds; null: every pair
  double d_max;
  double* distance;          // [m]
  uint8_t* status;           // [m] or null
  int32_t* pair;             // [m][2] or null
  double* witness;           // [m][6] or null
  double* grad;              // [m][NL] or null
  const double* S;           // env form: the state, [field][n] (null: the caller's rows)
  int32_t qpos_field, box_field;  // env form: Lay::QPOS; Lay::BOX + kBoxQ when the free body is tested, -1 otherwise
};

#if defined(__HIP__)

// ---- the point of a simplex nearest the origin
// The simplex is up to four points of A - B in FIXED slots (bit i of `used`: slot i holds a point).  Every sub-simplex of the used slots
// is solved for the origin's projection onto its affine hull (signed areas and volumes, relative to the sub-simplex's first point); a
// projection with non-negative weights lies in the simplex, the nearest of those is the simplex's nearest point.  Exhaustive -- fifteen
// candidates -- and free of run-time indices: slots and candidates are named at compile time (a run-time index would put the slots into
// scratch, see expand_portal and the gap selects of query_config), and every lane of the team does the same scalar work.
RCSH_D void gjk_edge(const double* a, const double* b, bool& ok, double& t, double& n2) {
  const double d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const double dd = dot3(d, d);
  t = dd > 0.0 ? -dot3(a, d) / dd : -1.0;
  ok = t >= 0.0 && t <= 1.0;
  const double p[3] = {a[0] + t * d[0], a[1] + t * d[1], a[2] + t * d[2]};
  n2 = dot3(p, p);
}
RCSH_D void gjk_tri(const double* a, const double* b, const double* c, bool& ok, double& s, double& t, double& n2) {
  const double e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double w[3] = {-a[0], -a[1], -a[2]};
  double n[3], c1[3], c2[3];
  cross3(e1, e2, n);
  cross3(w, e2, c1);
  cross3(e1, w, c2);
  const double nn = dot3(n, n);
  const bool solid = nn > 1e-20 * dot3(e1, e1) * dot3(e2, e2);  // (a sliver: its edges carry the answer)
  const double inv = solid ? 1.0 / nn : 0.0;
  s = dot3(c1, n) * inv;
  t = dot3(c2, n) * inv;
  ok = solid && s >= 0.0 && t >= 0.0 && s + t <= 1.0;
  const double p[3] = {a[0] + s * e1[0] + t * e2[0], a[1] + s * e1[1] + t * e2[1], a[2] + s * e1[2] + t * e2[2]};
  n2 = dot3(p, p);
}
// weights l0..l3 of the nearest point (zero outside the sub-simplex that carries it); returns true when the origin is inside the
// tetrahedron
RCSH_D bool gjk_nearest(const MprPt& y0, const MprPt& y1, const MprPt& y2, const MprPt& y3, uint32_t used, double& l0, double& l1,
                        double& l2, double& l3) {
  double best = INFINITY;
  l0 = l1 = l2 = l3 = 0.0;
  auto take = [&](bool ok, uint32_t need, double n2, double a0, double a1, double a2, double a3) {
    const bool t = ok && (used & need) == need && n2 < best;
    best = t ? n2 : best;
    l0 = t ? a0 : l0; l1 = t ? a1 : l1; l2 = t ? a2 : l2; l3 = t ? a3 : l3;
  };
  take(true, 1u, dot3(y0.v, y0.v), 1, 0, 0, 0);
  take(true, 2u, dot3(y1.v, y1.v), 0, 1, 0, 0);
  take(true, 4u, dot3(y2.v, y2.v), 0, 0, 1, 0);
  take(true, 8u, dot3(y3.v, y3.v), 0, 0, 0, 1);
  bool ok;
  double s, t, n2;
  gjk_edge(y0.v, y1.v, ok, t, n2); take(ok, 3u, n2, 1 - t, t, 0, 0);
  gjk_edge(y0.v, y2.v, ok, t, n2); take(ok, 5u, n2, 1 - t, 0, t, 0);
  gjk_edge(y0.v, y3.v, ok, t, n2); take(ok, 9u, n2, 1 - t, 0, 0, t);
  gjk_edge(y1.v, y2.v, ok, t, n2); take(ok, 6u, n2, 0, 1 - t, t, 0);
  gjk_edge(y1.v, y3.v, ok, t, n2); take(ok, 10u, n2, 0, 1 - t, 0, t);
  gjk_edge(y2.v, y3.v, ok, t, n2); take(ok, 12u, n2, 0, 0, 1 - t, t);
  gjk_tri(y0.v, y1.v, y2.v, ok, s, t, n2); take(ok, 7u, n2, 1 - s - t, s, t, 0);
  gjk_tri(y0.v, y1.v, y3.v, ok, s, t, n2); take(ok, 11u, n2, 1 - s - t, s, 0, t);
  gjk_tri(y0.v, y2.v, y3.v, ok, s, t, n2); take(ok, 13u, n2, 1 - s - t, 0, s, t);
  gjk_tri(y1.v, y2.v, y3.v, ok, s, t, n2); take(ok, 14u, n2, 0, 1 - s - t, s, t);
  // the tetrahedron: the origin inside it ends the iteration
  const double e1[3] = {y1.v[0] - y0.v[0], y1.v[1] - y0.v[1], y1.v[2] - y0.v[2]}, e2[3] = {y2.v[0] - y0.v[0], y2.v[1] - y0.v[1], y2.v[2] - y0.v[2]},
               e3[3] = {y3.v[0] - y0.v[0], y3.v[1] - y0.v[1], y3.v[2] - y0.v[2]}, w[3] = {-y0.v[0], -y0.v[1], -y0.v[2]};
  double c23[3], c31[3], c12[3];
  cross3(e2, e3, c23);
  cross3(e3, e1, c31);
  cross3(e1, e2, c12);
  const double det = dot3(e1, c23);
  const bool solid = det * det > 1e-24 * dot3(e1, e1) * dot3(e2, e2) * dot3(e3, e3);
  const double inv = solid ? 1.0 / det : 0.0;
  const double a = dot3(w, c23) * inv, b = dot3(w, c31) * inv, c = dot3(w, c12) * inv;
  const bool inside = used == 15u && solid && a >= 0.0 && b >= 0.0 && c >= 0.0 && a + b + c <= 1.0;
  take(inside, 15u, 0.0, 1 - a - b - c, a, b, c);
  return inside;
}

// Distance of two convex shapes: GJK on the 16 lanes of a team.  The support queries are the parallel part (mpr_support<TEAM>: hulls
// staged in LDS); the simplex arithmetic is the same on every lane.  Capsules enter as their core segments (size[0] = 0): with the
// rounded support the iteration would converge only asymptotically; the caller subtracts the radii.
// x: the simplex's nearest point (a point of A - B: |x| is never less than the distance); lower: the largest support bound
// x . w / |x| seen (never more than the distance, but for the support's tie band, kSupportTie, which the caller takes off).
// Returns 0 converged (|x| - lower <= kGjkBand), 1 the origin is inside A - B or within the band of it, 2 open: the cap was met, the
// new support point was in the simplex already, or a step did not come nearer.  wa, wb: the points of A and B behind x.
template <bool TEAM>
RCSH_D int gjk_distance(const Shape& A, const Shape& B, double* dist, double* lower, double* wa, double* wb) {
  MprPt y0, y1, y2, y3, w;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    y0.v[k] = y0.v1[k] = y0.v2[k] = 0.0; y1.v[k] = y1.v1[k] = y1.v2[k] = 0.0;
    y2.v[k] = y2.v1[k] = y2.v2[k] = 0.0; y3.v[k] = y3.v1[k] = y3.v2[k] = 0.0;
  }
  uint32_t used = 0;
  // the first direction: the centre difference
  double x[3] = {A.center[0] - B.center[0], A.center[1] - B.center[1], A.center[2] - B.center[2]};
  if (!(dot3(x, x) > 1e-24)) { x[0] = 1.0; x[1] = 0.0; x[2] = 0.0; }
  double low = 0.0;
  int rc = 2;
#pragma unroll
  for (int k = 0; k < 3; ++k) { wa[k] = A.center[k]; wb[k] = B.center[k]; }
  for (int it = 0; it < kGjkCap; ++it) {
    const double n2 = dot3(x, x);
    const double nx = sqrt(n2);
    if (used != 0 && !(nx > kGjkBand)) { rc = 1; break; }
    const double d[3] = {-x[0] / nx, -x[1] / nx, -x[2] / nx};
    mpr_support<TEAM>(A, B, d, w);
    const double h = -dot3(w.v, d);
    low = fmax(low, h);
    if (used != 0) {
      if (nx - low <= kGjkBand) { rc = 0; break; }
      const bool dup = ((used & 1u) && w.v[0] == y0.v[0] && w.v[1] == y0.v[1] && w.v[2] == y0.v[2]) ||
                       ((used & 2u) && w.v[0] == y1.v[0] && w.v[1] == y1.v[1] && w.v[2] == y1.v[2]) ||
                       ((used & 4u) && w.v[0] == y2.v[0] && w.v[1] == y2.v[1] && w.v[2] == y2.v[2]) ||
                       ((used & 8u) && w.v[0] == y3.v[0] && w.v[1] == y3.v[1] && w.v[2] == y3.v[2]);
      if (dup) break;
    }
    // the new point into the first free slot (a nearest point that is not inside rests on at most three)
    const bool f0 = !(used & 1u), f1 = !f0 && !(used & 2u), f2 = !f0 && !f1 && !(used & 4u), f3 = !f0 && !f1 && !f2;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      y0.v[k] = f0 ? w.v[k] : y0.v[k]; y0.v1[k] = f0 ? w.v1[k] : y0.v1[k]; y0.v2[k] = f0 ? w.v2[k] : y0.v2[k];
      y1.v[k] = f1 ? w.v[k] : y1.v[k]; y1.v1[k] = f1 ? w.v1[k] : y1.v1[k]; y1.v2[k] = f1 ? w.v2[k] : y1.v2[k];
      y2.v[k] = f2 ? w.v[k] : y2.v[k]; y2.v1[k] = f2 ? w.v1[k] : y2.v1[k]; y2.v2[k] = f2 ? w.v2[k] : y2.v2[k];
      y3.v[k] = f3 ? w.v[k] : y3.v[k]; y3.v1[k] = f3 ? w.v1[k] : y3.v1[k]; y3.v2[k] = f3 ? w.v2[k] : y3.v2[k];
    }
    const uint32_t with = used | (f0 ? 1u : f1 ? 2u : f2 ? 4u : 8u);
    double l0, l1, l2, l3;
    const bool inside = gjk_nearest(y0, y1, y2, y3, with, l0, l1, l2, l3);
    const double sum = l0 + l1 + l2 + l3;
    l0 /= sum; l1 /= sum; l2 /= sum; l3 /= sum;
    double nxt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nxt[k] = l0 * y0.v[k] + l1 * y1.v[k] + l2 * y2.v[k] + l3 * y3.v[k];
    if (used != 0 && !inside && !(dot3(nxt, nxt) < n2)) break;  // (no nearer: round-off has the last word; x and the witnesses stay)
    used = (l0 > 0.0 ? 1u : 0u) | (l1 > 0.0 ? 2u : 0u) | (l2 > 0.0 ? 4u : 0u) | (l3 > 0.0 ? 8u : 0u);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      x[k] = nxt[k];
      wa[k] = l0 * y0.v1[k] + l1 * y1.v1[k] + l2 * y2.v1[k] + l3 * y3.v1[k];
      wb[k] = l0 * y0.v2[k] + l1 * y1.v2[k] + l2 * y2.v2[k] + l3 * y3.v2[k];
    }
    if (inside) { rc = 1; break; }
  }
  *dist = used != 0 ? sqrt(dot3(x, x)) : 0.0;
  *lower = low;
  return rc;
}

// what the team knows about its best pair so far (the same on every lane of the team)
struct ClearBest {
  double value;   // distance; minus the depth of a penetrating pair
  int key;        // kind << 16 | index (kQueryNoPair: none)
  int la, lb;     // the links of the two geoms, in the list's order (-1: does not move)
  bool open;      // the distance iteration did not converge: value is the proven lower bound
  double wa[3], wb[3], n[3];
};
RCSH_D void clear_offer(ClearBest& B, double value, int key, int la, int lb, bool open, const double* wa, const double* wb, const double* n) {
  const bool t = value < B.value || (value == B.value && key < B.key);
  B.value = t ? value : B.value;
  B.key = t ? key : B.key;
  B.la = t ? la : B.la;
  B.lb = t ? lb : B.lb;
  B.open = t ? open : B.open;
#pragma unroll
  for (int k = 0; k < 3; ++k) { B.wa[k] = t ? wa[k] : B.wa[k]; B.wb[k] = t ? wb[k] : B.wb[k]; B.n[k] = t ? n[k] : B.n[k]; }
}

// where a key stands in the list of rcsh_clearance_pairs for the row's kinds (build_query_pairs): the floor pairs, the table, the free
// body's pairs
RCSH_D int clear_list_index(const QueryArgs& Q, int key) {
  const int kind = key >> 16, i = key & 0xffff;
  if (kind == 0) return __popc(Q.floor_bits & ((1u << i) - 1u));
  if (kind == 1) return __popc(Q.floor_bits) + i;
  return __popc(Q.floor_bits) + ((Q.kinds & kQuerySelf) ? Q.ck.npair : 0) + __popc(Q.box_bits & ((1u << i) - 1u));
}
RCSH_D bool clear_selected(const ClearArgs& A, int key) { return !A.pair_mask || A.pair_mask[clear_list_index(A.Q, key)] != 0; }

// Clearance query: one row per team.
template <class T>
__global__ void __launch_bounds__(64) k_clearance_query(ClearArgs A) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL;
  __shared__ QueryTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int tbase = threadIdx.x & 48;
  QueryTeamLds<T>& S = lds[team];
  const QueryArgs& Q = A.Q;
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < Q.m;
  const bool valid = t < NL;
  const CheckTable& ck = Q.ck;
  const int npair = ck.npair, ngeom = ck.ngeom;
  // ---- the row: the caller's, or the environment's own chain and free body
  double q, fq[7];
  bool use_box;
  if (A.S) {
    use_box = query_env_row(A.S, Q.m, e, live, valid, A.qpos_field, A.box_field, q, fq);
  } else {
    q = live && valid ? Q.q0[(size_t)e * NL + t] : 0.0;
    use_box = query_free_pose(Q, e, live, fq);
  }
  // ---- link frames, world boxes, the free body's frame (query_config's prologue)
  {
    KinK kk;
    kk.load(Q.links[valid ? t : NL - 1]);
    double R[9], p[3];
    link_local_frame(kk, q, R, p);
    scan_frames<T>(R, p);
    if (valid) {
#pragma unroll
      for (int k = 0; k < 9; ++k) S.F[t][k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) S.F[t][9 + k] = p[k];
    }
  }
  stage_fence();
  const double* F = &S.F[0][0];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int g = t + kTeamLanes * u;
    if (g < ngeom) {
      const int link = ck.glink[g];
      double cw[3], Rw[9];
      self_box_world(F, link, ck.geoms[g].c, ck.geoms[g].rot, cw, Rw);
#pragma unroll
      for (int k = 0; k < 3; ++k) S.wbox[g][k] = cw[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) S.wbox[g][3 + k] = Rw[k];
    }
  }
  stage_fence();
  double bp[3], bR[9];
  query_box_frame(fq, use_box, bp, bR);
  const double* bs = Q.box_size;
  const double d_max = A.d_max;
  // ---- the floor (exact: the lane's candidate with its witness) and the bounds of the free body's pairs: lane t takes geoms t, t + 16
  double pend_p[kCheckPer], pend_b[2];  // bounds of the lane's pending pairs: +inf not pending, -inf not proven apart
  double fl_val = INFINITY, fl_w[3] = {0, 0, 0};
  int fl_key = kQueryNoPair, fl_link = -1;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    pend_b[u] = INFINITY;
    const int g = t + kTeamLanes * u;
    if (!live || g >= ngeom) continue;
    const ContactGeom& cg = Q.geoms[g];
    double gR[9], gpos[3];
    query_geom_world(cg, F, gR, gpos);
    if (((Q.floor_bits >> g) & 1u) && clear_selected(A, (0 << 16) | g)) {
      const double* n = Q.plane_n;
      double nl[3], wl[3] = {0, 0, 0}, low, rad = 0.0;
      mulTv(gR, n, nl);
      const double c0 = dot3(n, gpos) - Q.plane_d;
      if (cg.type == 6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) wl[k] = nl[k] > 0.0 ? -cg.size[k] : cg.size[k];
        low = c0 + dot3(nl, wl);
      } else if (cg.type == 3) {
        wl[2] = nl[2] > 0.0 ? -cg.size[1] : cg.size[1];
        rad = cg.size[0];
        low = c0 + nl[2] * wl[2] - rad;
      } else {
        // the hull's bounding box first; its vertices only where the box comes within d_max
        low = c0 + dot3(nl, cg.aabb_c) - (fabs(nl[0]) * cg.aabb_h[0] + fabs(nl[1]) * cg.aabb_h[1] + fabs(nl[2]) * cg.aabb_h[2]);
        if (low < d_max) {
          const double* V = Q.verts + 3 * (size_t)cg.vert_adr;
          double lo = INFINITY;
          for (int i = 0; i < cg.vert_num; ++i) {
            const double vx = V[3 * i], vy = V[3 * i + 1], vz = V[3 * i + 2];
            const double h = nl[0] * vx + nl[1] * vy + nl[2] * vz;
            const bool lower = h < lo;  // (ties: the lowest index)
            lo = lower ? h : lo;
            wl[0] = lower ? vx : wl[0]; wl[1] = lower ? vy : wl[1]; wl[2] = lower ? vz : wl[2];
          }
          low = c0 + lo;
        } else {
          low = INFINITY;
        }
      }
      if (low < fl_val) {  // (u ascending: the lower geom keeps a tie)
        double ww[3];
        mulmv(gR, wl, ww);
        fl_val = low;
        fl_key = (0 << 16) | g;
        fl_link = cg.link;
#pragma unroll
        for (int k = 0; k < 3; ++k) fl_w[k] = ww[k] + gpos[k];  // (a capsule: the end of its core segment)
      }
    }
    if (use_box && ((Q.box_bits >> g) & 1u) && clear_selected(A, (2 << 16) | g)) {
      double hc[3], hh[3], oc[3];
      geom_obb(cg, hc, hh);
      mulmv(gR, hc, oc);
      const double cw[3] = {oc[0] + gpos[0], oc[1] + gpos[1], oc[2] + gpos[2]};
      const double d[3] = {cw[0] - bp[0], cw[1] - bp[1], cw[2] - bp[2]};
      const double rs = sqrt(dot3(hh, hh)) + sqrt(dot3(bs, bs));
      const double dd = sqrt(dot3(d, d));
      if (dd > rs) pend_b[u] = gap_lb(dd - rs);
      else {
        double bsz[3] = {bs[0], bs[1], bs[2]};
        const double sep = obb_face_sep(gR, cw, hh, bR, bp, bsz);
        pend_b[u] = sep > 0.0 ? gap_lb(sep) : -INFINITY;
      }
    }
  }
  // ---- the bounds of the lane's self pairs
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) {
    pend_p[j] = INFINITY;
    const int i = t + kTeamLanes * j;
    if (!live || !(Q.kinds & kQuerySelf) || i >= npair || !clear_selected(A, (1 << 16) | i)) continue;
    const CheckEntry en = ck.ent[i];
    const int g0 = en.geoms & 0xff, g1 = (en.geoms >> 8) & 0xff;
    const double* ca = S.wbox[g0];
    const double* cb = S.wbox[g1];
    const double d[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    const double dd = sqrt(dot3(d, d));
    if (dd > (double)en.rsum) { pend_p[j] = gap_lb(dd - (double)en.rsum); continue; }
    double Ra[9], Rb[9], pa[3], pb[3], ha[3], hb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pa[k] = ca[k]; pb[k] = cb[k]; ha[k] = ck.gh[g0][k]; hb[k] = ck.gh[g1][k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ra[k] = ca[3 + k]; Rb[k] = cb[3 + k]; }
    const double sep = obb_face_sep(Ra, pa, ha, Rb, pb, hb);
    pend_p[j] = sep > 0.0 ? gap_lb(sep) : -INFINITY;
  }
  // ---- the best floor pair of the team
  ClearBest B;
  B.value = INFINITY; B.key = kQueryNoPair; B.la = -1; B.lb = -1; B.open = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) { B.wa[k] = 0.0; B.wb[k] = 0.0; B.n[k] = 0.0; }
  {
    const double m = team_min(fl_val);
    const int key = (int)team_min(fl_val == m ? (double)fl_key : (double)kQueryNoPair);
    if (key != kQueryNoPair) {
      const int src = tbase + (key & (kTeamLanes - 1));
      double wb[3], wa[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) wb[k] = lane_get(fl_w[k], src);
      const int link = (int)lane_get((double)fl_link, src);
      const double h = dot3(Q.plane_n, wb) - Q.plane_d;
#pragma unroll
      for (int k = 0; k < 3; ++k) wa[k] = wb[k] - h * Q.plane_n[k];  // (the point of the plane below it)
      clear_offer(B, m, key, -1, link, false, wa, wb, Q.plane_n);
    }
  }
  // ---- best first: the pending pair of the smallest bound, one a round per team, on the team's 16 lanes
  for (;;) {
    // the lane's smallest pending bound and its key (ascending keys: the lowest keeps a tie)
    double lb = INFINITY;
    int lkey = kQueryNoPair;
#pragma unroll
    for (int j = 0; j < kCheckPer; ++j) {
      const bool s = pend_p[j] < lb;
      lb = s ? pend_p[j] : lb;
      lkey = s ? ((1 << 16) | (t + kTeamLanes * j)) : lkey;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool s = pend_b[u] < lb;
      lb = s ? pend_b[u] : lb;
      lkey = s ? ((2 << 16) | (t + kTeamLanes * u)) : lkey;
    }
    const double m = team_min(lb);
    const int key = (int)team_min(lb == m ? (double)lkey : (double)kQueryNoPair);
    const bool mine = live && key != kQueryNoPair && m < B.value && m < d_max;
    if (__ballot(mine) == 0) break;
    if (mine) {
      const int kind = key >> 16, idx = key & 0xffff;
      if (t == (idx & (kTeamLanes - 1))) {  // the holder strikes it off
        const int slot = idx / kTeamLanes;
        if (kind == 1) {
#pragma unroll
          for (int k = 0; k < kCheckPer; ++k) pend_p[k] = k == slot ? INFINITY : pend_p[k];
        } else {
#pragma unroll
          for (int k = 0; k < 2; ++k) pend_b[k] = k == slot ? INFINITY : pend_b[k];
        }
      }
      // the two geoms in the list's order (MuJoCo's within a contact); -1: the free body
      int ga, gb;
      if (kind == 1) {
        const uint32_t gg = ck.ent[idx].geoms;
        ga = gg & 0xff; gb = (gg >> 8) & 0xff;
      } else {
        const bool hull = Q.geoms[idx].type == 7;
        ga = hull ? -1 : idx; gb = hull ? idx : -1;
      }
      const int na = ga >= 0 && Q.geoms[ga].type == 7 ? 3 * Q.geoms[ga].vert_num : 0;
      const int nb = gb >= 0 && Q.geoms[gb].type == 7 ? 3 * Q.geoms[gb].vert_num : 0;
      if (na) {
        const double* va = Q.verts + 3 * (size_t)Q.geoms[ga].vert_adr;
        for (int k = t; k < na; k += kTeamLanes) S.stage[k] = va[k];
      }
      if (nb) {
        const double* vb = Q.verts + 3 * (size_t)Q.geoms[gb].vert_adr;
        for (int k = t; k < nb; k += kTeamLanes) S.stage[na + k] = vb[k];
      }
      stage_fence();
      Shape SA, SB;
      int la = -1, lb_ = -1;
      double ra = 0.0, rb = 0.0;
      if (ga >= 0) {
        const ContactGeom& a = Q.geoms[ga];
        double Ra[9], pa[3];
        query_geom_world(a, F, Ra, pa);
        SA = make_shape(a.type == 7 ? 0 : a.type == 6 ? 1 : 2, pa, Ra, a.size, S.stage, a.vert_num);
        if (a.type == 7) { mulmv(Ra, a.center, SA.center); SA.center[0] += pa[0]; SA.center[1] += pa[1]; SA.center[2] += pa[2]; }
        la = a.link;
        ra = a.type == 3 ? a.size[0] : 0.0;
      } else {
        SA = make_shape(1, bp, bR, bs, nullptr, 0);
      }
      if (gb >= 0) {
        const ContactGeom& b = Q.geoms[gb];
        double Rb[9], pb[3];
        query_geom_world(b, F, Rb, pb);
        SB = make_shape(b.type == 7 ? 0 : b.type == 6 ? 1 : 2, pb, Rb, b.size, S.stage + na, b.vert_num);
        if (b.type == 7) { mulmv(Rb, b.center, SB.center); SB.center[0] += pb[0]; SB.center[1] += pb[1]; SB.center[2] += pb[2]; }
        lb_ = b.link;
        rb = b.type == 3 ? b.size[0] : 0.0;
      } else {
        SB = make_shape(1, bp, bR, bs, nullptr, 0);
      }
      // the distance of the cores (capsules as their segments), then the radii
      Shape CA = SA, CB = SB;
      CA.size[0] = SA.type == 2 ? 0.0 : SA.size[0];
      CB.size[0] = SB.type == 2 ? 0.0 : SB.size[0];
      double dcore = 0.0, low = 0.0, wa[3], wb[3], n[3] = {0, 0, 0};
      const int rc = gjk_distance<true>(CA, CB, &dcore, &low, wa, wb);
      double value = dcore - (ra + rb);
      bool open = false;
      if (rc == 1 || value <= kGjkBand) {
        // overlapping or touching: the depth, normal and position of the contact pass's narrow phase
        double depth = 0.0, pos[3] = {0, 0, 0};
        bool deep = false;
        if (SA.type == 1 && SB.type == 1) {
          // (the collider is a call: what it is handed by address lives in private memory -- copies, so that the shapes stay in registers)
          double cpos[24], cdist[8], fa[15], fb[15], bn[3] = {0, 0, 0};
#pragma unroll
          for (int k = 0; k < 3; ++k) { fa[k] = SA.p[k]; fa[12 + k] = SA.size[k]; fb[k] = SB.p[k]; fb[12 + k] = SB.size[k]; }
#pragma unroll
          for (int k = 0; k < 9; ++k) { fa[3 + k] = SA.R[k]; fb[3 + k] = SB.R[k]; }
          const int nc = dev_box_box(fa, fa + 3, fa + 12, fb, fb + 3, fb + 12, cpos, bn, cdist, S.stage);
          n[0] = bn[0]; n[1] = bn[1]; n[2] = bn[2];
          for (int c = 0; c < nc; ++c) {
            if (-cdist[c] > depth) { depth = -cdist[c]; pos[0] = cpos[3 * c]; pos[1] = cpos[3 * c + 1]; pos[2] = cpos[3 * c + 2]; deep = true; }
          }
        } else {
          deep = mpr_penetration<true, kMprFull>(SA, SB, &depth, n, pos) != 0;
        }
        if (deep) {
          value = -depth;
#pragma unroll
          for (int k = 0; k < 3; ++k) { wa[k] = pos[k] + 0.5 * depth * n[k]; wb[k] = pos[k] - 0.5 * depth * n[k]; }
        } else {
          // (touching within the band: the cores' witnesses stand)
          const double dn = sqrt((wb[0] - wa[0]) * (wb[0] - wa[0]) + (wb[1] - wa[1]) * (wb[1] - wa[1]) + (wb[2] - wa[2]) * (wb[2] - wa[2]));
#pragma unroll
          for (int k = 0; k < 3; ++k) n[k] = dn > 0.0 ? (wb[k] - wa[k]) / dn : 0.0;
        }
      } else {
        if (rc == 2) {  // open: the proven bound
          open = true;
          value = fmax(low - kSupportTie, 0.0) - (ra + rb);
        }
        const double dn = sqrt((wb[0] - wa[0]) * (wb[0] - wa[0]) + (wb[1] - wa[1]) * (wb[1] - wa[1]) + (wb[2] - wa[2]) * (wb[2] - wa[2]));
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = dn > 0.0 ? (wb[k] - wa[k]) / dn : 0.0;
      }
      clear_offer(B, value, key, la, lb_, open, wa, wb, n);
      stage_fence();
    }
  }
  // ---- the row's answer
  const bool contact = B.value < -kCheckTouch;
  const bool beyond = !(B.value < d_max);
  const int status = beyond ? kClearBeyond : contact ? kClearContact : B.open ? kClearOpen : kClearApart;
  if (live && t == 0) {
    A.distance[e] = beyond ? d_max : B.value;
    if (A.status) A.status[e] = (uint8_t)status;
    if (A.pair) query_pair_ids(Q, beyond ? kQueryNoPair : B.key, A.pair + 2 * (size_t)e);
    if (A.witness) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        A.witness[6 * (size_t)e + k] = beyond ? 0.0 : B.wa[k];
        A.witness[6 * (size_t)e + 3 + k] = beyond ? 0.0 : B.wb[k];
      }
    }
  }
  // ---- the gradient: lane j, joint j.  A point w riding on a link below joint j moves by axis x (w - anchor) per radian of a hinge,
  // by axis per metre of a slide; the distance changes by n . (v_b - v_a)
  if (live && valid && A.grad) {
    const LinkRec& r = Q.links[t];
    const double* Fj = F + 12 * t;
    double Rj[9], ax[3], an[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rj[k] = Fj[k];
    mulmv(Rj, r.axis, ax);
    mulmv(Rj, r.jpos, an);
    an[0] += Fj[9]; an[1] += Fj[10]; an[2] += Fj[11];
    const bool slide = r.jtype == kSlide;
    const double ra_[3] = {B.wa[0] - an[0], B.wa[1] - an[1], B.wa[2] - an[2]}, rb_[3] = {B.wb[0] - an[0], B.wb[1] - an[1], B.wb[2] - an[2]};
    double va[3], vb[3];
    cross3(ax, ra_, va);
    cross3(ax, rb_, vb);
    const bool ma = (anc_mask<T>(B.la) >> t) & 1u, mb = (anc_mask<T>(B.lb) >> t) & 1u;
    double g = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) g += B.n[k] * ((mb ? (slide ? ax[k] : vb[k]) : 0.0) - (ma ? (slide ? ax[k] : va[k]) : 0.0));
    A.grad[(size_t)e * NL + t] = beyond ? 0.0 : g;
  }
}

// a robot without collision geoms: nothing is within d_max of anything
__global__ void k_clearance_fill(double* distance, uint8_t* status, int32_t* pair, double* witness, double* grad, double d_max, int m, int nl) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  distance[i] = d_max;
  if (status) status[i] = (uint8_t)kClearBeyond;
  if (pair) { pair[2 * (size_t)i] = -1; pair[2 * (size_t)i + 1] = -1; }
  if (witness) for (int k = 0; k < 6; ++k) witness[6 * (size_t)i + k] = 0.0;
  if (grad) for (int k = 0; k < nl; ++k) grad[(size_t)i * nl + k] = 0.0;
}

#endif  // __HIP__

}  // namespace rcsh
