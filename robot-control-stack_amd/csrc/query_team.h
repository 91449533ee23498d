// query_team.h -- collision queries on configurations the caller supplies (rcsh_collision_query / rcsh_motion_query).
//
// The reference answers "is the robot in collision at q?" with MuJoCo's collision pass on a scratch copy of the data
// (python/rcs/ompl/mj_ompl.py: MjORobot.check_collision -- write q, mj_fwdPosition + mj_collision, look at the contacts, restore).
// These kernels answer it for M configurations at once, and the motion validator's question -- "is any configuration on the
// straight joint-space segment between two rows in contact?" -- with the levers of the end-of-launch check (check_team.h).  Neither
// reads nor writes any per-environment state: the model tables are all they share with the stepping kernels.
//
// One query per TEAM of 16 lanes (team.h), four per wavefront, as k_ik_team.  The predicate is the check's: a pair of the selected
// kinds is in contact when it penetrates by more than kCheckTouch (1e-9).
//  * kind 0, robot geom <-> floor plane: the lowest point of each geom the plane admits (hull vertices, box corners, capsule end
//    spheres -- what MuJoCo's plane colliders test);
//  * kind 1, robot geom <-> robot geom: every pair of the check's table (MuJoCo's filters applied by the host): bounding spheres,
//    oriented boxes, then -- per team, one pair at a time on its 16 lanes -- Gilbert's iteration and the portal refinement (MPR);
//  * kind 2, robot geom <-> the free body (a box, at the pose the caller gives): the same levels.
// Two boxes are settled by their separating axes alone (obb_apart_or_touching).
//
// Motion (a segment q(s) = q_from + s (q_to - q_from), s in [0, 1]): pieces [a, b] are taken in increasing s from a per-team stack
// in LDS.  Every sampled configuration comes with LOWER BOUNDS of every selected pair's gap; a piece is certified free when, for
// every pair, gap(a) + gap(b) exceeds the most the piece's joint travel can move the two geoms relative to each other (the levers
// of build_self_levers, per geom: CheckTable::lev + kLevGeom).  On a straight piece |q - q_a| + |q - q_b| = |q_b - q_a| per joint, so
// this is the check's path-length ("psum") certificate as it stands.  A piece that is not certified is bisected until it is, until
// a sampled point is in contact (then only the pieces before that point are looked at any more), or until its largest joint
// travel is at most `resolution`.
//
// What the family's other kernels -- the clearance query (clearance_team.h) and the collision guard (guard_team.h) -- take from here:
// query_config and motion_decide whole (the guard), query_box_frame (the free body's frame: the one quaternion rule) and query_env_row
// (an environment's own row of the state).  query_row_setup is the row's link frames and world boxes.  Which pairs a query covers is
// decided once, on the host (model.cpp: build_query_pairs): QueryArgs carries the floor's and the free body's pairs as bits, the self
// pairs are the check's table.
#pragma once
#include "check_team.h"

namespace rcsh {

constexpr int kQueryStack = 48;  // pieces a team keeps pending (bisection depth): a piece that would go deeper stays undecided
// The work per motion row is bounded whatever the resolution: at most kQueryBudget configurations are evaluated by the bisection.  A row
// that runs out without a contact then samples the grid s = k / kQueryGrid beyond the last piece it settled, in increasing s, and stops
// at the first contact (result 1) or reports 2.  A contact that lasts longer than 1 / kQueryGrid of the segment always contains a sample
// of that grid -- and, when the bisection finishes, the end of a piece: no piece longer than that is left undecided --, so it is never
// reported as 2.
constexpr int kQueryBudget = 2048;
constexpr int kQueryGrid = 32;
constexpr int kQueryNoPair = 0x7fffffff;

struct QueryArgs {
  const LinkRec* links;       // the model's link records (behind the DevModel)
  CheckTable ck;              // pairs, geom boxes, levers (slack unused)
  const ContactGeom* geoms;   // the robot's collision geoms (ContactTable::geoms)
  const double* verts;        // their hull vertices
  double plane_n[3], plane_d;
  int32_t plane_geom;              // the floor's mjModel geom id
  int32_t box_geom;                // the free body's mjModel geom id (-1: no free body)
  uint32_t floor_bits, box_bits;   // bit g: (floor, geom g) / (geom g, free body) is a pair of the query (model.cpp build_query_pairs:
                                   // the filters, `solid`, the scene and `kinds` all folded in)
  double box_size[3];
  double slide_lo[12], slide_hi[12];  // the interval of each joint the levers hold for (slides: qpos0 -+ the stroke build_self_levers
                                      // charged; hinges: unbounded) -- a segment that leaves it is never certified
  int32_t m, kinds;
  double resolution;               // motion: the largest joint travel of a piece left undecided
  const double* q0;                // [m][NL]
  const double* q1;                // [m][NL] (motion) or null (point)
  const double* free_qpos;         // [m][7] or null
  uint8_t* hit;                    // point: [m]
  uint8_t* kinds_hit;              // point: [m] or null
  int32_t* pair;                   // point: [m][2] or null
  int32_t* result;                 // motion: [m]
  double* t_contact;               // motion: [m]
};

#if defined(__HIP__)

// LDS of one team
template <class T>
struct QueryTeamLds {
  double F[T::NL][12];           // link frames (R row-major, p)
  double wbox[kMaxCGeom][12];    // geoms' oriented boxes, world frame (centre, axes)
  double stage[kSelfStage];      // the hulls of the pair the narrow phase works on
  double stack[kQueryStack];     // motion: right ends of the pending pieces (top: the nearest)
};

// What one configuration says, per lane: the lane's pairs j (t + 16 j), its geoms u (t + 16 u) against the floor and the free body.
struct QueryGaps {
  double p[kCheckPer], f[2], b[2];
};

RCSH_D double gap_lb(double g) { return g > 0.0 ? g * (1.0 - 1e-9) - 1e-12 : 0.0; }  // (a lower bound, rounded down)

// world frame of a geom (ContactGeom record: frame in its link's frame) from the team's link frames
RCSH_D void query_geom_world(const ContactGeom& g, const double* F, double* R, double* p) {
  if (g.link < 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = g.rot[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = g.pos[k];
    return;
  }
  const double* L = F + 12 * g.link;
  double LR[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) LR[k] = L[k];
  mulmm(LR, g.rot, R);
  mulmv(LR, g.pos, p);
  p[0] += L[9]; p[1] += L[10]; p[2] += L[11];
}

// The row setup of every query kernel: the link frames (world) of the lane's joint value q into S.F, then the geoms' world boxes into
// S.wbox (lane t: geoms t, t + 16), each behind its fence.  Every lane of the wavefront calls it.
template <class T>
RCSH_D void query_row_setup(const QueryArgs& A, QueryTeamLds<T>& S, double q) {
  constexpr int NL = T::NL;
  const int t = threadIdx.x & (kTeamLanes - 1);
  const bool valid = t < NL;
  const CheckTable& ck = A.ck;
  {
    KinK kk;
    kk.load(A.links[valid ? t : NL - 1]);
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
    if (g < ck.ngeom) {
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
}

// the free body's frame from its pose fq (x y z qw qx qy qz); the identity at the origin when it is not tested
RCSH_D void query_box_frame(const double* fq, bool use_box, double* bp, double* bR) {
#pragma unroll
  for (int k = 0; k < 9; ++k) bR[k] = k % 4 == 0 ? 1.0 : 0.0;
  bp[0] = 0.0; bp[1] = 0.0; bp[2] = 0.0;
  if (use_box) {
    // (mju_normalize4: a quaternion of norm below mjMINVAL becomes the identity)
    const double qn = sqrt(fq[3] * fq[3] + fq[4] * fq[4] + fq[5] * fq[5] + fq[6] * fq[6]);
    const bool deg = !(qn >= 1e-15);
    const double w = deg ? 1.0 : fq[3] / qn, x = deg ? 0.0 : fq[4] / qn, y = deg ? 0.0 : fq[5] / qn, z = deg ? 0.0 : fq[6] / qn;
    bR[0] = 1 - 2 * (y * y + z * z); bR[1] = 2 * (x * y - w * z);     bR[2] = 2 * (x * z + w * y);
    bR[3] = 2 * (x * y + w * z);     bR[4] = 1 - 2 * (x * x + z * z); bR[5] = 2 * (y * z - w * x);
    bR[6] = 2 * (x * z - w * y);     bR[7] = 2 * (y * z + w * x);     bR[8] = 1 - 2 * (x * x + y * y);
    bp[0] = fq[0]; bp[1] = fq[1]; bp[2] = fq[2];
  }
}

// An environment's own row of the state S ([field][n]): the lane's joint value (0 off the chain) and the free body's pose (box_field
// < 0: not tested).  Returns use_box.
RCSH_D bool query_env_row(const double* S, int n, int e, bool live, bool valid, int qpos_field, int box_field, double& q, double* fq) {
  const size_t ec = live ? e : 0;
  const int t = threadIdx.x & (kTeamLanes - 1);
  q = live && valid ? S[(size_t)(qpos_field + t) * n + ec] : 0.0;
  const bool use_box = live && box_field >= 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) fq[k] = use_box ? S[(size_t)(box_field + k) * n + ec] : (k == 3 ? 1.0 : 0.0);
  return use_box;
}

// The collision test of one configuration per team.  Every lane of the wavefront calls it (wave-uniform control flow outside the
// narrow phase: the team primitives exchange across lanes).  q: the lane's joint (t < NL); fq: the free body's pose (x y z qw qx qy qz,
// every lane of the team), use_box: test kind 2.  Returns, on every lane of the team, the kinds in contact (bits), and in *pkey the
// smallest key of a penetrating pair (kind << 16 | index; kQueryNoPair: none).  gaps: lower bounds of the lane's pairs' gaps (0 for a
// pair in contact, +inf for a pair that is not selected).
template <class T>
RCSH_D uint32_t query_config(const QueryArgs& A, QueryTeamLds<T>& S, double q, bool live, const double* fq, bool use_box, bool want_gaps,
                             QueryGaps& gp, int* pkey) {
  const int t = threadIdx.x & (kTeamLanes - 1);
  const CheckTable& ck = A.ck;
  const int npair = ck.npair;
  query_row_setup<T>(A, S, q);
  const double* F = &S.F[0][0];
  uint32_t kinds = 0;
  int key = kQueryNoPair;
  double bp[3], bR[9];
  query_box_frame(fq, use_box, bp, bR);
  const double* bs = A.box_size;
  // ---- kind 0 (floor) and the broad levels of kind 2 (free body): lane t takes geoms t, t + 16
  const uint32_t fbits = live ? A.floor_bits : 0u, bbits = live && use_box ? A.box_bits : 0u;  // the pairs this call tests
  uint32_t bmask = 0;  // bit u: geom t + 16 u needs the narrow phase against the free body
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    gp.f[u] = INFINITY;
    gp.b[u] = INFINITY;
    const int g = t + kTeamLanes * u;
    const bool on_floor = (fbits >> g) & 1u, at_box = (bbits >> g) & 1u;
    if (!on_floor && !at_box) continue;
    const ContactGeom& cg = A.geoms[g];
    double gR[9], gpos[3];
    query_geom_world(cg, F, gR, gpos);
    if (on_floor) {
      const double* n = A.plane_n;
      double nl[3];
      mulTv(gR, n, nl);
      const double c0 = dot3(n, gpos) - A.plane_d;
      double low;
      if (cg.type == 6) low = c0 - (fabs(nl[0]) * cg.size[0] + fabs(nl[1]) * cg.size[1] + fabs(nl[2]) * cg.size[2]);
      else if (cg.type == 3) low = c0 - fabs(nl[2]) * cg.size[1] - cg.size[0];
      else {
        // the hull's bounding box first; its vertices only where the box comes within reach
        low = c0 + dot3(nl, cg.aabb_c) - (fabs(nl[0]) * cg.aabb_h[0] + fabs(nl[1]) * cg.aabb_h[1] + fabs(nl[2]) * cg.aabb_h[2]);
        if (low < 0.05) {
          const double* V = A.verts + 3 * (size_t)cg.vert_adr;
          low = INFINITY;
          for (int i = 0; i < cg.vert_num; ++i) low = fmin(low, c0 + nl[0] * V[3 * i] + nl[1] * V[3 * i + 1] + nl[2] * V[3 * i + 2]);
        }
      }
      if (low < -kCheckTouch) {
        kinds |= kQueryFloor;
        key = min(key, (0 << 16) | g);
      }
      gp.f[u] = gap_lb(low);
    }
    if (at_box) {
      double hc[3], hh[3], oc[3];
      geom_obb(cg, hc, hh);
      mulmv(gR, hc, oc);
      const double cw[3] = {oc[0] + gpos[0], oc[1] + gpos[1], oc[2] + gpos[2]};
      const double d[3] = {cw[0] - bp[0], cw[1] - bp[1], cw[2] - bp[2]};
      const double rs = sqrt(dot3(hh, hh)) + sqrt(dot3(bs, bs));
      const double dd = sqrt(dot3(d, d));
      if (dd > rs) gp.b[u] = gap_lb(dd - rs);
      else {
        double bsz[3] = {bs[0], bs[1], bs[2]};
        const bool apart = obb_apart_or_touching(gR, cw, hh, bR, bp, bsz, kCheckTouch, 0.0);
        const double sep = obb_face_sep(gR, cw, hh, bR, bp, bsz);
        if (apart && (cg.type == 6 || (want_gaps ? sep > 0.01 : true))) {
          gp.b[u] = gap_lb(sep);
        } else if (!apart && cg.type == 6) {
          kinds |= kQueryBox;  // (two boxes: their separating axes are the exact test)
          key = min(key, (2 << 16) | g);
          gp.b[u] = 0.0;
        } else {
          bmask |= 1u << u;
          gp.b[u] = gap_lb(sep);
        }
      }
    }
  }
  // ---- kind 1: the lane's pairs against their bounding spheres and boxes
  uint32_t cmask = 0;  // bit j: pair t + 16 j needs the narrow phase
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) {
    gp.p[j] = INFINITY;
    const int i = t + kTeamLanes * j;
    if (!live || !(A.kinds & kQuerySelf) || i >= npair) continue;
    const CheckEntry e = ck.ent[i];
    const int g0 = e.geoms & 0xff, g1 = (e.geoms >> 8) & 0xff;
    const double* ca = S.wbox[g0];
    const double* cb = S.wbox[g1];
    const double d[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    const double dd = sqrt(dot3(d, d));
    if (dd > (double)e.rsum) { gp.p[j] = gap_lb(dd - (double)e.rsum); continue; }
    double Ra[9], Rb[9], pa[3], pb[3], ha[3], hb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pa[k] = ca[k]; pb[k] = cb[k]; ha[k] = ck.gh[g0][k]; hb[k] = ck.gh[g1][k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ra[k] = ca[3 + k]; Rb[k] = cb[3 + k]; }
    const bool apart = obb_apart_or_touching(Ra, pa, ha, Rb, pb, hb, kCheckTouch, 0.0);
    const double sep = obb_face_sep(Ra, pa, ha, Rb, pb, hb);
    const bool boxes = ck.gtype[g0] == 6 && ck.gtype[g1] == 6;
    if (apart && (boxes || (want_gaps ? sep > 0.01 : true))) {
      gp.p[j] = gap_lb(sep);
    } else if (!apart && boxes) {
      kinds |= kQuerySelf;
      key = min(key, (1 << 16) | i);
      gp.p[j] = 0.0;
    } else {
      cmask |= 1u << j;
      gp.p[j] = gap_lb(sep);
    }
  }
  // ---- narrow phase: per team, one pair a round (a self pair, or a geom against the free body), on the team's 16 lanes
  for (;;) {
    const uint32_t tc = team_ballot(cmask != 0), tb = team_ballot(bmask != 0);
    const bool mine = tc != 0 || tb != 0;
    if (__ballot(mine) == 0) break;
    if (mine) {
      // the team's next job: the first lane (and its lowest bit) holding one; self pairs first
      const bool self = tc != 0;
      const int src = __ffs((int)(self ? tc : tb)) - 1;
      const uint32_t msk = (uint32_t)lane_get((double)(self ? cmask : bmask), (threadIdx.x & 48) + src);
      const int u = __ffs((int)msk) - 1;
      const bool holder = t == src;
      if (holder) { if (self) cmask &= ~(1u << u); else bmask &= ~(1u << u); }
      int ga, gb = -1;
      if (self) {
        const uint32_t gg = ck.ent[src + kTeamLanes * u].geoms;
        ga = gg & 0xff; gb = (gg >> 8) & 0xff;
      } else {
        ga = src + kTeamLanes * u;
      }
      const ContactGeom& a = A.geoms[ga];
      const int na = a.type == 7 ? 3 * a.vert_num : 0;
      const int nb = self && A.geoms[gb].type == 7 ? 3 * A.geoms[gb].vert_num : 0;
      {
        const double* va = A.verts + 3 * (size_t)a.vert_adr;
        for (int k = t; k < na; k += kTeamLanes) S.stage[k] = va[k];
        if (nb) {
          const double* vb = A.verts + 3 * (size_t)A.geoms[gb].vert_adr;
          for (int k = t; k < nb; k += kTeamLanes) S.stage[na + k] = vb[k];
        }
      }
      stage_fence();
      double Ra[9], pa[3];
      query_geom_world(a, F, Ra, pa);
      Shape SA = make_shape(a.type == 7 ? 0 : a.type == 6 ? 1 : 2, pa, Ra, a.size, S.stage, a.vert_num);
      if (a.type == 7) { mulmv(Ra, a.center, SA.center); SA.center[0] += pa[0]; SA.center[1] += pa[1]; SA.center[2] += pa[2]; }
      Shape SB;
      if (self) {
        const ContactGeom& b = A.geoms[gb];
        double Rb[9], pb[3];
        query_geom_world(b, F, Rb, pb);
        SB = make_shape(b.type == 7 ? 0 : b.type == 6 ? 1 : 2, pb, Rb, b.size, S.stage + na, b.vert_num);
        if (b.type == 7) { mulmv(Rb, b.center, SB.center); SB.center[0] += pb[0]; SB.center[1] += pb[1]; SB.center[2] += pb[2]; }
      } else {
        SB = make_shape(1, bp, bR, bs, nullptr, 0);
      }
      const double x0[3] = {SA.center[0] - SB.center[0], SA.center[1] - SB.center[1], SA.center[2] - SB.center[2]};
      double dg[3], gap = 0.0;
      bool in_contact = false;
      if (gilbert_apart<true>(SA, SB, x0, 12, 1e-5, dg, &gap, want_gaps ? 4 : 0)) {
        // apart: `gap` is proven along dg
      } else {
        double dir[3], depth = 0.0;
        gap = 0.0;
        if (mpr_penetration<true, kMprDepth>(SA, SB, &depth, dir, nullptr)) in_contact = depth > kCheckTouch;
        else if (dot3(dir, dir) > 0.5) gap = support_gap(SA, SB, dir);
      }
      if (in_contact) {
        kinds |= self ? kQuerySelf : kQueryBox;
        key = min(key, self ? ((1 << 16) | (src + kTeamLanes * u)) : ((2 << 16) | ga));
      }
      if (holder) {
        // (selects over the lane's registers: a run-time index would put the arrays into scratch)
        if (self) {
          double old = 0.0;
#pragma unroll
          for (int k = 0; k < kCheckPer; ++k) old = k == u ? gp.p[k] : old;
          const double gl = in_contact ? 0.0 : fmax(old, gap_lb(gap));
#pragma unroll
          for (int k = 0; k < kCheckPer; ++k) gp.p[k] = k == u ? gl : gp.p[k];
        } else {
          const double old = u == 0 ? gp.b[0] : gp.b[1];
          const double gl = in_contact ? 0.0 : fmax(old, gap_lb(gap));
#pragma unroll
          for (int k = 0; k < 2; ++k) gp.b[k] = k == u ? gl : gp.b[k];
        }
      }
      stage_fence();
    }
  }
  // the team's answer on every lane
  uint32_t kt = 0;
#pragma unroll
  for (int b = 0; b < 3; ++b) kt |= team_ballot((kinds >> b) & 1u) ? 1u << b : 0u;
  *pkey = (int)team_min((double)key);
  return kt;
}


// MuJoCo's order within a contact (by geom type, then by id) of the pair behind a query_config key: the floor first; self pairs as
// the check's table lists them; the free box (a box) before a hull, after a capsule, after a robot box (lower id)
RCSH_D void query_pair_ids(const QueryArgs& A, int key, int32_t* out) {
  const int kind = key >> 16, i = key & 0xffff;
  if (key == kQueryNoPair) { out[0] = -1; out[1] = -1; return; }
  if (kind == 0) { out[0] = A.plane_geom; out[1] = A.geoms[i].geom_id; return; }
  if (kind == 1) {
    const uint32_t gg = A.ck.ent[i].geoms;
    out[0] = A.geoms[gg & 0xff].geom_id; out[1] = A.geoms[(gg >> 8) & 0xff].geom_id;
    return;
  }
  const bool hull = A.geoms[i].type == 7;
  out[0] = hull ? A.box_geom : A.geoms[i].geom_id;
  out[1] = hull ? A.geoms[i].geom_id : A.box_geom;
}

// the free body's pose of the team's row (zeros: not tested)
RCSH_D bool query_free_pose(const QueryArgs& A, int e, bool live, double* fq) {
  const bool use = live && A.free_qpos && (A.kinds & kQueryBox) && A.box_geom >= 0;
#pragma unroll
  for (int k = 0; k < 7; ++k) fq[k] = use ? A.free_qpos[(size_t)e * 7 + k] : (k == 3 ? 1.0 : 0.0);
  return use;
}

// Point query: one row per team.
template <class T>
__global__ void __launch_bounds__(64) k_collision_query(QueryArgs A) {
  constexpr int kTeams = 64 / kTeamLanes;
  __shared__ QueryTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < A.m;
  const double q = live && t < T::NL ? A.q0[(size_t)e * T::NL + t] : 0.0;
  double fq[7];
  const bool use_box = query_free_pose(A, e, live, fq);
  QueryGaps g;
  int key = kQueryNoPair;
  const uint32_t kinds = query_config<T>(A, lds[team], q, live, fq, use_box, false, g, &key);
  if (live && t == 0) {
    A.hit[e] = kinds != 0;
    if (A.kinds_hit) A.kinds_hit[e] = (uint8_t)kinds;
    if (A.pair) query_pair_ids(A, key, A.pair + 2 * (size_t)e);
  }
}

// The motion validator of one segment per team (see the top of this file), for whoever supplies the segment: the motion query
// (caller's rows) and the environments' collision guard (guard_team.h: the environment's own state and action).  Every lane of the
// wavefront calls it; qa, qb: the lane's joint at the two ends (t < NL), fq / use_box: the free body as query_config takes it.
// result: 0 free (certified), 1 contact at tc, 2 undecided; tc: -1 unless result is 1.  The same on every lane of the team.
// kRigidPairsBySample: a pair of geoms none of whose separating joints travels over the segment keeps its relative pose, so its gap at
// s = 0 is its gap everywhere: not penetrating there, it is free without a certificate (which a gap of exactly 0 -- the closed hand's
// pads -- never passes).  The guard asks for it (its finger slides stand still by construction); the motion query keeps its rule.
template <class T, bool kRigidPairsBySample = false>
RCSH_D void motion_decide(const QueryArgs& A, QueryTeamLds<T>& S, bool live, double qa, double qb, const double* fq, bool use_box,
                          int& result, double& t_contact) {
  constexpr int NL = T::NL;
  const int t = threadIdx.x % kTeamLanes;
  const int tbase = threadIdx.x & 48;
  const double dq = qb - qa;
  const CheckTable& ck = A.ck;
  // how far each joint travels over the whole segment, on every lane; the largest of them
  double trav[NL], maxtrav = 0.0;
#pragma unroll
  for (int j = 0; j < NL; ++j) { trav[j] = lane_get(fabs(dq), tbase + j); maxtrav = fmax(maxtrav, trav[j]); }
  // the most the segment's travel can move a point of geom g (on link l) relative to the frame of link c (-1: the world): the per-geom
  // levers of the joints between the two (build_self_levers), rounded up.  A piece [a, b] is charged (b - a) times this.
  auto reach = [&](int g, int l, int c) -> double {
    if (l < 0) return 0.0;
    const uint32_t jm = anc_mask<T>(l) & ~anc_mask<T>(c);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) s += (jm >> j) & 1u ? (double)ck.lev[kLevGeom + 32 * j + g] * trav[j] : 0.0;
    return s;
  };
  double mp[kCheckPer], mg[2];
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) {
    const int i = t + kTeamLanes * j;
    mp[j] = 0.0;
    if (i < ck.npair) {
      const uint32_t gg = ck.ent[i].geoms;
      const int g0 = gg & 0xff, g1 = (gg >> 8) & 0xff, c = (int)((gg >> 16) & 0xff) - 1;
      const double rel = reach(g0, ck.glink[g0], c) + reach(g1, ck.glink[g1], c);
      // (mp = 0: the certificate skips the pair; every sampled configuration, the first one included, still tests it for contact)
      mp[j] = kRigidPairsBySample && rel == 0.0 ? 0.0 : rel * 1.000001 + 1e-12;
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int g = t + kTeamLanes * u;
    mg[u] = g < ck.ngeom ? reach(g, ck.glink[g], -1) * 1.000001 + 1e-12 : 0.0;
  }
  // the levers hold while every slide stays within the stroke they were built for (the segment is convex: its two ends suffice)
  const bool inside = !(live && t < NL) || (qa >= A.slide_lo[t] && qa <= A.slide_hi[t] && qb >= A.slide_lo[t] && qb <= A.slide_hi[t]);
  const bool can_certify = team_ballot(!inside) == 0;
  // team-uniform state (every lane of the team keeps the same copy)
  bool first = true, done = !live, have_hit = false, undecided = false, grid = false;
  double sL = 0.0, tc = -1.0;
  int top = 0, evals = 0, gk = 0;
  QueryGaps gL, gR;
  while (__ballot(!done)) {
    const double sR = grid ? (double)gk / kQueryGrid : first ? 0.0 : S.stack[top > 0 ? top - 1 : 0];
    const double q = sR == 1.0 ? qb : qa + sR * dq;
    int key = kQueryNoPair;
    const uint32_t kinds = query_config<T>(A, S, q, !done, fq, use_box, !grid, gR, &key);
    if (done) continue;
    const bool hitR = kinds != 0;
    evals += 1;
    if (grid) {
      // the budget is spent: the grid beyond the last settled piece, in increasing s
      if (hitR) { have_hit = true; tc = sR; done = true; }
      else if (++gk > kQueryGrid) { undecided = true; done = true; }
      continue;
    }
    if (first) {
      first = false;
      if (hitR) { have_hit = true; tc = 0.0; done = true; continue; }
      gL = gR;
      if (t == 0) S.stack[0] = 1.0;
      top = 1;
      stage_fence();
      continue;
    }
    // is the piece [sL, sR] certified: for every selected pair, the two ends' gaps exceed what the piece's travel can take from them
    const double w = sR - sL;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < kCheckPer; ++j) ok = ok && (!(mp[j] > 0.0) || gL.p[j] + gR.p[j] > w * mp[j]);
#pragma unroll
    for (int u = 0; u < 2; ++u) ok = ok && (!(mg[u] > 0.0) || (gL.f[u] + gR.f[u] > w * mg[u] && gL.b[u] + gR.b[u] > w * mg[u]));
    const bool certified = !hitR && can_certify && team_ballot(!ok) == 0;
    const double sm = 0.5 * (sL + sR);
    const bool fine = (w * maxtrav <= A.resolution && w <= 1.0 / kQueryGrid) || top >= kQueryStack || !(sm > sL && sm < sR);
    if (hitR) {
      // a contact at sR: what lies beyond it no longer matters; the piece before it is searched for an earlier one
      have_hit = true;
      tc = sR;
      if (fine) { done = true; continue; }
      if (t == 0) { S.stack[0] = sR; S.stack[1] = sm; }
      top = 2;
    } else if (certified || fine) {
      undecided = undecided || !certified;
      sL = sR;
      gL = gR;
      top -= 1;
      if (top == 0) done = true;
    } else {
      if (t == 0) S.stack[top] = sm;
      top += 1;
    }
    stage_fence();
    if (!done && evals >= kQueryBudget) {
      if (have_hit) done = true;  // (a sampled contact stands; one before it may have gone unsampled)
      else { grid = true; gk = (int)floor(sL * kQueryGrid) + 1; if (gk > kQueryGrid) { undecided = true; done = true; } }
    }
  }
  result = have_hit ? 1 : (undecided ? 2 : 0);
  t_contact = have_hit ? tc : -1.0;
}

// Motion query: one segment per team.
template <class T>
__global__ void __launch_bounds__(64) k_motion_query(QueryArgs A) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL;
  __shared__ QueryTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < A.m;
  const double qa = live && t < NL ? A.q0[(size_t)e * NL + t] : 0.0;
  const double qb = live && t < NL ? A.q1[(size_t)e * NL + t] : 0.0;
  double fq[7];
  const bool use_box = query_free_pose(A, e, live, fq);
  int result = 0;
  double tc = -1.0;
  motion_decide<T>(A, lds[team], live, qa, qb, fq, use_box, result, tc);
  if (live && t == 0) {
    A.result[e] = result;
    A.t_contact[e] = tc;
  }
}

#endif  // __HIP__

}  // namespace rcsh
