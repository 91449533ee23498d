// swept_team.h -- swept clearance: the smallest distance along a joint-space motion (rcsh_swept_clearance / rcsh_env_swept_clearance).
//
// The motion query (query_team.h) says whether a straight segment q(s) = q_from + s (q_to - q_from), s in [0, 1], is free; the clearance
// query (clearance_team.h) says how far ONE configuration is from the nearest obstacle.  This kernel joins them: how close does the robot
// come to anything along the segment, where, and to what -- bracketed, not sampled.
//
// The bound.  Over the whole segment the distance d_p of a pair p changes by at most L_p per unit of s: L_p is the motion certificate's
// lever sum (motion_decide's `reach`: the per-geom levers CheckTable::lev + kLevGeom of the joints between the two links, times the
// segment's joint travel, rounded up the same way; against the floor and the free body, which stand still, the geom's own reach).  Over a
// piece [a, b] of width w, with lower bounds v_p(a) <= d_p(a) and v_p(b) <= d_p(b),
//     min over [a, b] of d_p  >=  (v_p(a) + v_p(b) - w L_p) / 2                                        (Piyavskii-Shubert)
// and the piece's bound is the smallest of these over the selected pairs.  The motion certificate "gap(a) + gap(b) > w L_p" is the case
// "the bound is positive".  A pair no separating joint moves (L_p = 0) keeps its distance: it is looked at in the first sample alone
// (its value there bounds it everywhere and is never below that sample's clearance), so it is refined at most once per row.
//
// The walk is motion_decide's: pieces in increasing s from a per-team stack of right ends in LDS, one sampled configuration a round.
// `best` is the smallest exact clearance sampled so far (an upper bound of the minimum, attained at `s`).  A piece is DISCARDED when its
// bound is >= min(best - tolerance, d_max) and positive (so every discarded piece is also certified free, which is what the contact
// search below relies on); otherwise it is bisected, until its largest joint travel is at most `resolution` (and it is no longer than
// 1 / kQueryGrid), the stack is full or the budget is spent: then it is left UNSPLIT.  lower = min(best, the smallest bound of any
// discarded or unsplit piece).  Because `best` only falls, a piece discarded against an earlier `best` still satisfies
// bound >= final best - tolerance: when every piece was discarded, best - lower <= tolerance, which is status 0's promise.
//
// A sample.  Every selected pair gets its cheap lower bound, a lane per pair (bounding spheres, oriented boxes' face separation; the floor
// exact) -- as the clearance kernel has them; -inf where the boxes overlap.  A pair is refined to its exact distance (gjk_distance; in
// contact the narrow phase's depth) only (a) while its bound is below the smallest exact value of this sample and below min(best, d_max)
// -- so a sample that improves `best` carries the point query's answer, best first, ties to the lowest key -- or (b) when the piece
// [sL, sR] could not be discarded with the cheap value: v_p(sR) < 2 threshold + w L_p - v_p(sL).  Only one configuration's frames are in
// LDS at a time: the left end keeps the values it was given when it was the right end.
//
// Contact.  A sample that penetrates by more than kCheckTouch (the point query's predicate) ends the minimisation: what lies beyond it
// no longer matters, and the piece before it is searched as motion_decide searches it (everything before that piece has been discarded,
// i.e. certified free, or was left unsplit at `resolution`): certified free (bound > 0) or bisected down to `resolution`.  The row
// reports the smallest sampled parameter in contact and the point query's status-2 answer there.  The deepest penetration along the path
// is not looked for.
//
// Work per row: at most kSweptBudget configurations for the minimisation, and at most kSweptContactBudget more once a contact has been
// sampled: evals <= kSweptBudget + kSweptContactBudget.  The final frames for the gradient are not counted.
//
// What is shared with the family: query_row_setup, query_box_frame, query_env_row, query_free_pose, query_geom_world, query_pair_ids,
// gap_lb (query_team.h), gjk_distance, clear_offer, clear_selected, ClearBest, ClearArgs (clearance_team.h) are CALLED.  The bounds of a
// sample, the narrow phase's set-up and the gradient are restated here from k_clearance_query, and the lever sums from motion_decide:
// sharing their text has made the existing kernels slower before (profiles/query_rows/), so those kernels are not touched.
#pragma once
#include "clearance_team.h"

namespace rcsh {

constexpr int kSweptBracketed = 0, kSweptBeyond = 1, kSweptContact = 2, kSweptOpen = 3;  // the status byte of a row
constexpr int kSweptBudget = 2048;         // configurations a row may evaluate while it minimises (kQueryBudget's size)
constexpr int kSweptContactBudget = 256;   // ... and on top of them once a contact has been sampled (the search for the first one)

struct SweptArgs {
  ClearArgs C;        // Q.q0 / Q.q1: the segment's ends ([m][NL]; env form: q0 unused), Q.resolution; pair_mask, d_max, the point outputs
  double tolerance;   // the bracket width asked for
  double* lower;      // [m] or null
  double* s;          // [m] or null
  int32_t* evals;     // [m] or null
};

#if defined(__HIP__)

// per lane: the lane's pairs j (t + 16 j), its geoms u (t + 16 u) against the floor and against the free body
struct SweptVals {
  double p[kCheckPer], f[2], b[2];
};
constexpr int kSweptBitF = kCheckPer, kSweptBitB = kCheckPer + 2;  // bits of the lane's selection mask: pairs, floor, free body

// One configuration of a swept row, per team (every lane of the wavefront calls it; a finished team with live = false).
// sel: the lane's entries that take part; cut: exact values are wanted below it (min(best, d_max); 0 in the contact search); an entry is
// also refined while its bound is below base + w L - vL (the value the piece [sL, sR] needs of it; base = -inf: no piece).
// v: lower bounds of the lane's entries at this configuration (+inf: takes no part), exact where refined.  B: the sample's best pair.
template <class T>
RCSH_D void swept_sample(const ClearArgs& A, QueryTeamLds<T>& S, double q, bool live, const double* bp, const double* bR, bool use_box, uint32_t sel,
                         double cut, double base, double w, const SweptVals& L, const SweptVals& vL, SweptVals& v, ClearBest& B) {
  const int t = threadIdx.x & (kTeamLanes - 1);
  const int tbase = threadIdx.x & 48;
  const QueryArgs& Q = A.Q;
  const CheckTable& ck = Q.ck;
  const int ngeom = ck.ngeom;
  query_row_setup<T>(Q, S, q);
  const double* F = &S.F[0][0];
  const double* bs = Q.box_size;
  uint32_t pend = 0;  // the lane's entries whose value is a bound still
  // ---- the floor (exact, with its witness) and the bounds of the free body's pairs
  double fl_val = INFINITY, fl_w[3] = {0, 0, 0};
  int fl_key = kQueryNoPair, fl_link = -1;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    v.f[u] = INFINITY;
    v.b[u] = INFINITY;
    const int g = t + kTeamLanes * u;
    const bool on_floor = live && ((sel >> (kSweptBitF + u)) & 1u), at_box = live && ((sel >> (kSweptBitB + u)) & 1u);
    if (!on_floor && !at_box) continue;
    const ContactGeom& cg = Q.geoms[g < ngeom ? g : 0];
    double gR[9], gpos[3];
    query_geom_world(cg, F, gR, gpos);
    if (on_floor) {
      const double* n = Q.plane_n;
      double nl[3], wl[3] = {0, 0, 0}, low;
      bool exact = true;
      mulTv(gR, n, nl);
      const double c0 = dot3(n, gpos) - Q.plane_d;
      if (cg.type == 6) {
#pragma unroll
        for (int k = 0; k < 3; ++k) wl[k] = nl[k] > 0.0 ? -cg.size[k] : cg.size[k];
        low = c0 + dot3(nl, wl);
      } else if (cg.type == 3) {
        wl[2] = nl[2] > 0.0 ? -cg.size[1] : cg.size[1];
        low = c0 + nl[2] * wl[2] - cg.size[0];
      } else {
        // the hull's bounding box first; its vertices only where the box's bound does not do
        low = c0 + dot3(nl, cg.aabb_c) - (fabs(nl[0]) * cg.aabb_h[0] + fabs(nl[1]) * cg.aabb_h[1] + fabs(nl[2]) * cg.aabb_h[2]);
        if (low < cut || low < base + w * L.f[u] - vL.f[u]) {
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
          low = low - 1e-12;  // (the box's bound, rounded down)
          exact = false;
        }
      }
      v.f[u] = low;
      if (exact && low < fl_val) {  // (u ascending: the lower geom keeps a tie)
        double ww[3];
        mulmv(gR, wl, ww);
        fl_val = low;
        fl_key = (0 << 16) | g;
        fl_link = cg.link;
#pragma unroll
        for (int k = 0; k < 3; ++k) fl_w[k] = ww[k] + gpos[k];  // (a capsule: the end of its core segment)
      }
    }
    if (at_box) {
      double hc[3], hh[3], oc[3];
      geom_obb(cg, hc, hh);
      mulmv(gR, hc, oc);
      const double cw[3] = {oc[0] + gpos[0], oc[1] + gpos[1], oc[2] + gpos[2]};
      const double d[3] = {cw[0] - bp[0], cw[1] - bp[1], cw[2] - bp[2]};
      const double rs = sqrt(dot3(hh, hh)) + sqrt(dot3(bs, bs));
      const double dd = sqrt(dot3(d, d));
      if (dd > rs) v.b[u] = gap_lb(dd - rs);
      else {
        double bsz[3] = {bs[0], bs[1], bs[2]}, bRc[9], bpc[3] = {bp[0], bp[1], bp[2]};
#pragma unroll
        for (int k = 0; k < 9; ++k) bRc[k] = bR[k];
        const double sep = obb_face_sep(gR, cw, hh, bRc, bpc, bsz);
        v.b[u] = sep > 0.0 ? gap_lb(sep) : -INFINITY;
      }
      pend |= 1u << (kSweptBitB + u);
    }
  }
  // ---- the bounds of the lane's self pairs
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) {
    v.p[j] = INFINITY;
    if (!live || !((sel >> j) & 1u)) continue;
    const CheckEntry en = ck.ent[t + kTeamLanes * j];
    const int g0 = en.geoms & 0xff, g1 = (en.geoms >> 8) & 0xff;
    const double* ca = S.wbox[g0];
    const double* cb = S.wbox[g1];
    const double d[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    const double dd = sqrt(dot3(d, d));
    pend |= 1u << j;
    if (dd > (double)en.rsum) { v.p[j] = gap_lb(dd - (double)en.rsum); continue; }
    double Ra[9], Rb[9], pa[3], pb[3], ha[3], hb[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { pa[k] = ca[k]; pb[k] = cb[k]; ha[k] = ck.gh[g0][k]; hb[k] = ck.gh[g1][k]; }
#pragma unroll
    for (int k = 0; k < 9; ++k) { Ra[k] = ca[3 + k]; Rb[k] = cb[3 + k]; }
    const double sep = obb_face_sep(Ra, pa, ha, Rb, pb, hb);
    v.p[j] = sep > 0.0 ? gap_lb(sep) : -INFINITY;
  }
  // ---- the best floor pair of the team
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
  // ---- refinement, best first: the pending entry of the smallest bound among those wanted, one a round per team on its 16 lanes
  for (;;) {
    const double cb = fmin(B.value, cut);
    double lb = INFINITY;
    int lkey = kQueryNoPair;
#pragma unroll
    for (int j = 0; j < kCheckPer; ++j) {
      const bool s = ((pend >> j) & 1u) && (v.p[j] < cb || v.p[j] < base + w * L.p[j] - vL.p[j]) && v.p[j] < lb;
      lb = s ? v.p[j] : lb;
      lkey = s ? ((1 << 16) | (t + kTeamLanes * j)) : lkey;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool s = ((pend >> (kSweptBitB + u)) & 1u) && (v.b[u] < cb || v.b[u] < base + w * L.b[u] - vL.b[u]) && v.b[u] < lb;
      lb = s ? v.b[u] : lb;
      lkey = s ? ((2 << 16) | (t + kTeamLanes * u)) : lkey;
    }
    const double m = team_min(lb);
    const int key = (int)team_min(lb == m ? (double)lkey : (double)kQueryNoPair);
    const bool mine = live && key != kQueryNoPair;
    if (__ballot(mine) == 0) break;
    if (mine) {
      const int kind = key >> 16, idx = key & 0xffff;
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
      double bpc[3] = {bp[0], bp[1], bp[2]}, bRc[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) bRc[k] = bR[k];
      if (ga >= 0) {
        const ContactGeom& a = Q.geoms[ga];
        double Ra[9], pa[3];
        query_geom_world(a, F, Ra, pa);
        SA = make_shape(a.type == 7 ? 0 : a.type == 6 ? 1 : 2, pa, Ra, a.size, S.stage, a.vert_num);
        if (a.type == 7) { mulmv(Ra, a.center, SA.center); SA.center[0] += pa[0]; SA.center[1] += pa[1]; SA.center[2] += pa[2]; }
        la = a.link;
        ra = a.type == 3 ? a.size[0] : 0.0;
      } else {
        SA = make_shape(1, bpc, bRc, bs, nullptr, 0);
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
        SB = make_shape(1, bpc, bRc, bs, nullptr, 0);
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
      if (t == (idx & (kTeamLanes - 1))) {  // the holder: the value in place of the bound (selects: the arrays stay in registers)
        const int slot = idx / kTeamLanes;
        if (kind == 1) {
#pragma unroll
          for (int k = 0; k < kCheckPer; ++k) v.p[k] = k == slot ? value : v.p[k];
          pend &= ~(1u << slot);
        } else {
#pragma unroll
          for (int k = 0; k < 2; ++k) v.b[k] = k == slot ? value : v.b[k];
          pend &= ~(1u << (kSweptBitB + slot));
        }
      }
      clear_offer(B, value, key, la, lb_, open, wa, wb, n);
      stage_fence();
    }
  }
}

// Swept clearance: one segment per team.
template <class T>
__global__ void __launch_bounds__(64) k_swept_clearance(SweptArgs W) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL;
  __shared__ QueryTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int tbase = threadIdx.x & 48;
  QueryTeamLds<T>& S = lds[team];
  const ClearArgs& A = W.C;
  const QueryArgs& Q = A.Q;
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < Q.m;
  const bool valid = t < NL;
  const CheckTable& ck = Q.ck;
  // ---- the row: the caller's, or the environment's own chain and free body as the start
  double qa, fq[7];
  bool use_box;
  if (A.S) {
    use_box = query_env_row(A.S, Q.m, e, live, valid, A.qpos_field, A.box_field, qa, fq);
  } else {
    qa = live && valid ? Q.q0[(size_t)e * NL + t] : 0.0;
    use_box = query_free_pose(Q, e, live, fq);
  }
  const double qb = live && valid ? Q.q1[(size_t)e * NL + t] : 0.0;
  const double dq = qb - qa;
  double bp[3], bR[9];
  query_box_frame(fq, use_box, bp, bR);
  const double d_max = A.d_max, tol = W.tolerance;
  // ---- per-pair constants: the most the whole segment's travel can move the two geoms of an entry relative to each other
  // (motion_decide's arithmetic); an entry nothing moves is rigid
  double trav[NL], maxtrav = 0.0;
#pragma unroll
  for (int j = 0; j < NL; ++j) { trav[j] = lane_get(fabs(dq), tbase + j); maxtrav = fmax(maxtrav, trav[j]); }
  auto reach = [&](int g, int l, int c) -> double {
    if (l < 0) return 0.0;
    const uint32_t jm = anc_mask<T>(l) & ~anc_mask<T>(c);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) s += (jm >> j) & 1u ? (double)ck.lev[kLevGeom + 32 * j + g] * trav[j] : 0.0;
    return s;
  };
  SweptVals L;
  uint32_t sel = 0, rigid = 0;
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) {
    const int i = t + kTeamLanes * j;
    L.p[j] = 0.0;
    if (live && (Q.kinds & kQuerySelf) && i < ck.npair && clear_selected(A, (1 << 16) | i)) {
      const uint32_t gg = ck.ent[i].geoms;
      const int g0 = gg & 0xff, g1 = (gg >> 8) & 0xff, c = (int)((gg >> 16) & 0xff) - 1;
      const double rel = reach(g0, ck.glink[g0], c) + reach(g1, ck.glink[g1], c);
      L.p[j] = rel == 0.0 ? 0.0 : rel * 1.000001 + 1e-12;
      sel |= 1u << j;
      rigid |= rel == 0.0 ? 1u << j : 0u;
    }
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int g = t + kTeamLanes * u;
    L.f[u] = 0.0;
    L.b[u] = 0.0;
    if (!live || g >= ck.ngeom) continue;
    const double rel = reach(g, ck.glink[g], -1);
    const double lg = rel == 0.0 ? 0.0 : rel * 1.000001 + 1e-12;
    if (((Q.floor_bits >> g) & 1u) && clear_selected(A, (0 << 16) | g)) {
      L.f[u] = lg;
      sel |= 1u << (kSweptBitF + u);
      rigid |= rel == 0.0 ? 1u << (kSweptBitF + u) : 0u;
    }
    if (use_box && ((Q.box_bits >> g) & 1u) && clear_selected(A, (2 << 16) | g)) {
      L.b[u] = lg;
      sel |= 1u << (kSweptBitB + u);
      rigid |= rel == 0.0 ? 1u << (kSweptBitB + u) : 0u;
    }
  }
  // the levers hold while every slide stays within the stroke they were built for (the segment is convex: its two ends suffice)
  const bool inside = !(live && valid) || (qa >= Q.slide_lo[t] && qa <= Q.slide_hi[t] && qb >= Q.slide_lo[t] && qb <= Q.slide_hi[t]);
  const bool can_certify = team_ballot(!inside) == 0;
  const double res_min = can_certify ? Q.resolution : INFINITY;  // (nothing can be proven: the grid of 1 / kQueryGrid is sampled)
  // ---- team-uniform state (every lane of the team keeps the same copy)
  bool first = true, done = !live, contact = false;
  double sL = 0.0, best_s = 0.0, lowacc = INFINITY;
  int top = 0, evals = 0, cevals = 0;
  ClearBest best, B;
  best.value = INFINITY; best.key = kQueryNoPair; best.la = -1; best.lb = -1; best.open = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) { best.wa[k] = 0.0; best.wb[k] = 0.0; best.n[k] = 0.0; }
  SweptVals vL, vR;
#pragma unroll
  for (int j = 0; j < kCheckPer; ++j) vL.p[j] = INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u) { vL.f[u] = INFINITY; vL.b[u] = INFINITY; }
  while (__ballot(!done)) {
    const double sR = first ? 0.0 : S.stack[top > 0 ? top - 1 : 0];
    const double q = sR == 1.0 ? qb : qa + sR * dq;
    const double w = sR - sL;
    // what a piece must reach to be discarded: min(best - tolerance, d_max), and more than 0
    const double thr0 = contact ? 0.0 : fmax(fmin(best.value - tol, d_max), 0.0);
    const double base = first || !can_certify ? -INFINITY : 2.0 * thr0;
    const double cut = contact ? 0.0 : fmin(best.value, d_max);
    swept_sample<T>(A, S, q, !done, bp, bR, use_box, sel, cut, base, w, L, vL, vR, B);
    if (done) continue;
    const bool hitR = B.value < -kCheckTouch;
    if (contact) cevals += 1; else evals += 1;
    // the sample is the best so far: the point query's answer at q(sR) (an iteration that did not converge is no attained value: it
    // is taken only while there is no other)
    if (hitR || (!contact && B.value < best.value && (!B.open || best.key == kQueryNoPair))) { best = B; best_s = sR; }
    if (first) {
      first = false;
      if (hitR) { contact = true; done = true; continue; }
      vL = vR;
      sel &= ~rigid;  // (a rigid entry's value here is its value everywhere, and no smaller than this sample's clearance)
      if (!(maxtrav > 0.0)) { done = true; continue; }
      if (t == 0) S.stack[0] = 1.0;
      top = 1;
      stage_fence();
      continue;
    }
    // the piece [sL, sR]: its bound, the same on every lane of the team
    double lo = INFINITY;
#pragma unroll
    for (int j = 0; j < kCheckPer; ++j) lo = fmin(lo, (sel >> j) & 1u ? 0.5 * (vL.p[j] + vR.p[j] - w * L.p[j]) : INFINITY);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      lo = fmin(lo, (sel >> (kSweptBitF + u)) & 1u ? 0.5 * (vL.f[u] + vR.f[u] - w * L.f[u]) : INFINITY);
      lo = fmin(lo, (sel >> (kSweptBitB + u)) & 1u ? 0.5 * (vL.b[u] + vR.b[u] - w * L.b[u]) : INFINITY);
    }
    const double bound = can_certify ? team_min(lo) : -INFINITY;
    const bool now_contact = contact || hitR;
    const double thr = now_contact ? 0.0 : fmin(best.value - tol, d_max);
    const bool ok = !hitR && bound >= thr && bound > 0.0;
    const double sm = 0.5 * (sL + sR);
    const double res = now_contact ? Q.resolution : res_min;
    const bool fine = (w * maxtrav <= res && w <= 1.0 / kQueryGrid) || top >= kQueryStack || !(sm > sL && sm < sR);
    if (hitR) {
      // a contact at sR: what lies beyond it no longer matters; the piece before it is searched for an earlier one
      contact = true;
      if (fine) { done = true; continue; }
      if (t == 0) { S.stack[0] = sR; S.stack[1] = sm; }
      top = 2;
    } else if (ok || fine) {
      lowacc = fmin(lowacc, bound);
      sL = sR;
      vL = vR;
      top -= 1;
      if (top == 0) done = true;
    } else {
      if (t == 0) S.stack[top] = sm;
      top += 1;
    }
    stage_fence();
    if (!done && (contact ? cevals >= kSweptContactBudget : evals >= kSweptBudget)) {
      // the budget is spent: what is left of the segment is bounded from its left end alone
      double rem = INFINITY;
#pragma unroll
      for (int j = 0; j < kCheckPer; ++j) rem = fmin(rem, (sel >> j) & 1u ? vL.p[j] - (1.0 - sL) * L.p[j] : INFINITY);
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        rem = fmin(rem, (sel >> (kSweptBitF + u)) & 1u ? vL.f[u] - (1.0 - sL) * L.f[u] : INFINITY);
        rem = fmin(rem, (sel >> (kSweptBitB + u)) & 1u ? vL.b[u] - (1.0 - sL) * L.b[u] : INFINITY);
      }
      lowacc = fmin(lowacc, team_min(rem));
      done = true;
    }
  }
  // ---- the row's answer
  const bool beyond = !contact && !(best.value < d_max);
  const double distance = beyond ? d_max : best.value;
  const double lower = contact || !can_certify ? -INFINITY : fmin(distance, lowacc);
  const int status = contact ? kSweptContact : beyond ? (lower >= d_max ? kSweptBeyond : kSweptOpen)
                                                      : (!best.open && distance - lower <= tol ? kSweptBracketed : kSweptOpen);
  if (live && t == 0) {
    A.distance[e] = distance;
    if (W.lower) W.lower[e] = lower;
    if (W.s) W.s[e] = beyond ? -1.0 : best_s;
    if (W.evals) W.evals[e] = evals + cevals;
    if (A.status) A.status[e] = (uint8_t)status;
    if (A.pair) query_pair_ids(Q, beyond ? kQueryNoPair : best.key, A.pair + 2 * (size_t)e);
    if (A.witness) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        A.witness[6 * (size_t)e + k] = beyond ? 0.0 : best.wa[k];
        A.witness[6 * (size_t)e + 3 + k] = beyond ? 0.0 : best.wb[k];
      }
    }
  }
  // ---- the gradient at q(s), as the clearance query has it: the frames of that configuration once more (the same arithmetic on the same
  // joint values: the same bits)
  if (A.grad) {  // (the same on every lane of the wavefront)
    query_row_setup<T>(Q, S, best_s == 1.0 ? qb : qa + best_s * dq);
    if (live && valid) {
      const double* F = &S.F[0][0];
      const LinkRec& r = Q.links[t];
      const double* Fj = F + 12 * t;
      double Rj[9], ax[3], an[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) Rj[k] = Fj[k];
      mulmv(Rj, r.axis, ax);
      mulmv(Rj, r.jpos, an);
      an[0] += Fj[9]; an[1] += Fj[10]; an[2] += Fj[11];
      const bool slide = r.jtype == kSlide;
      const double ra_[3] = {best.wa[0] - an[0], best.wa[1] - an[1], best.wa[2] - an[2]}, rb_[3] = {best.wb[0] - an[0], best.wb[1] - an[1], best.wb[2] - an[2]};
      double va[3], vb[3];
      cross3(ax, ra_, va);
      cross3(ax, rb_, vb);
      const bool ma = (anc_mask<T>(best.la) >> t) & 1u, mb = (anc_mask<T>(best.lb) >> t) & 1u;
      double g = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) g += best.n[k] * ((mb ? (slide ? ax[k] : vb[k]) : 0.0) - (ma ? (slide ? ax[k] : va[k]) : 0.0));
      A.grad[(size_t)e * NL + t] = beyond ? 0.0 : g;
    }
  }
}

// a robot without collision geoms: nothing is within d_max of anything, anywhere on the segment
__global__ void k_swept_fill(double* lower, double* s, int32_t* evals, double d_max, int m) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  if (lower) lower[i] = d_max;
  if (s) s[i] = -1.0;
  if (evals) evals[i] = 0;
}

#endif  // __HIP__

}  // namespace rcsh
