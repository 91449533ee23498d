// dynamics_team.h -- dynamics queries on configurations the caller supplies (rcsh_dynamics_query / rcsh_env_dynamics).
//
// The stepping kernels compute the joint-space inertia, the bias forces and the gravity compensation inside every substep
// (dyn_team.h, team_substep) and the site Jacobian inside the CLIK (ik_team.h); none of it leaves them.  This kernel returns those
// intermediates for M rows (q, qvel, qacc_in, qfrc_in) at once: what a model-based controller reads off mjData (qM, qfrc_bias,
// qfrc_gravcomp, mj_jac) plus rigid-body inverse and forward dynamics of the unconstrained chain.
//
// One row per TEAM of 16 lanes (team.h), lane t owning link / joint t, four rows per wavefront, as the other query kernels.  Per row:
//  1. link frames (link_local_frame, scan_frames), motion axes about the world origin, velocities and velocity-product accelerations
//     (scan_from_root) -- team_substep's first two phases;
//  2. spatial inertias about the world origin, composite inertias, the subtree's bias wrench and, beside it, the subtree's wrench under
//     gravity alone (I a_g, no velocity terms: one more leaf-to-root scan, not a second pass), the gravity-compensation moment
//     (scan_from_leaves; the general path and the team_gc_is_mass shortcut) -- team_substep's third phase;
//  3. the mass-matrix rows through the team's LDS block, the lower triangle as team_substep leaves it; the upper is mirrored on the way
//     out;
//  4. qfrc_inverse = M qacc_in + qfrc_bias from the block's rows; qacc = M^-1 (qfrc_in - qfrc_bias) by ldl_factor / ldl_solve, every
//     lane solving the same system and keeping its own entry;
//  5. the TCP's geometric Jacobian, lane j forming joint j's column in the robot-base frame.
// The phase sequence is restated here, not shared with team_substep: a shared function would change the stepping kernels' text.  Every
// output is computed by the same instructions whichever others are asked for; a phase whose results nobody reads (the solve, the
// Jacobian) is skipped as a whole.  No actuator, damping, limit, equality, friction or contact term enters any output.
#pragma once
#include "query_team.h"

namespace rcsh {

struct DynOut {
  double* qM;             // [m][nl][nl]
  double* qfrc_bias;      // [m][nl]
  double* gravity;        // [m][nl]
  double* qfrc_gravcomp;  // [m][nl]
  double* jac;            // [m][6][nl]
  double* qfrc_inverse;   // [m][nl]
  double* qacc;           // [m][nl]
};

struct DynArgs {
  const LinkRec* links;  // the model's link records (behind the DevModel)
  int32_t m;
  int32_t site_link;     // link carrying the attachment site (-1: static -- the Jacobian is zero)
  double gravity[3];
  double tcp_p[3];       // the TCP point in the site link's frame
  double base_R[9];      // world <- robot base
  const double *q, *qvel, *qacc_in, *qfrc_in;  // [m][nl]; qvel null: zero; the last two only where their outputs are asked for
  DynOut o;
  const double* S;       // env form: the state, [field][n] with n = m (null: the caller's rows)
  int32_t qpos_field, qvel_field;
};

#if defined(__HIP__)

// LDS block of one team: the motion axes, the mass-matrix rows (lower triangle valid), qacc_in and the forward dynamics' right-hand side
template <class T>
struct DynTeamLds {
  static constexpr int NLP = even_up(T::NL);
  double S[T::NL][6];
  double M[T::NL][NLP];
  double a[NLP];
  double r[NLP];
};

template <class T>
__global__ void __launch_bounds__(64) k_dynamics_query(DynArgs A) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM;
  static_assert(!T::GRIP || NA + 1 < 8 || NA == 7, "the chain rounds of the scans reach 8 lanes; NARM = 7 uses the bank masks");
  __shared__ DynTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int tbase = threadIdx.x & 48;
  DynTeamLds<T>& B = lds[team];
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < A.m;
  const bool valid = t < NL;
  const bool mine = live && valid;
  const int tl = valid ? t : NL - 1;
  const LinkRec* links = A.links;
  const LinkRec& lk = links[tl];
  const DynOut& o = A.o;
  // ---- the row: the caller's, or the environment's own chain (dead teams and lanes off the chain compute on zeros and store nothing)
  double q, qd = 0.0, qa = 0.0, qf = 0.0;
  const size_t at = (size_t)(live ? e : 0) * NL + tl;
  if (A.S) {
    double fq[7];
    query_env_row(A.S, A.m, e, live, valid, A.qpos_field, -1, q, fq);
    qd = mine ? A.S[(size_t)(A.qvel_field + t) * A.m + e] : 0.0;
  } else {
    q = mine ? A.q[at] : 0.0;
    if (A.qvel) qd = mine ? A.qvel[at] : 0.0;
  }
  if (o.qfrc_inverse) qa = mine ? A.qacc_in[at] : 0.0;
  if (o.qacc) qf = mine ? A.qfrc_in[at] : 0.0;
  const bool gc_is_mass = team_gc_is_mass<T>(links, t);
  KinK kk;
  kk.load(lk);
  InertK ik;
  ik.load(lk);
  const double armature = lk.armature, gcm_sub = lk.gcm_sub;
  const bool is_slide = kk.jtype == kSlide;

  // ---- world frame of the link
  double R[9], p[3];
  link_local_frame(kk, q, R, p);
  scan_frames<T>(R, p);

  // ---- motion axis about the world origin, velocity and velocity-product acceleration of the link
  double S[6], ax[3], anchor[3];
  {
    mulmv(R, kk.axis, ax);
    mulmv(R, kk.jpos, anchor);
    anchor[0] += p[0]; anchor[1] += p[1]; anchor[2] += p[2];
    double mom[3];
    cross3(anchor, ax, mom);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      S[k] = is_slide ? 0.0 : ax[k];
      S[3 + k] = is_slide ? ax[k] : mom[k];
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < 6; ++k) B.S[tl][k] = S[k];
    B.a[tl] = qa;
  }
  double vel[6], acc[6];
  const double chain = t <= NA ? 1.0 : 0.0, second = t == NA + 1 ? 1.0 : 0.0;  // (only read by archetypes with a gripper)
#pragma unroll
  for (int k = 0; k < 6; ++k) vel[k] = scan_from_root<T>(S[k] * qd, chain, second);
  {
    double sd[6];
    cross_motion(vel, S, sd);  // S x S = 0: the link's own joint velocity does not contribute
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = scan_from_root<T>(sd[k] * qd, chain, second);
    acc[3] -= A.gravity[0]; acc[4] -= A.gravity[1]; acc[5] -= A.gravity[2];
  }
  const double ag[6] = {0.0, 0.0, 0.0, -A.gravity[0], -A.gravity[1], -A.gravity[2]};  // every link's acceleration at rest

  // ---- spatial inertia about the world origin, composite inertia, bias and gravity wrenches, gravity-compensation first moment
  double Ic[10], F[6], Fg[6], hs[3];
  {
    const double ms = valid ? ik.mass : 0.0;
    const double gcm = valid ? ik.gcm : 0.0;
    double c[3], cg[3];
    mulmv(R, ik.com, c);
    c[0] += p[0]; c[1] += p[1]; c[2] += p[2];
    if (ik.gc_same_com) {
      cg[0] = c[0]; cg[1] = c[1]; cg[2] = c[2];
    } else {
      mulmv(R, lk.gccom, cg);
      cg[0] += p[0]; cg[1] += p[1]; cg[2] += p[2];
    }
    const double* J = ik.J;
    const double vz = valid ? 1.0 : 0.0;
    const double Jm[9] = {vz * J[0], vz * J[3], vz * J[4], vz * J[3], vz * J[1], vz * J[5], vz * J[4], vz * J[5], vz * J[2]};
    double Tm[9];
    mulmm(R, Jm, Tm);
    double Ii[10];
    Ii[0] = Tm[0] * R[0] + Tm[1] * R[1] + Tm[2] * R[2] + ms * (c[1] * c[1] + c[2] * c[2]);
    Ii[1] = Tm[3] * R[3] + Tm[4] * R[4] + Tm[5] * R[5] + ms * (c[0] * c[0] + c[2] * c[2]);
    Ii[2] = Tm[6] * R[6] + Tm[7] * R[7] + Tm[8] * R[8] + ms * (c[0] * c[0] + c[1] * c[1]);
    Ii[3] = Tm[0] * R[3] + Tm[1] * R[4] + Tm[2] * R[5] - ms * c[0] * c[1];
    Ii[4] = Tm[0] * R[6] + Tm[1] * R[7] + Tm[2] * R[8] - ms * c[0] * c[2];
    Ii[5] = Tm[3] * R[6] + Tm[4] * R[7] + Tm[5] * R[8] - ms * c[1] * c[2];
    Ii[6] = ms * c[0]; Ii[7] = ms * c[1]; Ii[8] = ms * c[2];
    Ii[9] = ms;
    double Ia[6], Ig[6], Iv[6], vf[6];
    inert_mul(Ii, acc, Ia);
    inert_mul(Ii, ag, Ig);
    inert_mul(Ii, vel, Iv);
    cross_force(vel, Iv, vf);
    const bool ff = T::GRIP && t == NA;
#pragma unroll
    for (int k = 0; k < 9; ++k) Ic[k] = scan_from_leaves<T>(Ii[k], ff);
#pragma unroll
    for (int k = 0; k < 6; ++k) F[k] = scan_from_leaves<T>(Ia[k] + vf[k], ff);
#pragma unroll
    for (int k = 0; k < 6; ++k) Fg[k] = scan_from_leaves<T>(Ig[k], ff);
    if (gc_is_mass) {
      // every body fully gravity-compensated (gravcomp = 1, the RCS scenes): the compensated first moment IS the first moment of the
      // composite inertia, and the subtree mass is the model constant gcm_sub
      Ic[9] = valid ? gcm_sub : 0.0;
      hs[0] = Ic[6]; hs[1] = Ic[7]; hs[2] = Ic[8];
    } else {
      Ic[9] = scan_from_leaves<T>(Ii[9], ff);
#pragma unroll
      for (int k = 0; k < 3; ++k) hs[k] = scan_from_leaves<T>(gcm * cg[k], ff);
    }
  }

  // (a scheduling fence between the scans and the matrix phases: scheduled as one region under the iterative-ilp strategy, the
  // Topo<7, true> instance crashes the register allocator of the ROCm 7.2 compiler)
  sched_fence();

  // ---- mass-matrix row of the link: M[t][j] = S_j . (Ic_t S_t) for the ancestors j (and itself), armature on the diagonal
  double G[6];
  inert_mul(Ic, S, G);
  team_sync();  // every lane's S and qacc_in are in the block
  double row[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    double Sj[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Sj[k] = B.S[j][k];
    row[j] = dot6(Sj, G);
  }
  if (T::GRIP) row[NA] = t == NA + 1 ? 0.0 : row[NA];  // the fingers are siblings
#pragma unroll
  for (int j = 0; j < NL; ++j) row[j] += j == tl ? armature : 0.0;
  const double bias = dot6(S, F);
  const double grav = dot6(S, Fg);
  double gc;
  {
    const double ng[3] = {-A.gravity[0], -A.gravity[1], -A.gravity[2]};
    double w[6];
    cross3(hs, ng, w);
    w[3] = gcm_sub * ng[0]; w[4] = gcm_sub * ng[1]; w[5] = gcm_sub * ng[2];
    gc = dot6(S, w);
  }
  if (valid) {
#pragma unroll
    for (int j = 0; j < NL; ++j) B.M[tl][j] = row[j];  // (entries right of the diagonal: not ancestors, never read)
    B.r[tl] = qf - bias;
  }
  team_sync();
  // the full row: left of the diagonal the lane's own entries, right of it the column below the diagonal
  double full[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) full[j] = j <= tl ? row[j] : B.M[j][tl];
  if (mine) {
    if (o.qM) {
#pragma unroll
      for (int j = 0; j < NL; ++j) o.qM[at * NL + j] = full[j];
    }
    if (o.qfrc_bias) o.qfrc_bias[at] = bias;
    if (o.gravity) o.gravity[at] = grav;
    if (o.qfrc_gravcomp) o.qfrc_gravcomp[at] = gc;
  }

  // ---- inverse dynamics of the chain: M qacc_in + qfrc_bias
  if (o.qfrc_inverse) {
    double s = bias;
#pragma unroll
    for (int j = 0; j < NL; ++j) s += full[j] * B.a[j];
    if (mine) o.qfrc_inverse[at] = s;
  }

  // ---- forward dynamics of the unconstrained chain: every lane factors the same matrix and keeps its joint's entry
  if (o.qacc) {
    double H[T::NTRI], x[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) H[tri(i, j)] = B.M[i][j];
      x[i] = B.r[i];
    }
    ldl_factor<NL>(H);
    ldl_solve<NL>(H, x);
    double xt = 0.0;
#pragma unroll
    for (int i = 0; i < NL; ++i) xt = i == tl ? x[i] : xt;
    if (mine) o.qacc[at] = xt;
  }

  // ---- the TCP's geometric Jacobian in the robot-base frame: lane j, joint j.  The TCP rides on the site's link: per radian of a hinge
  // above it the point moves by axis x (point - anchor) and the frame turns about the axis; per metre of a slide it moves by the axis
  if (o.jac) {
    const int sl = A.site_link;
    double pt[3];
    mulmv(R, A.tcp_p, pt);
    const int src = tbase + (sl >= 0 ? sl : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] = lane_get(pt[k] + p[k], src);
    const double rr[3] = {pt[0] - anchor[0], pt[1] - anchor[1], pt[2] - anchor[2]};
    double lin[3], ang[3];
    cross3(ax, rr, lin);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lin[k] = is_slide ? ax[k] : lin[k];
      ang[k] = is_slide ? 0.0 : ax[k];
    }
    const bool above = sl >= 0 && ((anc_mask<T>(sl) >> tl) & 1u);  // (joints off the site's chain -- the fingers -- do not move it)
    const double* Rb = A.base_R;
    if (mine) {
      double* Jo = o.jac + (size_t)e * 6 * NL + t;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double vl = Rb[k] * lin[0] + Rb[3 + k] * lin[1] + Rb[6 + k] * lin[2];
        const double va = Rb[k] * ang[0] + Rb[3 + k] * ang[1] + Rb[6 + k] * ang[2];
        Jo[(size_t)k * NL] = above ? vl : 0.0;
        Jo[(size_t)(3 + k) * NL] = above ? va : 0.0;
      }
    }
  }
}

#endif  // __HIP__

}  // namespace rcsh
