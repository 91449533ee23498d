// dynamics_grad_team.h -- analytic derivatives of the dynamics queries (rcsh_dynamics_derivatives / rcsh_env_dynamics_derivatives).
//
// k_dynamics_query (dynamics_team.h) returns qfrc_inverse = M(q) qacc_in + qfrc_bias(q, qvel) and qacc = M^-1 (qfrc_in - qfrc_bias)
// for M rows at once; this kernel returns how the two change with the state:
//   dqfrc_inverse_dq, dqfrc_inverse_dqvel   the Jacobians of the inverse dynamics,
//   dqacc_dq, dqacc_dqvel, qM_inv           those of the forward dynamics (qM_inv = dqacc / dqfrc_in),
// each [m][nl][nl] row-major, element [i][k] the derivative of component i by variable k.
//
// Same layout as k_dynamics_query: one row per TEAM of 16 lanes (team.h), lane t owning link / joint t, four rows per wavefront.  The
// frame, velocity and inertia phases are restated from it, not shared -- dynamics_team.h keeps its text --; the scans, the spatial
// products and the LDL^T are the shared helpers.  Everything is held in Pluecker coordinates about the WORLD origin, where a link's
// quantities change with a joint k above it by the motion of that joint alone:
//   dS_i / dq_k = S_k xm S_i              for k a strict ancestor of i (the axis of a joint does not move with the joint itself),
//   dI_i / dq_k = S_k x* I_i - I_i S_k xm  for k an ancestor of i or i itself (the link does move with its own joint),
// both zero otherwise; slides (S = (0; axis)) follow the same rule.  Per column k the recursive Newton-Euler pass is differentiated
// term by term: the tangents of the velocity and of the acceleration run root-to-leaf (scan_from_root), the tangent of
// I a + v x* I v is summed leaf-to-root (scan_from_leaves), and lane t takes S_t . dF_t + dS_t . F_t.  The velocity columns are the
// same recursion seeded with S_k.  dID/dq is evaluated at qacc_in for the inverse dynamics and at the solved qacc for the forward
// dynamics: the same function, called twice.  The forward derivatives are -M^-1 times those matrices: the matrix passes through the
// team's LDS block and lane k solves column k with the team's factor (computed by every lane, kept once in the block).  No finite
// difference anywhere.
//
// Every output is computed by the same instructions whichever others are asked for; a phase whose results nobody reads is skipped as
// a whole.  Armature is part of M; no actuator, damping, gravity-compensation, limit, equality, friction or contact term enters.
#pragma once
#include "query_team.h"

namespace rcsh {

struct DynGradOut {
  double* dqfrc_inverse_dq;     // [m][nl][nl]
  double* dqfrc_inverse_dqvel;  // [m][nl][nl]
  double* dqacc_dq;             // [m][nl][nl]
  double* dqacc_dqvel;          // [m][nl][nl]
  double* qM_inv;               // [m][nl][nl]
};

struct DynGradArgs {
  const LinkRec* links;  // the model's link records (behind the DevModel)
  int32_t m;
  double gravity[3];
  const double *q, *qvel, *qacc_in, *qfrc_in;  // [m][nl]; qvel null: zero; qacc_in / qfrc_in only where dqfrc_inverse_dq / dqacc_dq are asked for
  DynGradOut o;
  const double* S;       // env form: the state, [field][n] with n = m (null: the caller's rows)
  int32_t qpos_field, qvel_field;
};

#if defined(__HIP__)

// LDS block of one team: the motion axes, the mass-matrix rows (lower triangle valid), the forward dynamics' right-hand side, the
// matrix on its way out (row i written by lane i, column k solved by lane k, the whole flushed by the team) and the factor of M
template <class T>
struct DynGradLds {
  static constexpr int NLP = even_up(T::NL);
  double S[T::NL][6];
  double M[T::NL][NLP];
  double r[NLP];
  double X[T::NL][NLP];
  double H[even_up(T::NTRI)];  // the packed LDL^T factor of M (ldl_factor's layout): the same on every lane, so it is kept once
};

// what a lane holds of its link after the restated phases
struct GradLink {
  double S[6];    // motion axis about the world origin
  double vel[6];  // spatial velocity
  double avp[6];  // velocity-product acceleration, gravity included (the link's acceleration at qacc = 0)
  double Ii[10];  // spatial inertia about the world origin (zero on lanes off the chain)
  double qd;
  double chain, second;  // scan_from_root's masks
  uint32_t anc;          // bit j: joint j is an ancestor-or-self joint of the link
  int tl;                // the lane's link (lanes off the chain: the last one, computing on zero inertia and storing nothing)
  bool valid;            // the lane is on the chain
  bool ff;               // scan_from_leaves: the first finger
};

// d(I x)/dq_k at fixed x for a joint k that moves the link: S_k x* (I x) - I (S_k xm x)
RCSH_D void inert_tangent_mul(const double* Ii, const double* Sk, const double* x, double* r) {
  double Ix[6], sx[6], Isx[6];
  inert_mul(Ii, x, Ix);
  cross_force(Sk, Ix, r);
  cross_motion(Sk, x, sx);
  inert_mul(Ii, sx, Isx);
#pragma unroll
  for (int k = 0; k < 6; ++k) r[k] -= Isx[k];
}

// d(M qdd + qfrc_bias)/dq: row tl of the matrix into B.X, one column per round.  qdd: the lane's own joint acceleration.
template <class T>
RCSH_D void grad_q_columns(DynGradLds<T>& B, const GradLink& L, double qdd) {
  constexpr int NL = T::NL;
  // the link's acceleration and the subtree's wrench at this qdd
  double acc[6], F[6], Iv[6];
  inert_mul(L.Ii, L.vel, Iv);
  {
#pragma unroll
    for (int c = 0; c < 6; ++c) acc[c] = L.avp[c] + scan_from_root<T>(L.S[c] * qdd, L.chain, L.second);
    double Ia[6], vf[6];
    inert_mul(L.Ii, acc, Ia);
    cross_force(L.vel, Iv, vf);
#pragma unroll
    for (int c = 0; c < 6; ++c) F[c] = scan_from_leaves<T>(Ia[c] + vf[c], L.ff);
  }
#pragma unroll 1
  for (int k = 0; k < NL; ++k) {
    double Sk[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) Sk[c] = B.S[k][c];
    const bool moves = (L.anc >> k) & 1u;   // joint k moves the link
    const bool turns = moves && k != L.tl;  // ... and the link's own joint axis
    double dS[6];
    cross_motion(Sk, L.S, dS);
#pragma unroll
    for (int c = 0; c < 6; ++c) dS[c] = turns ? dS[c] : 0.0;
    double dv[6], da[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) dv[c] = scan_from_root<T>(dS[c] * L.qd, L.chain, L.second);
    {
      double a[6], b[6];
      cross_motion(dv, L.S, a);
      cross_motion(L.vel, dS, b);
#pragma unroll
      for (int c = 0; c < 6; ++c) da[c] = scan_from_root<T>(dS[c] * qdd + (a[c] + b[c]) * L.qd, L.chain, L.second);
    }
    // tangent of I a + v x* I v
    double df[6];
    {
      double dIa[6], dIv[6], Ida[6], Idv[6], w[6], u[6];
      inert_tangent_mul(L.Ii, Sk, acc, dIa);
      inert_tangent_mul(L.Ii, Sk, L.vel, dIv);
      inert_mul(L.Ii, da, Ida);
      inert_mul(L.Ii, dv, Idv);
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        dIa[c] = moves ? dIa[c] : 0.0;
        dIv[c] = (moves ? dIv[c] : 0.0) + Idv[c];
      }
      cross_force(dv, Iv, w);
      cross_force(L.vel, dIv, u);
#pragma unroll
      for (int c = 0; c < 6; ++c) df[c] = dIa[c] + Ida[c] + w[c] + u[c];
    }
    double dF[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) dF[c] = scan_from_leaves<T>(df[c], L.ff);
    const double d = dot6(L.S, dF) + dot6(dS, F);
    if (L.valid) B.X[L.tl][k] = d;
  }
}

// d qfrc_bias / d qvel: row tl of the matrix into B.X
template <class T>
RCSH_D void grad_v_columns(DynGradLds<T>& B, const GradLink& L) {
  constexpr int NL = T::NL;
  double Iv[6], sd[6];
  inert_mul(L.Ii, L.vel, Iv);
  cross_motion(L.vel, L.S, sd);
#pragma unroll 1
  for (int k = 0; k < NL; ++k) {
    double dv[6];
    const bool moves = (L.anc >> k) & 1u;
#pragma unroll
    for (int c = 0; c < 6; ++c) dv[c] = moves ? B.S[k][c] : 0.0;
    double da[6];
    {
      double a[6];
      cross_motion(dv, L.S, a);  // (k the link's own joint: S x S = 0)
      const double own = k == L.tl ? 1.0 : 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) da[c] = scan_from_root<T>(a[c] * L.qd + own * sd[c], L.chain, L.second);
    }
    double df[6];
    {
      double Ida[6], Idv[6], w[6], u[6];
      inert_mul(L.Ii, da, Ida);
      inert_mul(L.Ii, dv, Idv);
      cross_force(dv, Iv, w);
      cross_force(L.vel, Idv, u);
#pragma unroll
      for (int c = 0; c < 6; ++c) df[c] = Ida[c] + w[c] + u[c];
    }
    double dF[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) dF[c] = scan_from_leaves<T>(df[c], L.ff);
    const double d = dot6(L.S, dF);
    if (L.valid) B.X[L.tl][k] = d;
  }
}

// the team's matrix block out to the row's [nl][nl], consecutive lanes writing consecutive entries
template <class T>
RCSH_D void grad_flush(const DynGradLds<T>& B, double* out, size_t e, int t, bool live) {
  constexpr int NL = T::NL;
  team_sync();
  if (live) {
    double* dst = out + e * NL * NL;
    for (int idx = t; idx < NL * NL; idx += kTeamLanes) dst[idx] = B.X[idx / NL][idx % NL];
  }
  team_sync();
}

// column tl of the block <- -M^-1 column (lane k solves column k; lanes off the chain solve the last one again and store nothing)
template <class T>
RCSH_D void grad_solve_columns(DynGradLds<T>& B, const double* H, int tl, bool valid) {
  constexpr int NL = T::NL;
  team_sync();
  double x[NL];
#pragma unroll
  for (int i = 0; i < NL; ++i) x[i] = B.X[i][tl];
  ldl_solve<NL>(H, x);
  if (valid) {
#pragma unroll
    for (int i = 0; i < NL; ++i) B.X[i][tl] = -x[i];
  }
}

// (two wavefronts per SIMD: 256 registers a lane, which every instance fits without scratch; left to itself Topo<7, true> takes 258)
template <class T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) k_dynamics_derivatives(DynGradArgs A) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM;
  static_assert(!T::GRIP || NA + 1 < 8 || NA == 7, "the chain rounds of the scans reach 8 lanes; NARM = 7 uses the bank masks");
  __shared__ DynGradLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  DynGradLds<T>& B = lds[team];
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < A.m;
  const bool valid = t < NL;
  const bool mine = live && valid;
  const int tl = valid ? t : NL - 1;
  const LinkRec* links = A.links;
  const LinkRec& lk = links[tl];
  const DynGradOut& o = A.o;
  const bool want_solve = o.dqacc_dq || o.dqacc_dqvel || o.qM_inv;
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
  if (o.dqfrc_inverse_dq) qa = mine ? A.qacc_in[at] : 0.0;
  if (o.dqacc_dq) qf = mine ? A.qfrc_in[at] : 0.0;
  KinK kk;
  kk.load(lk);
  InertK ik;
  ik.load(lk);
  const double armature = lk.armature;
  const bool is_slide = kk.jtype == kSlide;

  // ---- world frame of the link
  double R[9], p[3];
  link_local_frame(kk, q, R, p);
  scan_frames<T>(R, p);

  // ---- motion axis about the world origin, velocity and velocity-product acceleration of the link
  GradLink L;
  L.qd = qd;
  L.tl = tl;
  L.valid = valid;
  L.anc = anc_mask<T>(tl);
  L.chain = t <= NA ? 1.0 : 0.0;
  L.second = t == NA + 1 ? 1.0 : 0.0;  // (only read by archetypes with a gripper)
  L.ff = T::GRIP && t == NA;
  {
    double ax[3], anchor[3], mom[3];
    mulmv(R, kk.axis, ax);
    mulmv(R, kk.jpos, anchor);
    anchor[0] += p[0]; anchor[1] += p[1]; anchor[2] += p[2];
    cross3(anchor, ax, mom);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      L.S[k] = is_slide ? 0.0 : ax[k];
      L.S[3 + k] = is_slide ? ax[k] : mom[k];
    }
  }
  if (valid) {
#pragma unroll
    for (int k = 0; k < 6; ++k) B.S[tl][k] = L.S[k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) L.vel[k] = scan_from_root<T>(L.S[k] * qd, L.chain, L.second);
  {
    double sd[6];
    cross_motion(L.vel, L.S, sd);  // S x S = 0: the link's own joint velocity does not contribute
#pragma unroll
    for (int k = 0; k < 6; ++k) L.avp[k] = scan_from_root<T>(sd[k] * qd, L.chain, L.second);
    L.avp[3] -= A.gravity[0]; L.avp[4] -= A.gravity[1]; L.avp[5] -= A.gravity[2];
  }

  // ---- spatial inertia about the world origin, composite inertia, the subtree's bias wrench
  double Ic[10], Fb[6];
  {
    const double ms = valid ? ik.mass : 0.0;
    double c[3];
    mulmv(R, ik.com, c);
    c[0] += p[0]; c[1] += p[1]; c[2] += p[2];
    const double* J = ik.J;
    const double vz = valid ? 1.0 : 0.0;
    const double Jm[9] = {vz * J[0], vz * J[3], vz * J[4], vz * J[3], vz * J[1], vz * J[5], vz * J[4], vz * J[5], vz * J[2]};
    double Tm[9];
    mulmm(R, Jm, Tm);
    double* Ii = L.Ii;
    Ii[0] = Tm[0] * R[0] + Tm[1] * R[1] + Tm[2] * R[2] + ms * (c[1] * c[1] + c[2] * c[2]);
    Ii[1] = Tm[3] * R[3] + Tm[4] * R[4] + Tm[5] * R[5] + ms * (c[0] * c[0] + c[2] * c[2]);
    Ii[2] = Tm[6] * R[6] + Tm[7] * R[7] + Tm[8] * R[8] + ms * (c[0] * c[0] + c[1] * c[1]);
    Ii[3] = Tm[0] * R[3] + Tm[1] * R[4] + Tm[2] * R[5] - ms * c[0] * c[1];
    Ii[4] = Tm[0] * R[6] + Tm[1] * R[7] + Tm[2] * R[8] - ms * c[0] * c[2];
    Ii[5] = Tm[3] * R[6] + Tm[4] * R[7] + Tm[5] * R[8] - ms * c[1] * c[2];
    Ii[6] = ms * c[0]; Ii[7] = ms * c[1]; Ii[8] = ms * c[2];
    Ii[9] = ms;
    if (want_solve) {
      double Ia[6], Iv[6], vf[6];
      inert_mul(Ii, L.avp, Ia);
      inert_mul(Ii, L.vel, Iv);
      cross_force(L.vel, Iv, vf);
#pragma unroll
      for (int k = 0; k < 10; ++k) Ic[k] = scan_from_leaves<T>(Ii[k], L.ff);
#pragma unroll
      for (int k = 0; k < 6; ++k) Fb[k] = scan_from_leaves<T>(Ia[k] + vf[k], L.ff);
    }
  }

  // (a scheduling fence between the scans and the matrix phases, as in k_dynamics_query: scheduled as one region under the
  // iterative-ilp strategy the Topo<7, true> instance crashes the register allocator of the ROCm 7.2 compiler)
  sched_fence();
  team_sync();  // every lane's S is in the block

  // ---- the forward dynamics' matrix and right-hand side: M[t][j] = S_j . (Ic_t S_t) for the ancestors j (and itself), armature on
  // the diagonal; every lane factors the same matrix and solves for the same qacc
  double qacc = 0.0;
  if (want_solve) {
    double H[T::NTRI];
    double G[6];
    inert_mul(Ic, L.S, G);
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
    const double bias = dot6(L.S, Fb);
    if (valid) {
#pragma unroll
      for (int j = 0; j < NL; ++j) B.M[tl][j] = row[j];  // (entries right of the diagonal: not ancestors, never read)
      B.r[tl] = qf - bias;
    }
    team_sync();
#pragma unroll
    for (int i = 0; i < NL; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) H[tri(i, j)] = B.M[i][j];
    }
    ldl_factor<NL>(H);
    // the factor is the same on every lane: parked in the block (lane 0 writes it), so that it does not occupy 2 NTRI registers of
    // every lane through the column loops; the solves read it back with constant offsets
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < T::NTRI; ++k) B.H[k] = H[k];
    }
    team_sync();
    if (o.dqacc_dq) {
      double x[NL];
#pragma unroll
      for (int i = 0; i < NL; ++i) x[i] = B.r[i];
      ldl_solve<NL>(B.H, x);
#pragma unroll
      for (int i = 0; i < NL; ++i) qacc = i == tl ? x[i] : qacc;
    }
  }

  // ---- inverse dynamics by q, at qacc_in
  if (o.dqfrc_inverse_dq) {
    grad_q_columns<T>(B, L, qa);
    grad_flush<T>(B, o.dqfrc_inverse_dq, (size_t)e, t, live);
  }
  // ---- bias forces by qvel, and the forward dynamics' -M^-1 times it
  if (o.dqfrc_inverse_dqvel || o.dqacc_dqvel) {
    grad_v_columns<T>(B, L);
    if (o.dqfrc_inverse_dqvel) grad_flush<T>(B, o.dqfrc_inverse_dqvel, (size_t)e, t, live);
    if (o.dqacc_dqvel) {
      grad_solve_columns<T>(B, B.H, tl, valid);
      grad_flush<T>(B, o.dqacc_dqvel, (size_t)e, t, live);
    }
  }
  // ---- forward dynamics by q: -M^-1 dID/dq at the solved qacc
  if (o.dqacc_dq) {
    grad_q_columns<T>(B, L, qacc);
    grad_solve_columns<T>(B, B.H, tl, valid);
    grad_flush<T>(B, o.dqacc_dq, (size_t)e, t, live);
  }
  // ---- M^-1: lane k solves for the k-th unit vector
  if (o.qM_inv) {
    double x[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) x[i] = i == tl ? 1.0 : 0.0;
    ldl_solve<NL>(B.H, x);
    if (valid) {
#pragma unroll
      for (int i = 0; i < NL; ++i) B.X[i][tl] = x[i];
    }
    grad_flush<T>(B, o.qM_inv, (size_t)e, t, live);
  }
}

#endif  // __HIP__

}  // namespace rcsh
