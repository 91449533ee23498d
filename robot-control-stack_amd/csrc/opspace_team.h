// opspace_team.h -- operational-space dynamics of the TCP (rcsh_opspace_query / rcsh_env_opspace).
//
// k_dynamics_query (dynamics_team.h) returns qM, qfrc_bias and the TCP's Jacobian; a task-space controller then forms, per row and on
// the host, the operational-space inertia, the dynamically consistent inverse and the null-space projector.  This kernel forms them
// on the device, for M rows at once, together with the one quantity the queries did not carry at all, the TCP's velocity-product
// acceleration.  With J the TCP's Jacobian [6][nl] in the robot-base frame, the rows not selected by task_mask zeroed, Minv the full
// chain's M^-1 (finger slides included), b = qfrc_bias and A = J Minv J^T + damping I_sel:
//   twist       J qvel                                    jdot_qvel   the TCP's acceleration at qacc = 0 (classical; no gravity)
//   lambda_inv  A                                         lambda      A^-1 on the selected rows and columns
//   jbar        Minv J^T lambda                           op_bias     jbar^T b - lambda jdot_qvel
//   null_proj   I - J^T jbar^T                            qfrc        J^T (lambda xacc_des + op_bias) + null_proj qfrc_null
//   status      1 where A is not positive definite to working precision (ops_factor6), and then the five outputs of the right-hand
//               column and lambda are NaN.
//
// Same layout as k_dynamics_query: one row per TEAM of 16 lanes (team.h), lane t owning link / joint t, four rows per wavefront.  The
// frame, velocity and inertia phases, the mass-matrix rows and the Jacobian column are restated from it, not shared -- dynamics_team.h
// keeps its text --; the scans, the spatial products and M's LDL^T are the shared helpers.  The site link's lane turns the scans'
// spatial velocity (omega; v_O) and velocity-product acceleration (alpha; a_O), both about the WORLD origin, into the motion of the
// TCP point p:  v_p = v_O + omega x p,  a_p = a_O + alpha x p + omega x v_p  (the classical acceleration d^2 p / dt^2), and rotates
// them into the base frame.  No finite difference anywhere.  The factor of M is parked in the team's LDS block (as
// k_dynamics_derivatives does); lane k < 6 solves M y_k = J^T e_k, so that Y = Minv J^T stands in the block, and forms column k of
// A = J Y.  Every lane then factors the same 6 x 6 (an unselected row takes a unit diagonal: its off-diagonals are exact zeros, so
// the selected rows see the arithmetic of the restricted matrix), lane k solves for the k-th unit vector, lane i forms row i of
// jbar = Y lambda and of the projector.
//
// Every output is computed by the same instructions whichever others are asked for; a phase whose results nobody reads is skipped as
// a whole (M and its factor when only twist / jdot_qvel are wanted, the 6 x 6 factor when lambda_inv is the last one wanted, the
// inverse when status is, the assembly of qfrc otherwise).  Outputs pass through the block and leave it with consecutive lanes on
// consecutive entries.  Armature is part of M; no actuator, damping, gravity-compensation, limit, equality, friction or contact term
// enters.
//
// Order.  The TCP phase stands BEHIND the scheduling fence that k_dynamics_query keeps between the scans and the matrix phases, the
// link's frame and velocities staying in registers across the inertia scans: placed between the velocity and the inertia scans -- where
// a twist-only call could leave earliest -- the Topo<7, true> instance crashes the register allocator of the ROCm 7.2 compiler under
// the iterative-ilp strategy, fence or no fence.
#pragma once
#include "query_team.h"

namespace rcsh {

constexpr int kTaskRows = 6;

struct OpsOut {
  double* twist;       // [m][6]
  double* jdot_qvel;   // [m][6]
  double* lambda_inv;  // [m][6][6]
  double* lambda;      // [m][6][6]
  double* jbar;        // [m][nl][6]
  double* op_bias;     // [m][6]
  double* null_proj;   // [m][nl][nl]
  double* qfrc;        // [m][nl]
  int32_t* status;     // [m]
};

struct OpsArgs {
  const LinkRec* links;  // the model's link records (behind the DevModel)
  int32_t m;
  int32_t site_link;     // link carrying the attachment site (-1: static -- the Jacobian is zero)
  uint32_t task_mask;    // bit r: row r of the Jacobian is part of the task
  double damping;        // added to A's selected diagonal
  double rel_pivot;      // the status rule's bound on d_i / A_ii (RCSH_OPSPACE_REL_PIVOT)
  double gravity[3];
  double tcp_p[3];       // the TCP point in the site link's frame
  double base_R[9];      // world <- robot base
  const double *q, *qvel;          // [m][nl]; qvel null: zero
  const double* xacc_des;          // [m][6]; only where qfrc is asked for
  const double* qfrc_null;         // [m][nl]; null: zero
  OpsOut o;
  const double* S;       // env form: the state, [field][n] with n = m (null: the caller's rows)
  int32_t qpos_field, qvel_field;
};

#if defined(__HIP__)

// LDS block of one team.  Matrices on their way out lie in the layout of the output row.
template <class T>
struct OpsLds {
  static constexpr int NL = T::NL, NLP = even_up(T::NL);
  double S[NL][6];              // motion axes
  double M[NL][NLP];            // mass-matrix rows (lower triangle valid)
  double H[even_up(T::NTRI)];   // the packed LDL^T factor of M: the same on every lane, kept once
  double Jt[NL][kTaskRows];     // J^T, masked rows zero
  double Y[NL][kTaskRows];      // Minv J^T
  double A[kTaskRows * kTaskRows];
  double Lm[kTaskRows * kTaskRows];
  double Jb[NL * kTaskRows];
  double N[even_up(NL * NL)];
  double b[NLP], tau0[NLP], tau[NLP];
  double tw[kTaskRows], jd[kTaskRows], xa[kTaskRows], ob[kTaskRows], F[kTaskRows];
};

// Packed LDL^T of the task-space matrix, in place as ldl_factor leaves it (strict lower part <- L, diagonal <- 1/D), without pivoting.
// Returns true where the matrix is not positive definite to working precision: on a selected row A_ii <= 0, or a pivot
// d_i <= rel_pivot * A_ii, or d_i not finite.
RCSH_D bool ops_factor6(double* A, uint32_t mask, double rel_pivot) {
  constexpr int N = kTaskRows;
  bool bad = false;
  double D[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double w[N];
    const double ajj = A[tri(j, j)];
    double d = ajj;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      w[k] = A[tri(j, k)] * D[k];
      d -= A[tri(j, k)] * w[k];
    }
    const bool fine = (ajj > 0.0) & (d > rel_pivot * ajj) & (d < __builtin_huge_val());
    bad |= (bool)((mask >> j) & 1u) & !fine;
    D[j] = d;
    const double inv = fast_rcp(d);
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = A[tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= A[tri(i, k)] * w[k];
      A[tri(i, j)] = s * inv;
    }
    A[tri(j, j)] = inv;
  }
  return bad;
}

// n entries of the team's block out to the row's place, consecutive lanes writing consecutive entries (nan: a status-1 row)
RCSH_D void ops_flush(const double* src, double* dst, int n, int t, bool live, bool nan) {
  team_sync();
  if (live) {
    for (int idx = t; idx < n; idx += kTeamLanes) dst[idx] = nan ? __builtin_nan("") : src[idx];
  }
}

// (two wavefronts per SIMD, as k_dynamics_derivatives: 256 registers a lane, no scratch)
template <class T>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) k_opspace_query(OpsArgs A) {
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM, NR = kTaskRows;
  static_assert(!T::GRIP || NA + 1 < 8 || NA == 7, "the chain rounds of the scans reach 8 lanes; NARM = 7 uses the bank masks");
  __shared__ OpsLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int tbase = threadIdx.x & 48;
  OpsLds<T>& B = lds[team];
  const int e = blockIdx.x * kTeams + team;
  const bool live = e < A.m;
  const bool valid = t < NL;
  const bool mine = live && valid;
  const int tl = valid ? t : NL - 1;
  const bool task = t < NR;        // the lane owns a task row / column
  const int tr = task ? t : NR - 1;
  const LinkRec* links = A.links;
  const LinkRec& lk = links[tl];
  const OpsOut& o = A.o;
  const uint32_t mask = A.task_mask;
  const bool want_inv = o.lambda || o.jbar || o.op_bias || o.null_proj || o.qfrc;
  const bool want_factor = want_inv || o.status;
  const bool want_A = want_factor || o.lambda_inv;
  const size_t row = (size_t)(live ? e : 0);
  // ---- the row: the caller's, or the environment's own chain (dead teams and lanes off the chain compute on zeros and store nothing)
  double q, qd = 0.0;
  const size_t at = row * NL + tl;
  if (A.S) {
    double fq[7];
    query_env_row(A.S, A.m, e, live, valid, A.qpos_field, -1, q, fq);
    qd = mine ? A.S[(size_t)(A.qvel_field + t) * A.m + e] : 0.0;
  } else {
    q = mine ? A.q[at] : 0.0;
    if (A.qvel) qd = mine ? A.qvel[at] : 0.0;
  }
  if (o.qfrc) {
    const double xa = live && task ? A.xacc_des[row * NR + tr] : 0.0;
    const double t0 = mine && A.qfrc_null ? A.qfrc_null[at] : 0.0;
    if (task) B.xa[tr] = xa;
    if (valid) B.tau0[tl] = t0;
  }
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
    double Ii[10];
    Ii[0] = Tm[0] * R[0] + Tm[1] * R[1] + Tm[2] * R[2] + ms * (c[1] * c[1] + c[2] * c[2]);
    Ii[1] = Tm[3] * R[3] + Tm[4] * R[4] + Tm[5] * R[5] + ms * (c[0] * c[0] + c[2] * c[2]);
    Ii[2] = Tm[6] * R[6] + Tm[7] * R[7] + Tm[8] * R[8] + ms * (c[0] * c[0] + c[1] * c[1]);
    Ii[3] = Tm[0] * R[3] + Tm[1] * R[4] + Tm[2] * R[5] - ms * c[0] * c[1];
    Ii[4] = Tm[0] * R[6] + Tm[1] * R[7] + Tm[2] * R[8] - ms * c[0] * c[2];
    Ii[5] = Tm[3] * R[6] + Tm[4] * R[7] + Tm[5] * R[8] - ms * c[1] * c[2];
    Ii[6] = ms * c[0]; Ii[7] = ms * c[1]; Ii[8] = ms * c[2];
    Ii[9] = ms;
    double Ia[6], Iv[6], vf[6];
    const double accg[6] = {acc[0], acc[1], acc[2], acc[3] - A.gravity[0], acc[4] - A.gravity[1], acc[5] - A.gravity[2]};
    inert_mul(Ii, accg, Ia);
    inert_mul(Ii, vel, Iv);
    cross_force(vel, Iv, vf);
    const bool ff = T::GRIP && t == NA;
#pragma unroll
    for (int k = 0; k < 10; ++k) Ic[k] = scan_from_leaves<T>(Ii[k], ff);
#pragma unroll
    for (int k = 0; k < 6; ++k) Fb[k] = scan_from_leaves<T>(Ia[k] + vf[k], ff);
  }

  // (a scheduling fence between the scans and the matrix phases, as in k_dynamics_query: scheduled as one region under the
  // iterative-ilp strategy the Topo<7, true> instance crashes the register allocator of the ROCm 7.2 compiler)
  sched_fence();
  team_sync();  // every lane's S is in the block

  // ---- the TCP: its point in the world, its Jacobian column (lane j, joint j), its twist and velocity-product acceleration (the
  // site link's lane).  The TCP rides on the site's link: per radian of a hinge above it the point moves by axis x (point - anchor)
  // and the frame turns about the axis; per metre of a slide it moves by the axis
  const int sl = A.site_link;
  const double* Rb = A.base_R;
  double jt[NR];
  {
    double own[3], pt[3];
    mulmv(R, A.tcp_p, own);
    own[0] += p[0]; own[1] += p[1]; own[2] += p[2];
    const int src = tbase + (sl >= 0 ? sl : 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] = lane_get(own[k], src);
    const double rr[3] = {pt[0] - anchor[0], pt[1] - anchor[1], pt[2] - anchor[2]};
    double lin[3], ang[3];
    cross3(ax, rr, lin);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      lin[k] = is_slide ? ax[k] : lin[k];
      ang[k] = is_slide ? 0.0 : ax[k];
    }
    const bool above = sl >= 0 && ((anc_mask<T>(sl) >> tl) & 1u);  // (joints off the site's chain -- the fingers -- do not move it)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double vl = Rb[k] * lin[0] + Rb[3 + k] * lin[1] + Rb[6 + k] * lin[2];
      const double va = Rb[k] * ang[0] + Rb[3 + k] * ang[1] + Rb[6 + k] * ang[2];
      jt[k] = (above & (bool)((mask >> k) & 1u)) ? vl : 0.0;
      jt[3 + k] = (above & (bool)((mask >> (3 + k)) & 1u)) ? va : 0.0;
    }
    if (valid) {
#pragma unroll
      for (int k = 0; k < NR; ++k) B.Jt[tl][k] = jt[k];
    }
    // on the site link's lane `own` is the TCP point and vel / acc are its link's: (omega; v_O) and (alpha; a_O) about the world origin
    double wp[3], vp[3], ap[3], wv[3];
    cross3(vel, own, wp);
#pragma unroll
    for (int k = 0; k < 3; ++k) vp[k] = vel[3 + k] + wp[k];
    cross3(acc, own, ap);
    cross3(vel, vp, wv);
#pragma unroll
    for (int k = 0; k < 3; ++k) ap[k] += acc[3 + k] + wv[k];
    if (sl < 0 ? t == 0 : t == sl) {
      const double on = sl < 0 ? 0.0 : 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ml = (mask >> k) & 1u ? on : 0.0, ma = (mask >> (3 + k)) & 1u ? on : 0.0;
        B.tw[k] = ml * (Rb[k] * vp[0] + Rb[3 + k] * vp[1] + Rb[6 + k] * vp[2]);
        B.tw[3 + k] = ma * (Rb[k] * vel[0] + Rb[3 + k] * vel[1] + Rb[6 + k] * vel[2]);
        B.jd[k] = ml * (Rb[k] * ap[0] + Rb[3 + k] * ap[1] + Rb[6 + k] * ap[2]);
        B.jd[3 + k] = ma * (Rb[k] * acc[0] + Rb[3 + k] * acc[1] + Rb[6 + k] * acc[2]);
      }
    }
  }
  if (o.twist) ops_flush(B.tw, o.twist + row * NR, NR, t, live, false);
  if (o.jdot_qvel) ops_flush(B.jd, o.jdot_qvel + row * NR, NR, t, live, false);
  if (!want_A) return;

  // ---- mass-matrix row of the link: M[t][j] = S_j . (Ic_t S_t) for the ancestors j (and itself), armature on the diagonal; the bias
  // force; every lane factors the same matrix, lane 0 parks the factor in the block
  {
    double G[6];
    inert_mul(Ic, S, G);
    double mrow[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      double Sj[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) Sj[k] = B.S[j][k];
      mrow[j] = dot6(Sj, G);
    }
    if (T::GRIP) mrow[NA] = t == NA + 1 ? 0.0 : mrow[NA];  // the fingers are siblings
#pragma unroll
    for (int j = 0; j < NL; ++j) mrow[j] += j == tl ? armature : 0.0;
    const double bias = dot6(S, Fb);
    if (valid) {
#pragma unroll
      for (int j = 0; j < NL; ++j) B.M[tl][j] = mrow[j];  // (entries right of the diagonal: not ancestors, never read)
      B.b[tl] = bias;
    }
    team_sync();
    double H[T::NTRI];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) H[tri(i, j)] = B.M[i][j];
    }
    ldl_factor<NL>(H);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < T::NTRI; ++k) B.H[k] = H[k];
    }
    team_sync();
  }

  // ---- Y = Minv J^T (lane k < 6 solves for column k) and column k of A = J Y + damping I_sel
  {
    double y[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) y[i] = B.Jt[i][tr];
    ldl_solve<NL>(B.H, y);
    if (task) {
#pragma unroll
      for (int i = 0; i < NL; ++i) B.Y[i][tr] = y[i];
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < NL; ++i) s += B.Jt[i][r] * y[i];
      s += ((r == tr) & (bool)((mask >> r) & 1u)) ? A.damping : 0.0;
      if (task) B.A[r * NR + tr] = s;
    }
  }
  if (o.lambda_inv) ops_flush(B.A, o.lambda_inv + row * NR * NR, NR * NR, t, live, false);
  if (!want_factor) return;
  team_sync();

  // ---- the 6 x 6 factor, by every lane; the status
  double H6[NR * (NR + 1) / 2];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) H6[tri(i, j)] = B.A[i * NR + j];
    H6[tri(i, i)] = (mask >> i) & 1u ? H6[tri(i, i)] : 1.0;
  }
  const bool bad = ops_factor6(H6, mask, A.rel_pivot);
  if (o.status && live && t == 0) o.status[row] = bad ? 1 : 0;
  if (!want_inv) return;

  // ---- lambda: lane k solves for the k-th unit vector
  {
    double x[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) x[i] = i == tr ? 1.0 : 0.0;
    ldl_solve<NR>(H6, x);
    const bool col = (mask >> tr) & 1u;
    if (task) {
#pragma unroll
      for (int i = 0; i < NR; ++i) B.Lm[i * NR + tr] = (col & (bool)((mask >> i) & 1u)) ? x[i] : 0.0;
    }
  }
  if (o.lambda) ops_flush(B.Lm, o.lambda + row * NR * NR, NR * NR, t, live, bad);
  team_sync();

  // ---- jbar = Y lambda: lane i, row i
  {
    double yr[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) yr[r] = B.Y[tl][r];
#pragma unroll
    for (int c = 0; c < NR; ++c) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) s += yr[r] * B.Lm[r * NR + c];
      if (valid) B.Jb[tl * NR + c] = s;
    }
  }
  if (o.jbar) ops_flush(B.Jb, o.jbar + row * NL * NR, NL * NR, t, live, bad);
  team_sync();

  // ---- op_bias = jbar^T b - lambda jdot_qvel: lane r, entry r
  double ob = 0.0;
  if (o.op_bias || o.qfrc) {
#pragma unroll
    for (int i = 0; i < NL; ++i) ob += B.Jb[i * NR + tr] * B.b[i];
#pragma unroll
    for (int c = 0; c < NR; ++c) ob -= B.Lm[tr * NR + c] * B.jd[c];
    if (o.op_bias) {
      if (task) B.ob[tr] = ob;
      ops_flush(B.ob, o.op_bias + row * NR, NR, t, live, bad);
    }
  }

  // ---- null_proj = I - J^T jbar^T: lane i, row i
  if (o.null_proj || o.qfrc) {
    double nrow[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      double s = j == tl ? 1.0 : 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) s -= jt[r] * B.Jb[j * NR + r];
      nrow[j] = s;
    }
    if (o.null_proj) {
      if (valid) {
#pragma unroll
        for (int j = 0; j < NL; ++j) B.N[tl * NL + j] = nrow[j];
      }
      ops_flush(B.N, o.null_proj + row * NL * NL, NL * NL, t, live, bad);
    }
    // ---- qfrc = J^T (lambda xacc_des + op_bias) + null_proj qfrc_null
    if (o.qfrc) {
      double f = ob;
#pragma unroll
      for (int c = 0; c < NR; ++c) f += B.Lm[tr * NR + c] * B.xa[c];
      if (task) B.F[tr] = f;
      team_sync();
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < NR; ++r) s += jt[r] * B.F[r];
#pragma unroll
      for (int j = 0; j < NL; ++j) s += nrow[j] * B.tau0[j];
      if (valid) B.tau[tl] = s;
      ops_flush(B.tau, o.qfrc + row * NL, NL, t, live, bad);
    }
  }
}

#endif  // __HIP__

}  // namespace rcsh
