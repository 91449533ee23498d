// torque_team.h -- torque control at substep rate (rcsh_sim_step_torque): k substeps of a torque-actuated scene, an operational-space /
// joint impedance law evaluated before each of them.
//
// The stepping kernels hold ctrl over a launch; a torque law held over the 17 substeps of an env-step is not the law.  This kernel
// steps like k_run_team without free box, contact phase and detection, and between the substeps forms, from the state the substep
// starts on (base frame, the TCP of the dynamics queries for the same tcp_offset7):
//   x_err     = [p_des - p ; rotvec(R_des R^T)]
//   xacc      = task_k * x_err - task_d * twist
//   qfrc_null = joint_k * (q_des - q) - joint_d * qvel  (+ qfrc_bias)       finger entries: 0 (+ qfrc_bias)
//   tau       = J^T (lambda xacc + op_bias) + null_proj qfrc_null - qfrc_gravcomp
//   ctrl[arm] = tau[arm]
// which team_substep then clamps and applies like any ctrl.  task_mask = 0: tau = qfrc_null - qfrc_gravcomp, no 6 x 6 at all.
//
// Same layout as the stepping and query kernels: one environment per TEAM of 16 lanes (team.h), lane t owning link / joint t, four
// environments per wavefront; the environment's state sits in a StageTeam block for the whole launch and goes back once, ctrl
// included (rcsh_sim_get_ctrl: the last torque applied).  A substep is two phases:
//  1. the law (torque_law): the frame, velocity and inertia phases, the mass-matrix rows, the Jacobian column and the 6 x 6 of
//     k_opspace_query, qfrc_bias and qfrc_gravcomp as k_dynamics_query forms them -- restated, not shared: those kernels keep their
//     text --, the scans, spatial products, LDL^T and ops_factor6 being the shared helpers; the rotation error as the quaternion
//     q_des conj(q) of pose.h's products, its logarithm taken on the shorter arc;
//  2. team_substep, with hooks that do nothing.
// team_substep recomputes the frames and the mass matrix the law has just formed: sharing them means editing team_substep.
// Where the opspace status would be 1 (ops_factor6 at RCSH_OPSPACE_REL_PIVOT) the substep leaves ctrl as it is -- the torque of the
// substep before -- and raises the environment's sticky `singular` byte; nothing of that substep's law reaches the state.  A torque
// that comes out non-finite (a NaN or zero-quaternion target written through the _dev form, which cannot validate) is treated the same.
// Not carried over from run_team_body: the leader's bookkeeping.  The plain callbacks (is_moving / is_arrived) and their timestamps do
// not run here -- they describe position servos --, so after step_torque those flags are what they were and `time` is ahead of `cb`.
#pragma once
#include "opspace_team.h"
#include "pose.h"
#include "sim_kernels.h"

namespace rcsh {

// the law as the device reads it: rcsh_torque_law with its TCP resolved into the site link's frame
struct TorqueLawDev {
  uint32_t task_mask;
  int32_t compensate_bias;
  double damping, rel_pivot;
  double tcp_p[3], tcp_R[9];    // the TCP in the site link's frame: point, link <- TCP rotation
  double base_p[3], base_R[9];  // world <- robot base
  double task_k[kTaskRows], task_d[kTaskRows], joint_k[kMaxArm], joint_d[kMaxArm];
};
static_assert(sizeof(TorqueLawDev) % 8 == 0, "copied in 8-byte words");

constexpr int kTorquePose = 7;  // targets, [kTorquePose + NARM][n]: the TCP's pose in the base frame (x y z qx qy qz qw), then q_des

struct TorqueArgs {
  const DevModel* model;
  double* S;
  int32_t n, k;              // environments, substeps
  int32_t keep_qpre, enabled;
  const double* target;
  uint8_t* singular;         // [n], sticky
  TorqueLawDev law;
};

#if defined(__HIP__)

// LDS block of one team's law phase (OpsLds without the outputs nobody reads here)
template <class T>
struct TorqueLds {
  static constexpr int NL = T::NL, NLP = even_up(T::NL);
  double S[NL][6];
  double M[NL][NLP];
  double H[even_up(T::NTRI)];
  double Jt[NL][kTaskRows];
  double Y[NL][kTaskRows];
  double A[kTaskRows * kTaskRows];
  double Lm[kTaskRows * kTaskRows];
  double Jb[NL * kTaskRows];
  double b[NLP], tau0[NLP];
  double jd[kTaskRows], xa[kTaskRows], F[kTaskRows];
  double pose[kTorquePose + 1];
};

// The TCP's pose in the robot-base frame from the world frame (R, p) of the site's link: position, quaternion x y z w
RCSH_D void torque_tcp_pose(const TorqueLawDev& law, const double* R, const double* own, double* pos, double* quat) {
  const double* Rb = law.base_R;
  const double d[3] = {own[0] - law.base_p[0], own[1] - law.base_p[1], own[2] - law.base_p[2]};
  double Rw[9], Rl[9];
  mulmm(R, law.tcp_R, Rw);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pos[r] = Rb[r] * d[0] + Rb[3 + r] * d[1] + Rb[6 + r] * d[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) Rl[3 * r + c] = Rb[r] * Rw[c] + Rb[3 + r] * Rw[3 + c] + Rb[6 + r] * Rw[6 + c];
  }
  mat_to_quat(Rl, quat);
  quat_normalize(quat);
}

// The law at the block's q / qvel.  Every lane of the wavefront calls it (team_sync inside).  Writes ctrl[arm] into the block unless
// the task-space matrix is not positive definite; returns that verdict (the same on every lane of the team).
template <class T>
RCSH_D bool torque_law(const TorqueLawDev& law, const double* gravity, int sl, const LinkRec* links, const StageTeam<T>& st, TorqueLds<T>& B,
                       int t, bool live, bool gc_is_mass, double q_des) {
  constexpr int NL = T::NL, NA = T::NARM, NR = kTaskRows;
  const int tbase = threadIdx.x & 48;
  const bool valid = t < NL;
  const bool mine = live && valid;
  const int tl = valid ? t : NL - 1;
  const int ta = t < NA ? t : NA - 1;
  const bool task = t < NR;
  const int tr = task ? t : NR - 1;
  const LinkRec& lk = links[tl];
  const uint32_t mask = law.task_mask;
  const double q = mine ? st.q(tl) : 0.0, qd = mine ? st.v(tl) : 0.0;
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
  }
  double vel[6], acc[6];
  const double chain = t <= NA ? 1.0 : 0.0, second = t == NA + 1 ? 1.0 : 0.0;  // (only read by archetypes with a gripper)
#pragma unroll
  for (int k = 0; k < 6; ++k) vel[k] = scan_from_root<T>(S[k] * qd, chain, second);
  {
    double sd[6];
    cross_motion(vel, S, sd);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = scan_from_root<T>(sd[k] * qd, chain, second);
  }

  // ---- spatial inertia about the world origin, composite inertia, the subtree's bias wrench, the gravity-compensation first moment
  double Ic[10], Fb[6], hs[3];
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
    double Ia[6], Iv[6], vf[6];
    const double accg[6] = {acc[0], acc[1], acc[2], acc[3] - gravity[0], acc[4] - gravity[1], acc[5] - gravity[2]};
    inert_mul(Ii, accg, Ia);
    inert_mul(Ii, vel, Iv);
    cross_force(vel, Iv, vf);
    const bool ff = T::GRIP && t == NA;
#pragma unroll
    for (int k = 0; k < 9; ++k) Ic[k] = scan_from_leaves<T>(Ii[k], ff);
#pragma unroll
    for (int k = 0; k < 6; ++k) Fb[k] = scan_from_leaves<T>(Ia[k] + vf[k], ff);
    if (gc_is_mass) {
      Ic[9] = valid ? gcm_sub : 0.0;
      hs[0] = Ic[6]; hs[1] = Ic[7]; hs[2] = Ic[8];
    } else {
      Ic[9] = scan_from_leaves<T>(Ii[9], ff);
#pragma unroll
      for (int k = 0; k < 3; ++k) hs[k] = scan_from_leaves<T>(gcm * cg[k], ff);
    }
  }

  // (the scheduling fence k_dynamics_query and k_opspace_query keep between the scans and the matrix phases)
  sched_fence();

  // ---- qfrc_bias, qfrc_gravcomp, the null-space torque of the lane's joint
  const double bias = dot6(S, Fb);
  double gc;
  {
    const double ng[3] = {-gravity[0], -gravity[1], -gravity[2]};
    double w[6];
    cross3(hs, ng, w);
    w[3] = gcm_sub * ng[0]; w[4] = gcm_sub * ng[1]; w[5] = gcm_sub * ng[2];
    gc = dot6(S, w);
  }
  double tau0 = t < NA ? law.joint_k[ta] * (q_des - q) - law.joint_d[ta] * qd : 0.0;
  tau0 += law.compensate_bias ? bias : 0.0;
  if (mask == 0) {  // (wave-uniform) the pure joint law: null_proj = I
    const bool wild = team_ballot(t < NA && !(fabs(tau0 - gc) < __builtin_huge_val())) != 0;  // (a non-finite target: as a singular substep)
    if (live && !wild && t < NA) st.c(t) = tau0 - gc;
    return wild;
  }
  if (valid) {
    B.b[tl] = bias;
    B.tau0[tl] = tau0;
  }
  team_sync();  // every lane's S, b and tau0 are in the block

  // ---- the TCP: its Jacobian column (lane j, joint j); on the site link's lane its pose, twist and velocity-product acceleration,
  // and from them the commanded task acceleration
  const double* Rb = law.base_R;
  double jt[NR];
  {
    double own[3], pt[3];
    mulmv(R, law.tcp_p, own);
    own[0] += p[0]; own[1] += p[1]; own[2] += p[2];
    const int src = tbase + sl;
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
    const bool above = (anc_mask<T>(sl) >> tl) & 1u;  // (joints off the site's chain -- the fingers -- do not move it)
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
    if (t == sl) {
      double wp[3], vp[3], ap[3], wv[3];
      cross3(vel, own, wp);
#pragma unroll
      for (int k = 0; k < 3; ++k) vp[k] = vel[3 + k] + wp[k];
      cross3(acc, own, ap);
      cross3(vel, vp, wv);
#pragma unroll
      for (int k = 0; k < 3; ++k) ap[k] += acc[3 + k] + wv[k];
      // the pose error: position, and the logarithm of q_des conj(q) on the shorter arc
      double pos[3], qc[4], xe[NR];
      torque_tcp_pose(law, R, own, pos, qc);
      {
        double qt[4] = {B.pose[3], B.pose[4], B.pose[5], B.pose[6]};
        quat_normalize(qt);
        const double conj[4] = {-qc[0], -qc[1], -qc[2], qc[3]};
        double qe[4];
        quat_mul(qt, conj, qe);
        const double sg = qe[3] < 0.0 ? -1.0 : 1.0;
        const double nv = sqrt(qe[0] * qe[0] + qe[1] * qe[1] + qe[2] * qe[2]);
        const double f = nv > 1e-12 ? sg * 2.0 * atan2(nv, sg * qe[3]) / nv : 2.0 * sg;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          xe[k] = B.pose[k] - pos[k];
          xe[3 + k] = f * qe[k];
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double ml = (mask >> k) & 1u ? 1.0 : 0.0, ma = (mask >> (3 + k)) & 1u ? 1.0 : 0.0;
        const double twl = ml * (Rb[k] * vp[0] + Rb[3 + k] * vp[1] + Rb[6 + k] * vp[2]);
        const double twa = ma * (Rb[k] * vel[0] + Rb[3 + k] * vel[1] + Rb[6 + k] * vel[2]);
        B.jd[k] = ml * (Rb[k] * ap[0] + Rb[3 + k] * ap[1] + Rb[6 + k] * ap[2]);
        B.jd[3 + k] = ma * (Rb[k] * acc[0] + Rb[3 + k] * acc[1] + Rb[6 + k] * acc[2]);
        B.xa[k] = law.task_k[k] * xe[k] - law.task_d[k] * twl;
        B.xa[3 + k] = law.task_k[3 + k] * xe[3 + k] - law.task_d[3 + k] * twa;
      }
    }
  }

  // ---- mass-matrix row of the link; every lane factors the same matrix, lane 0 parks the factor in the block
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
    if (valid) {
#pragma unroll
      for (int j = 0; j < NL; ++j) B.M[tl][j] = mrow[j];  // (entries right of the diagonal: not ancestors, never read)
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
      s += ((r == tr) & (bool)((mask >> r) & 1u)) ? law.damping : 0.0;
      if (task) B.A[r * NR + tr] = s;
    }
  }
  team_sync();

  // ---- the 6 x 6 factor, by every lane; the verdict
  double H6[NR * (NR + 1) / 2];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) H6[tri(i, j)] = B.A[i * NR + j];
    H6[tri(i, i)] = (mask >> i) & 1u ? H6[tri(i, i)] : 1.0;
  }
  const bool bad = ops_factor6(H6, mask, law.rel_pivot);

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
  team_sync();

  // ---- the task force lambda xacc + op_bias, op_bias = jbar^T b - lambda jdot_qvel: lane r, entry r
  {
    double f = 0.0;
#pragma unroll
    for (int i = 0; i < NL; ++i) f += B.Jb[i * NR + tr] * B.b[i];
#pragma unroll
    for (int c = 0; c < NR; ++c) f -= B.Lm[tr * NR + c] * B.jd[c];
#pragma unroll
    for (int c = 0; c < NR; ++c) f += B.Lm[tr * NR + c] * B.xa[c];
    if (task) B.F[tr] = f;
  }
  team_sync();

  // ---- tau = J^T F + (I - J^T jbar^T) qfrc_null: lane i, entry i
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < NR; ++r) s += jt[r] * B.F[r];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    double nj = j == tl ? 1.0 : 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) nj -= jt[r] * B.Jb[j * NR + r];
    s += nj * B.tau0[j];
  }
  // (a torque that is not finite -- a target the caller left NaN or with a zero quaternion -- is held back like a singular substep's)
  const bool hold = bad || team_ballot(t < NA && !(fabs(s - gc) < __builtin_huge_val())) != 0;
  if (live && !hold && t < NA) st.c(t) = s - gc;
  return hold;
}

// k substeps of every environment, the law before each (rcsh_sim_step_torque).  Scenes without a free body, robot contacts not
// resolved, no rate-driven cameras: the host checks.
template <class T, bool FRIC>
__global__ void __launch_bounds__(64) k_run_torque(TorqueArgs A) {
  using ST = StageTeam<T>;
  using L = Lay<T>;
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM;
  __shared__ DevModelHead lm;
  __shared__ LinkRec llinks[NL];
  __shared__ TorqueLawDev llaw;
  __shared__ __attribute__((aligned(16))) double lds[ST::COUNT * kTeams];
  __shared__ TorqueLds<T> lawlds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const int n = A.n;
  const bool live = e < n;
  const size_t ec = (size_t)(live ? e : 0);
  // ---- the environment's state: asked for first, stored to the block after the model has been staged
  double in_q = 0.0, in_v = 0.0, in_c = 0.0, in_xs = 0.0, in_qdes = 0.0, in_pose = 0.0, time = 0.0;
  if (live) {
    if (t < NL) {
      in_q = A.S[(size_t)(L::QPOS + t) * n + ec];
      in_v = A.S[(size_t)(L::QVEL + t) * n + ec];
      if constexpr (FRIC) in_xs = A.S[(size_t)(L::XS + t) * n + ec];
    }
    if (t < T::NU) in_c = A.S[(size_t)(L::CTRL + t) * n + ec];
    if (t < NA) in_qdes = A.target[(size_t)(kTorquePose + t) * n + ec];
    if (t < kTorquePose) in_pose = A.target[(size_t)t * n + ec];
    if (t == 0) time = A.S[(size_t)L::TIME * n + ec];
  }
  stage_team_model<NL>(A.model, lm, llinks);
  {
    const double* src = reinterpret_cast<const double*>(&A.law);
    double* dst = reinterpret_cast<double*>(&llaw);
    for (int k = threadIdx.x; k < (int)(sizeof(TorqueLawDev) / 8); k += 64) dst[k] = src[k];
  }
  for (int k = threadIdx.x; k < ST::COUNT * kTeams; k += 64) lds[k] = 0.0;
  __syncthreads();
  const ST st{lds + team * ST::COUNT};
  TorqueLds<T>& B = lawlds[team];
  if (t < NL) {
    st.q(t) = in_q;
    st.v(t) = in_v;
    st.qpre(t) = in_q;
    if constexpr (FRIC) st.xs(t) = in_xs;
  }
  if (t < T::NU) st.c(t) = in_c;
  B.pose[t < kTorquePose ? t : kTorquePose] = t < kTorquePose ? in_pose : 0.0;
  __syncthreads();
  const DevModelHead& m = lm;
  const bool gc_is_mass = team_gc_is_mass<T>(llinks, t);
  SubstepK sk;
  sk.load(m);
  const double timestep = m.timestep;
  const bool use_law = A.enabled != 0;  // (wave-uniform)
  bool singular = false;
  for (int step = 0; step < A.k; ++step) {
    if (use_law) {
      singular |= torque_law<T>(llaw, sk.gravity, sk.site_link, llinks, st, B, t, live, gc_is_mass, in_qdes);
      __syncthreads();  // ctrl is in the block
    }
    sched_fence();
    team_substep<T, FRIC>(m, sk, llinks, st, t, live, gc_is_mass, [](const double*, const double*) {}, [] { return false; });
    time += timestep;
    __syncthreads();
  }
  // ---- back to memory, once
  if (live && A.k > 0) {
    if (t < NL) {
      A.S[(size_t)(L::QPOS + t) * n + ec] = st.q(t);
      A.S[(size_t)(L::QVEL + t) * n + ec] = st.v(t);
      if (A.keep_qpre) A.S[(size_t)(L::QPRE + t) * n + ec] = st.qpre(t);
      if constexpr (FRIC) A.S[(size_t)(L::XS + t) * n + ec] = st.xs(t);
    }
    if (t < NA) A.S[(size_t)(L::CTRL + t) * n + ec] = st.c(t);
    if (t < 12) A.S[(size_t)(L::SITE + t) * n + ec] = st.link(t);
    if (t == 0) {
      A.S[(size_t)L::TIME * n + ec] = time;
      if (singular) A.singular[ec] = 1;
    }
  }
}

// The TCP's pose in the base frame at the targets' q_des (the fingers where the environment has them): what set_joint_position,
// move_home and the resets leave as the pose target of a torque-actuated robot.  One environment per team.
template <class T>
__global__ void __launch_bounds__(64) k_torque_target_pose(TorqueArgs A, const uint8_t* mask) {
  using L = Lay<T>;
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM;
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const int n = A.n;
  const bool live = e < n && !(mask && !mask[e < n ? e : 0]);
  const size_t ec = (size_t)(live ? e : 0);
  const bool valid = t < NL;
  const int tl = valid ? t : NL - 1;
  const LinkRec* links = reinterpret_cast<const LinkRec*>(reinterpret_cast<const char*>(A.model) + sizeof(DevModel));
  double q = 0.0;
  if (live && valid) q = t < NA ? A.target[(size_t)(kTorquePose + t) * n + ec] : A.S[(size_t)(L::QPOS + t) * n + ec];
  KinK kk;
  kk.load(links[tl]);
  double R[9], p[3];
  link_local_frame(kk, q, R, p);
  scan_frames<T>(R, p);
  const int sl = A.model->site_link;
  if (live && t == sl) {
    double own[3], pos[3], qc[4];
    mulmv(R, A.law.tcp_p, own);
    own[0] += p[0]; own[1] += p[1]; own[2] += p[2];
    torque_tcp_pose(A.law, R, own, pos, qc);
    double* out = const_cast<double*>(A.target);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[(size_t)k * n + ec] = pos[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) out[(size_t)(3 + k) * n + ec] = qc[k];
  }
}

#endif  // __HIP__

}  // namespace rcsh
