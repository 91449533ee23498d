// env_torque_team.h -- the fused env step of torque-actuated robots (rcsh_env_step / rcsh_env_reset in RCSH_MODE_TORQUE,
// RCSH_MODE_JOINT_IMPEDANCE, RCSH_MODE_CARTESIAN_IMPEDANCE_TRPY / _TQUAT): the wrappers' action(), the write of the law's target
// and the step's substeps, the law before each of them, in ONE launch.
//
// k_env_torque is k_run_torque (torque_team.h) with a prologue in front and a reset form of its own.  Same layout: one environment
// per TEAM of 16 lanes, four per wavefront, the state in a StageTeam block through Lay<T>, loaded once and stored once, the site
// frame parked at the end.  The observation is NOT formed here: the handle's observing pass (launch_run, nsteps = 0, observe_only)
// follows on the stream, so the observation is the JOINTS mode's by construction.
//  prologue (a step):
//   gripper    GripperWrapper.action, restated from env_prologue_team / cart_prepare: last commanded width and the gripper's ctrl
//              to memory, kGripCmd / kHasGripCmd;
//   TORQUE     ctrl[arm] = action.  No relative action space, no gate, no law;
//   JOINT_IMPEDANCE  the joint branch of env_prologue_team, restated WITHOUT SimRobot::set_joint_position: RelativeActionSpace
//              (ORIGIN / LASTA / kHasLastAction, max_mov[0], the joint-limit clamp), RobotEnv.step's 1e-3 gate against PREVA; a
//              commanded action becomes the law's q_des, a gated-out one leaves it.  ctrl, target / previous angles, kIsMoving /
//              kIsArrived are not touched;
//   CARTESIAN_IMPEDANCE  cart_prepare as it is, by the leader lane, BEFORE the block is loaded (it works on memory: GRIP, the
//              gripper's ctrl, PREVA, ORIGIN, LASTA); a commanded pose becomes the law's pose target.  The host hands P.env.mode as
//              the position mode of the same action row (1 / 2): that is what cart_prepare reads.
//  reset form: GripperWrapper.reset, Sim::reset (qpos0, zero qvel / ctrl / time / callback timestamps / warm start, sticky
//   contact flags), the arm at q_home with ZERO torque (ctrl is a torque here), the singular byte cleared, the law's q_des at q_home
//   and its pose target at the TCP's pose there (what torque_rest_at leaves: the frame phase of k_torque_target_pose on the block's
//   q); ONE substep; the relative-action origin from the state after it (joint vector; or cartesian_position of the parked site
//   frame, as env_epilogue takes it); kHasLastAction cleared, PREVA / kHasPrevAction not (the reference's quirk).
// SHARED: torque_law, team_substep, stage_team_model, torque_tcp_pose, cart_prepare, cartesian_position, store_pose7, clampd, pose.h.
// RESTATED: k_run_torque's load / loop / store skeleton (its text stays), the joint branch and the gripper piece of
// env_prologue_team, the reset branch of env_prologue_team with zero torque in place of q_home, the origin refresh of env_epilogue.
#pragma once
#include "torque_team.h"

namespace rcsh {

// rcsh_env_desc::control_mode of the modes this kernel serves (include/rcs_hip.h; the C-ABI file asserts the match)
enum : int32_t { kEnvModeTorque = 3, kEnvModeJointImpedance = 4, kEnvModeCartImpedanceTrpy = 5, kEnvModeCartImpedanceTquat = 6 };

struct EnvTorqueOp {
  int32_t mode;          // kEnvModeTorque .. kEnvModeCartImpedanceTquat
  int32_t do_reset;      // the reset form (one substep); else a step of TorqueArgs::k substeps
  const uint8_t* mask;   // optional, device: a zero byte sits the environment out
  const double* action;  // [n][action width], device (a step)
  const float* gripper;  // [n], device, may be null
  int32_t* substeps;     // [n], may be null: the substeps this launch ran
};

#if defined(__HIP__)

static_assert(sizeof(Params) + sizeof(EnvTorqueOp) + sizeof(TorqueArgs) <= 4096, "the three argument blocks fit the kernel-argument segment");

template <class T, bool FRIC>
__global__ void __launch_bounds__(64) k_env_torque(Params P, EnvTorqueOp op, TorqueArgs A) {
  using ST = StageTeam<T>;
  using L = Lay<T>;
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL, NA = T::NARM, NU = T::NU;
  __shared__ DevModelHead lm;
  __shared__ LinkRec llinks[NL];
  __shared__ TorqueLawDev llaw;
  __shared__ __attribute__((aligned(16))) double lds[ST::COUNT * kTeams];
  __shared__ TorqueLds<T> lawlds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const int n = A.n;
  const bool live = e < n && !(op.mask && !op.mask[e < n ? e : 0]);
  const size_t ec = (size_t)(live ? e : 0);
  const bool leader = live && t == 0, joint = t < NA;
  const int ti = joint ? t : 0;
  const bool reset = op.do_reset != 0;                   // (wave-uniform, like the three below)
  const bool cart = op.mode >= kEnvModeCartImpedanceTrpy;
  const bool raw = op.mode == kEnvModeTorque;
  const bool has_g = T::GRIP && P.grip.present;
  double* S = A.S;
  double* tgt = const_cast<double*>(A.target);
  uint32_t flags = live ? P.flags[ec] : 0u;  // (every lane of the team carries the word; the leader's copy goes back)
  stage_team_model<NL>(A.model, lm, llinks);
  {
    const double* src = reinterpret_cast<const double*>(&A.law);
    double* dst = reinterpret_cast<double*>(&llaw);
    for (int k = threadIdx.x; k < (int)(sizeof(TorqueLawDev) / 8); k += 64) dst[k] = src[k];
  }
  for (int k = threadIdx.x; k < ST::COUNT * kTeams; k += 64) lds[k] = 0.0;
  __syncthreads();
  const DevModelHead& m = lm;

  // ---- the wrappers' action(), on memory: what the block load below picks up
  double cmd_qdes = 0.0;
  bool has_qdes = false;
  if (!reset && cart) {
    if (leader) {
      CartOp cop{};
      cop.env_layer = 1;
      cop.action = op.action;
      cop.gripper = op.gripper;
      Pose target;
      if (cart_prepare<T>(P, cop, m, e, flags, target)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tgt[(size_t)k * n + ec] = target.t[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) tgt[(size_t)(3 + k) * n + ec] = target.q[k];
      }
    }
  } else if (!reset) {
    // GripperWrapper.action (base.py:721-735), as env_prologue_team has it
    if (has_g && op.gripper) {
      float g = live ? op.gripper[ec] : 0.0f;
      if (P.env.binary_gripper) g = rintf(g);  // np.round: half to even
      g = fminf(fmaxf(g, 0.0f), 1.0f);
      const double w = P.env.binary_gripper ? (g == 0.0f ? 0.0 : 1.0) : (double)g;  // binary: grasp() = shut() : open()
      if (leader) {
        S[(size_t)(L::GRIP + 0) * n + ec] = w;
        S[(size_t)(L::CTRL + NU - 1) * n + ec] = w * (P.grip.max_act - P.grip.min_act) + P.grip.min_act;
      }
      set_flag(flags, kGripCmd, P.env.binary_gripper ? g != 0.0f : g >= 0.5f);
      flags |= kHasGripCmd;
    }
    if (!raw) {
      // RelativeActionSpace.action (base.py:468-488), JOINTS mode: lane i, joint i
      const bool mine = live && joint;
      double a = mine ? op.action[ec * NA + ti] : 0.0;
      if (P.env.relative_to != 0) {
        const bool last_step = P.env.relative_to == 1;
        const bool fresh = last_step || !(flags & kHasLastAction);
        if (mine) {
          const double origin = S[(size_t)((last_step ? L::QPOS : L::ORIGIN) + ti) * n + ec];
          const double in_lasta = fresh ? 0.0 : S[(size_t)(L::LASTA + ti) * n + ec];
          const double lim = fresh ? clampd(a, -P.env.max_mov[0], P.env.max_mov[0]) : clampd(a - in_lasta, -P.env.max_mov[0], P.env.max_mov[0]) + in_lasta;
          if (last_step) S[(size_t)(L::ORIGIN + ti) * n + ec] = origin;
          S[(size_t)(L::LASTA + ti) * n + ec] = lim;
          a = clampd(origin + lim, P.env.low[ti], P.env.high[ti]);
        }
        flags |= kHasLastAction;
      }
      // RobotEnv.step (base.py:255-288): command only when the action moved by more than atol = 1e-3, or on the first action
      const double in_preva = mine ? S[(size_t)(L::PREVA + ti) * n + ec] : 0.0;
      const bool moved = mine && !(fabs(a - in_preva) <= 1e-3);
      const bool changed = !(flags & kHasPrevAction) || team_ballot(moved) != 0;
      if (mine) S[(size_t)(L::PREVA + ti) * n + ec] = a;
      if (changed && mine) {  // the command: the law's q_des (no SimRobot::set_joint_position: there is no servo)
        tgt[(size_t)(kTorquePose + ti) * n + ec] = a;
        cmd_qdes = a;
        has_qdes = true;
      }
      flags |= kHasPrevAction;
    }
  }
  __syncthreads();  // (and its fences: the prologue's stores are in memory before the loads below)

  // ---- the environment's state: from memory, or the reset's
  double in_q = 0.0, in_v = 0.0, in_c = 0.0, in_xs = 0.0, in_qdes = 0.0, in_pose = 0.0, time = 0.0;
  if (live && !reset) {
    if (t < NL) {
      in_q = S[(size_t)(L::QPOS + t) * n + ec];
      in_v = S[(size_t)(L::QVEL + t) * n + ec];
      if constexpr (FRIC) in_xs = S[(size_t)(L::XS + t) * n + ec];
    }
    if (t < NU) in_c = S[(size_t)(L::CTRL + t) * n + ec];
    if (raw && joint) in_c = op.action[ec * NA + ti];  // TORQUE: held over the launch, clamped by ctrlrange in the substep
    if (joint) in_qdes = has_qdes ? cmd_qdes : A.target[(size_t)(kTorquePose + t) * n + ec];
    if (t < kTorquePose) in_pose = A.target[(size_t)t * n + ec];
    if (t == 0) time = S[(size_t)L::TIME * n + ec];
  }
  if (reset) {
    // GripperWrapper.reset -> SimGripper::m_reset; RobotSimWrapper.reset -> Sim::reset = mj_resetData + reset_callbacks, which
    // overwrites what the gripper reset wrote to qpos / ctrl; RobotEnv.reset -> set_joints_hard(q_home), whose
    // ctrl on a torque-actuated robot is zero torque (torque_rest_at)
    if (t < NL) in_q = joint ? P.robot.q_home[ti] : m.qpos0[t < NL ? t : 0];
    if (joint) in_qdes = P.robot.q_home[ti];
    if (has_g) flags &= ~(kGripMoving | kGripCollision | kHasGripCmd | kGripCmd);
    flags &= ~(kContactOverflow | kContactUnresolved | kContactResolved | kEscQuiet);  // (sticky until Sim::reset: this is it)
    if (live) {
      if (t < 6) S[(size_t)(L::CB + t) * n + ec] = 0.0;
      if (t < kCheckSep) S[(size_t)(L::SEP + t) * n + ec] = 0.0;
      if (joint) tgt[(size_t)(kTorquePose + ti) * n + ec] = in_qdes;
      if (has_g && t < 2) S[(size_t)(L::GRIP + t) * n + ec] = 0.0;
    }
  }
  const ST st{lds + team * ST::COUNT};
  TorqueLds<T>& B = lawlds[team];
  if (t < NL) {
    st.q(t) = in_q;
    st.v(t) = in_v;
    st.qpre(t) = in_q;
    if constexpr (FRIC) st.xs(t) = in_xs;
  }
  if (t < NU) st.c(t) = in_c;
  B.pose[t < kTorquePose ? t : kTorquePose] = t < kTorquePose ? in_pose : 0.0;
  SubstepK sk;
  sk.load(m);
  if (reset) {
    // the pose target a reset leaves: the TCP at the block's q (k_torque_target_pose's frame phase)
    const bool valid = t < NL;
    const int tl = valid ? t : NL - 1;
    KinK kk;
    kk.load(llinks[tl]);
    double R[9], p[3];
    link_local_frame(kk, live && valid ? in_q : 0.0, R, p);
    scan_frames<T>(R, p);
    __syncthreads();  // (every lane has written its slot of B.pose above)
    if (t == sk.site_link) {
      double own[3], pos[3], qc[4];
      mulmv(R, llaw.tcp_p, own);
      own[0] += p[0]; own[1] += p[1]; own[2] += p[2];
      torque_tcp_pose(llaw, R, own, pos, qc);
#pragma unroll
      for (int k = 0; k < 3; ++k) B.pose[k] = pos[k];
#pragma unroll
      for (int k = 0; k < 4; ++k) B.pose[3 + k] = qc[k];
      if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) tgt[(size_t)k * n + ec] = pos[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) tgt[(size_t)(3 + k) * n + ec] = qc[k];
      }
    }
  }
  __syncthreads();
  const bool gc_is_mass = team_gc_is_mass<T>(llinks, t);
  const double timestep = m.timestep;
  const bool use_law = A.enabled != 0 && !raw;  // (wave-uniform)
  const int nsub = reset ? 1 : A.k;
  bool singular = false;
  for (int step = 0; step < nsub; ++step) {
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
  if (live) {
    if (t < NL) {
      S[(size_t)(L::QPOS + t) * n + ec] = st.q(t);
      S[(size_t)(L::QVEL + t) * n + ec] = st.v(t);
      if (A.keep_qpre) S[(size_t)(L::QPRE + t) * n + ec] = st.qpre(t);
      else if (reset) S[(size_t)(L::QPRE + t) * n + ec] = m.qpos0[t];  // (Sim::reset; nobody advances it without a render scene)
      if constexpr (FRIC) S[(size_t)(L::XS + t) * n + ec] = st.xs(t);
    }
    if (reset ? t < NU : joint) S[(size_t)(L::CTRL + t) * n + ec] = st.c(t);
    if (t < 12) S[(size_t)(L::SITE + t) * n + ec] = st.link(t);
    if (reset && P.env.relative_to != 0) {
      // RelativeActionSpace.reset (base.py:461-466): origin := current, _last_action := None
      if (!cart) {
        if (joint) S[(size_t)(L::ORIGIN + ti) * n + ec] = st.q(ti);
      } else if (t == 0) {
        double oR[9], oP[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) oR[k] = st.link(k);
#pragma unroll
        for (int k = 0; k < 3; ++k) oP[k] = st.link(9 + k);
        Pose origin;
        cartesian_position(m, P.robot, oR, oP, origin);
        store_pose7<T>(S, n, e, L::ORIGIN, origin);
      }
      flags &= ~kHasLastAction;
    }
    if (t == 0) {
      S[(size_t)L::TIME * n + ec] = time;
      P.flags[ec] = flags;
      if (singular) A.singular[ec] = 1;
      else if (reset) A.singular[ec] = 0;
      if (op.substeps) op.substeps[ec] = nsub;
    }
  }
}

#endif  // __HIP__

}  // namespace rcsh
