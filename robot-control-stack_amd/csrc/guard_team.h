// guard_team.h -- the environments' collision guard (rcsh_env_configure_guard / rcsh_env_guard_peek).
//
// The reference's CollisionGuard (python/rcs/envs/sim.py:156-287) is an action filter: before every step it tries the action on a
// second MuJoCo instance, and if that reports a collision the robot is commanded to stay where it is and the episode is truncated.
// Here the question is answered kinematically, for every environment at once, by the motion validator of query_team.h: an action
// passes when the straight joint-space motion from where the arm IS to where the action SENDS it is proven free.
//
// One environment per TEAM of 16 lanes, four per wavefront, as k_motion_query -- but the segment is the environment's own:
//  * start: the chain configuration the stepping kernels will load (Lay::QPOS: arm joints and finger slides), read by
//    query_env_row (query_team.h) as the env form of the clearance query reads it;
//  * end, arm joints: the absolute joint command RobotEnv.step would receive for this action -- the RelativeActionSpace arithmetic of
//    env_prologue_team (sim_kernels.h), recomputed READ-ONLY: ORIGIN, LASTA and kHasLastAction are read, never written;
//  * end, finger slides: where they are (the gripper action is not guarded: the reference's gripper wrapper strips that key before the
//    guard sees the action) -- so a pair of geoms that only finger slides separate keeps its relative pose over the segment and is
//    decided by the sample at its start (motion_decide<T, true>): the closed hand's pads, touching at a gap of exactly 0 after every
//    reset, pass no certificate, and without this every fresh episode would be blocked;
//  * the free body, in scenes that have one and when `kinds` asks for it: at the environment's own current pose (Lay::BOX + kBoxQ).
// The kernel writes its record and nothing else: result / t_contact as the motion query, `blocked`, and -- for a guarded step --
// the byte per environment the stepping launch reads as its mask (RunOp::mask: bit 0 takes part, bit 1 hold).
#pragma once
#include "query_team.h"
#include "sim_kernels.h"

namespace rcsh {

constexpr uint8_t kGuardLive = 1, kGuardHold = 2;  // RunOp::mask of a guarded step (RunOp::apply_action == 2)

struct GuardArgs {
  QueryArgs Q;             // tables, kinds, resolution; m: the environments (q0 / q1 / free_qpos and the outputs are unused)
  const double* S;         // the state, [field][n]
  const uint32_t* flags;   // [n]
  const double* action;    // [n][NARM]
  EnvCfg env;
  int32_t box_field;       // Lay::BOX + kBoxQ when the free body is tested, -1 otherwise
  int32_t block_undecided;
  int32_t* result;         // [n] 0 free / 1 contact / 2 undecided
  double* t_contact;       // [n] -1 where result != 1
  uint8_t* blocked;        // [n]
  uint8_t* hold;           // [n] or null: kGuardLive | (blocked ? kGuardHold : 0)
};

#if defined(__HIP__)

template <class T>
__global__ void __launch_bounds__(64) k_env_guard(GuardArgs G) {
  using L = Lay<T>;
  constexpr int kTeams = 64 / kTeamLanes, NL = T::NL;
  __shared__ QueryTeamLds<T> lds[kTeams];
  const int team = threadIdx.x / kTeamLanes, t = threadIdx.x % kTeamLanes;
  const int e = blockIdx.x * kTeams + team;
  const int n = G.Q.m;
  const bool live = e < n;
  const size_t ec = live ? e : 0;
  double qa, fq[7];
  const bool use_box = query_env_row(G.S, n, e, live, t < NL, L::QPOS, G.box_field, qa, fq);
  double qb = qa;
  if (live && t < T::NARM) {
    // RelativeActionSpace.action (python/rcs/envs/base.py:468-488), JOINTS mode: env_prologue_team without its stores
    double a = G.action[ec * T::NARM + t];
    if (G.env.relative_to != 0) {
      const bool last_step = G.env.relative_to == 1;
      const bool fresh = last_step || !(G.flags[ec] & kHasLastAction);
      const double origin = last_step ? qa : G.S[(size_t)(L::ORIGIN + t) * n + ec];
      double lim;
      if (fresh) {
        lim = clampd(a, -G.env.max_mov[0], G.env.max_mov[0]);
      } else {
        const double la = G.S[(size_t)(L::LASTA + t) * n + ec];
        lim = clampd(a - la, -G.env.max_mov[0], G.env.max_mov[0]) + la;
      }
      a = clampd(origin + lim, G.env.low[t], G.env.high[t]);
    }
    qb = a;
  }
  int result = 0;
  double tc = -1.0;
  motion_decide<T, true>(G.Q, lds[team], live, qa, qb, fq, use_box, result, tc);
  if (live && t == 0) {
    const bool blocked = result == 1 || (result == 2 && G.block_undecided);
    G.result[e] = result;
    G.t_contact[e] = tc;
    G.blocked[e] = blocked ? 1 : 0;
    if (G.hold) G.hold[e] = (uint8_t)(kGuardLive | (blocked ? kGuardHold : 0));
  }
}

#endif  // __HIP__

}  // namespace rcsh
