// episode_team.h -- the end of an episode inside the fused env step (rcsh_env_configure_autoreset): Gymnasium's VectorEnv autoreset in
// its SAME_STEP mode.  After the stepping launch of an env step k_episode_end decides, per environment, whether its episode is over
// (the pick task's success, RobotSimWrapper's truncation, a time limit), keeps the terminal step's outputs in the record, counts, and
// writes the mask the masked reset launch that follows on the stream runs with.  With draw_box it also places the new episode's cube.
//
// The placement is COUNTER-BASED: Philox4x32-10 keyed by the seed, the counter made of the environment's index in the sharded batch,
// the number of autoresets it has had, and the block's number -- an environment's draws depend on nothing else (not on the batch
// size, not on who else finishes, not on how the batch is cut into handles).  autoreset_draw is one function for host and device
// (rcsh_autoreset_draw, csrc/episode_host.cpp) with floating-point contraction off, so both agree with a numpy restatement bit for bit.
#pragma once
#include <cstdint>

#include "../../include/rcs_hip.h"

#ifndef __HIP__  // a plain C++ compilation (csrc/episode_host.cpp by a host compiler)
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

namespace rcsh {

// what a draw needs of rcsh_autoreset_desc
struct EpisodeDraw {
  int32_t include_position, include_rotation;
  int64_t env_offset;
  uint32_t key[2];  // (seed & 0xffffffff, seed >> 32)
  double box_pose[7];
  double rotation_minus;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011): the counter block in place
__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// a uniform in [0, 1) from two words: 53 bits
__host__ __device__ inline double philox_uniform(uint32_t a, uint32_t b) {
  return (double)((((uint64_t)a << 32) | b) >> 11) * 0x1p-53;
}

// The cube pose of environment `env` (index in the handle) for its episode after `episode` autoresets.  Three uniforms are always
// consumed: u0, u1 from block 0, u2 from block 1.
__host__ __device__ inline void autoreset_draw(const EpisodeDraw& d, int64_t env, int64_t episode, double qpos7[7]) {
#if defined(__clang__)
#pragma clang fp contract(off)  // (a * b - c must round twice, as numpy does: hipcc would contract it into one fma)
#endif
  const uint32_t e = (uint32_t)(uint64_t)(d.env_offset + env), klo = (uint32_t)(uint64_t)episode, khi = (uint32_t)((uint64_t)episode >> 32);
  uint32_t b0[4] = {e, klo, khi, 0u}, b1[4] = {e, klo, khi, 1u};
  philox4x32_10(b0, d.key[0], d.key[1]);
  philox4x32_10(b1, d.key[0], d.key[1]);
  const double u0 = philox_uniform(b0[0], b0[1]), u1 = philox_uniform(b0[2], b0[3]), u2 = philox_uniform(b1[0], b1[1]);
  const double* p = d.box_pose;
  double sx = u0 * 0.2, sy = u1 * 0.2, w2 = 2.0 * u2;
  sx = p[0] + sx; sy = p[1] + sy;
  qpos7[0] = d.include_position ? sx - 0.1 : p[0];
  qpos7[1] = d.include_position ? sy - 0.1 : p[1];
  qpos7[2] = p[2];
  qpos7[3] = d.include_rotation ? w2 - d.rotation_minus : p[3];
  qpos7[4] = p[4]; qpos7[5] = p[5]; qpos7[6] = p[6];
}

inline EpisodeDraw episode_draw_of(const rcsh_autoreset_desc& a) {
  EpisodeDraw d{};
  d.include_position = a.include_position != 0;
  d.include_rotation = a.include_rotation != 0;
  d.env_offset = a.env_offset;
  d.key[0] = (uint32_t)(a.seed & 0xffffffffu);
  d.key[1] = (uint32_t)(a.seed >> 32);
  for (int k = 0; k < 7; ++k) d.box_pose[k] = a.box_pose[k];
  d.rotation_minus = a.rotation_minus;
  return d;
}

// What is wrong with a description for a handle of n_envs environments (0: the handle-free check of rcsh_autoreset_draw); null: nothing.
const char* autoreset_desc_error(const rcsh_autoreset_desc* a, int64_t n_envs);
// the C-ABI's error return (the message is what rcsh_last_error reports); defined next to the other entry points
int episode_fail(int code, const char* msg);

#if defined(__HIP__) && !defined(RCSH_EPISODE_HOST_ONLY)

constexpr int kEpisodeBlock = 256;
constexpr int kEpisodeInfo = 8, kEpisodeTask = 9;  // bytes of an info row; doubles of a task row (box pose 7, reward, success)

struct EpisodeArgs {
  int32_t n, obs_w, max_steps, draw_box;
  int32_t envs_per_block;  // kEpisodeBlock / row_items(obs_w)
  // the step's outputs, rows [n][w]; task: null without the pick task.  info: byte 4 of a row also receives the time limit
  const double* obs; uint8_t* info; const double* gw; const double* task;
  // the record (rcsh_autoreset_record)
  uint8_t *done, *terminated, *truncated, *time_limit;
  double* final_obs; uint8_t* final_info; double* final_gw; double* final_task;
  double* episode_return; int32_t* episode_length;
  int64_t* episodes; int32_t* elapsed; double* running_return;
  double* reset_box_qpos;
  EpisodeDraw draw;
};

// items of an environment: its observation row, its task row, its gripper width, and one for everything that is per environment
__host__ __device__ inline int episode_row_items(int obs_w) { return obs_w + kEpisodeTask + 2; }

// One lane per ITEM: consecutive lanes copy consecutive elements of a row (and the next environment's row follows); the last item of
// an environment is its scalar lane -- counters, verdict bytes, the info row as one 8-byte word, the draw.  Every lane derives `done`
// of its environment from the step's outputs and the counters BEFORE the barrier, the writes come after it: all items of an
// environment sit in one workgroup, so no lane reads what a scalar lane has already rewritten.
__global__ void __launch_bounds__(kEpisodeBlock) k_episode_end(EpisodeArgs A) {
  const int items = episode_row_items(A.obs_w);
  const int tid = (int)threadIdx.x;
  const int slot = tid / items, j = tid - slot * items;
  const int64_t e = (int64_t)blockIdx.x * A.envs_per_block + slot;
  const bool live = slot < A.envs_per_block && e < A.n;
  bool time_limit = false, terminated = false, truncated = false;
  int32_t elapsed = 0;
  if (live) {
    elapsed = A.elapsed[e] + 1;
    time_limit = A.max_steps > 0 && elapsed >= A.max_steps;
    terminated = A.task != nullptr && A.task[e * kEpisodeTask + 8] != 0.0;
    truncated = A.info[e * kEpisodeInfo + 4] != 0 || time_limit;
  }
  const bool done = terminated || truncated;
  __syncthreads();
  if (!live) return;
  if (j < A.obs_w) {
    if (done) A.final_obs[e * A.obs_w + j] = A.obs[e * A.obs_w + j];
  } else if (j < A.obs_w + kEpisodeTask) {
    const int k = j - A.obs_w;
    if (done && A.task) A.final_task[e * kEpisodeTask + k] = A.task[e * kEpisodeTask + k];
  } else if (j == A.obs_w + kEpisodeTask) {
    if (done) A.final_gw[e] = A.gw[e];
  } else {
    uint64_t row = *reinterpret_cast<const uint64_t*>(A.info + e * kEpisodeInfo);
    if (time_limit) {  // RobotSimWrapper's `truncated` (byte 4), as k_guard_truncate sets it for a blocked environment
      row = (row & ~(0xffull << 32)) | (1ull << 32);
      *reinterpret_cast<uint64_t*>(A.info + e * kEpisodeInfo) = row;
    }
    const double ret = A.running_return[e] + (A.task ? A.task[e * kEpisodeTask + 7] : 0.0);
    A.done[e] = done; A.terminated[e] = terminated; A.truncated[e] = truncated; A.time_limit[e] = time_limit;
    if (done) {
      *reinterpret_cast<uint64_t*>(A.final_info + e * kEpisodeInfo) = row;
      A.episode_return[e] = ret;
      A.episode_length[e] = elapsed;
      const int64_t k = A.episodes[e];
      A.episodes[e] = k + 1;
      if (A.draw_box) {
        double q[7];
        autoreset_draw(A.draw, e, k, q);
        for (int i = 0; i < 7; ++i) A.reset_box_qpos[e * 7 + i] = q[i];
      }
    }
    A.elapsed[e] = done ? 0 : elapsed;
    A.running_return[e] = done ? 0.0 : ret;
  }
}

// an explicit env reset under a configured autoreset: the episode of a reset environment begins again (`episodes` stays)
__global__ void k_episode_clear(const uint8_t* mask, int32_t* elapsed, double* running_return, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && (!mask || mask[i])) { elapsed[i] = 0; running_return[i] = 0.0; }
}

#endif  // __HIP__

}  // namespace rcsh
