// episode_host.cpp -- the host-only part of the autoreset (csrc/episode_team.h): what is wrong with a description, and
// rcsh_autoreset_draw, the device's cube placement computed on the host.  No handle, no device, no HIP: the file compiles with any
// C++17 compiler, which is how tests/host/autoreset_draw_main.cpp runs it under the host sanitizers.
#define RCSH_EPISODE_HOST_ONLY
#include "episode_team.h"

#include <cmath>

namespace rcsh {

const char* autoreset_desc_error(const rcsh_autoreset_desc* a, int64_t n_envs) {
  if (!a) return "null autoreset description";
  if (a->max_episode_steps < 0) return "max_episode_steps must not be negative (0: no time limit)";
  if (a->env_offset < 0) return "env_offset must not be negative";
  if (a->env_offset > (int64_t(1) << 32) - n_envs) return "env_offset + n_envs exceeds 2^32: the placement's counter holds an environment's index in 32 bits";
  for (int k = 0; k < 7; ++k)
    if (!std::isfinite(a->box_pose[k])) return "box_pose must be finite";
  if (!std::isfinite(a->rotation_minus)) return "rotation_minus must be finite";
  return nullptr;
}

}  // namespace rcsh

extern "C" int rcsh_autoreset_draw(const rcsh_autoreset_desc* desc, int64_t env, int64_t episode, double qpos7[7]) {
  if (const char* why = rcsh::autoreset_desc_error(desc, 0)) return rcsh::episode_fail(RCSH_ERR_ARG, why);
  if (!qpos7) return rcsh::episode_fail(RCSH_ERR_ARG, "null pose output");
  if (env < 0 || episode < 0) return rcsh::episode_fail(RCSH_ERR_ARG, "env and episode must not be negative");
  if (env >= (int64_t(1) << 32) - desc->env_offset) return rcsh::episode_fail(RCSH_ERR_ARG, "env_offset + env exceeds 2^32 - 1");
  rcsh::autoreset_draw(rcsh::episode_draw_of(*desc), env, episode, qpos7);
  return RCSH_OK;
}
