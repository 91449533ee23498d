// autoreset_draw_main.cpp -- calls rcsh_autoreset_draw (csrc/episode_host.cpp) over a few thousand (seed, env, episode) triples on the
// CPU, for both placement rules and every combination of the include_* flags, and checks the ranges the rule promises.  Meant to be
// built with the host sanitizers (clang: the draw switches floating-point contraction off with a clang pragma):
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I<csrc> autoreset_draw_main.cpp
//       <csrc>/episode_host.cpp -o autoreset_draw && ./autoreset_draw
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "episode_team.h"

namespace {
std::string g_msg;
}
int rcsh::episode_fail(int code, const char* msg) {
  g_msg = msg;
  return code;
}

int main() {
  uint64_t state = 0x9E3779B97F4A7C15ull;
  auto next = [&] {  // splitmix64: the triples
    uint64_t z = (state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  };
  long draws = 0, bad = 0;
  double sum = 0;
  for (int rule = 0; rule < 2; ++rule)
    for (int flags = 0; flags < 4; ++flags)
      for (int t = 0; t < 500; ++t) {
        rcsh_autoreset_desc d;
        std::memset(&d, 0, sizeof(d));
        d.enabled = 1; d.draw_box = 1;
        d.include_position = flags & 1; d.include_rotation = flags >> 1;
        d.seed = next();
        const double iso[7] = {0.498, 0.0, 0.0144, 0, 0, 0, 1}, obj[7] = {0.45, -0.1, 0.03, 0.92, 0.0, 0.0, 0.39};
        std::memcpy(d.box_pose, rule ? obj : iso, sizeof(iso));
        d.rotation_minus = rule ? obj[3] : 1.0;
        d.env_offset = (int64_t)(next() % 1000);
        const int64_t env = (int64_t)(next() >> (t % 2 ? 33 : 50)), episode = (int64_t)(next() >> (t % 3 ? 1 : 40));
        double q[7];
        if (rcsh_autoreset_draw(&d, env, episode, q) != RCSH_OK) { std::printf("refused: %s\n", g_msg.c_str()); ++bad; continue; }
        ++draws;
        const double* p = d.box_pose;
        const bool in_x = d.include_position ? (q[0] >= p[0] - 0.1 - 1e-15 && q[0] < p[0] + 0.1 + 1e-15) : q[0] == p[0];
        const bool in_y = d.include_position ? (q[1] >= p[1] - 0.1 - 1e-15 && q[1] < p[1] + 0.1 + 1e-15) : q[1] == p[1];
        const bool in_w = d.include_rotation ? (q[3] >= -d.rotation_minus && q[3] < 2.0 - d.rotation_minus) : q[3] == p[3];
        if (!in_x || !in_y || !in_w || q[2] != p[2] || q[4] != p[4] || q[5] != p[5] || q[6] != p[6]) ++bad;
        for (int k = 0; k < 7; ++k) sum += q[k];
      }
  // the refusals: every one leaves the output alone
  rcsh_autoreset_desc d;
  std::memset(&d, 0, sizeof(d));
  double q[7] = {7, 7, 7, 7, 7, 7, 7};
  bad += rcsh_autoreset_draw(nullptr, 0, 0, q) != RCSH_ERR_ARG;
  bad += rcsh_autoreset_draw(&d, -1, 0, q) != RCSH_ERR_ARG;
  bad += rcsh_autoreset_draw(&d, 0, -1, q) != RCSH_ERR_ARG;
  bad += rcsh_autoreset_draw(&d, int64_t(1) << 32, 0, q) != RCSH_ERR_ARG;
  bad += rcsh_autoreset_draw(&d, 0, 0, nullptr) != RCSH_ERR_ARG;
  d.env_offset = -1;
  bad += rcsh_autoreset_draw(&d, 0, 0, q) != RCSH_ERR_ARG;
  for (int k = 0; k < 7; ++k) bad += q[k] != 7;
  std::printf("%ld draws, checksum %.17g, %ld failures\n", draws, sum, bad);
  return bad ? 1 : 0;
}
