// The layout part of the host-pointer staging (csrc/host_stage.h) over the declaration lists of its eight call sites in
// csrc/rcs_hip.hip.  Stand-alone; built with the host compiler and its address and undefined-behaviour sanitizers by
// tests/test_host_stage_cpu.py.  Every layout is also laid over a heap block of exactly `total` bytes and every slice written through
// its view: a slice that overlaps a neighbour or runs past the total ends the run with a report.  Exit status 0 and "ok" on the last
// line: every check held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "host_stage.h"

namespace {

using rcsh::StageLayout;
using rcsh::StageRef;

int g_failures = 0;
#define CHECK(cond)                                                                                    \
  do {                                                                                                 \
    if (!(cond)) { std::printf("FAILED line %d (%s): %s\n", __LINE__, g_what, #cond); ++g_failures; }  \
  } while (0)
char g_what[128] = "";

enum Kind { kIn, kOut, kOutAlways, kOutFrom };  // kOutFrom: downloaded from a device array outside the staging
alignas(8) char g_outside[8];  // stands for that array
struct Decl {
  const char* name;
  Kind kind;
  size_t elem, count;  // element size in bytes, elements
  bool optional;       // the caller may pass null
};

// one declaration through the typed interface a call site uses; returns the slice's view in `base` (null before there is a base)
template <class T>
void* declare(StageLayout& L, const Decl& d, bool present, T* host, void* base, int slot) {
  if (!base && d.kind == kOutFrom) {
    L.out_from(present ? host : nullptr, reinterpret_cast<const T*>(g_outside), d.count);
    CHECK(L.count - 1 == slot);
    return nullptr;
  }
  if (!base) {
    const int got = d.kind == kIn ? L.in(static_cast<const T*>(present ? host : nullptr), d.count).slot
                  : d.kind == kOut ? L.out(present ? host : nullptr, d.count).slot
                                   : L.out_always(present ? host : nullptr, d.count).slot;
    CHECK(got == slot);
    return nullptr;
  }
  return d.kind == kIn ? const_cast<T*>(L.view(base, StageRef<const T>{slot})) : L.view(base, StageRef<T>{slot});
}
void* declare_sized(StageLayout& L, const Decl& d, bool present, void* host, void* base, int slot) {
  switch (d.elem) {
    case 1: return declare(L, d, present, static_cast<uint8_t*>(host), base, slot);
    case 2: return declare(L, d, present, static_cast<uint16_t*>(host), base, slot);
    case 4: return declare(L, d, present, static_cast<int32_t*>(host), base, slot);
    default: return declare(L, d, present, static_cast<double*>(host), base, slot);
  }
}

// one call site's list with the optional array `absent` (an index into it, -1: none) passed as null
void check_site(const char* site, size_t n, const std::vector<Decl>& decls, int absent) {
  std::snprintf(g_what, sizeof(g_what), "%s, n = %zu, absent = %s", site, n, absent < 0 ? "none" : decls[(size_t)absent].name);
  alignas(8) static char host[8];  // stands for every caller's array: the layout keeps the pointer and never follows it
  StageLayout L;
  for (size_t i = 0; i < decls.size(); ++i) declare_sized(L, decls[i], (int)i != absent, host, nullptr, (int)i);
  CHECK(L.count == (int)decls.size());
  size_t end = 0;
  for (size_t i = 0; i < decls.size(); ++i) {
    const Decl& d = decls[i];
    const StageLayout::Slice& e = L.slice[i];
    const bool present = (int)i != absent && d.count > 0;
    const bool staged = d.kind != kOutFrom && (present || (d.kind == kOutAlways && d.count > 0));
    // an absent array takes no bytes; an always-staged one takes its own; one read from outside has its download's size and no room
    CHECK(e.bytes == (staged || (d.kind == kOutFrom && present) ? d.elem * d.count : 0));
    CHECK(e.from == (d.kind == kOutFrom && present ? g_outside : nullptr));
    if (staged) {
      CHECK(e.at % 8 == 0);
      CHECK(e.at >= end);             // declaration order, and disjoint from everything before it
      CHECK(e.at < end + 8);          // no more than the alignment's padding between neighbours
      end = e.at + e.bytes;
    }
    CHECK(e.src == (d.kind == kIn && present ? host : nullptr));   // uploaded: the present inputs
    CHECK(e.dst == (d.kind != kIn && present ? host : nullptr));   // downloaded: the outputs asked for, always-staged or not
  }
  CHECK(L.total >= end && L.total < end + 8 && L.total % 8 == 0);  // the total is the (padded) end of the last slice
  // over a block of exactly `total` bytes: fill every slice with its number, then read them all back
  std::unique_ptr<char[]> block(new char[L.total]);
  for (size_t i = 0; i < decls.size(); ++i) {
    void* v = declare_sized(L, decls[i], true, host, block.get(), (int)i);
    CHECK((v != nullptr) == (L.slice[i].bytes != 0 && !L.slice[i].from));
    if (v) {
      CHECK(v == block.get() + L.slice[i].at);
      std::memset(v, (int)i + 1, L.slice[i].bytes);
    }
  }
  for (size_t i = 0; i < decls.size(); ++i)
    for (size_t b = 0; b < (L.slice[i].from ? 0 : L.slice[i].bytes); ++b)
      if (block[L.slice[i].at + b] != (char)(i + 1)) { CHECK(!"a slice was overwritten by a neighbour"); break; }
}

void check_all(size_t n) {
  const size_t nl = 9, narm = 7, npair = 37, px = n * 5 * 3;  // links, arm joints, masked pairs, pixels of a 5 x 3 camera
  const size_t pose = 7, wit = 6, pr = 2, jac = 6, campose = 12, rgb = 3;
  const struct { const char* site; std::vector<Decl> decls; } sites[] = {
      {"rcsh_collision_query",
       {{"q", kIn, 8, n * nl, false}, {"free_qpos", kIn, 8, n * pose, true}, {"hit", kOutAlways, 1, n, false},
        {"kinds_hit", kOutAlways, 1, n, true}, {"pair", kOutAlways, 4, n * pr, true}}},
      {"rcsh_motion_query",
       {{"q_from", kIn, 8, n * nl, false}, {"q_to", kIn, 8, n * nl, false}, {"free_qpos", kIn, 8, n * pose, true},
        {"result", kOut, 4, n, false}, {"t_contact", kOut, 8, n, false}}},
      {"clearance_host",
       {{"q", kIn, 8, n * nl, true}, {"free_qpos", kIn, 8, n * pose, true}, {"pair_mask", kIn, 1, npair, true},
        {"distance", kOutAlways, 8, n, false}, {"witness", kOutAlways, 8, n * wit, true}, {"grad", kOutAlways, 8, n * nl, true},
        {"pair", kOutAlways, 4, n * pr, true}, {"status", kOutAlways, 1, n, true}}},
      {"swept_host",
       {{"q_from", kIn, 8, n * nl, true}, {"q_to", kIn, 8, n * nl, false}, {"free_qpos", kIn, 8, n * pose, true},
        {"pair_mask", kIn, 1, npair, true}, {"distance", kOut, 8, n, false}, {"lower", kOut, 8, n, true}, {"s", kOut, 8, n, true},
        {"pair", kOut, 4, n * pr, true}, {"witness", kOut, 8, n * wit, true}, {"grad", kOut, 8, n * nl, true},
        {"evals", kOut, 4, n, true}, {"status", kOut, 1, n, true}}},
      {"dynamics_host",
       {{"q", kIn, 8, n * nl, true}, {"qvel", kIn, 8, n * nl, true}, {"qacc_in", kIn, 8, n * nl, true}, {"qfrc_in", kIn, 8, n * nl, true},
        {"qM", kOut, 8, n * nl * nl, true}, {"qfrc_bias", kOut, 8, n * nl, true}, {"gravity", kOut, 8, n * nl, true},
        {"qfrc_gravcomp", kOut, 8, n * nl, true}, {"jac", kOut, 8, n * jac * nl, true}, {"qfrc_inverse", kOut, 8, n * nl, true},
        {"qacc", kOut, 8, n * nl, true}}},
      {"rcsh_env_guard_peek",  // (its outputs come from the guard's scratch record)
       {{"action", kIn, 8, n * narm, false}, {"result", kOutFrom, 4, n, true}, {"t_contact", kOutFrom, 8, n, true},
        {"blocked", kOutFrom, 1, n, true}}},
      {"rcsh_env_guard_last",  // nothing staged: the last step's record is read where it lies
       {{"result", kOutFrom, 4, n, true}, {"t_contact", kOutFrom, 8, n, true}, {"blocked", kOutFrom, 1, n, true}}},
      {"rcsh_camera_render_rgb",
       {{"depth_gl", kOut, 4, px, true}, {"depth_mm", kOut, 2, px, true}, {"cam_pose", kOut, 8, n * campose, true},
        {"rgb", kOut, 1, rgb * px, true}}},
  };
  for (const auto& s : sites) {
    check_site(s.site, n, s.decls, -1);
    for (size_t i = 0; i < s.decls.size(); ++i)
      if (s.decls[i].optional) check_site(s.site, n, s.decls, (int)i);
  }
}

}  // namespace

int main() {
  for (size_t n : {1, 5, 67}) check_all(n);
  // an always-staged output with a null host pointer: a slice, a view, and no download
  {
    std::snprintf(g_what, sizeof(g_what), "always-staged, null host");
    StageLayout L;
    double d[5];
    const auto a = L.out(d, 5);
    const auto b = L.out_always(static_cast<uint8_t*>(nullptr), 5);
    const auto c = L.out(static_cast<int32_t*>(nullptr), 5);
    const auto e = L.out(d, 5);
    std::unique_ptr<char[]> block(new char[L.total]);
    CHECK(L.slice[b.slot].bytes == 5 && L.slice[b.slot].at == 40 && L.slice[b.slot].dst == nullptr);
    CHECK(L.view(block.get(), b) == reinterpret_cast<uint8_t*>(block.get() + 40));
    CHECK(L.slice[c.slot].bytes == 0 && L.view(block.get(), c) == nullptr);
    CHECK(L.slice[e.slot].at == 48 && L.total == 88);
    CHECK(L.view(block.get(), a) == reinterpret_cast<double*>(block.get()));
  }
  if (g_failures) { std::printf("%d checks failed\n", g_failures); return 1; }
  std::printf("ok\n");
  return 0;
}
