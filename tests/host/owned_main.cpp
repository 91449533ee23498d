// The owner of csrc/owned.h with a counting release function: what is released, how often, and when.  Stand-alone; built with the host
// compiler and its address and undefined-behaviour sanitizers by tests/test_owned_cpu.py.  Exit status 0 and "ok" on the last line:
// every check held.
#include <cstdio>
#include <utility>
#include <vector>

#include "owned.h"

namespace {

std::vector<int> g_released;  // every resource handed to the release function, in order
void count_release(int r) { g_released.push_back(r); }
using Res = rcsh::Owned<int, count_release>;  // a resource is a non-zero int; 0: none

int* g_freed = nullptr;  // the pointer form, over heap memory the address sanitizer watches: a double release or a leak fails the run
void free_ints(int* p) { g_freed = p; delete[] p; }
using Buf = rcsh::Owned<int*, free_ints>;

int g_failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

bool released_are(std::vector<int> want) {
  const bool same = g_released == want;
  g_released.clear();
  return same;
}

struct Group { Res a, b, c; };  // three resources that belong together (rcsh_sim::EscBufs, RenderBufs, Comm)
int g_fail_at = 0;              // the create call that fails (1-based); 0: none
int g_created = 0;
bool create(int id, int* out) {
  if (++g_created == g_fail_at) return false;
  *out = id;
  return true;
}
// an entry point that replaces a group: build in locals, commit after the last step that can fail
bool replace_group(Group& attached, int base) {
  g_created = 0;
  Group fresh;
  if (!create(base + 1, fresh.a.out())) return false;
  if (!create(base + 2, fresh.b.out())) return false;
  if (!create(base + 3, fresh.c.out())) return false;
  attached = std::move(fresh);
  return true;
}

}  // namespace

int main() {
  // an empty owner releases nothing: destroyed, reset, moved from, moved into another empty one
  {
    Res e;
    CHECK(!e && e.get() == 0);
    e.reset();
    Res f(std::move(e));
    Res g;
    g = std::move(f);
    CHECK(!e && !f && !g);
    CHECK(e.release() == 0);
  }
  CHECK(released_are({}));

  // destruction releases exactly once
  {
    Res a(7);
    CHECK(a && a.get() == 7);
    CHECK(released_are({}));
  }
  CHECK(released_are({7}));

  // move construction: the source is empty, nothing is released until the target goes
  {
    Res a(1);
    Res b(std::move(a));
    CHECK(!a && a.get() == 0 && b.get() == 1);
    CHECK(released_are({}));
  }
  CHECK(released_are({1}));

  // move assignment: the target's old resource is released exactly once, then and there; the source is empty
  {
    Res a(1), b(2);
    b = std::move(a);
    CHECK(released_are({2}));
    CHECK(!a && b.get() == 1);
    Res& self = b;
    b = std::move(self);  // (onto itself: nothing happens)
    CHECK(released_are({}) && b.get() == 1);
    Res empty;
    b = std::move(empty);  // an empty owner moved in releases what was held
    CHECK(released_are({1}) && !b);
  }
  CHECK(released_are({}));

  // reset(p) releases the old resource and holds the new one; reset() leaves it empty
  {
    Res a(3);
    a.reset(4);
    CHECK(released_are({3}) && a.get() == 4);
    a.reset();
    CHECK(released_are({4}) && !a);
    a.reset(5);
    CHECK(released_are({}) && a.get() == 5);
  }
  CHECK(released_are({5}));

  // release() hands the resource out and releases nothing, then or later
  {
    Res a(9);
    CHECK(a.release() == 9);
    CHECK(!a && a.get() == 0);
  }
  CHECK(released_are({}));

  // out(): the creating call's out-parameter -- what was held is released first; a call that writes nothing leaves the owner empty
  {
    Res a(11);
    *a.out() = 12;
    CHECK(released_are({11}) && a.get() == 12);
    (void)a.out();
    CHECK(released_are({12}) && !a);
  }
  CHECK(released_are({}));

  // a vector of owners (the profiling event rings): grown empty, filled, moved as a whole, every element released once
  {
    std::vector<Res> ring(4), attached;
    for (int i = 0; i < 4; ++i) *ring[i].out() = 20 + i;
    attached = std::move(ring);
    CHECK(released_are({}) && attached.size() == 4 && attached[3].get() == 23);
  }
  CHECK(released_are({20, 21, 22, 23}));

  // build a group of three in locals, fail at the third, return: the two that existed are released (in reverse), and the group
  // committed before is untouched
  {
    Group attached;
    g_fail_at = 0;
    CHECK(replace_group(attached, 100));
    CHECK(released_are({}));
    CHECK(attached.a.get() == 101 && attached.b.get() == 102 && attached.c.get() == 103);
    g_fail_at = 3;
    CHECK(!replace_group(attached, 200));
    CHECK(released_are({202, 201}));
    CHECK(attached.a.get() == 101 && attached.b.get() == 102 && attached.c.get() == 103);
    g_fail_at = 1;
    CHECK(!replace_group(attached, 300));
    CHECK(released_are({}));
    // ... and a replacement that succeeds releases the old group, each member once
    g_fail_at = 0;
    CHECK(replace_group(attached, 400));
    CHECK(released_are({101, 102, 103}));
    CHECK(attached.a.get() == 401 && attached.b.get() == 402 && attached.c.get() == 403);
  }
  CHECK(released_are({403, 402, 401}));  // members go in reverse order of declaration: what is declared first goes last

  // the pointer form over real heap memory
  {
    Buf a(new int[4]), b;
    int* p = a.get();
    p[3] = 1;
    b = std::move(a);
    CHECK(!a && b.get() == p && g_freed == nullptr);
    b.reset(new int[2]);
    CHECK(g_freed == p);
    int* q = b.release();
    CHECK(!b);
    delete[] q;
  }

  if (g_failures) return 1;
  std::printf("ok\n");
  return 0;
}
