// The verify launch of per-environment escalation (sim_kernels.h: RunOp::esc_role, RunOp::esc_part == 2).
//
// The lean launch of a step steps EVERY environment and records the joint positions every substep began on (RunOp::trace).  An
// environment it cannot certify is in esc[1].  Whether substep k of such an environment is in contact depends on q_k alone
// (contact_collide reads the joint positions and the tables), and while no substep is, the lean launch's trajectory IS the
// contact-resolving kernel's: so the collision passes of one environment's substeps do not wait for each other.  One 64-lane
// workgroup takes one (substep, environment) item at a time -- items are numbered through esc[1]'s population by rank, as esc_select
// ranks -- and a pass that finds a contact of the robot's geoms puts the environment into esc[3] ("touch"): the set the
// contact-resolving launch redoes from the copy.  No workgroup waits for another one.  (More environments marked than
// kVerifyMaxFlagged: nobody is verified, all of them are redone.)
#pragma once

#include "sim_kernels.h"

namespace rcsh {

#if defined(__HIP__)

// the r-th set bit of the mask row `W` (nw words), or -1; every lane of the wavefront calls this
__device__ __forceinline__ int mask_select_rank(const uint64_t* W, int nw, int n, int r) {
  const int lane = (int)(threadIdx.x & 63u);
  int base = 0;
  for (int c0 = 0; c0 < nw; c0 += 64) {
    const int wi = c0 + lane;
    uint64_t w = 0;
    if (wi < nw) {
      const uint64_t valid = (wi == nw - 1 && (n & 63)) ? ((1ull << (n & 63)) - 1) : ~0ull;
      w = W[wi] & valid;
    }
    const int pc = __popcll(w);
    const int incl = wave_incl_scan(pc);
    const int total = __builtin_amdgcn_readlane(incl, 63);
    const int rk = r - base;
    if (rk < total) {  // (wave-uniform)
      const int L = __ffsll((long long)__ballot(incl > rk)) - 1;
      const int excl = __builtin_amdgcn_readlane(incl, L) - __builtin_amdgcn_readlane(pc, L);
      uint64_t wl = wave_read_u64(w, L);
      for (int q = rk - excl; q > 0; --q) wl &= wl - 1;
      return (c0 + L) * 64 + (__ffsll((long long)wl) - 1);
    }
    base += total;
  }
  return -1;
}

// workgroups of the verify launch: one per SIMD of the chip -- the kernel's registers allow one wavefront
// per SIMD; the empty launch of a step in which nobody failed the certificate measured the same with 256 and with 1024
constexpr int kVerifyGrid = 1024;
// Verification pays while the step waits for a FEW environments: their substeps' passes run side by side instead of one behind the
// other.  With more environments marked than this (RCSH_VERIFY_MAX, read on every launch) the contact-resolving launch fills the chip
// anyway and those that touch nothing finish in the shadow of those that do: the verify launch then hands every marked environment
// on unverified -- each is redone from the copy, as the two-launch step redoes a newly marked one (the 1000-step rollout ends with
// ~1000 marked; verifying them all cost it 10 % with 1024 workgroups, 21 % with 256: profiles/substep_verify/bench.txt).
// The figure is a quarter of the contact-resolving launch's workgroups at the headline batch (4096 environments: 1024 workgroups, one
// marked environment each) and rests on that one rollout; it is an absolute count, not derived from n or the grid.  Either side of
// it the results are the same -- whoever is handed on is redone from the copy --, only the time differs.
constexpr int kVerifyMaxFlagged = 256;

// grid: any (a stride loop over the items); block: 64.  nsub: substeps of the lean launch (rows of the trace that are valid).
template <class T>
__global__ void __launch_bounds__(64) k_verify_team(Params Pk, RunOp opk, int nsub, int max_flagged) {
  if (opk.esc_ctr[2] == 0) return;  // nobody failed the certificate in this step: one scalar load
  using ST = StageTeam<T>;
  using Arena = ContactArena<T, kMaxConNoBox>;
  __shared__ Params lp;
  __shared__ LinkRec llinks[T::NL];
  __shared__ BoxTaskCfg lbt[1];
  __shared__ __attribute__((aligned(16))) double lst[ST::COUNT];
  __shared__ double lbox[kBoxState + 1];
  __shared__ Arena larena[1];
  static_assert(sizeof(Params) % 8 == 0 && sizeof(LinkRec) % 8 == 0 && sizeof(BoxTaskCfg) % 8 == 0 && sizeof(Arena) % 8 == 0, "copied in 8-byte words");
  const int lane = (int)threadIdx.x;
  const int nw = (Pk.n + 63) >> 6;
  const uint64_t* fail_row = opk.esc + nw;
  const int nflag = (int)opk.esc_ctr[2];
  const int nitem = nflag * nsub;
  if (nflag > max_flagged) {
    for (int wi = (int)blockIdx.x * 64 + lane; wi < nw; wi += (int)gridDim.x * 64) {
      const uint64_t w = fail_row[wi];
      if (w) {
        const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(opk.esc + 3 * nw + wi), (unsigned long long)w);
        atomicAdd(opk.esc_ctr + 3, (uint32_t)__popcll(w & ~old));
      }
    }
    return;
  }
  if ((int)blockIdx.x >= nitem) return;
  {
    // tables, link records and the phantom box, as the contact-resolving kernel's prologue stages them
    LdsCopy<sizeof(Params) / 8> cp_params;
    LdsCopy<sizeof(LinkRec) * T::NL / 8> cp_links;
    LdsCopy<sizeof(BoxTaskCfg) / 8> cp_bt;
    cp_params.load(&Pk);
    cp_links.load(reinterpret_cast<const char*>(Pk.model) + sizeof(DevModel));
    cp_bt.load(Pk.boxtask);
    cp_params.store(&lp);
    cp_links.store(&llinks[0]);
    cp_bt.store(&lbt[0]);
    for (int k = lane; k < ST::COUNT; k += 64) lst[k] = 0.0;
    double* az = reinterpret_cast<double*>(&larena[0]);
    for (int k = lane; k < (int)(sizeof(Arena) / 8); k += 64) az[k] = 0.0;
    __syncthreads();
    // no record of remaining gaps: every pair is looked at, nothing is shared between items, frames come from the pass's own kinematics
    if (lane == 0) lp.chk.slack = nullptr;
    for (int k = lane; k < kBoxState + 1; k += 64)
      lbox[k] = k < 7 ? lbt[0].box.qpos0[k] : (k >= kBoxPre && k < kBoxPre + 7 ? lbt[0].box.qpos0[k - kBoxPre] : 0.0);
    __syncthreads();
  }
  const ST st{lst};
  for (int item = (int)blockIdx.x; item < nitem; item += (int)gridDim.x) {
    // (substep-major: the first substeps of all environments go first, and an environment that begins its launch in contact is known
    // to touch before its later substeps come up)
    const int k = item / nflag, r = item - k * nflag;
    const int e = mask_select_rank(fail_row, nw, Pk.n, r);
    if (e < 0) continue;  // (wave-uniform)
    // already known to touch: nothing left to find out
    if ((__hip_atomic_load(opk.esc + 3 * nw + (e >> 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (e & 63)) & 1ull) continue;
    if (lane < T::NL) st.q(lane) = opk.trace[((size_t)k * T::NL + lane) * Pk.n + e];
    __syncthreads();
    const uint32_t res = contact_collide<T, Arena>(lp.ctab, lp.chk, lbt[0].box, llinks, st, lbox, larena[0], e, false);
    __syncthreads();
    if ((res & 1u) && lane == 0) {
      // (esc_ctr[3] counts the members of esc[3]: whoever sets an environment's bit first counts it)
      const uint64_t old = atomicOr(reinterpret_cast<unsigned long long*>(opk.esc + 3 * nw + (e >> 6)), 1ull << (e & 63));
      if (!((old >> (e & 63)) & 1ull)) atomicAdd(opk.esc_ctr + 3, 1u);
    }
  }
}

#endif

}  // namespace rcsh
