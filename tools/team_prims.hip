// team_prims.hip -- development check of the DPP / bpermute semantics team.h relies on, plus their cost.
#include <hip/hip_runtime.h>
#include <cstdio>
#include "../robot-control-stack_amd/csrc/team.h"
using namespace rcsh;
__global__ void k(double* out, long long* cyc) {
  const int l = threadIdx.x;
  const double x = 100.0 + l;
  out[0 * 64 + l] = row_up<1>(x);
  out[1 * 64 + l] = row_up<2>(x);
  out[2 * 64 + l] = row_down<1>(x);
  out[3 * 64 + l] = row_up_or<4>(-1.0, x);
  out[4 * 64 + l] = lane_get(x, (l & 48) + 6);
  out[5 * 64 + l] = (double)team_ballot((l & 15) < 3 || l == 63);
  // cost of a 12-double shift + add round
  double v[12];
  for (int k2 = 0; k2 < 12; ++k2) v[k2] = x * (k2 + 1);
  long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < 100; ++it) {
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) v[k2] += row_up<1>(v[k2]);
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) v[k2] += row_up<2>(v[k2]);
  }
  long long t1 = __builtin_readcyclecounter();
  double s = 0;
  for (int k2 = 0; k2 < 12; ++k2) s += v[k2];
  out[6 * 64 + l] = s;
  __shared__ double buf[64 * 12];
  long long t2 = __builtin_readcyclecounter();
  for (int it = 0; it < 100; ++it) {
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) buf[l * 12 + k2] = v[k2];
    __syncthreads();
#pragma unroll
    for (int k2 = 0; k2 < 12; ++k2) v[k2] += buf[((l + 63) & 63) * 12 + k2];
    __syncthreads();
  }
  long long t3 = __builtin_readcyclecounter();
  for (int k2 = 0; k2 < 12; ++k2) s += v[k2];
  out[7 * 64 + l] = s;
  if (l == 0) { cyc[0] = t1 - t0; cyc[1] = t3 - t2; }
}
// The step across the four DPP rows that a support scan over 32 or 64 lanes adds to the row rotations (contact_team.h: span_max): the
// largest of the rows' values in every lane, three ways.  Every row's lanes hold the row's value on entry.
__device__ inline double rows_max_readlane(double x) {
  const double r0 = wave_read(x, 0), r1 = wave_read(x, 16), r2 = wave_read(x, 32), r3 = wave_read(x, 48);
  return fmax(fmax(r0, r1), fmax(r2, r3));
}
__device__ inline double rows_max_bpermute(double x, int l) {
  x = fmax(x, lane_get(x, l ^ 16));
  return fmax(x, lane_get(x, l ^ 32));
}
__device__ inline double rows_max_swap(double x) {
#if __has_builtin(__builtin_amdgcn_permlane16_swap) && __has_builtin(__builtin_amdgcn_permlane32_swap)
  // (v_permlane16_swap: the odd rows of the first operand change places with the even rows of the second; v_permlane32_swap: the halves)
  auto lo = __builtin_amdgcn_permlane16_swap(lo32(x), lo32(x), false, false);
  auto hi = __builtin_amdgcn_permlane16_swap(hi32(x), hi32(x), false, false);
  x = fmax(mk64(hi[0], lo[0]), mk64(hi[1], lo[1]));
  lo = __builtin_amdgcn_permlane32_swap(lo32(x), lo32(x), false, false);
  hi = __builtin_amdgcn_permlane32_swap(hi32(x), hi32(x), false, false);
  return fmax(mk64(hi[0], lo[0]), mk64(hi[1], lo[1]));
#else
  return x;
#endif
}
__global__ void k_rows(double* out, long long* cyc) {
  const int l = threadIdx.x;
  const double x = 100.0 + (l >> 4) * ((l & 32) ? -3.0 : 5.0);  // rows hold 100, 105, 94, 91
  out[0 * 64 + l] = rows_max_readlane(x);
  out[1 * 64 + l] = rows_max_bpermute(x, l);
  out[2 * 64 + l] = rows_max_swap(x);
  double v = x;
  long long t[4];
  t[0] = __builtin_readcyclecounter();
  for (int it = 0; it < 256; ++it) v = rows_max_readlane(v + (double)(l >> 4)) - 1.0;
  t[1] = __builtin_readcyclecounter();
  for (int it = 0; it < 256; ++it) v = rows_max_bpermute(v + (double)(l >> 4), l) - 1.0;
  t[2] = __builtin_readcyclecounter();
  for (int it = 0; it < 256; ++it) v = rows_max_swap(v + (double)(l >> 4)) - 1.0;
  t[3] = __builtin_readcyclecounter();
  out[3 * 64 + l] = v;
  if (l == 0) for (int k2 = 0; k2 < 3; ++k2) cyc[k2] = t[k2 + 1] - t[k2];
}
int main() {
  {
    double* o2; long long* c2;
    hipMalloc(&o2, 4 * 64 * 8); hipMalloc(&c2, 64);
    k_rows<<<1, 64>>>(o2, c2);
    double h2[4 * 64]; long long hc2[3];
    hipMemcpy(h2, o2, sizeof(h2), hipMemcpyDeviceToHost); hipMemcpy(hc2, c2, sizeof(hc2), hipMemcpyDeviceToHost);
    const char* n2[3] = {"rows max, 4 x readlane", "rows max, 2 x bpermute", "rows max, permlane swaps"};
    for (int r = 0; r < 3; ++r) {
      printf("%-24s:", n2[r]);
      for (int l = 0; l < 64; l += 16) printf(" row %d %g", l / 16, h2[r * 64 + l]);
      printf("  -- %.1f cycles a step in a dependent chain (with one add and one subtraction)\n", hc2[r] / 256.0);
    }
    hipFree(o2); hipFree(c2);
  }
  double* out; long long* cyc;
  hipMalloc(&out, 8 * 64 * 8); hipMalloc(&cyc, 64);
  k<<<1, 64>>>(out, cyc);
  double h[8 * 64]; long long hc[2];
  hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost); hipMemcpy(hc, cyc, 16, hipMemcpyDeviceToHost);
  const char* names[6] = {"row_up<1>", "row_up<2>", "row_down<1>", "row_up_or<4>(-1)", "lane_get(team lane 6)", "team_ballot"};
  for (int r = 0; r < 6; ++r) { printf("%-22s:", names[r]); for (int l = 0; l < 20; ++l) printf(" %g", h[r * 64 + l]); printf(" ... l63 %g\n", h[r * 64 + 63]); }
  printf("24 x (2 dpp mov + add) : %.1f cycles per double-shift-add\n", hc[0] / 2400.0);
  printf("LDS exchange of 12 doubles (write, sync, read+add, sync): %.1f cycles per round\n", hc[1] / 100.0);
  return 0;
}
