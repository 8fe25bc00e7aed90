// pgtg_rollout.h -- generalised advantage estimation over a device-resident rollout (include/pgtg.h
// pgtg_gae): RolloutBuffer.compute_returns_and_advantage of the PPO the reference's caller trains
// (pgtg/train.py:61-74), with the time-limit bootstrap of its collect_rollouts, as one backward scan.
// Included by pgtg_env.hip (device code only).
#ifndef PGTG_ROLLOUT_H_
#define PGTG_ROLLOUT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pgtg.h"

namespace pgtg {

// Per env e, rows t = T-1 .. 0, last = 0, float32 throughout, no fused multiply-add:
//   r     = truncated_only[t][e] ? rewards[t][e] + g * terminal_values[t][e] : rewards[t][e]
//   nnt   = 1 - (dones[t+1][e] != 0);   nv = t == T-1 ? last_values[e] : values[t+1][e]
//   delta = (r + (g * nv) * nnt) - values[t][e];   last = delta + (gl * nnt) * last
//   advantages[t][e] = last;   returns[t][e] = last + values[t][e]
// One lane per env: every access of a row is 64 consecutive values per wave.  nv is the values entry the
// lane read one row earlier, so a row costs 4 + 4 + 1 + 1 bytes read and 4 + 4 written: 18 B per sample,
// plus 4 where truncated_only is set.
struct GaeArgs {
  const float* rew;
  const float* val;
  const uint8_t* dones;  // [T + 1][N]
  const uint8_t* tonly;
  const float* tval;
  const float* last_values;
  float* adv;
  float* ret;
  uint64_t n, steps;
  float g, gl;
};

// A lane's chain is four dependent float operations per row, but no load depends on it: the loads of
// kGaeAhead rows are in flight ahead of the row being consumed, or a launch would be T memory round
// trips long (65 536 envs are 1 024 waves, one per SIMD: nothing else hides the latency).  Only the
// terminal value's load depends on another load, the truncated-only flag's, so the flags run another
// kGaeAhead rows ahead and have arrived when their row's other loads are issued.  That load is a select
// of the address, not a branch: a lane whose flag is clear reads its own reward again (a line the wave
// is fetching anyway), so terminal_values is read only where the flag is set and the steady state has no
// divergent block -- behind one, the compiler's wait for a row drained the whole ring.  The depth is
// bounded by the wave's memory counter, which counts loads and stores in order up to 63: a row is five
// loads and two stores, so eight rows ahead keep about 50 operations outstanding and the wait for a
// row's loads still leaves the seven younger rows in flight; sixteen would not be expressible.
// Workgroups of one wave: there is no LDS and no barrier to share, the batch spreads over the most
// SIMDs, and a row's addresses are one scalar base per array plus the lane's offset -- rows may start at
// any 4-byte (flags: any byte) offset, every load being one dword or one byte per lane.
constexpr int kGaeBlock = 64;
constexpr int kGaeAhead = 8;

// The wave-uniform row cursors of a scan: step j = 0 .. T-1 is row T-1-j, every array moving back one
// row of n values per step (scalar arithmetic; a lane adds only its own offset).
struct GaeCursor {
  const float* rew;
  const float* val;
  const uint8_t* dn;  // dones row t + 1
  const float* tval;
  __device__ __forceinline__ void back(uint64_t n) {
    rew -= n;
    val -= n;
    dn -= n;
    tval -= n;
  }
};

template <bool BOOT>
__global__ void __launch_bounds__(kGaeBlock) k_gae(GaeArgs a) {
  constexpr int P = kGaeAhead;
  const uint32_t ln = threadIdx.x;
  const uint32_t T = (uint32_t)a.steps;  // (< 2^31: pgtg_gae)
  const uint64_t n = a.n;
  const uint64_t base = (uint64_t)blockIdx.x * kGaeBlock;
  if (base + ln >= n) return;
  const float g = a.g, gl = a.gl;
  // Ring slots are compile-time constants.  A step past the end loads row 0 again (in bounds, never
  // consumed): the cursors stop there, so no load sits behind a branch.
  float R[P], V[P], TV[P];
  uint8_t D[P], TO[2 * P];
  const uint64_t top = (uint64_t)(T - 1) * n + base;
  GaeCursor b = {a.rew + top, a.val + top, a.dones + top + n, a.tval + (BOOT ? top : 0)};  // row of step j + P
  const uint8_t* fl = a.tonly + (BOOT ? top : 0);                                           // flag row of step j + 2 P
  float* adv = a.adv + top;                                                                 // row of step j
  float* ret = a.ret + top;
  // (the oldest load, not the youngest: the loop's first use of nv must not wait for the whole ring)
  float nv = a.last_values[base + ln], last = 0.f;
#pragma unroll
  for (int k = 0; k < 2 * P; k++) {
    TO[k] = BOOT ? fl[ln] : (uint8_t)0;
    if ((uint32_t)k + 1 < T) fl -= n;
  }
#pragma unroll
  for (int k = 0; k < P; k++) {
    R[k] = b.rew[ln];
    V[k] = b.val[ln];
    D[k] = b.dn[ln];
    TV[k] = BOOT ? *(TO[k] ? b.tval + ln : b.rew + ln) : 0.f;
    if ((uint32_t)k + 1 < T) b.back(n);
  }
  // One group of 2 P steps from step j0.  Steady: every step up to j0 + 4 P exists, so nothing is guarded
  // and every cursor moves -- the group's last move leaves the flag cursor on step j0 + 4 P, which must be
  // a row of the rollout (with j0 + 4 P == T it would be the row in front of truncated_only, and the next
  // group would load from there).
  auto group = [&](uint32_t j0, auto steady) {
    constexpr bool S = decltype(steady)::value;
#pragma unroll
    for (int k = 0; k < 2 * P; k++) {
      const uint32_t j = j0 + (uint32_t)k;
      const int s = k % P;
      const float v = V[s];
      float r = R[s];
      if (BOOT && TO[k]) r = r + g * TV[s];  // (a select: a terminal value elsewhere never enters)
      const float nnt = 1.0f - (D[s] != 0 ? 1.0f : 0.0f);
      const float delta = (r + (g * nv) * nnt) - v;
      last = delta + (gl * nnt) * last;
      if (S || j < T) {
        adv[ln] = last;
        ret[ln] = last + v;
      }
      adv -= n;  // (past step T - 1 the store cursors are not used again)
      ret -= n;
      nv = v;
      // the row of step j + P into the slots just read, its flag having been loaded P steps ago; then
      // the flag of step j + 2 P
      R[s] = b.rew[ln];
      V[s] = b.val[ln];
      D[s] = b.dn[ln];
      if (BOOT) TV[s] = *(TO[(k + P) % (2 * P)] ? b.tval + ln : b.rew + ln);
      if (S || j + P + 1 < T) b.back(n);
      if (BOOT) {
        TO[k] = fl[ln];
        if (S || j + 2 * P + 1 < T) fl -= n;
      }
      // (steps stay in program order: moved together by the scheduler, their waits drained the ring)
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  uint32_t j0 = 0;
  for (; (uint64_t)j0 + 4 * P < T; j0 += 2 * P) group(j0, std::true_type{});
  for (; j0 < T; j0 += 2 * P) group(j0, std::false_type{});  // the last groups: cursors stop at row 0, stores guarded
}

}  // namespace pgtg
#endif  // PGTG_ROLLOUT_H_
