// pgtg_cost.h -- the safety cost of a device-resident rollout (include/pgtg.h pgtg_cost_scan): the
// info["cost"] channel of separate_reward_cost (pgtg/environment.py:1130-1276) summed per episode, the
// Lagrangian penalty r - lambda * c on the reward (RCPO, Tessler et al. 2018) and the dual ascent of the
// multiplier on the mean episode cost against a budget, as one forward scan and a one-workgroup finish.
// Included by pgtg_env.hip (device code only).
#ifndef PGTG_COST_H_
#define PGTG_COST_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pgtg.h"

namespace pgtg {

// Per env e, lam = *lambda (read once, before anything is written), acc = ep_cost[e], rows t = 0 .. T-1,
// no fused multiply-add:
//   penalised[t][e] = rewards[t][e] - lam * costs[t][e]            (float32: the product rounds, then the difference)
//   acc += (double)costs[t][e]
//   dones[t+1][e]:  s += acc;  k += 1;  m = max(m, acc);  acc = 0   (fp64; s = 0, k = 0, m = -inf at the start)
// and ep_cost[e] = acc at the end.  One lane per env: every access of a row is 64 consecutive values per
// wave, 4 + 4 + 1 bytes read and 4 written per sample.
constexpr int kCostBlock = 256;
// Rows whose loads are in flight ahead of the row being consumed, as k_gae's kGaeAhead and for its reason
// (pgtg_rollout.h): no load depends on the lane's chain, and at 65 536 envs there is one wave per SIMD, so
// nothing else hides T memory round trips.  A row is three loads and one store on the wave's in-order memory
// counter (63 at most): eight rows ahead keep 4 x 7 = 28 operations younger than the row being waited for.
constexpr int kCostAhead = 8;

struct CostPartial {
  double s;    // sum of the finished episodes' costs
  uint64_t k;  // finished episodes
  double m;    // the largest of them (-inf: none)
};

__device__ __forceinline__ void cost_merge(CostPartial& a, const CostPartial& b) {
  a.s = a.s + b.s;
  a.k += b.k;
  a.m = fmax(a.m, b.m);
}

// The workgroup's 256 lane values into thread 0's, in one order: each wave by a shuffle tree (lane 0 ends
// with (((v0 + v32) + (v16 + v48)) + ...), then the four waves in wave order through LDS -- k_eval's
// pattern (pgtg_eval.h eval_block_reduce).  Every lane of the workgroup calls it.
__device__ __forceinline__ void cost_block_reduce(CostPartial& p, CostPartial* part) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    CostPartial q;
    q.s = __shfl_down(p.s, o);
    q.k = __shfl_down((unsigned long long)p.k, o);
    q.m = __shfl_down(p.m, o);
    cost_merge(p, q);
  }
  if ((t & 63) == 0) part[t >> 6] = p;
  __syncthreads();
  if (t == 0) {
    p = part[0];
    for (int w = 1; w < kCostBlock / 64; w++) cost_merge(p, part[w]);
  }
}

struct CostArgs {
  const float* rew;
  const float* cost;
  const uint8_t* dones;  // [T + 1][N]
  double* ep_cost;
  float* pen;
  float* lambda;
  PgtgCostSummary* summary;
  CostPartial* rows;  // [ceil(N / 256)] per-workgroup partials (the caller's workspace)
  uint64_t n, steps, n_rows;
  double cost_limit, lambda_lr, lambda_max;
};

// Grid ceil(N / 256) whatever the device: workgroup b covers envs [256 b, 256 b + 256), so the partition,
// and with it the order of every fp64 sum, is a function of N alone.  A lane past the last env reads the
// last env's column (in bounds), stores nothing and adds the identity: no lane leaves before the barrier.
__global__ void __launch_bounds__(kCostBlock) k_cost_scan(CostArgs a) {
  constexpr int P = kCostAhead;
  __shared__ CostPartial part[kCostBlock / 64];
  const uint32_t T = (uint32_t)a.steps;  // (< 2^31: pgtg_cost_scan)
  const uint64_t n = a.n;
  const uint64_t e = (uint64_t)blockIdx.x * kCostBlock + (uint64_t)threadIdx.x;
  const bool live = e < n;
  const uint64_t col = live ? e : n - 1;
  const float lam = *a.lambda;  // (uniform: one scalar load)
  // Ring slots are compile-time constants.  A step past the end loads row T - 1 again (in bounds, never
  // consumed): the cursors stop there, so no load sits behind a branch.
  float R[P], Cs[P];
  uint8_t D[P];
  const float* rew = a.rew + col;          // row of step j + P
  const float* cst = a.cost + col;
  const uint8_t* dn = a.dones + n + col;   // dones row t + 1
  float* pen = a.pen + col;                // row of step j
  double acc = a.ep_cost[col];             // (the oldest load: the loop's first sum must not wait for the ring)
#pragma unroll
  for (int k = 0; k < P; k++) {
    R[k] = *rew;
    Cs[k] = *cst;
    D[k] = *dn;
    if ((uint32_t)k + 1 < T) rew += n, cst += n, dn += n;
  }
  CostPartial p = {0.0, 0, -INFINITY};
  // One group of P steps from step j0.  Steady: every step up to j0 + 2 P exists, so nothing is guarded and
  // every cursor moves -- the group's last move leaves the cursors on step j0 + 2 P, a row of the rollout.
  auto group = [&](uint32_t j0, auto steady) {
    constexpr bool S = decltype(steady)::value;
#pragma unroll
    for (int k = 0; k < P; k++) {
      const uint32_t j = j0 + (uint32_t)k;
      const float c = Cs[k];
      const float out = R[k] - lam * c;
      if (S || j < T) {
        if (live) *pen = out;
        acc = acc + (double)c;
        if (D[k] != 0) {  // (selects)
          p.s = p.s + acc;
          p.k += 1;
          p.m = fmax(p.m, acc);
          acc = 0.0;
        }
      }
      pen += n;  // (past step T - 1 the store cursor is not used again)
      // the row of step j + P into the slot just read
      R[k] = *rew;
      Cs[k] = *cst;
      D[k] = *dn;
      if (S || j + P + 1 < T) rew += n, cst += n, dn += n;
      // (steps stay in program order: moved together by the scheduler, their waits would drain the ring)
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  uint32_t j0 = 0;
  for (; (uint64_t)j0 + 2 * P < T; j0 += P) group(j0, std::true_type{});
  for (; j0 < T; j0 += P) group(j0, std::false_type{});  // the last groups: cursors stop at row T - 1, steps guarded
  if (live) a.ep_cost[e] = acc;
  else p = {0.0, 0, -INFINITY};
  cost_block_reduce(p, part);
  if (threadIdx.x == 0) a.rows[blockIdx.x] = p;
}

// One workgroup, launched after k_cost_scan on the same stream: lane t merges rows t, t + 256, ... in that
// order, the workgroup reduces as above, and thread 0 writes the summary and, with at least one finished
// episode, the multiplier's dual ascent in fp64:
//   mean = sum / episodes;  l = (double)lambda + lambda_lr * (mean - cost_limit);  l = min(max(l, 0), lambda_max)
// Rollout k is therefore penalised with the multiplier rollouts 0 .. k-1 produced, and no kernel reads a
// word written in its own launch.
__global__ void __launch_bounds__(kCostBlock) k_cost_dual(CostArgs a) {
  __shared__ CostPartial part[kCostBlock / 64];
  CostPartial p = {0.0, 0, -INFINITY};
  for (uint64_t r = threadIdx.x; r < a.n_rows; r += kCostBlock) cost_merge(p, a.rows[r]);
  cost_block_reduce(p, part);
  if (threadIdx.x != 0) return;
  const float lam = *a.lambda;
  float next = lam;
  double mean = 0.0;
  if (p.k) {
    mean = p.s / (double)p.k;
    double l = (double)lam + a.lambda_lr * (mean - a.cost_limit);
    l = l < 0.0 ? 0.0 : l;
    l = l > a.lambda_max ? a.lambda_max : l;
    next = (float)l;
    *a.lambda = next;
  }
  PgtgCostSummary* s = a.summary;
  s->episodes = p.k;
  s->cost_sum = p.s;
  s->cost_mean = mean;
  s->cost_max = p.k ? p.m : 0.0;
  s->lambda_before = lam;
  s->lambda_after = next;
}

}  // namespace pgtg
#endif  // PGTG_COST_H_
