// pgtg_norm.h -- running return normalisation of the reward of a device-resident rollout (include/pgtg.h
// pgtg_reward_norm): the reward half of SB3's VecNormalize.  Per step the discounted return of every env, its
// batch moments over the envs, RunningMeanStd.update_from_moments on the running (mean, var, count), and the
// reward divided by sqrt(var + epsilon) and clipped -- a forward scan, a per-step merge, a one-lane walk and an
// elementwise pass.  Included by pgtg_env.hip (device code only).
#ifndef PGTG_NORM_H_
#define PGTG_NORM_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/pgtg.h"

namespace pgtg {

constexpr int kNormBlock = 256;
// Envs per partial: one wave.  The step's moments of a wave come out of a shuffle tree alone, so the scan has
// no barrier and no LDS; a workgroup-wide partial would put a barrier into every step.
constexpr int kNormPartial = 64;
// Rows whose loads are in flight ahead of the row being consumed, k_cost_scan's kCostAhead and for its reason
// (pgtg_cost.h): no load depends on the lane's chain, and at 65 536 envs there is one wave per SIMD.  A row is
// two loads; the group's kNormAhead partial stores (three each, lane 0) follow its last load.  The same number
// is the count of steps whose trees are reduced side by side: a tree is six dependent shuffle-and-merge
// levels, and only the other steps' trees fill the latency of each.
constexpr int kNormAhead = 8;
// Envs per workgroup of k_ret_apply: four columns a lane, 256 apart, of one row (one square root for four)
constexpr int kNormApplyCols = 4;

// Moments of a set of values: count, mean and the sum of squared deviations from it
struct RetPartial {
  double n, mean, m2;
};

// Chan, Golub, LeVeque: a then b.  An empty operand returns the other unchanged.
__device__ __forceinline__ RetPartial ret_merge(const RetPartial& a, const RetPartial& b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  RetPartial r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean;
  r.mean = a.mean + d * (b.n / r.n);
  r.m2 = a.m2 + b.m2 + d * d * (a.n * b.n / r.n);
  return r;
}

struct NormArgs {
  const float* rew;
  const uint8_t* dones;  // [T + 1][N]
  double* ret;           // [N] in/out
  double* rms;           // mean, var, count in/out
  double* row_var;       // [T]
  float* out;            // [T][N]
  RetPartial* rows;      // [T][n_part]: the waves' partials of every step
  RetPartial* batch;     // [T]: every step's moments over all envs
  uint64_t n, steps, n_part;
  double gamma, epsilon, clip;
  int training;
};

// Grid ceil(N / 256), workgroup b covering envs [256 b, 256 b + 256), wave w of it the 64 from 256 b + 64 w:
// the partition is a function of N alone.  Per env e, r = ret[e], t = 0 .. T-1, no fused multiply-add:
//   r = r * gamma + (double)rewards[t][e];   the wave's (n, mean, m2) of r -> rows[t][wave];   dones[t+1][e]: r = 0
// and ret[e] = r at the end.  The tree: leaves (1, r, 0), lane i merges lane i + o into itself for o = 32, 16,
// .. 1 (ret_merge), lane 0 stores.  The counts on the tree, and with them b.n / n and a.n * b.n / n of every
// merge, depend on the lane and N only: they are computed once, by the same divisions, ahead of the loop.
// A lane past the last env reads the last env's column (in bounds), is a leaf with n = 0 and stores nothing; a
// wave without a live lane stores no partial (rows has ceil(N / 64) columns).  There is no barrier to leave.
__global__ void __launch_bounds__(kNormBlock) k_ret_scan(NormArgs a) {
  constexpr int P = kNormAhead;
  const uint32_t T = (uint32_t)a.steps;  // (< 2^31: pgtg_reward_norm)
  const uint64_t n = a.n;
  const uint64_t e = (uint64_t)blockIdx.x * kNormBlock + (uint64_t)threadIdx.x;
  const bool live = e < n;
  const uint64_t col = live ? e : n - 1;
  const uint64_t wave = e / kNormPartial;
  const bool writer = (threadIdx.x & 63) == 0 && live;
  const double gamma = a.gamma;
  // the weights of the six merges this lane makes
  double w1[6], w2[6];
  uint64_t keep[6];  // all ones: the other operand is empty, this lane's moments stay as they are
  double cn = live ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const double nb = __shfl_down(cn, 32 >> k);
    const double nn = cn + nb;
    keep[k] = nb == 0.0 ? ~0ull : 0ull;  // (a live lane never merges into a dead one: the live lanes are the low ones)
    w1[k] = nb / nn;
    w2[k] = cn * nb / nn;
    cn = nn;
  }
  // a ? x : y on the bits (a is all ones or zero): a select the compiler cannot turn into a branch around the
  // merge -- eight trees advance together only while their levels stay in one block
  auto pick = [](uint64_t a, double x, double y) {
    return __longlong_as_double((long long)((__double_as_longlong(x) & a) | (__double_as_longlong(y) & ~a)));
  };
  // Ring slots are compile-time constants.  A step past the end loads row T - 1 again (in bounds, never
  // consumed): the cursors stop there, so no load sits behind a branch.
  float R[P];
  uint8_t D[P];
  const float* rew = a.rew + col;         // row of step j + P
  const uint8_t* dn = a.dones + n + col;  // dones row t + 1
  RetPartial* row = a.rows + wave;        // rows[j][wave]
  double r = a.ret[col];
#pragma unroll
  for (int k = 0; k < P; k++) {
    R[k] = *rew;
    D[k] = *dn;
    if ((uint32_t)k + 1 < T) rew += n, dn += n;
  }
  // One group of P steps from step j0.  Steady: every step up to j0 + 2 P exists, so nothing is guarded.
  auto group = [&](uint32_t j0, auto steady) {
    constexpr bool S = decltype(steady)::value;
    double mean[P], m2[P];
#pragma unroll
    for (int k = 0; k < P; k++) {
      const uint32_t j = j0 + (uint32_t)k;
      if (S || j < T) {
        r = r * gamma + (double)R[k];
        mean[k] = r;
        if (D[k] != 0) r = 0.0;  // (a select)
      } else {
        mean[k] = 0.0;
      }
      m2[k] = 0.0;
      // the row of step j + P into the slot just read
      R[k] = *rew;
      D[k] = *dn;
      if (S || j + P + 1 < T) rew += n, dn += n;
      // (steps stay in program order: moved together by the scheduler, their waits would drain the ring)
      __builtin_amdgcn_sched_barrier(0);
    }
    // the P trees level by level: P independent chains per level
#pragma unroll
    for (int l = 0; l < 6; l++) {
#pragma unroll
      for (int k = 0; k < P; k++) {
        const double mb = __shfl_down(mean[k], 32 >> l);
        const double sb = __shfl_down(m2[k], 32 >> l);
        const double d = mb - mean[k];
        const double nm = mean[k] + d * w1[l];
        const double ns = m2[k] + sb + d * d * w2[l];
        mean[k] = pick(keep[l], mean[k], nm);
        m2[k] = pick(keep[l], m2[k], ns);
      }
    }
#pragma unroll
    for (int k = 0; k < P; k++) {
      if (writer && (S || j0 + (uint32_t)k < T)) *row = RetPartial{cn, mean[k], m2[k]};
      row += a.n_part;  // (past step T - 1 the store cursor is not used again)
    }
  };
  uint32_t j0 = 0;
  for (; (uint64_t)j0 + 2 * P < T; j0 += P) group(j0, std::true_type{});
  for (; j0 < T; j0 += P) group(j0, std::false_type{});  // the last groups: cursors stop at row T - 1, steps guarded
  if (live) a.ret[e] = r;
}

// The 256 lane values into thread 0's, in one order: each wave by the shuffle tree (lane i merges lane i + o,
// o = 32 .. 1), then the four waves in wave order through LDS -- cost_block_reduce's pattern.  Every lane of the
// workgroup calls it.
__device__ __forceinline__ void ret_block_reduce(RetPartial& p, RetPartial* part) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    RetPartial q;
    q.n = __shfl_down(p.n, o);
    q.mean = __shfl_down(p.mean, o);
    q.m2 = __shfl_down(p.m2, o);
    p = ret_merge(p, q);
  }
  if ((t & 63) == 0) part[t >> 6] = p;
  __syncthreads();
  if (t == 0) {
    p = part[0];
    for (int w = 1; w < kNormBlock / 64; w++) p = ret_merge(p, part[w]);
  }
}

// Launched twice behind k_ret_scan on the same stream, so that no launch reads a word it wrote.
// Walk = false, grid T: workgroup t merges the partials of step t -- lane l takes partials l, l + 256, ... in that
// order, then ret_block_reduce -- into batch[t].  The order is a function of N alone.
// Walk = true, one workgroup: the steps in chunks of 256 through LDS (loaded and stored by all lanes, coalesced),
// thread 0 walking them in order with RunningMeanStd.update_from_moments, in fp64 and as SB3 writes it:
//   vb = m2 / nb;  delta = mb - mean;  tot = count + nb
//   mean' = mean + delta * nb / tot
//   var'  = (var * count + vb * nb + delta * delta * count * nb / tot) / tot;   count' = tot
// row_var[t] = var', and (mean, var, count) go back into rms after the last step.
template <bool Walk>
__global__ void __launch_bounds__(kNormBlock) k_ret_stats(NormArgs a) {
  if constexpr (!Walk) {
    __shared__ RetPartial part[kNormBlock / 64];
    const RetPartial* rows = a.rows + (uint64_t)blockIdx.x * a.n_part;
    RetPartial p = {0.0, 0.0, 0.0};
    for (uint64_t i = threadIdx.x; i < a.n_part; i += kNormBlock) p = ret_merge(p, rows[i]);
    ret_block_reduce(p, part);
    if (threadIdx.x == 0) a.batch[blockIdx.x] = p;
  } else {
    __shared__ RetPartial in[kNormBlock];
    __shared__ double out[kNormBlock];
    double mean = 0.0, var = 0.0, count = 0.0;
    if (threadIdx.x == 0) mean = a.rms[0], var = a.rms[1], count = a.rms[2];
    for (uint64_t t0 = 0; t0 < a.steps; t0 += kNormBlock) {
      const uint64_t m = a.steps - t0 < (uint64_t)kNormBlock ? a.steps - t0 : (uint64_t)kNormBlock;
      if (threadIdx.x < m) in[threadIdx.x] = a.batch[t0 + threadIdx.x];
      __syncthreads();
      if (threadIdx.x == 0) {
        for (uint32_t i = 0; i < (uint32_t)m; i++) {
          const double nb = in[i].n, mb = in[i].mean;
          const double vb = in[i].m2 / nb;
          const double delta = mb - mean;
          const double tot = count + nb;
          const double next = mean + delta * nb / tot;
          var = (var * count + vb * nb + delta * delta * count * nb / tot) / tot;
          mean = next;
          count = tot;
          out[i] = var;
        }
      }
      __syncthreads();
      if (threadIdx.x < m) a.row_var[t0 + threadIdx.x] = out[threadIdx.x];
    }
    if (threadIdx.x == 0) a.rms[0] = mean, a.rms[1] = var, a.rms[2] = count;
  }
}

// normalised[t][e] = (float)clip((double)rewards[t][e] / sqrt(var_t + epsilon), -clip, +clip) in fp64, var_t =
// row_var[t] when training and the stored rms[1] otherwise.  Grid (ceil(N / 1024), min(T, 65535)): a lane takes
// the columns x, x + 256, x + 512, x + 768 of the rows y, y + gridDim.y, ...
__global__ void __launch_bounds__(kNormBlock) k_ret_apply(NormArgs a) {
  constexpr int V = kNormApplyCols;
  const uint64_t n = a.n;
  const uint64_t e0 = (uint64_t)blockIdx.x * (kNormBlock * V) + (uint64_t)threadIdx.x;
  const double lo = -a.clip, hi = a.clip;
  for (uint64_t t = blockIdx.y; t < a.steps; t += gridDim.y) {
    const double var = a.training ? a.row_var[t] : a.rms[1];
    const double s = sqrt(var + a.epsilon);
    const float* __restrict__ src = a.rew + t * n;
    float* __restrict__ dst = a.out + t * n;
    float x[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
      const uint64_t e = e0 + (uint64_t)v * kNormBlock;
      x[v] = e < n ? src[e] : 0.0f;
    }
#pragma unroll
    for (int v = 0; v < V; v++) {
      const uint64_t e = e0 + (uint64_t)v * kNormBlock;
      double q = (double)x[v] / s;
      q = q < lo ? lo : q;
      q = q > hi ? hi : q;
      if (e < n) dst[e] = (float)q;
    }
  }
}

}  // namespace pgtg
#endif  // PGTG_NORM_H_
