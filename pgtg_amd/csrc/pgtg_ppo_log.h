// pgtg_ppo_log.h -- what is left of SB3's PPO.train around the minibatches (include/pgtg.h pgtg_ppo_expl_var,
// pgtg_ppo_log, pgtg_ppo_perm): the explained variance of the rollout's values, the train log reduced from the
// per-minibatch statistics, and the epoch's sample permutation.  No floating-point atomic: every sum runs in a
// fixed order over a partition that depends on the element count alone, in double.
//   k_ppo_expl_var<0>  per-workgroup partial sums of y = returns and of d = returns - values, to the workspace
//   k_ppo_expl_var<1>  every workgroup adds those partials in the same order (the two means), then its partial
//                      sums of (y - mean y)^2 and (d - mean d)^2
//   k_ppo_expl_var<2>  one workgroup: the tree over those, var d / var y and 1 - var d / var y as float32
//   k_ppo_log          one wave: a thread per logged mean, the rows of the [M][8] statistics in order
//   k_ppo_perm         one thread per element: a keyed Feistel bijection with cycle walking
// Included by pgtg_env.hip (device code only) after pgtg_ppo_step.h.
#ifndef PGTG_PPO_LOG_H_
#define PGTG_PPO_LOG_H_

#include "pgtg_ppo_step.h"

namespace pgtg {

constexpr int kEvThreads = 256;
constexpr int kEvMaxBlocks = 256;  // workgroups of the first two passes at most: the next pass adds one partial per thread
constexpr int kPermThreads = 256;
constexpr int kPermRounds = 6;
constexpr int kPermWalkCap = 64;   // Feistel applications per element at most (the domain is below 2 total: a
                                   // walk of k steps has probability below 2^-k)

// workgroups of the first two passes: a function of the element count alone
__host__ __device__ inline uint64_t ev_blocks(uint64_t n) {
  const uint64_t b = (n + (uint64_t)kEvThreads * kStepSets - 1) / ((uint64_t)kEvThreads * kStepSets);
  return b < 1 ? 1 : b < (uint64_t)kEvMaxBlocks ? b : (uint64_t)kEvMaxBlocks;
}

struct ExplVarArgs {
  const float *values, *returns;
  uint64_t n;
  double* ws;  // [4][kEvMaxBlocks]: sums of y, of d, of (y - mean)^2, of (d - mean)^2
  float* out;  // {1 - var d / var y, var d / var y}; NaN where var y == 0
};

template <int kPass>
__global__ void __launch_bounds__(kEvThreads) k_ppo_expl_var(ExplVarArgs a) {
  __shared__ double red[kEvMaxBlocks];
  static_assert(kEvMaxBlocks == kEvThreads, "one partial per thread");
  const uint32_t tid = threadIdx.x;
  const uint64_t n = a.n, blocks = ev_blocks(n);
  if (kPass == 2) {
    red[tid] = tid < blocks ? a.ws[2 * kEvMaxBlocks + tid] : 0.0;
    const double vy = step_tree<kEvMaxBlocks>(red, tid);
    __syncthreads();  // (every thread has read red[0])
    red[tid] = tid < blocks ? a.ws[3 * kEvMaxBlocks + tid] : 0.0;
    const double vd = step_tree<kEvMaxBlocks>(red, tid);
    if (tid == 0) {
      const double ratio = vy == 0.0 ? (double)NAN : vd / vy;  // (the two 1 / n cancel)
      a.out[0] = (float)(1.0 - ratio);
      a.out[1] = (float)ratio;
    }
    return;
  }
  double my = 0.0, md = 0.0;
  if (kPass == 1) {
    red[tid] = tid < blocks ? a.ws[tid] : 0.0;
    my = step_tree<kEvMaxBlocks>(red, tid) / (double)n;
    __syncthreads();
    red[tid] = tid < blocks ? a.ws[kEvMaxBlocks + tid] : 0.0;
    md = step_tree<kEvMaxBlocks>(red, tid) / (double)n;
    __syncthreads();
  }
  const uint64_t stride = blocks * kEvThreads;
  double sy[kStepSets] = {0.0, 0.0, 0.0, 0.0}, sd[kStepSets] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t i0 = (uint64_t)blockIdx.x * kEvThreads + tid; i0 < n; i0 += kStepSets * stride)
#pragma unroll
    for (int j = 0; j < kStepSets; j++) {
      const uint64_t i = i0 + j * stride;
      if (i < n) {
        const double y = a.returns[i], d = y - (double)a.values[i];
        if (kPass == 0) {
          sy[j] += y;
          sd[j] += d;
        } else {
          sy[j] += (y - my) * (y - my);
          sd[j] += (d - md) * (d - md);
        }
      }
    }
  red[tid] = (sy[0] + sy[1]) + (sy[2] + sy[3]);
  const double ty = step_tree<kEvThreads>(red, tid);
  __syncthreads();
  red[tid] = (sd[0] + sd[1]) + (sd[2] + sd[3]);
  const double td = step_tree<kEvThreads>(red, tid);
  if (tid == 0) {
    a.ws[(2 * kPass) * kEvMaxBlocks + blockIdx.x] = ty;
    a.ws[(2 * kPass + 1) * kEvMaxBlocks + blockIdx.x] = td;
  }
}

struct PpoLogArgs {
  const float* stats;       // [M][8]: k_ppo_reduce's rows
  uint64_t M, per_epoch;    // minibatches launched, minibatches per epoch
  const uint32_t* stop_at;  // the update's stop word or NULL
  const float* expl_var;    // k_ppo_expl_var's out or NULL
  PgtgPpoLog* out;
};

__global__ void __launch_bounds__(64) k_ppo_log(PpoLogArgs a) {
  const uint32_t tid = threadIdx.x;
  const uint32_t stop = a.stop_at ? *a.stop_at : 0;
  const uint64_t run = stop != 0 && stop < a.M ? stop : a.M;  // rows k_ppo_reduce wrote
  const uint64_t first = run ? (run - 1) / a.per_epoch * a.per_epoch : 0;  // the last run epoch's first row
  // thread: column of the statistics row, first row of its mean
  //   0 entropy loss, 1 policy loss, 2 value loss, 3 clip fraction over all rows run; 4 approx_kl over the last epoch
  if (tid < 5) {
    const int col = tid == 0 ? 3 : tid == 1 ? 1 : tid == 2 ? 2 : tid == 3 ? 5 : 4;
    const uint64_t lo = tid == 4 ? first : 0;
    double s = 0.0;
    for (uint64_t r = lo; r < run; r++) s += (double)a.stats[r * 8 + col];
    const float mean = run ? (float)(s / (double)(run - lo)) : NAN;
    float* dst = tid == 0 ? &a.out->entropy_loss : tid == 1 ? &a.out->policy_gradient_loss : tid == 2 ? &a.out->value_loss
                 : tid == 3 ? &a.out->clip_fraction : &a.out->approx_kl;
    *dst = mean;
  } else if (tid == 5) {
    a.out->minibatches = (uint32_t)run;
    a.out->epochs = run ? (uint32_t)((run - 1) / a.per_epoch + 1) : 0;
    a.out->early_stop = stop != 0 ? 1u : 0u;
    a.out->reserved = 0;
    a.out->loss = run ? a.stats[(run - 1) * 8] : NAN;
    a.out->explained_variance = a.expl_var ? a.expl_var[0] : NAN;
    a.out->variance_ratio = a.expl_var ? a.expl_var[1] : NAN;
  }
}

struct PermArgs {
  int64_t* perm;
  uint64_t total, key;  // key = seed ^ counter * golden ^ the domain constant
  uint32_t lo_bits, hi_bits;
  uint8_t* err;
  uint64_t err_n;
};

// policy_uniform's splitmix64 finaliser over (key, round, half)
__device__ __forceinline__ uint64_t perm_round(uint64_t key, uint64_t half, uint32_t rnd) {
  uint64_t z = key ^ (half * 0xD1B54A32D192ED03ull) ^ ((uint64_t)(rnd + 1) * 0xA0761D6478BD642Full);
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void __launch_bounds__(kPermThreads) k_ppo_perm(PermArgs a) {
  const uint64_t s = (uint64_t)blockIdx.x * kPermThreads + threadIdx.x;
  if (s >= a.total) return;
  const uint64_t mask_lo = (1ull << a.lo_bits) - 1, mask_hi = (1ull << a.hi_bits) - 1;  // (both below 32 bits)
  uint64_t x = s;
  int walk = 0;
  do {
    uint64_t lo = x & mask_lo, hi = x >> a.lo_bits;
#pragma unroll
    for (int r = 0; r < kPermRounds; r++) {
      if (r & 1) hi ^= perm_round(a.key, lo, r) & mask_hi;
      else lo ^= perm_round(a.key, hi, r) & mask_lo;
    }
    x = (hi << a.lo_bits) | lo;
    walk++;
  } while (x >= a.total && walk < kPermWalkCap);
  if (x >= a.total) {  // (the walk ran into its cap: flagged, and an index that is at least in range)
    if (a.err_n) a.err[s % a.err_n] = (uint8_t)(-PGTG_E_DEVICE);
    x = s;
  }
  a.perm[s] = (int64_t)x;
}

}  // namespace pgtg
#endif  // PGTG_PPO_LOG_H_
