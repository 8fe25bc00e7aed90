// pgtg_eval.h -- quota-aware policy evaluation on the device (include/pgtg.h pgtg_eval_step,
// pgtg_eval_summary): ModularEvaluator.evaluate of pgtg/evaluator.py:284-339 for the whole batch, with the
// per-env episode quotas of SB3's evaluate_policy, as a pass of its own after the step kernels.
// Included by pgtg_env.hip (device code and its launch arguments only).
#ifndef PGTG_EVAL_H_
#define PGTG_EVAL_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pgtg.h"

namespace pgtg {

constexpr int kEvalBlock = 256;

// Per env e with quota_e = (n_episodes + e) / N, at evaluation step s, from the outputs the step kernels
// just wrote (fp64, no fused multiply-add: every product and sum rounds as numpy's does):
//   cnt[e] < quota_e:  ret += r;  disc += r * g;  g *= gamma;  len += 1
//     terminated | truncated:  record[cnt[e]][e] = {ret, disc, len, r, s, flags};  cnt[e] += 1;
//                              ret = disc = 0;  g = 1;  len = 0
// 8 + 1 + 1 bytes of inputs and the 4 bytes of cnt read, 28 bytes of accumulators read and written (an env
// at its quota: cnt alone), a record row of 33 bytes and cnt written where an episode ends.  One lane per
// env, consecutive lanes consecutive envs: every access is coalesced, the record rows of the envs that
// finish their k-th episode in one step included ([Q][N], episode slot major).
__global__ void __launch_bounds__(kEvalBlock) k_eval(PgtgEval a) {
  __shared__ int32_t part[kEvalBlock / 64];
  const int t = threadIdx.x;
  const uint64_t e = (uint64_t)blockIdx.x * kEvalBlock + (uint64_t)t;
  int32_t open = 0;
  if (e < a.n) {
    const int64_t quota = (int64_t)((a.n_episodes + e) / a.n);
    int32_t k = a.cnt[e];
    if (k >= 0 && (int64_t)k < quota) {  // (a negative count, which the kernel never writes, is left alone)
      const double r = a.reward[e];
      const uint8_t te = a.terminated[e], tr = a.truncated[e];
      const double g = a.g[e];
      double ret = a.ret[e] + r;
      double disc = a.disc[e] + r * g;
      double gn = g * a.gamma;
      int32_t l = a.len[e] + 1;
      if ((te | tr) != 0) {
        const uint64_t row = (uint64_t)k * a.n + e;  // (k < quota <= Q: inside the [Q][N] arrays)
        a.rec_return[row] = ret;
        a.rec_discounted[row] = disc;
        a.rec_length[row] = l;
        a.rec_last_reward[row] = r;
        a.rec_end_step[row] = (int32_t)a.step;
        a.rec_flags[row] = (uint8_t)((te ? 1 : 0) | (tr ? 2 : 0));
        k += 1;
        a.cnt[e] = k;
        ret = 0.0;
        disc = 0.0;
        gn = 1.0;
        l = 0;
      }
      a.ret[e] = ret;
      a.disc[e] = disc;
      a.g[e] = gn;
      a.len[e] = l;
      open = (int64_t)k < quota ? 1 : 0;
    }
  }
  // the workgroup's envs still under quota: lanes by a shuffle tree, the four waves in wave order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) open += __shfl_down(open, o);
  if ((t & 63) == 0) part[t >> 6] = open;
  __syncthreads();
  if (t == 0) {
    int32_t s = part[0];
    for (int w = 1; w < kEvalBlock / 64; w++) s += part[w];
    a.open_rows[blockIdx.x] = s;
  }
}

// What one workgroup (and then the batch) knows of the recorded episodes.  Pass 0 fills everything but the
// squared deviations, pass 1 those alone, about the means pass 0's final stage left in the summary.
struct EvalPartial {
  uint64_t episodes, open_envs, terminated, truncated_only, lr_pos, lr_neg, neg_disc, length_sum;
  int32_t length_min, length_max;
  double ret_sum, disc_sum, ret_min, ret_max, ret_dev2, disc_dev2;
};

__device__ __forceinline__ void eval_identity(EvalPartial& p) {
  p.episodes = p.open_envs = p.terminated = p.truncated_only = p.lr_pos = p.lr_neg = p.neg_disc = p.length_sum = 0;
  p.length_min = INT32_MAX;
  p.length_max = 0;
  p.ret_sum = p.disc_sum = p.ret_dev2 = p.disc_dev2 = 0.0;
  p.ret_min = INFINITY;
  p.ret_max = -INFINITY;
}

__device__ __forceinline__ void eval_merge(EvalPartial& a, const EvalPartial& b) {
  a.episodes += b.episodes;
  a.open_envs += b.open_envs;
  a.terminated += b.terminated;
  a.truncated_only += b.truncated_only;
  a.lr_pos += b.lr_pos;
  a.lr_neg += b.lr_neg;
  a.neg_disc += b.neg_disc;
  a.length_sum += b.length_sum;
  a.length_min = min(a.length_min, b.length_min);
  a.length_max = max(a.length_max, b.length_max);
  a.ret_sum = a.ret_sum + b.ret_sum;
  a.disc_sum = a.disc_sum + b.disc_sum;
  a.ret_min = fmin(a.ret_min, b.ret_min);
  a.ret_max = fmax(a.ret_max, b.ret_max);
  a.ret_dev2 = a.ret_dev2 + b.ret_dev2;
  a.disc_dev2 = a.disc_dev2 + b.disc_dev2;
}

__device__ __forceinline__ EvalPartial eval_shfl_down(const EvalPartial& p, int o) {
  EvalPartial q;
  q.episodes = __shfl_down((unsigned long long)p.episodes, o);
  q.open_envs = __shfl_down((unsigned long long)p.open_envs, o);
  q.terminated = __shfl_down((unsigned long long)p.terminated, o);
  q.truncated_only = __shfl_down((unsigned long long)p.truncated_only, o);
  q.lr_pos = __shfl_down((unsigned long long)p.lr_pos, o);
  q.lr_neg = __shfl_down((unsigned long long)p.lr_neg, o);
  q.neg_disc = __shfl_down((unsigned long long)p.neg_disc, o);
  q.length_sum = __shfl_down((unsigned long long)p.length_sum, o);
  q.length_min = __shfl_down(p.length_min, o);
  q.length_max = __shfl_down(p.length_max, o);
  q.ret_sum = __shfl_down(p.ret_sum, o);
  q.disc_sum = __shfl_down(p.disc_sum, o);
  q.ret_min = __shfl_down(p.ret_min, o);
  q.ret_max = __shfl_down(p.ret_max, o);
  q.ret_dev2 = __shfl_down(p.ret_dev2, o);
  q.disc_dev2 = __shfl_down(p.disc_dev2, o);
  return q;
}

// The workgroup's 256 lane values into lane 0's, in one order: each wave by a shuffle tree (lane 0 ends
// with ((((v0 + v32) + (v16 + v48)) + ...), then the four waves in wave order through LDS.  Every lane of
// the workgroup calls it; the result is valid in thread 0.
__device__ __forceinline__ void eval_block_reduce(EvalPartial& p, EvalPartial* part) {
  const int t = threadIdx.x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const EvalPartial q = eval_shfl_down(p, o);
    eval_merge(p, q);
  }
  if ((t & 63) == 0) part[t >> 6] = p;
  __syncthreads();
  if (t == 0) {
    p = part[0];
    for (int w = 1; w < kEvalBlock / 64; w++) eval_merge(p, part[w]);
  }
}

struct EvalReduceArgs {
  PgtgEval ev;
  EvalPartial* rows;       // [ceil(N / 256)] per-workgroup partials (the caller's workspace)
  PgtgEvalSummary* out;    // device
  uint64_t n_rows;
  int32_t pass;            // 0: counts, sums, extrema;  1: squared deviations about out's means
};

// Stage 1, grid ceil(N / 256) whatever the device: workgroup b covers envs [256 b, 256 b + 256), each lane
// walks its env's records k = 0 .. cnt - 1 in slot order, then the workgroup reduces in eval_block_reduce's
// order into its own row.  The partition is a function of N alone, so the summary has one order of every
// fp64 sum: the same records give the same bits on any device.
__global__ void __launch_bounds__(kEvalBlock) k_eval_reduce(EvalReduceArgs a) {
  __shared__ EvalPartial part[kEvalBlock / 64];
  const uint64_t e = (uint64_t)blockIdx.x * kEvalBlock + (uint64_t)threadIdx.x;
  EvalPartial p;
  eval_identity(p);
  if (e < a.ev.n) {
    const int64_t quota = (int64_t)((a.ev.n_episodes + e) / a.ev.n);
    int64_t c = a.ev.cnt[e];
    c = c < 0 ? 0 : (c > quota ? quota : c);  // (a count the kernel never writes reads no row outside [Q][N])
    if (a.pass == 0) {
      p.open_envs = c < quota ? 1 : 0;
      for (int64_t k = 0; k < c; k++) {
        const uint64_t row = (uint64_t)k * a.ev.n + e;
        const double ret = a.ev.rec_return[row], disc = a.ev.rec_discounted[row], lr = a.ev.rec_last_reward[row];
        const int32_t l = a.ev.rec_length[row];
        const uint8_t f = a.ev.rec_flags[row];
        p.episodes += 1;
        p.terminated += (f & 1) ? 1 : 0;
        p.truncated_only += (f & 3) == 2 ? 1 : 0;
        p.lr_pos += lr > 0.0 ? 1 : 0;
        p.lr_neg += lr < 0.0 ? 1 : 0;
        p.neg_disc += disc < 0.0 ? 1 : 0;
        p.length_sum += (uint64_t)(uint32_t)l;
        p.length_min = min(p.length_min, l);
        p.length_max = max(p.length_max, l);
        p.ret_sum = p.ret_sum + ret;
        p.disc_sum = p.disc_sum + disc;
        p.ret_min = fmin(p.ret_min, ret);
        p.ret_max = fmax(p.ret_max, ret);
      }
    } else {
      const double rm = a.out->return_mean, dm = a.out->discounted_mean;
      for (int64_t k = 0; k < c; k++) {
        const uint64_t row = (uint64_t)k * a.ev.n + e;
        const double dr = a.ev.rec_return[row] - rm, dd = a.ev.rec_discounted[row] - dm;
        p.ret_dev2 = p.ret_dev2 + dr * dr;
        p.disc_dev2 = p.disc_dev2 + dd * dd;
      }
    }
  }
  eval_block_reduce(p, part);
  if (threadIdx.x == 0) a.rows[blockIdx.x] = p;
}

// Stage 2, one workgroup: lane t merges rows t, t + 256, ... in that order, the workgroup reduces as above,
// and thread 0 writes the summary (pass 0: everything but the stds, which it zeroes; pass 1: the stds).
__global__ void __launch_bounds__(kEvalBlock) k_eval_final(EvalReduceArgs a) {
  __shared__ EvalPartial part[kEvalBlock / 64];
  EvalPartial p;
  eval_identity(p);
  for (uint64_t r = threadIdx.x; r < a.n_rows; r += kEvalBlock) eval_merge(p, a.rows[r]);
  eval_block_reduce(p, part);
  if (threadIdx.x != 0) return;
  PgtgEvalSummary* s = a.out;
  if (a.pass == 0) {
    const double n = (double)p.episodes;
    s->episodes = p.episodes;
    s->open_envs = p.open_envs;
    s->terminated = p.terminated;
    s->truncated_only = p.truncated_only;
    s->last_reward_positive = p.lr_pos;
    s->last_reward_negative = p.lr_neg;
    s->negative_discounted = p.neg_disc;
    s->length_sum = p.length_sum;
    s->length_min = p.length_min;
    s->length_max = p.length_max;
    s->return_mean = p.episodes ? p.ret_sum / n : 0.0;
    s->return_std = 0.0;
    s->return_min = p.ret_min;
    s->return_max = p.ret_max;
    s->discounted_mean = p.episodes ? p.disc_sum / n : 0.0;
    s->discounted_std = 0.0;
  } else if (s->episodes) {
    const double n = (double)s->episodes;
    s->return_std = sqrt(p.ret_dev2 / n);
    s->discounted_std = sqrt(p.disc_dev2 / n);
  }
}

}  // namespace pgtg
#endif  // PGTG_EVAL_H_
