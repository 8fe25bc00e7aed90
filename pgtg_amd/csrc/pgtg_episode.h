// pgtg_episode.h -- episode returns and lengths on the device (include/pgtg.h pgtg_set_episode_stats):
// the VecMonitor wrapper of pgtg/train.py:55 for the whole batch, as a pass of its own after the step
// kernels.  Included by pgtg_env.hip (device code and its launch arguments only).
#ifndef PGTG_EPISODE_H_
#define PGTG_EPISODE_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/pgtg.h"

namespace pgtg {

// Per env e, from the outputs the step kernels just wrote (VecMonitor.step_wait):
//   ret[e] += (float)reward[e];  len[e] += 1;  ep_return[e] = ret[e];  ep_length[e] = len[e]
//   terminated[e] | truncated[e]:  (ret, len, truncated-only) joins the summary, ret[e] = len[e] = 0
// 8 + 1 + 1 bytes read, 8 read and 8 written for the accumulators, 8 written for the outputs: 34 B per
// env-step, every access coalesced (one lane per env, consecutive lanes consecutive envs).
struct EpisodeArgs {
  const double* rew;
  const uint8_t* term;
  const uint8_t* trunc;
  float* ret;    // the handle's accumulators
  int32_t* len;
  float* out_ret;  // the caller's [N] buffers
  int32_t* out_len;
  PgtgEpisodeSummary* rows;  // [gridDim.x] partial summaries, all-zero bytes = no episode yet
  uint64_t n;
};

constexpr int kEpisodeBlock = 256;

__device__ __forceinline__ void episode_merge(PgtgEpisodeSummary& a, const PgtgEpisodeSummary& b) {
  a.episodes += b.episodes;
  a.truncated_only += b.truncated_only;
  a.length_sum += b.length_sum;
  a.length_min = min(a.length_min, b.length_min);
  a.length_max = max(a.length_max, b.length_max);
  a.return_sum = a.return_sum + b.return_sum;
  a.return_min = fminf(a.return_min, b.return_min);
  a.return_max = fmaxf(a.return_max, b.return_max);
}

// Grid ceil(N / 256) whatever the device: workgroup b always covers envs [256 b, 256 b + 256), reduces
// its finished envs in a fixed order (lanes by a shuffle tree, then its four waves in wave order through
// LDS) and adds the result to its own row with ordinary loads and stores from lane 0 -- launches on one
// stream are ordered, so no atomic is needed, and the fp64 sum of a row has one order: the summary is
// reproducible bit for bit, which a floating-point atomic over the batch would not be.
__global__ void __launch_bounds__(kEpisodeBlock) k_episode(EpisodeArgs a) {
  __shared__ PgtgEpisodeSummary part[kEpisodeBlock / 64];
  const int t = threadIdx.x;
  const uint64_t e = (uint64_t)blockIdx.x * kEpisodeBlock + (uint64_t)t;
  bool done = false, tonly = false;
  float r = 0.f;
  int32_t l = 0;
  if (e < a.n) {
    const uint8_t te = a.term[e], tr = a.trunc[e];
    r = a.ret[e] + (float)a.rew[e];
    l = a.len[e] + 1;
    a.out_ret[e] = r;
    a.out_len[e] = l;
    done = (te | tr) != 0;
    tonly = tr != 0 && te == 0;
    a.ret[e] = done ? 0.f : r;
    a.len[e] = done ? 0 : l;
  }
  if (!__syncthreads_or(done ? 1 : 0)) return;  // (no episode ended in this workgroup: its row stays)
  uint32_t cnt = done ? 1u : 0u, tcnt = tonly ? 1u : 0u;
  unsigned long long ls = done ? (unsigned long long)(uint32_t)l : 0ull;
  int32_t lmin = done ? l : INT32_MAX, lmax = done ? l : 0;
  double rs = done ? (double)r : 0.0;
  float rmin = done ? r : INFINITY, rmax = done ? r : -INFINITY;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // lane 0 ends with ((((v0 + v32) + (v16 + v48)) + ...: one order
    cnt += __shfl_down(cnt, o);
    tcnt += __shfl_down(tcnt, o);
    ls += __shfl_down(ls, o);
    lmin = min(lmin, __shfl_down(lmin, o));
    lmax = max(lmax, __shfl_down(lmax, o));
    rs = rs + __shfl_down(rs, o);
    rmin = fminf(rmin, __shfl_down(rmin, o));
    rmax = fmaxf(rmax, __shfl_down(rmax, o));
  }
  if ((t & 63) == 0) {
    PgtgEpisodeSummary& p = part[t >> 6];
    p.episodes = cnt;
    p.truncated_only = tcnt;
    p.length_sum = ls;
    p.length_min = lmin;
    p.length_max = lmax;
    p.return_sum = rs;
    p.return_min = rmin;
    p.return_max = rmax;
  }
  __syncthreads();
  if (t == 0) {
    PgtgEpisodeSummary s = part[0];
    for (int w = 1; w < kEpisodeBlock / 64; w++) episode_merge(s, part[w]);
    PgtgEpisodeSummary row = a.rows[blockIdx.x];
    if (row.episodes == 0) {  // a zeroed row: the sentinels of an empty summary
      row.length_min = INT32_MAX;
      row.length_max = 0;
      row.return_min = INFINITY;
      row.return_max = -INFINITY;
    }
    episode_merge(row, s);
    a.rows[blockIdx.x] = row;
  }
}

// The accumulators of the envs a reset restarts (mask[e] != 0; NULL: all) go back to zero.
__global__ void __launch_bounds__(kEpisodeBlock) k_episode_zero(float* ret, int32_t* len, const uint8_t* mask, uint64_t n) {
  const uint64_t e = (uint64_t)blockIdx.x * kEpisodeBlock + (uint64_t)threadIdx.x;
  if (e < n && (!mask || mask[e])) {
    ret[e] = 0.f;
    len[e] = 0;
  }
}

}  // namespace pgtg
#endif  // PGTG_EPISODE_H_
