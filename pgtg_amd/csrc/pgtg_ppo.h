// pgtg_ppo.h -- one PPO minibatch of SB3's PPO.train (clip_range_vf optional) over a finished
// rollout's int8 rows: the loss, its six statistics and the gradient with respect to the twelve MlpPolicy
// tensors (include/pgtg.h pgtg_ppo_grad).  Three kernels and no floating-point atomic:
//   k_ppo_loss    64 samples per workgroup: gathers their rows, runs k_policy's forward and heads (the functions
//                 of pgtg_policy.h themselves: the log-probs a rollout stored are the ones recomputed here), the
//                 loss terms and the backward pass down to dZ1 [64][128]; writes dZ1 and the workgroup's partial
//                 sums of every gradient but W1's to its own workspace slot
//   k_ppo_dw1     dW1 [128][D] = dZ1^T X on v_mfma_f32_16x16x4_f32: a workgroup owns 128 observation columns
//                 and one segment of the batch, gathers the int8 rows again and converts them in registers
//   k_ppo_reduce  sums the slots and the segments in a fixed order into the twelve tensors and the statistics
// Included by pgtg_env.hip (device code only).
#ifndef PGTG_PPO_H_
#define PGTG_PPO_H_

#include "pgtg_policy.h"

namespace pgtg {

constexpr int kPpoRows = 64;       // samples per workgroup of k_ppo_loss and per stage of k_ppo_dw1
constexpr int kPpoThreads = 256;
constexpr int kPpoDTile = 128;     // observation columns per workgroup of k_ppo_dw1
constexpr int kPpoXPitch = kPpoDTile + 16;  // LDS bytes per staged row of k_ppo_dw1
constexpr int kPpoWant = 512;      // workgroups k_ppo_dw1 aims at (the split of the batch into segments)
constexpr int kPpoSets = 4;        // independent accumulators of a fixed-order reduction, added (0 + 1) + (2 + 3)

// A workgroup's slot of partial sums, in floats: dW2 [2 towers][64][64], db2 [128], dWa [9][64], dba [9],
// dWv [64], dbv [1], db1 [128], five statistics (policy, value, entropy loss, approx_kl, clip fraction)
constexpr int kPpoW2 = 0, kPpoB2 = 8192, kPpoWa = 8320, kPpoBa = 8896, kPpoWv = 8912, kPpoBv = 8976, kPpoB1 = 8992,
              kPpoSt = 9120, kPpoSlot = 9136;
constexpr int kPpoStats = 5;

// The partition of the batch and of the workspace: a function of (B, D) alone.
struct PpoPlan {
  uint64_t blocks, dtiles, seg_blocks, segs;  // 64-sample blocks, 128-column tiles, blocks per segment, segments
  uint64_t dz1, part_a, part_b, total;        // workspace offsets and size in floats
};
__host__ __device__ inline PpoPlan ppo_plan(uint64_t B, uint64_t D) {
  PpoPlan p;
  p.blocks = (B + kPpoRows - 1) / kPpoRows;
  p.dtiles = (D + kPpoDTile - 1) / kPpoDTile;
  uint64_t want = (uint64_t)kPpoWant / p.dtiles;
  if (want < 1) want = 1;
  if (want > p.blocks) want = p.blocks;
  p.seg_blocks = want ? (p.blocks + want - 1) / want : 1;
  p.segs = want ? (p.blocks + p.seg_blocks - 1) / p.seg_blocks : 0;
  p.dz1 = 0;
  p.part_a = p.dz1 + p.blocks * kPpoRows * 128;
  p.part_b = p.part_a + p.blocks * kPpoSlot;
  p.total = p.part_b + p.segs * 128 * D;
  return p;
}

struct PpoArgs {
  const int8_t* obs;
  uint64_t pitch, T, N, D, B;
  const int64_t* indices;
  const uint8_t* actions;
  const float *old_logp, *adv, *ret;
  const float* packed;
  const float* adv_stats;
  float clip, clip_lo, clip_hi, ent_coef, vf_coef;
  float* ws;
  uint8_t* err;      // the handle's per-env error bytes, err_n of them
  uint64_t err_n;
  PolicyTensors<float> g;
  float* stats;
  // pgtg_ppo_grad_ex's extras, all absent (NULL, 0) from pgtg_ppo_grad
  const float* old_values;  // value clipping: SB3's clip_range_vf over the rollout's values; NULL: none
  float clip_vf;
  uint32_t* stop_at;        // the update's stop word (target_kl); NULL: no gate
  uint32_t ordinal;         // this minibatch's place m = 1, 2, ... within the update
  uint32_t has_kl;          // k_ppo_reduce stores stop_at = m once approx_kl > kl_limit
  float kl_limit;           // 1.5f * target_kl
};

// The gate of an update with target_kl: the launch set of minibatch m does nothing once an earlier minibatch
// has stopped the update (stop_at < m), and its optimiser step nothing from the stopping minibatch on
// (stop_at <= m).  One uniform load; no kernel is gated by a value written in its own launch (k_ppo_reduce of
// ordinal m stores m, which gates neither itself nor its own k_ppo_loss and k_ppo_dw1).
__device__ __forceinline__ bool ppo_gated(const uint32_t* stop_at, uint32_t ordinal, bool step) {
  if (!stop_at) return false;
  const uint32_t s = *stop_at;
  return s != 0 && (step ? s <= ordinal : s < ordinal);
}

// Sample idx of a rollout of T steps of N envs (SB3's flat order, env-major): its env and its step; false for
// an index outside [0, T N), which no kernel dereferences.
__device__ __forceinline__ bool ppo_sample(int64_t idx, uint64_t T, uint64_t N, uint64_t* env, uint64_t* step) {
  if (idx < 0 || (uint64_t)idx >= T * N) return false;
  *env = (uint64_t)idx / T;
  *step = (uint64_t)idx % T;
  return true;
}

// sum of n floats p[0], p[stride], ...: kPpoSets accumulators take them round robin, added (0 + 1) + (2 + 3)
__device__ __forceinline__ float ppo_sum(const float* p, uint64_t n, uint64_t stride) {
  float s[kPpoSets] = {0.f, 0.f, 0.f, 0.f};
  for (uint64_t i = 0; i < n; i += kPpoSets)
#pragma unroll
    for (int j = 0; j < kPpoSets; j++)
      if (i + j < n) s[j] += p[(i + j) * stride];
  return (s[0] + s[1]) + (s[2] + s[3]);
}

// sum over a workgroup's 64 rows of f(r): eight accumulators take the rows round robin (chains of eight),
// added ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))
template <typename F>
__device__ __forceinline__ float ppo_sum_rows(F f) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < kPpoRows; r += 8)
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] += f(r + j);
  return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

__global__ void __launch_bounds__(kPpoThreads) k_ppo_loss(PpoArgs a) {
  // h1 [64][kPolHPitch], then h2 the same, as in k_policy
  __shared__ __attribute__((aligned(16))) float lds[2 * kPpoRows * kPolHPitch];
  __shared__ float sdl[kPpoRows * 12];  // per sample: dloss/dlogit [9], dloss/dvalue at [9]
  __shared__ float sst[kPpoRows * 8];   // per sample: the five statistics' terms
  __shared__ float red[4 * 128];        // the two row halves of db2 and of db1
  __shared__ uint64_t rowp[kPpoRows];   // byte address of the sample's row; 0: skipped
  __shared__ uint64_t soff[kPpoRows];   // t * N + e
  float* h1 = lds;
  float* h2 = lds + kPpoRows * kPolHPitch;
  static_assert(kPpoRows == kPolRows && kPpoThreads == kPolThreads, "k_policy's tiling");
  if (ppo_gated(a.stop_at, a.ordinal, false)) return;

  const uint32_t tid = threadIdx.x, w = tid >> 6;
  const uint64_t D = a.D, B = a.B, blk = blockIdx.x;
  const PolicyLayout L = policy_layout(D);
  const PpoPlan pl = ppo_plan(B, D);
  const float* P = a.packed;
  const uintptr_t lo = (uintptr_t)a.obs, hi = lo + (a.T - 1) * a.pitch + a.N * D;
  float* slot = a.ws + pl.part_a + blk * kPpoSlot;

  if (tid < kPpoRows) {
    const uint64_t s = blk * kPpoRows + tid;
    uint64_t rp = 0, so = 0;
    if (s < B) {
      uint64_t e, t;
      if (ppo_sample(a.indices[s], a.T, a.N, &e, &t)) {
        so = t * a.N + e;
        if (a.actions[so] < kPolAct) rp = lo + t * a.pitch + e * D;
      }
      if (!rp && a.err_n) a.err[s % a.err_n] = (uint8_t)(-PGTG_E_INVALID);
    }
    rowp[tid] = rp;
    soff[tid] = so;
  }
  __syncthreads();

  // ---- the forward pass (pgtg_policy.h), over the gathered rows ------------------------------------------
  policy_hidden<2>(P, L, D, lo, hi, 32 * w, h1, h2, [&](uint32_t r, uintptr_t* p) { return (*p = rowp[r]) != 0; });

  // ---- the heads, the loss terms and their derivatives -------------------------------------------------
  {
    const uint32_t r = tid >> 2, part = tid & 3;
    float val, lg[kPolAct];
    policy_heads<false>(P, L, h2, r, part, &val, lg);
    if (part == 0) {
      float dl[kPolAct + 1], st[kPpoStats];
#pragma unroll
      for (int c = 0; c <= kPolAct; c++) dl[c] = 0.f;
#pragma unroll
      for (int j = 0; j < kPpoStats; j++) st[j] = 0.f;
      if (rowp[r]) {
        const uint64_t so = soff[r];
        const int act = a.actions[so];
        const float inv_b = 1.f / (float)B;
        float mx, ex[kPolAct], sum;
        policy_softmax(lg, &mx, ex, &sum);
        const float lse = mx + logf(sum);
        float la = lg[0];
#pragma unroll
        for (int c = 1; c < kPolAct; c++)
          if (act == c) la = lg[c];
        const float logp = la - lse;
        float p[kPolAct], lp[kPolAct], ent = 0.f;
#pragma unroll
        for (int c = 0; c < kPolAct; c++) {
          p[c] = ex[c] / sum;
          lp[c] = lg[c] - lse;
          ent -= p[c] * lp[c];
        }
        float adv = a.adv[so];
        if (a.adv_stats) adv = (adv - a.adv_stats[0]) * a.adv_stats[1];
        const float lr = logp - a.old_logp[so];
        const float ratio = expf(lr);
        const float rc = fminf(fmaxf(ratio, a.clip_lo), a.clip_hi);
        const float p1 = adv * ratio, p2 = adv * rc;
        const bool through = p1 < p2 || (ratio >= a.clip_lo && ratio <= a.clip_hi);
        const float gr = through ? -adv * ratio : 0.f;  // d policy term / d logp
        float dv = a.ret[so] - val;
        bool vthrough = true;
        if (a.old_values) {  // values_pred = old + clamp(value - old, -c, c): torch's clamp passes the closed interval,
          const float ov = a.old_values[so], dd = val - ov;  // where values_pred is the value itself
          vthrough = dd >= -a.clip_vf && dd <= a.clip_vf;
          if (!vthrough) dv = a.ret[so] - (ov + fminf(fmaxf(dd, -a.clip_vf), a.clip_vf));
        }
#pragma unroll
        for (int c = 0; c < kPolAct; c++)
          dl[c] = (gr * ((act == c ? 1.f : 0.f) - p[c]) + a.ent_coef * (p[c] * (lp[c] + ent))) * inv_b;
        dl[kPolAct] = vthrough ? a.vf_coef * (-2.f * dv) * inv_b : 0.f;
        st[0] = -fminf(p1, p2);
        st[1] = dv * dv;
        st[2] = -ent;
        st[3] = (ratio - 1.f) - lr;
        st[4] = fabsf(ratio - 1.f) > a.clip ? 1.f : 0.f;
      }
#pragma unroll
      for (int c = 0; c <= kPolAct; c++) sdl[r * 12 + c] = dl[c];
#pragma unroll
      for (int j = 0; j < kPpoStats; j++) sst[r * 8 + j] = st[j];
    }
  }
  __syncthreads();

  // ---- the heads' gradients and the statistics: one output per thread, rows in order ------------------
  for (uint32_t o = tid; o < 650 + kPpoStats; o += kPpoThreads) {
    if (o < 576) {
      const uint32_t c = o >> 6, k = o & 63;
      slot[kPpoWa + o] = ppo_sum_rows([&](int r) { return sdl[r * 12 + c] * h2[r * kPolHPitch + k]; });
    } else if (o < 640) {
      const uint32_t k = o - 576;
      slot[kPpoWv + k] = ppo_sum_rows([&](int r) { return sdl[r * 12 + kPolAct] * h2[r * kPolHPitch + 64 + k]; });
    } else if (o < 650) {
      const uint32_t c = o - 640;  // (9: the value head's bias)
      slot[c < (uint32_t)kPolAct ? kPpoBa + c : kPpoBv] = ppo_sum_rows([&](int r) { return sdl[r * 12 + c]; });
    } else {
      const uint32_t j = o - 650;
      slot[kPpoSt + j] = ppo_sum_rows([&](int r) { return sst[r * 8 + j]; });
    }
  }
  __syncthreads();  // (h2 is read no more)

  // ---- dZ2 = dH2 (1 - h2^2) over h2; thread = column, 32 rows ------------------------------------------
  const uint32_t col = tid & 127, rh = tid >> 7;
  {
    float wh[kPolAct];
#pragma unroll
    for (int c = 0; c < kPolAct; c++) wh[c] = col < 64 ? P[L.wa + c * 64 + col] : 0.f;
    const float wvc = col < 64 ? 0.f : P[L.wv + col - 64];
    float bs[4] = {0.f, 0.f, 0.f, 0.f};  // (rows round robin: chains of eight)
#pragma unroll 4
    for (int rr = 0; rr < 32; rr++) {
      const uint32_t r = 32 * rh + rr;
      float dh;
      if (col < 64) {
        dh = 0.f;
#pragma unroll
        for (int c = 0; c < kPolAct; c++) dh += sdl[r * 12 + c] * wh[c];
      } else {
        dh = sdl[r * 12 + kPolAct] * wvc;
      }
      const float h = h2[r * kPolHPitch + col];
      const float dz = dh * (1.f - h * h);
      h2[r * kPolHPitch + col] = dz;
      bs[rr & 3] += dz;
    }
    red[rh * 128 + col] = (bs[0] + bs[1]) + (bs[2] + bs[3]);
  }
  __syncthreads();
  if (tid < 128) slot[kPpoB2 + tid] = red[tid] + red[128 + tid];

  // ---- dW2 [tower][c][k] = sum_r dZ2[r][c] h1[r][k]; thread = (tower, k), 32 c ---------------------------
  {
    const uint32_t k = tid & 63, t = (tid >> 6) & 1, chh = tid >> 7;
    float s[32];
#pragma unroll
    for (int j = 0; j < 32; j++) s[j] = 0.f;
    for (int r = 0; r < kPpoRows; r++) {
      const float h = h1[r * kPolHPitch + 64 * t + k];
      const float* dz = h2 + r * kPolHPitch + 64 * t + 32 * chh;
#pragma unroll
      for (int j = 0; j < 32; j++) s[j] += dz[j] * h;
    }
#pragma unroll
    for (int j = 0; j < 32; j++) slot[kPpoW2 + t * 4096 + (32 * chh + j) * 64 + k] = s[j];
  }

  // ---- dZ1 = (dZ2 W2) (1 - h1^2) to the workspace, db1; thread = column, 32 rows -------------------------
  {
    const uint32_t t = col >> 6, k = col & 63;
    float wc[64];
#pragma unroll
    for (int c = 0; c < 64; c++) wc[c] = P[L.w2 + (((uint64_t)t * 4 + (k >> 4)) * 64 + c) * 16 + (k & 15)];
    float bs[4] = {0.f, 0.f, 0.f, 0.f};
    float* out = a.ws + pl.dz1 + blk * kPpoRows * 128;
#pragma unroll 4
    for (int rr = 0; rr < 32; rr++) {
      const uint32_t r = 32 * rh + rr;
      const float* dz = h2 + r * kPolHPitch + 64 * t;
      float dh = 0.f;
#pragma unroll
      for (int c = 0; c < 64; c++) dh += dz[c] * wc[c];
      const float h = h1[r * kPolHPitch + col];
      const float d1 = dh * (1.f - h * h);
      out[r * 128 + col] = d1;
      bs[rr & 3] += d1;
    }
    red[256 + rh * 128 + col] = (bs[0] + bs[1]) + (bs[2] + bs[3]);
  }
  __syncthreads();
  if (tid < 128) slot[kPpoB1 + tid] = red[256 + tid] + red[384 + tid];
}

__global__ void __launch_bounds__(kPpoThreads) k_ppo_dw1(PpoArgs a) {
  __shared__ __attribute__((aligned(16))) float dzs[kPpoRows * kPolHPitch];
  __shared__ __attribute__((aligned(16))) uint8_t xs[kPpoRows * kPpoXPitch];
  __shared__ uint64_t rowp[kPpoRows];
  static_assert(kPpoDTile == 128 && kPpoRows == 64, "a stage is 64 rows of 32 dwords: idx & 31 of row idx >> 5");
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t n16 = lane & 15, q = lane >> 4;
  const uint64_t D = a.D, B = a.B;
  if (ppo_gated(a.stop_at, a.ordinal, false)) return;
  const PpoPlan pl = ppo_plan(B, D);
  const uint64_t k0 = (uint64_t)blockIdx.x * kPpoDTile, seg = blockIdx.y;
  const uint64_t blk0 = seg * pl.seg_blocks;
  const uint64_t blk1 = blk0 + pl.seg_blocks < pl.blocks ? blk0 + pl.seg_blocks : pl.blocks;
  const uintptr_t lo = (uintptr_t)a.obs, hi = lo + (a.T - 1) * a.pitch + a.N * D;

  // wave w: hidden columns 32 w .. 32 w + 31 (two tiles) x the 128 observation columns (eight tiles: lane
  // n16 holds the eight consecutive bytes k0 + 8 n16 .. + 7 of a row, byte j being its column of tile j)
  pol_f32x4 acc[2][8];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 8; j++) acc[i][j] = pol_f32x4{0.f, 0.f, 0.f, 0.f};

  for (uint64_t blk = blk0; blk < blk1; blk++) {
    if (blk != blk0) __syncthreads();  // (the last stage's readers are done)
    if (tid < kPpoRows) {
      const uint64_t s = blk * kPpoRows + tid;
      uint64_t rp = 0;
      uint64_t e, t;
      if (s < B && ppo_sample(a.indices[s], a.T, a.N, &e, &t)) rp = lo + t * a.pitch + e * D;
      rowp[tid] = rp;
    }
    const float* src = a.ws + pl.dz1 + blk * kPpoRows * 128;
#pragma unroll
    for (int it = 0; it < kPpoRows * 32 / kPpoThreads; it++) {
      const uint32_t i = it * kPpoThreads + tid, r = i >> 5, c4 = i & 31;
      *(pol_f32x4*)(dzs + r * kPolHPitch + 4 * c4) = *(const pol_f32x4*)(src + r * 128 + 4 * c4);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < kPpoRows * (kPpoDTile / 4) / kPpoThreads; it++) {
      const uint32_t i = it * kPpoThreads + tid, r = i >> 5, dw = i & 31;
      const uint64_t k = k0 + 4 * dw, rp = rowp[r];
      uint32_t v = 0;
      if (rp && k < D) v = policy_row_dword((uintptr_t)rp, k, D, lo, hi);
      *(uint32_t*)(xs + r * kPpoXPitch + 4 * dw) = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int st = 0; st < kPpoRows / 4; st++) {
      const uint32_t s = 4 * st + q;
      const float a0 = dzs[s * kPolHPitch + 32 * w + n16], a1 = dzs[s * kPolHPitch + 32 * w + 16 + n16];
      const uint32_t x0 = *(const uint32_t*)(xs + s * kPpoXPitch + 8 * n16);
      const uint32_t x1 = *(const uint32_t*)(xs + s * kPpoXPitch + 8 * n16 + 4);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float x = (float)(int)(int8_t)((j < 4 ? x0 : x1) >> (8 * (j & 3)));
        acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, x, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, x, acc[1][j], 0, 0, 0);
      }
    }
  }
  // tile (i, j), register u: hidden column 32 w + 16 i + 4 q + u, observation column k0 + 8 n16 + j
  float* out = a.ws + pl.part_b + seg * 128 * D;
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t c = 32 * w + 16 * i + 4 * q + u;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint64_t k = k0 + 8 * n16 + j;
        if (k < D) out[c * D + k] = acc[i][j][u];
      }
    }
}

__global__ void __launch_bounds__(kPpoThreads) k_ppo_reduce(PpoArgs a) {
  const uint64_t D = a.D, B = a.B;
  const uint32_t stop = a.stop_at ? *a.stop_at : 0;  // (this launch alone may store it, and stores a.ordinal)
  if (stop != 0 && stop < a.ordinal) return;
  const PpoPlan pl = ppo_plan(B, D);
  const uint64_t gid = (uint64_t)blockIdx.x * kPpoThreads + threadIdx.x;
  if (gid < 128 * D) {
    const uint64_t c = gid / D, k = gid % D;
    const float s = ppo_sum(a.ws + pl.part_b + gid, pl.segs, 128 * D);
    if (c < 64) a.g.w1p[c * D + k] = s;
    else a.g.w1v[(c - 64) * D + k] = s;
    return;
  }
  const uint64_t j = gid - 128 * D;
  if (j >= (uint64_t)kPpoSlot) return;
  const float* part = a.ws + pl.part_a;
  if (j == (uint64_t)kPpoSt) {
    float m[kPpoStats];
#pragma unroll
    for (int i = 0; i < kPpoStats; i++) m[i] = ppo_sum(part + kPpoSt + i, pl.blocks, kPpoSlot) / (float)B;
    a.stats[0] = m[0] + a.ent_coef * m[2] + a.vf_coef * m[1];
    a.stats[1] = m[0];
    a.stats[2] = m[1];
    a.stats[3] = m[2];
    a.stats[4] = m[3];
    a.stats[5] = m[4];
    a.stats[6] = 0.f;
    a.stats[7] = 0.f;
    if (a.has_kl && stop == 0 && m[3] > a.kl_limit) *a.stop_at = a.ordinal;  // (a NaN compares false, as in torch)
    return;
  }
  float* dst;
  if (j < (uint64_t)kPpoB2) dst = (j < 4096 ? a.g.w2p : a.g.w2v) + (j & 4095);
  else if (j < (uint64_t)kPpoWa) dst = j - kPpoB2 < 64 ? a.g.b2p + (j - kPpoB2) : a.g.b2v + (j - kPpoB2 - 64);
  else if (j < (uint64_t)kPpoBa) dst = a.g.wa + (j - kPpoWa);
  else if (j < (uint64_t)kPpoBa + kPolAct) dst = a.g.ba + (j - kPpoBa);
  else if (j < (uint64_t)kPpoWv) return;
  else if (j < (uint64_t)kPpoBv) dst = a.g.wv + (j - kPpoWv);
  else if (j == (uint64_t)kPpoBv) dst = a.g.bv;
  else if (j < (uint64_t)kPpoB1) return;
  else if (j < (uint64_t)kPpoSt) dst = j - kPpoB1 < 64 ? a.g.b1p + (j - kPpoB1) : a.g.b1v + (j - kPpoB1 - 64);
  else return;
  *dst = ppo_sum(part + j, pl.blocks, kPpoSlot);
}

}  // namespace pgtg
#endif  // PGTG_PPO_H_
