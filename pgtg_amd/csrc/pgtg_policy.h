// pgtg_policy.h -- the acting forward pass of SB3's MlpPolicy (ActorCriticPolicy with separate 64-64 tanh
// towers, a 9-way categorical head and a scalar value head: PPO("MlpPolicy", ...) of pgtg/train.py:61-74)
// as one kernel over the int8 flat rows k_flatten writes (include/pgtg.h pgtg_policy), and the repack of
// SB3's nn.Linear weights into the layout that kernel streams (pgtg_policy_pack).  The forward pass
// (policy_hidden, policy_heads, policy_softmax) and the walk of the packed layout (policy_packed_word) are
// functions that the PPO kernels of pgtg_ppo.h and pgtg_ppo_step.h call too.  Included by pgtg_env.hip
// (device code only).
#ifndef PGTG_POLICY_H_
#define PGTG_POLICY_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pgtg.h"

namespace pgtg {

// Tiling.  A workgroup of four waves owns kPolRows = 64 consecutive envs.  The first layer is
// [64 envs][D] x [D][128] (columns 0..63 the pi tower's hidden units, 64..127 the vf tower's) on the exact
// float32 matrix instruction v_mfma_f32_16x16x4_f32: wave w accumulates all 64 rows of columns
// 32 w .. 32 w + 31 (VALUE_ONLY: 16 columns of the vf tower each), 4 x 2 tiles of 16 x 16.  That
// instruction issues every 32 cycles, so a group of 16 k (4 k-steps x 8 tiles = 1 024 cycles of matrix
// pipe) needs one LDS dword per row tile and one 16-byte weight load per column tile and lane: the kernel
// is bound by the matrix pipe by a wide margin and nothing else is tuned.
//
// The observation bytes of the 64 rows are staged through LDS kPolChunk = 256 bytes of every row at a
// time; the weights are never staged: W1 is packed [k / 16][column][16 k] float32 (pgtg_policy_pack), so
// the 64 lanes of a wave read one contiguous KiB per column tile and group, straight from L2.
// Within a group lane (n, q) (n = lane & 15, q = lane >> 4) holds k = 16 g + 4 q + s at step s for both
// operands: the instruction's own k order is q, so the chain of one output element runs over k in the
// order s-major, q-minor inside a group.  kPolSets independent accumulator sets take the groups round
// robin (set = g mod kPolSets) and are added as (0 + 1) + (2 + 3): a chain is a quarter of D long, which
// is what keeps the first layer's rounding error near that of a blocked CPU dot product.
//
// The 64 x 64 layers run the same way out of LDS (h1 as the A operand, one accumulator set), the heads
// on the vector ALU, four lanes per env.  h1 and h2 live in LDS only.
constexpr int kPolRows = 64;
constexpr int kPolThreads = 256;
constexpr int kPolChunk = 256;          // observation bytes of a row per LDS stage (exported: pgtg_policy_chunk)
constexpr int kPolXPitch = kPolChunk + 16;  // LDS bytes per staged row (the pad spreads the rows over the banks)
constexpr int kPolHPitch = 128 + 4;     // floats per row of h1 / h2
constexpr int kPolSets = 4;
constexpr int kPolHid = 64;
constexpr int kPolAct = 9;
constexpr uint64_t kPolMaxObsDim = PGTG_POLICY_MAX_OBS_DIM;

// The packed weights, in floats from the buffer's start (a function of obs_dim alone):
//   w1   [G][128][16]   G = ceil(D / 16); k >= D is zero
//   b1   [128]
//   w2   [2 towers][4][64][16]
//   b2   [128]
//   wa [9][64], ba [9] (padded to 16), wv [64], bv [1] (padded to 16)
struct PolicyLayout {
  uint64_t groups, w1, b1, w2, b2, wa, ba, wv, bv, total;
};
__host__ __device__ inline PolicyLayout policy_layout(uint64_t obs_dim) {
  PolicyLayout L;
  L.groups = (obs_dim + 15) / 16;
  L.w1 = 0;
  L.b1 = L.w1 + L.groups * 128 * 16;
  L.w2 = L.b1 + 128;
  L.b2 = L.w2 + 2 * 4 * 64 * 16;
  L.wa = L.b2 + 128;
  L.ba = L.wa + kPolAct * kPolHid;
  L.wv = L.ba + 16;
  L.bv = L.wv + kPolHid;
  L.total = L.bv + 16;
  return L;
}

// The twelve tensors of SB3's nn.Linear layouts, in PgtgPolicyWeights' order of fields: the one set of
// pointers every kernel takes (T = const float: read only).
template <typename T>
struct PolicyTensors {
  T *w1p, *b1p, *w2p, *b2p, *wa, *ba, *w1v, *b1v, *w2v, *b2v, *wv, *bv;
};

enum { PT_W1P, PT_B1P, PT_W2P, PT_B2P, PT_WA, PT_BA, PT_W1V, PT_B1V, PT_W2V, PT_B2V, PT_WV, PT_BV };

template <typename T>
__device__ __forceinline__ T* policy_tensor(const PolicyTensors<T>& s, int t) {
  switch (t) {
    case PT_W1P: return s.w1p;
    case PT_B1P: return s.b1p;
    case PT_W2P: return s.w2p;
    case PT_B2P: return s.b2p;
    case PT_WA: return s.wa;
    case PT_BA: return s.ba;
    case PT_W1V: return s.w1v;
    case PT_B1V: return s.b1v;
    case PT_W2V: return s.w2v;
    case PT_B2V: return s.b2v;
    case PT_WV: return s.wv;
    default: return s.bv;
  }
}

// word i of the packed buffer (policy_layout): its tensor and its offset there, -1 for a padding word
// (k >= D of the last W1 group, the pads after ba and bv).  The one walk of the layout: k_policy_pack
// writes the buffer through it and k_ppo_adam (pgtg_ppo_step.h) rewrites it through it.
__device__ __forceinline__ int policy_packed_word(uint64_t i, const PolicyLayout& L, uint64_t D, uint64_t* off) {
  if (i < L.b1) {
    const uint64_t g = i / 2048, c = (i / 16) % 128, k = g * 16 + (i % 16);
    if (k >= D) return -1;
    return c < 64 ? (*off = c * D + k, PT_W1P) : (*off = (c - 64) * D + k, PT_W1V);
  }
  if (i < L.w2) {
    const uint64_t c = i - L.b1;
    return c < 64 ? (*off = c, PT_B1P) : (*off = c - 64, PT_B1V);
  }
  if (i < L.b2) {
    const uint64_t j = i - L.w2, t = j / 4096, g = (j / 1024) % 4, c = (j / 16) % 64, k = g * 16 + (j % 16);
    *off = c * 64 + k;
    return t ? PT_W2V : PT_W2P;
  }
  if (i < L.wa) {
    const uint64_t c = i - L.b2;
    return c < 64 ? (*off = c, PT_B2P) : (*off = c - 64, PT_B2V);
  }
  if (i < L.ba) return *off = i - L.wa, PT_WA;
  if (i < L.wv) return i - L.ba < (uint64_t)kPolAct ? (*off = i - L.ba, PT_BA) : -1;
  if (i < L.bv) return *off = i - L.wv, PT_WV;
  if (i == L.bv) return *off = 0, PT_BV;
  return -1;
}

struct PolicyPackArgs {
  PolicyTensors<const float> src;
  float* out;
  uint64_t obs_dim;
};

__global__ void __launch_bounds__(256) k_policy_pack(PolicyPackArgs a) {
  const PolicyLayout L = policy_layout(a.obs_dim);
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < L.total; i += stride) {
    uint64_t off = 0;
    const int t = policy_packed_word(i, L, a.obs_dim, &off);
    a.out[i] = t >= 0 ? policy_tensor(a.src, t)[off] : 0.f;
  }
}

// u in [0, 1), a multiple of 2^-24: splitmix64 of (seed, draw counter, global env index), as
// k_random_actions hashes (seed, t, env), in a domain of its own.  pgtg_amd.policy.policy_uniform.
__device__ __forceinline__ float policy_uniform(uint64_t seed, uint64_t counter, uint64_t env) {
  uint64_t z = seed ^ (counter * 0x9E3779B97F4A7C15ull) ^ (env * 0xD1B54A32D192ED03ull) ^ 0x706F6C6963795F75ull;
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (float)(uint32_t)(z >> 40) * 5.9604644775390625e-08f;  // (24 bits: exact)
}

struct PolicyArgs {
  const int8_t* obs;
  const float* packed;
  const float* uniforms;
  uint8_t* actions;
  float* values;
  float* log_probs;
  uint64_t n, obs_dim, seed, counter, env_offset;
};

typedef float pol_f32x4 __attribute__((ext_vector_type(4)));

enum { POLICY_SAMPLE = PGTG_POLICY_SAMPLE, POLICY_ARGMAX = PGTG_POLICY_ARGMAX, POLICY_VALUE_ONLY = PGTG_POLICY_VALUE_ONLY };

// The aligned dword at address a, of which only the bytes inside [lo, hi) may be touched: whole when it
// lies inside, byte by byte (absent bytes zero) at the buffer's two ends.
__device__ __forceinline__ uint32_t policy_load_dword(uintptr_t a, uintptr_t lo, uintptr_t hi) {
  if (a >= lo && a + 4 <= hi) return *(const uint32_t*)a;
  uint32_t v = 0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (a + j >= lo && a + j < hi) v |= (uint32_t) * (const uint8_t*)(a + j) << (8 * j);
  return v;
}

// The four bytes k .. k + 3 (k < D) of the row at byte address `row`, bytes at k >= D zero, assembled from
// the two aligned dwords around them; no byte outside [lo, hi) is touched.
__device__ __forceinline__ uint32_t policy_row_dword(uintptr_t row, uint64_t k, uint64_t D, uintptr_t lo, uintptr_t hi) {
  const uintptr_t p = row + k, al = p & ~(uintptr_t)3;
  const uint32_t sh = (uint32_t)(p & 3) * 8;
  uint32_t v = policy_load_dword(al, lo, hi);
  if (sh) v = (v >> sh) | (policy_load_dword(al + 4, lo, hi) << (32 - sh));
  if (k + 4 > D) v &= 0xffffffffu >> (8 * (uint32_t)(k + 4 - D));  // (bytes of the next row: zero)
  return v;
}

// The two hidden layers of a workgroup's kPolRows rows, for every kernel that runs the forward pass (k_policy
// here, k_ppo_loss in pgtg_ppo.h): row(r, &p) says whether the workgroup has a row r (the bytes of one it has
// not stand as zero) and gives its byte address -- the test apart from the address, so that a kernel whose rows
// are consecutive keeps its address arithmetic out of the stage loop; wave w owns the NT column tiles from
// column cb of the 128.  h1 and h2 are the two [kPolRows][kPolHPitch] float arrays in LDS, the observation
// bytes staged over h2 (they are dead before h2 is written); both are complete behind a barrier on return.
template <int NT, typename Row>
__device__ __forceinline__ void policy_hidden(const float* P, const PolicyLayout& L, uint64_t D, uintptr_t lo,
                                              uintptr_t hi, uint32_t cb, float* h1, float* h2, Row row) {
  static_assert(kPolChunk == 256, "the stage takes dword idx & 63 of row idx >> 6");
  static_assert(kPolRows * kPolXPitch <= kPolRows * kPolHPitch * 4, "the staged rows fit under h2");
  uint8_t* xs = (uint8_t*)h2;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t n16 = lane & 15, q = lane >> 4;

  // ---- layer 1 -------------------------------------------------------------------------------
  pol_f32x4 acc[kPolSets][4][NT];
#pragma unroll
  for (int s = 0; s < kPolSets; s++)
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int j = 0; j < NT; j++) acc[s][m][j] = pol_f32x4{0.f, 0.f, 0.f, 0.f};

  const uint64_t chunks = (D + kPolChunk - 1) / kPolChunk;
  for (uint64_t ch = 0; ch < chunks; ch++) {
    const uint64_t k0 = ch * kPolChunk;
    if (ch) __syncthreads();  // (the last chunk's readers are done)
    // stage: LDS dword dw of row r = the four bytes k0 + 4 dw .. + 3 of that row; a wave's 64 lanes are the
    // 64 consecutive dwords of one row
#pragma unroll 4
    for (int it = 0; it < kPolRows * (kPolChunk / 4) / kPolThreads; it++) {
      const uint32_t idx = it * kPolThreads + tid, r = idx >> 6, dw = idx & 63;
      const uint64_t k = k0 + 4 * dw;
      uintptr_t rp;
      uint32_t v = 0;
      if (row(r, &rp) && k < D) v = policy_row_dword(rp, k, D, lo, hi);
      *(uint32_t*)(xs + r * kPolXPitch + 4 * dw) = v;
    }
    __syncthreads();
    const uint64_t g0 = k0 / 16;
    const uint64_t gn = L.groups - g0 < (uint64_t)(kPolChunk / 16) ? L.groups - g0 : (uint64_t)(kPolChunk / 16);
    // groups in rounds of kPolSets, so that the set index is a compile-time constant
    for (uint64_t gb = 0; gb < gn; gb += kPolSets) {
#pragma unroll
      for (int s = 0; s < kPolSets; s++) {
        const uint64_t gl = gb + s;
        if (gl < gn) {  // (wave-uniform)
          const float* wg = P + L.w1 + ((g0 + gl) * 128 + cb + n16) * 16 + 4 * q;
          pol_f32x4 b[NT];
#pragma unroll
          for (int j = 0; j < NT; j++) b[j] = *(const pol_f32x4*)(wg + j * 256);
          uint32_t xa[4];
#pragma unroll
          for (int m = 0; m < 4; m++) xa[m] = *(const uint32_t*)(xs + (16 * m + n16) * kPolXPitch + 16 * gl + 4 * q);
#pragma unroll
          for (int st = 0; st < 4; st++)
#pragma unroll
            for (int m = 0; m < 4; m++) {
              const float x = (float)(int)(int8_t)(xa[m] >> (8 * st));
#pragma unroll
              for (int j = 0; j < NT; j++)
                acc[s][m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x, b[j][st], acc[s][m][j], 0, 0, 0);
            }
        }
      }
    }
  }
  // h1 = tanh(acc + b1): tile (m, j) holds rows 16 m + 4 q + i (i = register), column cb + 16 j + n16
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const uint32_t c = cb + 16 * j + n16;
    const float bias = P[L.b1 + c];
#pragma unroll
    for (int m = 0; m < 4; m++) {
      const pol_f32x4 t = (acc[0][m][j] + acc[1][m][j]) + (acc[2][m][j] + acc[3][m][j]);
#pragma unroll
      for (int i = 0; i < 4; i++) h1[(16 * m + 4 * q + i) * kPolHPitch + c] = tanhf(t[i] + bias);
    }
  }
  __syncthreads();  // (h1 complete; the staged bytes are dead)

  // ---- layer 2: the wave's columns again, K = the 64 hidden units of their tower ------------------
  const uint32_t tower = cb >> 6, c2 = cb & 63;
  pol_f32x4 a2[4][NT];
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int j = 0; j < NT; j++) a2[m][j] = pol_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < 4; g++) {
    const float* wg = P + L.w2 + (((uint64_t)tower * 4 + g) * 64 + c2 + n16) * 16 + 4 * q;
    pol_f32x4 b[NT], x[4];
#pragma unroll
    for (int j = 0; j < NT; j++) b[j] = *(const pol_f32x4*)(wg + j * 256);
#pragma unroll
    for (int m = 0; m < 4; m++) x[m] = *(const pol_f32x4*)(h1 + (16 * m + n16) * kPolHPitch + 64 * tower + 16 * g + 4 * q);
#pragma unroll
    for (int st = 0; st < 4; st++)
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int j = 0; j < NT; j++)
          a2[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[m][st], b[j][st], a2[m][j], 0, 0, 0);
  }
#pragma unroll
  for (int j = 0; j < NT; j++) {
    const uint32_t c = cb + 16 * j + n16;
    const float bias = P[L.b2 + c];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int i = 0; i < 4; i++) h2[(16 * m + 4 * q + i) * kPolHPitch + c] = tanhf(a2[m][j][i] + bias);
  }
  __syncthreads();
}

// The heads of row r: four lanes per row (part = 0 .. 3 in consecutive lanes), 16 hidden units each, summed
// as (0 + 1) + (2 + 3); every one of the four lanes ends with the value and, unless VO, the nine logits.
template <bool VO>
__device__ __forceinline__ void policy_heads(const float* P, const PolicyLayout& L, const float* h2, uint32_t r,
                                             uint32_t part, float* val, float* lg) {
  const float* hp = h2 + r * kPolHPitch + 16 * part;
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 16; k++) v += P[L.wv + 16 * part + k] * hp[64 + k];
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  *val = v + P[L.bv];
  if (VO) return;
#pragma unroll
  for (int c = 0; c < kPolAct; c++) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) s += P[L.wa + c * 64 + 16 * part + k] * hp[k];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    lg[c] = s + P[L.ba + c];
  }
}

// mx = the largest logit, ex[c] = exp(lg[c] - mx) and their sum in index order; returns the arg max
__device__ __forceinline__ int policy_softmax(const float* lg, float* mx, float* ex, float* sum) {
  float m = lg[0];
  int am = 0;
#pragma unroll
  for (int c = 1; c < kPolAct; c++)
    if (lg[c] > m) {  // (strict: the least index among the maxima)
      m = lg[c];
      am = c;
    }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kPolAct; c++) {
    ex[c] = expf(lg[c] - m);
    s += ex[c];
  }
  *mx = m;
  *sum = s;
  return am;
}

template <int MODE>
__global__ void __launch_bounds__(kPolThreads) k_policy(PolicyArgs a) {
  constexpr bool VO = MODE == POLICY_VALUE_ONLY;
  constexpr int NT = VO ? 1 : 2;  // column tiles of 16 per wave
  // one LDS array: h1 [64][kPolHPitch] floats, then h2 the same
  __shared__ __attribute__((aligned(16))) float lds[2 * kPolRows * kPolHPitch];
  float* h1 = lds;
  float* h2 = lds + kPolRows * kPolHPitch;

  const uint32_t tid = threadIdx.x, w = tid >> 6;
  const uint64_t D = a.obs_dim, N = a.n;
  const uint64_t row0 = (uint64_t)blockIdx.x * kPolRows;
  const PolicyLayout L = policy_layout(D);
  const float* P = a.packed;
  const uint32_t cb = VO ? 64 + 16 * w : 32 * w;  // the wave's first column of the 128
  const uintptr_t lo = (uintptr_t)a.obs, hi = lo + N * D;
  policy_hidden<NT>(P, L, D, lo, hi, cb, h1, h2, [&](uint32_t r, uintptr_t* p) {
    *p = lo + (row0 + r) * D;
    return row0 + r < N;
  });

  const uint32_t r = tid >> 2, part = tid & 3;
  const uint64_t e = row0 + r;
  float val, lg[kPolAct];
  policy_heads<VO>(P, L, h2, r, part, &val, lg);
  if (part != 0 || e >= N) return;
  if (a.values) a.values[e] = val;
  if (VO) return;
  float mx, ex[kPolAct], sum;
  int act = policy_softmax(lg, &mx, ex, &sum);  // (ARGMAX)
  if (MODE == POLICY_SAMPLE) {
    const float u = a.uniforms ? a.uniforms[e] : policy_uniform(a.seed, a.counter, a.env_offset + e);
    float cdf = 0.f;
    act = kPolAct - 1;  // (rounding may leave the last sum <= u)
    bool found = false;
#pragma unroll
    for (int c = 0; c < kPolAct; c++) {
      cdf += ex[c] / sum;
      if (!found && u < cdf) {
        act = c;
        found = true;
      }
    }
  }
  float la = lg[0];
#pragma unroll
  for (int c = 1; c < kPolAct; c++)
    if (act == c) la = lg[c];
  if (a.actions) a.actions[e] = (uint8_t)act;
  if (a.log_probs) a.log_probs[e] = la - (mx + logf(sum));
}

}  // namespace pgtg
#endif  // PGTG_POLICY_H_
