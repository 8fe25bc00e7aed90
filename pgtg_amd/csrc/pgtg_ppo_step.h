// pgtg_ppo_step.h -- the optimiser step of a PPO minibatch and the minibatch's advantage statistics
// (include/pgtg.h pgtg_ppo_step, pgtg_ppo_adv_stats): torch.nn.utils.clip_grad_norm_ followed by
// torch.optim.Adam (weight_decay = 0, amsgrad = False) over the twelve MlpPolicy tensors, and the repack of
// the updated weights into k_policy's layout, as two launches; the mean and 1 / (std + 1e-8) of the gathered
// advantages as one.  No floating-point atomic: every sum runs in a fixed order, and in double (the sums are
// a few adds per thread and a tree: the results are the float32 roundings of sums that carry no error of
// their own, which is what lets them stand within torch's float32 error of the float64 truth).
//   k_ppo_gnorm      per-workgroup partial sums of g^2 over the twelve gradient tensors, to the workspace
//   k_ppo_adam       one thread per word of the packed buffer (policy_packed_word, as k_policy_pack): every workgroup
//                    adds the partials in the same order, then clip, Adam and the packed word
//   k_ppo_adv_stats  one workgroup: the gathered advantages' mean, then their squared deviations
// Included by pgtg_env.hip (device code only) after pgtg_ppo.h.
#ifndef PGTG_PPO_STEP_H_
#define PGTG_PPO_STEP_H_

#include "pgtg_ppo.h"

namespace pgtg {

constexpr int kStepThreads = 256;
constexpr int kStepMaxBlocks = 256;    // workgroups of k_ppo_gnorm at most: k_ppo_adam adds one partial per thread
constexpr int kStepSets = 4;           // accumulators per thread, added (0 + 1) + (2 + 3)
constexpr int kStepPackMaxBlocks = 4096;  // (k_policy_pack's cap)
constexpr int kAdvThreads = 1024;
constexpr int kStepSmall = 2 * 4096 + 4 * 64 + kPolAct * kPolHid + kPolAct + kPolHid + 1;  // all but W1: 9 098

// The twelve tensors end to end in PgtgPpoGrads' order of fields, W1 of the two towers first:
//   [0, 64 D) w1p, [64 D, 128 D) w1v, then b1p b1v w2p w2v b2p b2v wa ba wv bv
__host__ __device__ inline uint64_t step_params(uint64_t D) { return 128 * D + kStepSmall; }
// workgroups of k_ppo_gnorm: a function of obs_dim alone
__host__ __device__ inline uint64_t step_blocks(uint64_t D) {
  const uint64_t b = (step_params(D) + kStepThreads - 1) / kStepThreads;
  return b < (uint64_t)kStepMaxBlocks ? b : (uint64_t)kStepMaxBlocks;
}

struct PpoStepArgs {
  PolicyTensors<float> p, m, v;
  PolicyTensors<const float> g;
  float* packed;
  double* ws;  // step_blocks(D) partial sums
  float* grad_norm;
  uint64_t D;
  float step_size, bc2_sqrt;  // lr / (1 - beta1^step), sqrt(1 - beta2^step): in double on the host, rounded once
  float w1, beta2, w2, eps;   // 1 - beta1, beta2, 1 - beta2
  float max_norm;
  const uint32_t* stop_at;  // pgtg_ppo_step_ex's gate (pgtg_ppo.h ppo_gated); NULL: none
  uint32_t ordinal;
};

// element i of the twelve tensors end to end (step_params' order): its tensor and its offset there
__device__ __forceinline__ int step_linear(uint64_t i, uint64_t D, uint64_t* off) {
  if (i < 64 * D) return *off = i, PT_W1P;
  if (i < 128 * D) return *off = i - 64 * D, PT_W1V;
  uint64_t j = i - 128 * D;
  if (j < 64) return *off = j, PT_B1P;
  if ((j -= 64) < 64) return *off = j, PT_B1V;
  if ((j -= 64) < 4096) return *off = j, PT_W2P;
  if ((j -= 4096) < 4096) return *off = j, PT_W2V;
  if ((j -= 4096) < 64) return *off = j, PT_B2P;
  if ((j -= 64) < 64) return *off = j, PT_B2V;
  if ((j -= 64) < (uint64_t)(kPolAct * kPolHid)) return *off = j, PT_WA;
  if ((j -= kPolAct * kPolHid) < (uint64_t)kPolAct) return *off = j, PT_BA;
  if ((j -= kPolAct) < (uint64_t)kPolHid) return *off = j, PT_WV;
  return *off = 0, PT_BV;
}

// the sum of red[0 .. n) (n a power of two, one value per thread) as a halving tree; every thread returns it
template <int n>
__device__ __forceinline__ double step_tree(double* red, uint32_t tid) {
  __syncthreads();
#pragma unroll
  for (int s = n / 2; s > 0; s >>= 1) {
    if (tid < (uint32_t)s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ void __launch_bounds__(kStepThreads) k_ppo_gnorm(PpoStepArgs a) {
  __shared__ double red[kStepThreads];
  const uint64_t D = a.D, n = step_params(D);
  if (ppo_gated(a.stop_at, a.ordinal, true)) return;
  const uint64_t stride = (uint64_t)gridDim.x * kStepThreads;
  double s[kStepSets] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t i0 = (uint64_t)blockIdx.x * kStepThreads + threadIdx.x; i0 < n; i0 += kStepSets * stride)
#pragma unroll
    for (int j = 0; j < kStepSets; j++) {
      const uint64_t i = i0 + j * stride;
      if (i < n) {
        uint64_t off;
        const int t = step_linear(i, D, &off);
        const double g = policy_tensor(a.g, t)[off];
        s[j] += g * g;
      }
    }
  red[threadIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
  const double total = step_tree<kStepThreads>(red, threadIdx.x);
  if (threadIdx.x == 0) a.ws[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kStepThreads) k_ppo_adam(PpoStepArgs a) {
  __shared__ double red[kStepMaxBlocks];
  static_assert(kStepMaxBlocks == kStepThreads, "one partial per thread");
  const uint64_t D = a.D;
  if (ppo_gated(a.stop_at, a.ordinal, true)) return;
  const PolicyLayout L = policy_layout(D);
  red[threadIdx.x] = threadIdx.x < step_blocks(D) ? a.ws[threadIdx.x] : 0.0;
  const float total = (float)sqrt(step_tree<kStepMaxBlocks>(red, threadIdx.x));
  const float coef = fminf(1.f, a.max_norm / (total + 1e-6f));
  if (blockIdx.x == 0 && threadIdx.x == 0 && a.grad_norm) *a.grad_norm = total;
  const uint64_t stride = (uint64_t)gridDim.x * kStepThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kStepThreads + threadIdx.x; i < L.total; i += stride) {
    uint64_t off = 0;
    const int t = policy_packed_word(i, L, D, &off);
    float w = 0.f;
    if (t >= 0) {
      float* pp = policy_tensor(a.p, t) + off;
      float* pm = policy_tensor(a.m, t) + off;
      float* pv = policy_tensor(a.v, t) + off;
      const float g = coef * policy_tensor(a.g, t)[off];
      float m = *pm, v = *pv;
      m = m + a.w1 * (g - m);
      v = a.beta2 * v + (a.w2 * g) * g;
      const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
      w = *pp + (-a.step_size * m) / denom;
      *pp = w;
      *pm = m;
      *pv = v;
    }
    a.packed[i] = w;
  }
}

struct AdvStatsArgs {
  const float* adv;
  const int64_t* indices;
  uint64_t B, T, N;
  float* out;
  const uint32_t* stop_at;  // pgtg_ppo_adv_stats_ex's gate; NULL: none
  uint32_t ordinal;
};

// the advantage of batch position s; an index outside the rollout stands as 0
__device__ __forceinline__ float adv_gather(const AdvStatsArgs& a, uint64_t s) {
  uint64_t e, t;
  return ppo_sample(a.indices[s], a.T, a.N, &e, &t) ? a.adv[t * a.N + e] : 0.f;
}

__global__ void __launch_bounds__(kAdvThreads) k_ppo_adv_stats(AdvStatsArgs a) {
  __shared__ double red[kAdvThreads];
  const uint32_t tid = threadIdx.x;
  const uint64_t B = a.B;
  if (ppo_gated(a.stop_at, a.ordinal, false)) return;
  double s[kStepSets] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t i0 = tid; i0 < B; i0 += kStepSets * kAdvThreads)
#pragma unroll
    for (int j = 0; j < kStepSets; j++)
      if (i0 + j * kAdvThreads < B) s[j] += adv_gather(a, i0 + j * kAdvThreads);
  red[tid] = (s[0] + s[1]) + (s[2] + s[3]);
  const double mean = step_tree<kAdvThreads>(red, tid) / (double)B;
  __syncthreads();  // (every thread has read red[0])
#pragma unroll
  for (int j = 0; j < kStepSets; j++) s[j] = 0.0;
  for (uint64_t i0 = tid; i0 < B; i0 += kStepSets * kAdvThreads)
#pragma unroll
    for (int j = 0; j < kStepSets; j++)
      if (i0 + j * kAdvThreads < B) {
        const double d = (double)adv_gather(a, i0 + j * kAdvThreads) - mean;
        s[j] += d * d;
      }
  red[tid] = (s[0] + s[1]) + (s[2] + s[3]);
  const double var = step_tree<kAdvThreads>(red, tid) / (double)(B - 1);
  if (tid == 0) {
    a.out[0] = (float)mean;
    a.out[1] = 1.f / ((float)sqrt(var) + 1e-8f);
  }
}

}  // namespace pgtg
#endif  // PGTG_PPO_STEP_H_
