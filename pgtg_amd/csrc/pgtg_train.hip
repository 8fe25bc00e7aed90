// pgtg_amd/csrc/pgtg_train.hip -- the training half of the C ABI: GAE, the cost scan, reward normalisation,
// evaluation, the MlpPolicy forward pass and the PPO update.
//
// Their kernels live in the eight headers below and know nothing of the environment's state, tables or build
// variants, so this file is compiled once and linked into the product library and every variant of it.  Of a
// handle it knows what pgtg_host.h gives and no more.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>

#include "pgtg_eval.h"
#include "pgtg_rollout.h"
#include "pgtg_cost.h"
#include "pgtg_norm.h"
#include "pgtg_policy.h"
#include "pgtg_ppo.h"
#include "pgtg_ppo_step.h"
#include "pgtg_ppo_log.h"
#include "pgtg_host.h"

using namespace pgtg;

// Where an entry point has refused all it refuses: the handle's device made current, and what it launches with
// in `c`.  (The text is the one HIPCHK gives the call where it stands in pgtg_env.hip's entry points.)
static int enter(pgtg_handle* h, pgtg_host* c) {
  *c = pgtg_host_of(h);
  const hipError_t e = hipSetDevice(c->device);
  return e == hipSuccess ? PGTG_OK : pgtg_hip_failed(h, e, "hipSetDevice(h->device)");
}

// What bounds a rollout for the launch geometry of a kernel with one env per thread of `block`
static bool rollout_too_large(uint64_t n, uint64_t steps, uint64_t block) {
  return (n + block - 1) / block > 0x7fffffffull || steps > 0x7fffffffull || steps + 1 > UINT64_MAX / 4 / n;
}

extern "C" {

// GAE over a rollout (pgtg_rollout.h): the handle gives the device, the stream and the error string
int pgtg_gae(pgtg_handle* h, const PgtgGae* a) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_gae: no arguments");
  if (a->steps == 0) return fail(h, PGTG_E_INVALID, "pgtg_gae: steps must be at least 1");
  if (!a->rewards || !a->values || !a->dones || !a->last_values || !a->advantages || !a->returns)
    return fail(h, PGTG_E_INVALID, "pgtg_gae: rewards, values, dones, last_values, advantages and returns are required");
  if ((a->truncated_only == nullptr) != (a->terminal_values == nullptr))
    return fail(h, PGTG_E_INVALID, "pgtg_gae: truncated_only and terminal_values: both or neither");
  if (!std::isfinite(a->gamma) || !std::isfinite(a->gae_lambda))
    return fail(h, PGTG_E_INVALID, "pgtg_gae: gamma and gae_lambda must be finite");
  if (a->n == 0) return PGTG_OK;
  const uint64_t grid = (a->n + kGaeBlock - 1) / kGaeBlock;
  if (rollout_too_large(a->n, a->steps, kGaeBlock))
    return fail(h, PGTG_E_UNSUPPORTED, "pgtg_gae: the rollout is too large for one launch");
  GaeArgs g;
  g.rew = a->rewards;
  g.val = a->values;
  g.dones = a->dones;
  g.tonly = a->truncated_only;
  g.tval = a->terminal_values;
  g.last_values = a->last_values;
  g.adv = a->advantages;
  g.ret = a->returns;
  g.n = a->n;
  g.steps = a->steps;
  g.g = (float)a->gamma;
  g.gl = (float)(a->gamma * a->gae_lambda);  // (SB3: the product in double, rounded once)
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  if (g.tonly) hipLaunchKernelGGL(k_gae<true>, dim3((unsigned)grid), dim3(kGaeBlock), 0, ctx.stream, g);
  else hipLaunchKernelGGL(k_gae<false>, dim3((unsigned)grid), dim3(kGaeBlock), 0, ctx.stream, g);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// The cost scan of a rollout and the multiplier's dual ascent (pgtg_cost.h): the handle gives the device,
// the stream and the error string
int pgtg_cost_workspace_bytes(uint64_t n, uint64_t* bytes) {
  if (!bytes || n > (1ull << 40)) return PGTG_E_INVALID;
  *bytes = (n + kCostBlock - 1) / kCostBlock * sizeof(CostPartial);
  return PGTG_OK;
}

int pgtg_cost_scan(pgtg_handle* h, const PgtgCost* a) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_cost_scan: no arguments");
  if (a->steps == 0) return fail(h, PGTG_E_INVALID, "pgtg_cost_scan: steps must be at least 1");
  if (!a->rewards || !a->costs || !a->dones || !a->ep_cost || !a->penalised || !a->lambda || !a->summary || !a->workspace)
    return fail(h, PGTG_E_INVALID,
                "pgtg_cost_scan: rewards, costs, dones, ep_cost, penalised, lambda, summary and workspace are required");
  if ((((uintptr_t)a->ep_cost | (uintptr_t)a->summary | (uintptr_t)a->workspace) & 7u) || ((uintptr_t)a->lambda & 3u))
    return fail(h, PGTG_E_INVALID, "pgtg_cost_scan: ep_cost, summary and workspace 8-byte aligned, lambda 4-byte aligned");
  if (!std::isfinite(a->cost_limit) || !std::isfinite(a->lambda_lr))
    return fail(h, PGTG_E_INVALID, "pgtg_cost_scan: cost_limit and lambda_lr must be finite");
  if (!(a->lambda_max >= 0.0)) return fail(h, PGTG_E_INVALID, "pgtg_cost_scan: lambda_max must be at least 0");
  if (a->n == 0) return PGTG_OK;
  const uint64_t grid = (a->n + kCostBlock - 1) / kCostBlock;
  if (rollout_too_large(a->n, a->steps, kCostBlock))
    return fail(h, PGTG_E_UNSUPPORTED, "pgtg_cost_scan: the rollout is too large for one launch");
  CostArgs c;
  c.rew = a->rewards;
  c.cost = a->costs;
  c.dones = a->dones;
  c.ep_cost = a->ep_cost;
  c.pen = a->penalised;
  c.lambda = a->lambda;
  c.summary = a->summary;
  c.rows = reinterpret_cast<CostPartial*>(a->workspace);
  c.n = a->n;
  c.steps = a->steps;
  c.n_rows = grid;
  c.cost_limit = a->cost_limit;
  c.lambda_lr = a->lambda_lr;
  c.lambda_max = a->lambda_max;
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_cost_scan, dim3((unsigned)grid), dim3(kCostBlock), 0, ctx.stream, c);
  hipLaunchKernelGGL(k_cost_dual, dim3(1), dim3(kCostBlock), 0, ctx.stream, c);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// Running return normalisation of a rollout's reward (pgtg_norm.h): the handle gives the device, the stream
// and the error string
int pgtg_reward_norm_workspace_bytes(uint64_t n, uint64_t steps, uint64_t* bytes) {
  if (!bytes || n > (1ull << 40) || steps > 0x7fffffffull) return PGTG_E_INVALID;
  if (n && steps && rollout_too_large(n, steps, kNormBlock)) return PGTG_E_UNSUPPORTED;
  // the waves' partials of every step, then every step's merged moments
  *bytes = steps * ((n + kNormPartial - 1) / kNormPartial + (n ? 1 : 0)) * sizeof(RetPartial);
  return PGTG_OK;
}

int pgtg_reward_norm(pgtg_handle* h, const PgtgRewardNorm* a) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: no arguments");
  if (a->steps == 0) return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: steps must be at least 1");
  if (!a->rewards || !a->dones || !a->returns || !a->rms || !a->row_var || !a->normalised || !a->workspace)
    return fail(h, PGTG_E_INVALID,
                "pgtg_reward_norm: rewards, dones, returns, rms, row_var, normalised and workspace are required");
  if (((uintptr_t)a->returns | (uintptr_t)a->rms | (uintptr_t)a->row_var | (uintptr_t)a->workspace) & 7u)
    return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: returns, rms, row_var and workspace 8-byte aligned");
  if ((uintptr_t)a->rewards & 3u || (uintptr_t)a->normalised & 3u)
    return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: rewards and normalised 4-byte aligned");
  if (!std::isfinite(a->epsilon) || a->epsilon < 0.0 || !std::isfinite(a->clip) || a->clip < 0.0)
    return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: epsilon and clip must be finite and at least 0");
  if (!(a->gamma >= 0.0 && a->gamma <= 1.0)) return fail(h, PGTG_E_INVALID, "pgtg_reward_norm: gamma must be in [0, 1]");
  if (a->n == 0) return PGTG_OK;
  if (rollout_too_large(a->n, a->steps, kNormBlock))
    return fail(h, PGTG_E_UNSUPPORTED, "pgtg_reward_norm: the rollout is too large for one launch");
  NormArgs c;
  c.rew = a->rewards;
  c.dones = a->dones;
  c.ret = a->returns;
  c.rms = a->rms;
  c.row_var = a->row_var;
  c.out = a->normalised;
  c.n = a->n;
  c.steps = a->steps;
  c.n_part = (a->n + kNormPartial - 1) / kNormPartial;
  c.rows = reinterpret_cast<RetPartial*>(a->workspace);
  c.batch = c.rows + a->steps * c.n_part;
  c.gamma = a->gamma;
  c.epsilon = a->epsilon;
  c.clip = a->clip;
  c.training = a->training != 0;
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  if (c.training) {
    const unsigned grid = (unsigned)((a->n + kNormBlock - 1) / kNormBlock);
    hipLaunchKernelGGL(k_ret_scan, dim3(grid), dim3(kNormBlock), 0, ctx.stream, c);
    hipLaunchKernelGGL(k_ret_stats<false>, dim3((unsigned)a->steps), dim3(kNormBlock), 0, ctx.stream, c);
    hipLaunchKernelGGL(k_ret_stats<true>, dim3(1), dim3(kNormBlock), 0, ctx.stream, c);
  }
  const uint64_t per = (uint64_t)kNormBlock * kNormApplyCols;
  const dim3 grid((unsigned)((a->n + per - 1) / per), (unsigned)std::min<uint64_t>(a->steps, 65535));
  hipLaunchKernelGGL(k_ret_apply, grid, dim3(kNormBlock), 0, ctx.stream, c);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// Quota-aware evaluation (pgtg_eval.h).  What both entry points check before they launch; 0 = fine.
static int eval_check(pgtg_handle* h, const PgtgEval* a, const char* who, bool step) {
  const std::string w(who);
  if (!a) return fail(h, PGTG_E_INVALID, w + ": no arguments");
  if (a->n != pgtg_host_of(h).n) return fail(h, PGTG_E_INVALID, w + ": n must be the handle's env count");
  if (a->n_episodes == 0) return fail(h, PGTG_E_INVALID, w + ": n_episodes must be at least 1");
  if (!(a->gamma >= 0.0 && a->gamma <= 1.0)) return fail(h, PGTG_E_INVALID, w + ": gamma must be in [0, 1]");
  if (!a->cnt || !a->rec_return || !a->rec_discounted || !a->rec_length || !a->rec_last_reward || !a->rec_end_step ||
      !a->rec_flags)
    return fail(h, PGTG_E_INVALID, w + ": cnt and the six record arrays are required");
  if (step && (!a->reward || !a->terminated || !a->truncated || !a->ret || !a->disc || !a->g || !a->len || !a->open_rows))
    return fail(h, PGTG_E_INVALID, w + ": reward, terminated, truncated, ret, disc, g, len and open_rows are required");
  const uint64_t q = a->n_episodes / a->n + (a->n_episodes % a->n ? 1 : 0);
  if (a->step > 0x7fffffffull || q > 0x7fffffffull || q > (1ull << 60) / a->n)
    return fail(h, PGTG_E_INVALID, w + ": step, or the episode slots per env, is too large");
  return 0;
}

int pgtg_eval_workspace_bytes(uint64_t n, uint64_t n_episodes, uint64_t* bytes) {
  (void)n_episodes;  // (the partials are per 256 envs whatever the quotas)
  if (!bytes || n == 0 || n > (1ull << 40)) return PGTG_E_INVALID;
  *bytes = (n + kEvalBlock - 1) / kEvalBlock * sizeof(EvalPartial);
  return PGTG_OK;
}

int pgtg_eval_step(pgtg_handle* h, const PgtgEval* a) {
  if (!h) return PGTG_E_INVALID;
  if (int rc = eval_check(h, a, "pgtg_eval_step", true)) return rc;
  const uint64_t grid = (a->n + kEvalBlock - 1) / kEvalBlock;
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_eval, dim3((unsigned)grid), dim3(kEvalBlock), 0, ctx.stream, *a);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

int pgtg_eval_summary(pgtg_handle* h, const PgtgEval* a, PgtgEvalSummary* out_dev, void* workspace) {
  if (!h) return PGTG_E_INVALID;
  if (int rc = eval_check(h, a, "pgtg_eval_summary", false)) return rc;
  if (!out_dev || !workspace || ((uintptr_t)workspace & 7) || ((uintptr_t)out_dev & 7))
    return fail(h, PGTG_E_INVALID, "pgtg_eval_summary: out_dev and workspace are required, 8-byte aligned");
  EvalReduceArgs r;
  r.ev = *a;
  r.rows = reinterpret_cast<EvalPartial*>(workspace);
  r.out = out_dev;
  r.n_rows = (a->n + kEvalBlock - 1) / kEvalBlock;
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  for (int pass = 0; pass < 2; pass++) {  // the means, then the squared deviations about them
    r.pass = pass;
    hipLaunchKernelGGL(k_eval_reduce, dim3((unsigned)r.n_rows), dim3(kEvalBlock), 0, ctx.stream, r);
    hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(kEvalBlock), 0, ctx.stream, r);
  }
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// The MlpPolicy forward pass (pgtg_policy.h): the handle gives the device, the stream and the error string
int pgtg_policy_chunk(void) { return kPolChunk; }

// The public structs of twelve pointers (PgtgPolicyWeights, PgtgPpoGrads, PgtgPpoConstGrads) share their
// field names with the kernels' PolicyTensors: all twelve set, and the copy of one into another
static const auto all12 = [](const auto& s) {
  return s.w1p && s.b1p && s.w2p && s.b2p && s.wa && s.ba && s.w1v && s.b1v && s.w2v && s.b2v && s.wv && s.bv;
};
static const auto put12 = [](auto& d, const auto& s) {
  d.w1p = s.w1p, d.b1p = s.b1p, d.w2p = s.w2p, d.b2p = s.b2p, d.wa = s.wa, d.ba = s.ba;
  d.w1v = s.w1v, d.b1v = s.b1v, d.w2v = s.w2v, d.b2v = s.b2v, d.wv = s.wv, d.bv = s.bv;
};

// The two refusals every entry point of the policy and of PPO shares, under the entry point's name `fn`
static bool obs_dim_ok(uint64_t obs_dim) { return obs_dim >= 1 && obs_dim <= kPolMaxObsDim; }
static int check_obs_dim(pgtg_handle* h, const char* fn, uint64_t obs_dim) {
  if (obs_dim_ok(obs_dim)) return PGTG_OK;
  return fail(h, PGTG_E_INVALID, std::string(fn) + ": obs_dim outside [1, PGTG_POLICY_MAX_OBS_DIM]");
}
static int check_packed(pgtg_handle* h, const char* fn, const void* packed) {
  if (!((uintptr_t)packed & 15u)) return PGTG_OK;
  return fail(h, PGTG_E_INVALID, std::string(fn) + ": packed must be 16-byte aligned");
}

int pgtg_policy_packed_bytes(uint64_t obs_dim, uint64_t* bytes) {
  if (!bytes || !obs_dim_ok(obs_dim)) return PGTG_E_INVALID;
  *bytes = policy_layout(obs_dim).total * sizeof(float);
  return PGTG_OK;
}

int pgtg_policy_pack(pgtg_handle* h, const PgtgPolicyWeights* raw, void* packed) {
  if (!h) return PGTG_E_INVALID;
  if (!raw || !packed) return fail(h, PGTG_E_INVALID, "pgtg_policy_pack: no weights or no packed buffer");
  if (int e = check_obs_dim(h, "pgtg_policy_pack", raw->obs_dim)) return e;
  if (!all12(*raw)) return fail(h, PGTG_E_INVALID, "pgtg_policy_pack: all twelve weight pointers are required");
  if (int e = check_packed(h, "pgtg_policy_pack", packed)) return e;
  PolicyPackArgs p;
  put12(p.src, *raw);
  p.out = (float*)packed;
  p.obs_dim = raw->obs_dim;
  const uint64_t total = policy_layout(raw->obs_dim).total;
  const uint64_t grid = std::min<uint64_t>((total + 255) / 256, 4096);
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_policy_pack, dim3((unsigned)grid), dim3(256), 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

int pgtg_policy(pgtg_handle* h, const PgtgPolicy* a) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_policy: no arguments");
  if (a->obs_dim == 0) return fail(h, PGTG_E_INVALID, "pgtg_policy: obs_dim must be at least 1");
  if (a->obs_dim > kPolMaxObsDim)
    return fail(h, PGTG_E_INVALID, "pgtg_policy: obs_dim beyond PGTG_POLICY_MAX_OBS_DIM, the largest the pack supports");
  if (!a->obs || !a->packed) return fail(h, PGTG_E_INVALID, "pgtg_policy: obs and packed are required");
  if (int e = check_packed(h, "pgtg_policy", a->packed)) return e;
  if (a->mode != PGTG_POLICY_SAMPLE && a->mode != PGTG_POLICY_ARGMAX && a->mode != PGTG_POLICY_VALUE_ONLY)
    return fail(h, PGTG_E_INVALID, "pgtg_policy: mode 0 sample, 1 argmax, 2 value only");
  if (a->mode == PGTG_POLICY_VALUE_ONLY && !a->values)
    return fail(h, PGTG_E_INVALID, "pgtg_policy: value-only mode needs the values output");
  if (a->n > (UINT64_MAX >> 1) / a->obs_dim || (uintptr_t)a->obs > UINTPTR_MAX - a->n * a->obs_dim)
    return fail(h, PGTG_E_INVALID, "pgtg_policy: n * obs_dim overflows");
  if (a->n == 0) return PGTG_OK;
  const uint64_t grid = (a->n + kPolRows - 1) / kPolRows;
  if (grid > 0x7fffffffull) return fail(h, PGTG_E_UNSUPPORTED, "pgtg_policy: the batch is too large for one launch");
  PolicyArgs p;
  p.obs = a->obs;
  p.packed = (const float*)a->packed;
  p.uniforms = a->uniforms;
  p.actions = a->actions;
  p.values = a->values;
  p.log_probs = a->log_probs;
  p.n = a->n;
  p.obs_dim = a->obs_dim;
  p.seed = a->seed;
  p.counter = a->counter;
  p.env_offset = a->env_offset;
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  const dim3 g((unsigned)grid), b(kPolThreads);
  if (a->mode == PGTG_POLICY_SAMPLE) hipLaunchKernelGGL(k_policy<POLICY_SAMPLE>, g, b, 0, ctx.stream, p);
  else if (a->mode == PGTG_POLICY_ARGMAX) hipLaunchKernelGGL(k_policy<POLICY_ARGMAX>, g, b, 0, ctx.stream, p);
  else hipLaunchKernelGGL(k_policy<POLICY_VALUE_ONLY>, g, b, 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// One PPO minibatch gradient (pgtg_ppo.h): the handle gives the device, the stream, the error string and
// the error bytes that count the skipped samples
int pgtg_ppo_workspace_bytes(uint64_t obs_dim, uint64_t batch, uint64_t* bytes) {
  if (!bytes || !obs_dim_ok(obs_dim)) return PGTG_E_INVALID;
  if (batch > (UINT64_MAX >> 12) / obs_dim) return PGTG_E_INVALID;  // (segments <= blocks: total < 2^11 batch obs_dim floats)
  *bytes = batch ? ppo_plan(batch, obs_dim).total * sizeof(float) : 0;
  return PGTG_OK;
}

// The refusals of a PgtgPpoExtra, under the entry point's name `fn`; reads_flags: `fn` is the one that reads
// clip_range_vf and target_kl (the others take the gate alone)
static int check_extra(pgtg_handle* h, const char* fn, const PgtgPpoExtra* x, bool reads_flags) {
  if (!x) return PGTG_OK;
  const std::string f(fn);
  if (x->flags & ~(PGTG_PPO_CLIP_VF | PGTG_PPO_TARGET_KL)) return fail(h, PGTG_E_INVALID, f + ": unknown flags in extra");
  if (reads_flags && (x->flags & PGTG_PPO_CLIP_VF)) {
    if (!(std::isfinite(x->clip_range_vf) && x->clip_range_vf >= 0.0))
      return fail(h, PGTG_E_INVALID, f + ": clip_range_vf must be finite and at least 0");
    if (!x->old_values) return fail(h, PGTG_E_INVALID, f + ": clip_range_vf needs old_values");
    if ((uintptr_t)x->old_values & 3u) return fail(h, PGTG_E_INVALID, f + ": old_values must be 4-byte aligned");
  }
  if (reads_flags && (x->flags & PGTG_PPO_TARGET_KL)) {
    if (!(std::isfinite(x->target_kl) && x->target_kl >= 0.0))
      return fail(h, PGTG_E_INVALID, f + ": target_kl must be finite and at least 0");
    if (!x->stop_at) return fail(h, PGTG_E_INVALID, f + ": target_kl needs stop_at");
  }
  if (x->stop_at) {
    if ((uintptr_t)x->stop_at & 3u) return fail(h, PGTG_E_INVALID, f + ": stop_at must be 4-byte aligned");
    if (x->ordinal == 0) return fail(h, PGTG_E_INVALID, f + ": ordinal counts from 1 where stop_at is set");
  }
  return PGTG_OK;
}

int pgtg_ppo_grad(pgtg_handle* h, const PgtgPpoGrad* a) { return pgtg_ppo_grad_ex(h, a, nullptr); }

int pgtg_ppo_grad_ex(pgtg_handle* h, const PgtgPpoGrad* a, const PgtgPpoExtra* x) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: no arguments");
  if (int e = check_obs_dim(h, "pgtg_ppo_grad", a->obs_dim)) return e;
  if (a->steps == 0 || a->n == 0) return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: steps and n must be at least 1");
  if (!a->obs || !a->indices || !a->actions || !a->log_probs || !a->advantages || !a->returns || !a->packed ||
      !a->workspace || !a->stats)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: obs, indices, the rollout arrays, packed, workspace and stats are required");
  if (!all12(a->grads)) return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: all twelve gradient pointers are required");
  if (int e = check_packed(h, "pgtg_ppo_grad", a->packed)) return e;
  if ((uintptr_t)a->workspace & 15u) return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: workspace must be 16-byte aligned");
  if (a->n > (UINT64_MAX >> 1) / a->obs_dim || a->steps > (UINT64_MAX >> 1) / a->n)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: n * obs_dim or steps * n overflows");
  if (a->obs_pitch < a->n * a->obs_dim) return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: obs_pitch is below n * obs_dim");
  if (a->obs_pitch > (UINT64_MAX >> 1) / a->steps || (uintptr_t)a->obs > UINTPTR_MAX - a->steps * a->obs_pitch)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: steps * obs_pitch overflows");
  if (a->batch > (UINT64_MAX >> 12) / a->obs_dim)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: batch * obs_dim overflows");
  if (!std::isfinite(a->clip_range) || !std::isfinite(a->ent_coef) || !std::isfinite(a->vf_coef))
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_grad: clip_range, ent_coef and vf_coef must be finite");
  if (int e = check_extra(h, "pgtg_ppo_grad_ex", x, true)) return e;
  if (a->batch == 0) return PGTG_OK;
  const PpoPlan pl = ppo_plan(a->batch, a->obs_dim);
  const uint64_t rgrid = (128 * a->obs_dim + kPpoSlot + kPpoThreads - 1) / kPpoThreads;
  if (pl.blocks > 0x7fffffffull || pl.dtiles > 0x7fffffffull || pl.segs > 65535 || rgrid > 0x7fffffffull)
    return fail(h, PGTG_E_UNSUPPORTED, "pgtg_ppo_grad: the batch is too large for one launch");
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  PpoArgs p;
  p.obs = a->obs;
  p.pitch = a->obs_pitch;
  p.T = a->steps;
  p.N = a->n;
  p.D = a->obs_dim;
  p.B = a->batch;
  p.indices = a->indices;
  p.actions = a->actions;
  p.old_logp = a->log_probs;
  p.adv = a->advantages;
  p.ret = a->returns;
  p.packed = (const float*)a->packed;
  p.adv_stats = a->adv_stats;
  p.clip = (float)a->clip_range;
  p.clip_lo = (float)(1.0 - a->clip_range);
  p.clip_hi = (float)(1.0 + a->clip_range);
  p.ent_coef = (float)a->ent_coef;
  p.vf_coef = (float)a->vf_coef;
  p.ws = (float*)a->workspace;
  p.err = ctx.err_bytes;
  p.err_n = ctx.err_bytes ? ctx.n : 0;
  put12(p.g, a->grads);
  p.stats = a->stats;
  const bool clip_vf = x && (x->flags & PGTG_PPO_CLIP_VF), kl = x && (x->flags & PGTG_PPO_TARGET_KL);
  p.old_values = clip_vf ? x->old_values : nullptr;
  p.clip_vf = clip_vf ? (float)x->clip_range_vf : 0.f;
  p.stop_at = x ? x->stop_at : nullptr;
  p.ordinal = x && x->stop_at ? x->ordinal : 0;
  p.has_kl = kl ? 1u : 0u;
  p.kl_limit = kl ? 1.5f * (float)x->target_kl : 0.f;
  hipLaunchKernelGGL(k_ppo_loss, dim3((unsigned)pl.blocks), dim3(kPpoThreads), 0, ctx.stream, p);
  hipLaunchKernelGGL(k_ppo_dw1, dim3((unsigned)pl.dtiles, (unsigned)pl.segs), dim3(kPpoThreads), 0, ctx.stream, p);
  hipLaunchKernelGGL(k_ppo_reduce, dim3((unsigned)rgrid), dim3(kPpoThreads), 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// The optimiser step of a PPO minibatch and the advantage statistics (pgtg_ppo_step.h): the handle gives the
// device, the stream and the error string
int pgtg_ppo_step_workspace_bytes(uint64_t obs_dim, uint64_t* bytes) {
  if (!bytes || !obs_dim_ok(obs_dim)) return PGTG_E_INVALID;
  *bytes = (step_blocks(obs_dim) * sizeof(double) + 15) & ~(uint64_t)15;
  return PGTG_OK;
}

// The double a caller rounded to the float x: its shortest decimal form that reads back as x (0.999f gives
// 0.999, where the plain widening gives 0.99900001287 and 1 - beta2 would be off by 1.3e-5 of itself).
static double widen_decimal(float x) {
  if (!std::isfinite(x)) return x;
  char buf[40];
  for (int prec = 1; prec <= 9; prec++) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)x);
    const double d = strtod(buf, nullptr);
    if ((float)d == x) return d;
  }
  return x;
}

int pgtg_ppo_step(pgtg_handle* h, const PgtgPpoStep* a) { return pgtg_ppo_step_ex(h, a, nullptr); }

int pgtg_ppo_step_ex(pgtg_handle* h, const PgtgPpoStep* a, const PgtgPpoExtra* x) {
  if (!h) return PGTG_E_INVALID;
  if (!a) return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: no arguments");
  if (int e = check_obs_dim(h, "pgtg_ppo_step", a->obs_dim)) return e;
  if (!all12(a->params) || !all12(a->grads) || !all12(a->exp_avg) || !all12(a->exp_avg_sq))
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: all twelve pointers of params, grads, exp_avg and exp_avg_sq are required");
  if (!a->packed || !a->workspace) return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: packed and workspace are required");
  if (int e = check_packed(h, "pgtg_ppo_step", a->packed)) return e;
  if ((uintptr_t)a->workspace & 7u) return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: workspace must be 8-byte aligned");
  if (a->step == 0) return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: step counts from 1");
  if (!std::isfinite(a->lr) || !std::isfinite(a->eps) || !std::isfinite(a->beta1) || !std::isfinite(a->beta2))
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: lr, eps, beta1 and beta2 must be finite");
  if (!(a->beta1 >= 0.f && a->beta1 < 1.f) || !(a->beta2 >= 0.f && a->beta2 < 1.f))
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: beta1 and beta2 must be in [0, 1)");
  if (!(a->max_grad_norm > 0.f))
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_step: max_grad_norm must be above 0 (+inf: no clip)");
  if (int e = check_extra(h, "pgtg_ppo_step_ex", x, false)) return e;
  PpoStepArgs p;
  p.stop_at = x ? x->stop_at : nullptr;
  p.ordinal = x && x->stop_at ? x->ordinal : 0;
  put12(p.p, a->params);
  put12(p.g, a->grads);
  put12(p.m, a->exp_avg);
  put12(p.v, a->exp_avg_sq);
  p.packed = (float*)a->packed;
  p.ws = (double*)a->workspace;
  p.grad_norm = a->grad_norm;
  p.D = a->obs_dim;
  // torch.optim.Adam's Python floats: the bias corrections and the step size in double, rounded once
  // (lr and the betas as the decimals the caller wrote: torch holds them as Python floats)
  const double b1 = widen_decimal(a->beta1), b2 = widen_decimal(a->beta2), st = (double)a->step;
  p.step_size = (float)(widen_decimal(a->lr) / (1.0 - pow(b1, st)));
  p.bc2_sqrt = (float)sqrt(1.0 - pow(b2, st));
  p.w1 = (float)(1.0 - b1);
  p.beta2 = a->beta2;
  p.w2 = (float)(1.0 - b2);
  p.eps = a->eps;
  p.max_norm = a->max_grad_norm;
  const uint64_t total = policy_layout(a->obs_dim).total;
  const uint64_t grid = std::min<uint64_t>((total + kStepThreads - 1) / kStepThreads, kStepPackMaxBlocks);
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_ppo_gnorm, dim3((unsigned)step_blocks(a->obs_dim)), dim3(kStepThreads), 0, ctx.stream, p);
  hipLaunchKernelGGL(k_ppo_adam, dim3((unsigned)grid), dim3(kStepThreads), 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

int pgtg_ppo_adv_stats(pgtg_handle* h, const void* advantages, const void* indices, uint64_t batch, uint64_t steps,
                       uint64_t n, float* out) {
  return pgtg_ppo_adv_stats_ex(h, advantages, indices, batch, steps, n, out, nullptr);
}

int pgtg_ppo_adv_stats_ex(pgtg_handle* h, const void* advantages, const void* indices, uint64_t batch, uint64_t steps,
                          uint64_t n, float* out, const PgtgPpoExtra* x) {
  if (!h) return PGTG_E_INVALID;
  if (!advantages || !indices || !out)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_adv_stats: advantages, indices and out are required");
  if (batch < 2) return fail(h, PGTG_E_INVALID, "pgtg_ppo_adv_stats: batch must be at least 2 (the unbiased std)");
  if (steps == 0 || n == 0) return fail(h, PGTG_E_INVALID, "pgtg_ppo_adv_stats: steps and n must be at least 1");
  if (steps > (UINT64_MAX >> 3) / n) return fail(h, PGTG_E_INVALID, "pgtg_ppo_adv_stats: steps * n overflows");
  if (int e = check_extra(h, "pgtg_ppo_adv_stats_ex", x, false)) return e;
  AdvStatsArgs p = {(const float*)advantages, (const int64_t*)indices, batch, steps, n, out, x ? x->stop_at : nullptr,
                    x && x->stop_at ? x->ordinal : 0};
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_ppo_adv_stats, dim3(1), dim3(kAdvThreads), 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

// The explained variance, the log and the permutation of an update (pgtg_ppo_log.h)
int pgtg_ppo_expl_var_workspace_bytes(uint64_t* bytes) {
  if (!bytes) return PGTG_E_INVALID;
  *bytes = 4 * (uint64_t)kEvMaxBlocks * sizeof(double);
  return PGTG_OK;
}

int pgtg_ppo_expl_var(pgtg_handle* h, const float* values, const float* returns, uint64_t count, void* workspace,
                      float* out) {
  if (!h) return PGTG_E_INVALID;
  if (!values || !returns || !workspace || !out)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_expl_var: values, returns, workspace and out are required");
  if (count == 0 || count > (1ull << 40)) return fail(h, PGTG_E_INVALID, "pgtg_ppo_expl_var: count must be in [1, 2^40]");
  if (((uintptr_t)values | (uintptr_t)returns | (uintptr_t)out) & 3u)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_expl_var: values, returns and out must be 4-byte aligned");
  if ((uintptr_t)workspace & 7u) return fail(h, PGTG_E_INVALID, "pgtg_ppo_expl_var: workspace must be 8-byte aligned");
  ExplVarArgs p = {values, returns, count, (double*)workspace, out};
  const dim3 g((unsigned)ev_blocks(count)), b(kEvThreads);
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_ppo_expl_var<0>, g, b, 0, ctx.stream, p);
  hipLaunchKernelGGL(k_ppo_expl_var<1>, g, b, 0, ctx.stream, p);
  hipLaunchKernelGGL(k_ppo_expl_var<2>, dim3(1), b, 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

int pgtg_ppo_log(pgtg_handle* h, const float* stats, uint64_t minibatches, uint64_t per_epoch, const uint32_t* stop_at,
                 const float* expl_var, PgtgPpoLog* out) {
  if (!h) return PGTG_E_INVALID;
  if (!stats || !out) return fail(h, PGTG_E_INVALID, "pgtg_ppo_log: stats and out are required");
  if ((uintptr_t)stats & 15u) return fail(h, PGTG_E_INVALID, "pgtg_ppo_log: stats must be 16-byte aligned");
  if (((uintptr_t)out | (uintptr_t)stop_at | (uintptr_t)expl_var) & 3u)
    return fail(h, PGTG_E_INVALID, "pgtg_ppo_log: out, stop_at and expl_var must be 4-byte aligned");
  if (per_epoch == 0) return fail(h, PGTG_E_INVALID, "pgtg_ppo_log: per_epoch must be at least 1");
  if (minibatches > (1ull << 31)) return fail(h, PGTG_E_INVALID, "pgtg_ppo_log: minibatches beyond 2^31");
  PpoLogArgs p = {stats, minibatches, per_epoch, stop_at, expl_var, out};
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  hipLaunchKernelGGL(k_ppo_log, dim3(1), dim3(64), 0, ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

int pgtg_ppo_perm(pgtg_handle* h, uint64_t total, uint64_t seed, uint64_t counter, int64_t* perm) {
  if (!h) return PGTG_E_INVALID;
  if (!perm) return fail(h, PGTG_E_INVALID, "pgtg_ppo_perm: perm is required");
  if ((uintptr_t)perm & 7u) return fail(h, PGTG_E_INVALID, "pgtg_ppo_perm: perm must be 8-byte aligned");
  if (total == 0 || total > (1ull << 38)) return fail(h, PGTG_E_INVALID, "pgtg_ppo_perm: total must be in [1, 2^38]");
  uint32_t bits = 0;
  while ((1ull << bits) < total) bits++;  // ceil(log2 total)
  pgtg_host ctx;
  if (int e = enter(h, &ctx)) return e;
  PermArgs p;
  p.perm = perm;
  p.total = total;
  p.key = seed ^ (counter * 0x9E3779B97F4A7C15ull) ^ 0x70706F5F7065726Dull;
  p.lo_bits = bits / 2;
  p.hi_bits = bits - bits / 2;
  p.err = ctx.err_bytes;
  p.err_n = ctx.err_bytes ? ctx.n : 0;
  hipLaunchKernelGGL(k_ppo_perm, dim3((unsigned)((total + kPermThreads - 1) / kPermThreads)), dim3(kPermThreads), 0,
                     ctx.stream, p);
  HIPCHK(h, hipGetLastError());
  return PGTG_OK;
}

}  // extern "C"
