// tests/csrc/rng_probe.hip -- TEST INFRASTRUCTURE ONLY.
// The device RNG of pgtg_amd/csrc/pgtg_device.h on its own, one lane per (seed, spawn key) stream:
// each lane seeds its stream like the product (ss_pool / ss_child), runs a host-given script of
// draws and writes every value and the final Pcg state, for comparison with live numpy on the host
// (tests/test_gpu_rng_probe.py).  Nothing of pgtg_env.hip is included; the product library and its
// ABI are untouched.
#include "../../pgtg_amd/csrc/pgtg_device.h"

using namespace pgtg;

// script op kinds ({kind, n} pairs); the value written per op is a u64
enum {
  OP_PCG_INT = 0,         // pcg_int(g, n)
  OP_DRAW_INT = 1,        // pcg_draw(g, true, n), n >= 2
  OP_DRAW_DBL = 2,        // pcg_draw(g, false, 0): random()'s 53-bit mantissa
  OP_AHEAD_DRAW_INT = 3,  // ahead_draw(a, true, n), n >= 2
  OP_AHEAD_DRAW_DBL = 4,  // ahead_draw(a, false, 0)
  OP_AHEAD_INT = 5,       // ahead_int(a, n)
  OP_NEXT32 = 6,          // pcg_next32(g)
  OP_ADVANCE_NEXT64 = 7,  // pcg_advance(g, n, kJumpBits) then pcg_next64(g)
  OP_ADVANCE = 8          // pcg_advance(g, n, kJumpBits) alone (value 0)
};

// persist != 0: the lane keeps one PcgAhead over the whole script (the OP_AHEAD_* kinds only), as the
// kernels' car loops do; else an ahead op wraps the plain state (ahead_init .. a.g) for that op alone.
// script_stride: u32 words between the scripts of consecutive streams (0: one script for all).
__global__ void k_rng_probe(const uint64_t* seeds, const uint32_t* keys, int n_streams, const uint32_t* script,
                            int n_ops, int script_stride, int persist, uint64_t* init_state, uint64_t* values,
                            uint64_t* final_state) {
  const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_streams) return;
  Pcg g = ss_child(ss_pool(seeds[s]), keys[s]);
  uint64_t* is = init_state + (size_t)s * 6;
  is[0] = g.shi; is[1] = g.slo; is[2] = g.ihi; is[3] = g.ilo; is[4] = g.buf; is[5] = g.has;
  const uint32_t* sc = script + (size_t)s * (size_t)script_stride;
  uint64_t* out = values + (size_t)s * (size_t)n_ops;
  PcgAhead pa = ahead_init(g);
  for (int j = 0; j < n_ops; j++) {
    const uint32_t kind = sc[2 * j], n = sc[2 * j + 1];
    uint64_t v = 0xDEADDEADDEADDEADull;
    if (kind >= OP_AHEAD_DRAW_INT && kind <= OP_AHEAD_INT) {
      PcgAhead a = persist ? pa : ahead_init(g);
      if (kind == OP_AHEAD_DRAW_INT) v = ahead_draw(a, true, n);
      else if (kind == OP_AHEAD_DRAW_DBL) v = ahead_draw(a, false, 0u);
      else v = ahead_int(a, n);
      if (persist) pa = a;
      else g = a.g;
    } else if (!persist) {
      if (kind == OP_PCG_INT) v = pcg_int(g, n);
      else if (kind == OP_DRAW_INT) v = pcg_draw(g, true, n);
      else if (kind == OP_DRAW_DBL) v = pcg_draw(g, false, 0u);
      else if (kind == OP_NEXT32) v = pcg_next32(g);
      else if (kind == OP_ADVANCE_NEXT64) {
        pcg_advance(g, n, kJumpBits);
        v = pcg_next64(g);
      } else if (kind == OP_ADVANCE) {
        pcg_advance(g, n, kJumpBits);
        v = 0;
      }
    }
    out[j] = v;
  }
  if (persist) g = pa.g;
  uint64_t* fs = final_state + (size_t)s * 6;
  fs[0] = g.shi; fs[1] = g.slo; fs[2] = g.ihi; fs[3] = g.ilo; fs[4] = g.buf; fs[5] = g.has;
}

// sizeof(Tables): the constant-table bytes that every k_traffic workgroup adds to its LDS budget
// (tests/test_gpu_lemire.py derives the envs a wave can hold from it)
extern "C" int rng_probe_tables_bytes() { return (int)sizeof(Tables); }

#define PROBE_TRY(x)                 \
  do {                               \
    hipError_t e_ = (x);             \
    if (e_ != hipSuccess) {          \
      rc = (int)e_;                  \
      goto done;                     \
    }                                \
  } while (0)

// Host entry (ctypes): all pointers are host memory.  script holds n_ops {kind, n} pairs, once
// (per_stream == 0) or per stream.  init_state / final_state: [n_streams][6] = shi, slo, ihi, ilo, buf,
// has; values: [n_streams][n_ops].  Returns 0 or the HIP error code.
extern "C" int rng_probe_run(const uint64_t* seeds, const uint32_t* keys, int n_streams, const uint32_t* script,
                             int n_ops, int per_stream, int persist, uint64_t* init_state, uint64_t* values,
                             uint64_t* final_state) {
  if (n_streams <= 0 || n_ops <= 0) return -1;
  int rc = 0;
  uint64_t *d_seeds = nullptr, *d_init = nullptr, *d_val = nullptr, *d_fin = nullptr;
  uint32_t *d_keys = nullptr, *d_script = nullptr;
  const size_t n_script = (size_t)2 * n_ops * (per_stream ? (size_t)n_streams : 1u);
  const size_t n_val = (size_t)n_streams * n_ops, n_st = (size_t)n_streams * 6;
  PROBE_TRY(hipMalloc(&d_seeds, sizeof(uint64_t) * n_streams));
  PROBE_TRY(hipMalloc(&d_keys, sizeof(uint32_t) * n_streams));
  PROBE_TRY(hipMalloc(&d_script, sizeof(uint32_t) * n_script));
  PROBE_TRY(hipMalloc(&d_init, sizeof(uint64_t) * n_st));
  PROBE_TRY(hipMalloc(&d_val, sizeof(uint64_t) * n_val));
  PROBE_TRY(hipMalloc(&d_fin, sizeof(uint64_t) * n_st));
  PROBE_TRY(hipMemcpy(d_seeds, seeds, sizeof(uint64_t) * n_streams, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_keys, keys, sizeof(uint32_t) * n_streams, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemcpy(d_script, script, sizeof(uint32_t) * n_script, hipMemcpyHostToDevice));
  PROBE_TRY(hipMemset(d_val, 0, sizeof(uint64_t) * n_val));
  hipLaunchKernelGGL(k_rng_probe, dim3((unsigned)((n_streams + 63) / 64)), dim3(64), 0, 0, d_seeds, d_keys, n_streams,
                     d_script, n_ops, per_stream ? 2 * n_ops : 0, persist, d_init, d_val, d_fin);
  PROBE_TRY(hipGetLastError());
  PROBE_TRY(hipDeviceSynchronize());
  PROBE_TRY(hipMemcpy(init_state, d_init, sizeof(uint64_t) * n_st, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(values, d_val, sizeof(uint64_t) * n_val, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(final_state, d_fin, sizeof(uint64_t) * n_st, hipMemcpyDeviceToHost));
done:
  (void)hipFree(d_seeds);
  (void)hipFree(d_keys);
  (void)hipFree(d_script);
  (void)hipFree(d_init);
  (void)hipFree(d_val);
  (void)hipFree(d_fin);
  return rc;
}
