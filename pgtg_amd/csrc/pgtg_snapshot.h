// pgtg_snapshot.h -- per-env state copies on the device (include/pgtg.h pgtg_snapshot_*): the gather /
// scatter kernel behind save, load and fork, and the table that describes the state sections to it.
// PGTGEnv.light_step's deepcopy (pgtg/environment.py:1283-1299) and env.clone() for single envs of a
// batch.  Included by pgtg_env.hip (device code and its launch arguments only).
#ifndef PGTG_SNAPSHOT_H_
#define PGTG_SNAPSHOT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgtg {

// How a state section (pgtg_env.hip state_sections) lays out its envs:
//   kSecRows   env-major [n][row bytes], an env's row contiguous;
//   kSecSlots  slot-major [rows][n] of 4-byte elements (the car slots and the occupancy counters);
//   kSecBatch  one value for the whole batch (the counters): in the blob, never copied per env.
enum : uint32_t { kSecRows = 0, kSecSlots = 1, kSecBatch = 2 };

constexpr int kCopyBlock = 256;      // lanes, and index pairs, per workgroup
constexpr int kMaxCopySections = 40; // (a traffic handle with the map queue has 35)

struct CopySection {
  const void* src;
  void* dst;
  uint64_t src_n, dst_n;  // envs of either side's arrays
  uint32_t kind;          // kSecRows / kSecSlots
  uint32_t row;           // kSecRows: bytes per env; kSecSlots: rows
  uint32_t unit;          // kSecRows: bytes per access, the largest of 16, 8, 4, 2, 1 that divides the
                          // row bytes and both base addresses
  uint32_t pad;
};

// passed by value (about 2 KB of kernel arguments)
struct CopyTable {
  CopySection sec[kMaxCopySections];
  const uint32_t* src_idx;  // [count] or null: k
  const uint32_t* dst_idx;
  uint64_t count;
  float* ep_ret;            // the destination handle's episode accumulators (zeroed for the envs
  int32_t* ep_len;          // written) or null
  uint32_t n_sections, pad;
};
static_assert(sizeof(CopyTable) <= 4096, "kernel argument block");

// env-major rows of one section for the workgroup's pairs: unit k of the flattened (pair, unit) list
// goes to lane k mod 256, so the lanes of a wave read and write consecutive units of a row, and of
// consecutive rows where the indices are consecutive
template <typename V>
__device__ __forceinline__ void copy_rows(const CopySection& e, const uint32_t* sp, const uint32_t* dp, uint32_t pairs) {
  const uint32_t U = e.row / (uint32_t)sizeof(V);
  const V* __restrict__ src = static_cast<const V*>(e.src);
  V* __restrict__ dst = static_cast<V*>(e.dst);
  const uint32_t total = pairs * U;  // (<= 256 pairs, rows far below 16 MiB)
  for (uint32_t i = threadIdx.x; i < total; i += kCopyBlock) {
    const uint32_t p = i / U, u = i - p * U;
    const uint64_t s = sp[p], d = dp[p];
    if (s < e.src_n && d < e.dst_n) dst[d * U + u] = src[s * U + u];
  }
}

// Pair k copies every section of env src_idx[k] of the source arrays to env dst_idx[k] of the
// destination arrays, bit for bit, with ordinary vector loads and stores.  A pair with an index
// outside its side is skipped (every access is behind the range test of both indices).  Workgroup b
// takes pairs [256 b, 256 b + 256): their indices staged in LDS, then section by section -- env-major
// rows by the whole workgroup (copy_rows), slot-major sections one lane per pair walking the rows, so
// that a side with consecutive indices is read or written 256 bytes per wave and row.  Two pairs with
// one destination race (the result is one of the two, word by word); nothing is read that was written
// here, so sources may repeat freely.
__global__ void __launch_bounds__(kCopyBlock) k_state_copy(CopyTable T) {
  __shared__ uint32_t sp[kCopyBlock], dp[kCopyBlock];
  const uint32_t t = threadIdx.x;
  const uint64_t k0 = (uint64_t)blockIdx.x * kCopyBlock;
  const uint32_t pairs = (uint32_t)min((uint64_t)kCopyBlock, T.count - k0);
  if (t < pairs) {
    sp[t] = T.src_idx ? T.src_idx[k0 + t] : (uint32_t)(k0 + t);
    dp[t] = T.dst_idx ? T.dst_idx[k0 + t] : (uint32_t)(k0 + t);
  }
  __syncthreads();
  for (uint32_t j = 0; j < T.n_sections; j++) {
    const CopySection& e = T.sec[j];
    if (e.kind == kSecRows) {
      switch (e.unit) {
        case 16: copy_rows<uint4>(e, sp, dp, pairs); break;
        case 8: copy_rows<uint2>(e, sp, dp, pairs); break;
        case 4: copy_rows<uint32_t>(e, sp, dp, pairs); break;
        case 2: copy_rows<uint16_t>(e, sp, dp, pairs); break;
        default: copy_rows<uint8_t>(e, sp, dp, pairs); break;
      }
    } else if (t < pairs) {
      const uint64_t s = sp[t], d = dp[t];
      if (s < e.src_n && d < e.dst_n) {
        const uint32_t* __restrict__ src = static_cast<const uint32_t*>(e.src) + s;
        uint32_t* __restrict__ dst = static_cast<uint32_t*>(e.dst) + d;
#pragma unroll 4
        for (uint32_t r = 0; r < e.row; r++) dst[(uint64_t)r * e.dst_n] = src[(uint64_t)r * e.src_n];
      }
    }
  }
  if (T.ep_ret && t < pairs) {
    const uint64_t s = sp[t], d = dp[t];
    if (s < T.sec[0].src_n && d < T.sec[0].dst_n) {
      T.ep_ret[d] = 0.f;
      T.ep_len[d] = 0;
    }
  }
}

}  // namespace pgtg
#endif  // PGTG_SNAPSHOT_H_
