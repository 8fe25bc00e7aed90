// Block shares of k_envq<BIG, true>'s workgroups: how many of the nblk blocks each workgroup of the
// persistent grid owns, from its measured time per block.  Plain C++ in integers, no HIP: k_shares composes
// these pieces with one lane per workgroup, shares_assign() below is the same composition in a serial loop
// (the host test's, tests/test_shares_cpu.py).  Deterministic: a tie goes to the lower index.
#pragma once
#include <stdint.h>

#ifndef PGTG_SHARE_FN
#define PGTG_SHARE_FN inline
#endif

// a time per block: 100 MHz clock ticks in 1/16, at least 1
constexpr uint32_t kShareFrac = 16;
constexpr int kSharePasses = 8;  // rounding passes at most (the clamps span 5 counts)

// the measured time per block of a workgroup that ran `ticks` ticks over `count` blocks in `dt` clock ticks
PGTG_SHARE_FN uint32_t share_measure(uint64_t dt, uint32_t ticks, uint32_t count) {
  const uint64_t d = (uint64_t)ticks * count;
  const uint64_t m = d ? dt * kShareFrac / d : 0;
  return m < 1 ? 1u : (m > 0x7fffffffull ? 0x7fffffffu : (uint32_t)m);
}
// the running estimate: an exponential average of weight 1/2
PGTG_SHARE_FN uint32_t share_blend(uint32_t est, uint32_t meas) { return (uint32_t)(((uint64_t)est + meas + 1) / 2); }
// a workgroup's weight, proportional to 1 / estimate (est >= 1)
PGTG_SHARE_FN uint64_t share_weight(uint32_t est) { return (1ull << 32) / (est < 1 ? 1u : est); }
// the clamps: [max(1, base - 2), min(base + 2, cap_blocks)], base = nblk / grid, cap_blocks = request cap / envs
PGTG_SHARE_FN uint32_t share_lo(uint64_t nblk, uint32_t grid) {
  const uint64_t base = nblk / grid;
  return base > 3 ? (uint32_t)(base - 2) : 1u;
}
PGTG_SHARE_FN uint32_t share_hi(uint64_t nblk, uint32_t grid, uint64_t cap_blocks) {
  const uint64_t h = nblk / grid + 2;
  return (uint32_t)(h < cap_blocks ? h : cap_blocks);
}
// workgroup's quota nblk * w / W, clamped: its whole part and, where the clamps did not bind, the remainder
PGTG_SHARE_FN uint32_t share_quota(uint64_t nblk, uint64_t w, uint64_t W, uint32_t lo, uint32_t hi, uint64_t* rem) {
  const uint64_t num = nblk * w;  // (nblk < 2^31, w <= 2^32)
  const uint64_t q = num / W;
  *rem = num % W;
  if (q >= hi) {
    *rem = 0;
    return hi;
  }
  if (q < lo) {
    *rem = 0;
    return lo;
  }
  return (uint32_t)q;
}
// rounding keys of a pass (0: not eligible).  Blocks left to hand out: the largest remainder first, among the
// counts below hi; blocks to take back (the lower clamp raised some counts): the smallest remainder first,
// among the counts above lo.
PGTG_SHARE_FN uint64_t share_key(bool up, uint32_t count, uint64_t rem, uint64_t W, uint32_t lo, uint32_t hi) {
  if (up) return count < hi ? rem + 1 : 0;
  return count > lo ? W - rem : 0;
}
// how many workgroups go before workgroup i in a pass: a larger key, or the same key and -- handing out -- a
// lower index, taking back a higher one: either way the lower index of a tie ends with no fewer blocks
PGTG_SHARE_FN uint32_t share_rank(bool up, const uint64_t* key, uint32_t n, uint32_t i) {
  uint32_t r = 0;
  const uint64_t k = key[i];
  for (uint32_t j = 0; j < n; j++) r += (key[j] > k || (key[j] == k && (up ? j < i : j > i))) ? 1u : 0u;
  return r;
}

// The whole rule, serially: count[i] for estimates est[i] (>= 1), summing to nblk inside the clamps; rem and key
// are scratch of n words.  Returns 0, or -1 where the clamps admit no such counts.
inline int shares_assign(const uint32_t* est, uint32_t n, uint64_t nblk, uint64_t cap_blocks, uint32_t* count,
                         uint64_t* rem, uint64_t* key) {
  if (n == 0 || nblk >= (1ull << 31)) return -1;
  const uint32_t lo = share_lo(nblk, n), hi = share_hi(nblk, n, cap_blocks);
  if (hi < lo || (uint64_t)lo * n > nblk || (uint64_t)hi * n < nblk) return -1;
  uint64_t W = 0;
  for (uint32_t i = 0; i < n; i++) W += share_weight(est[i]);
  int64_t left = (int64_t)nblk;
  for (uint32_t i = 0; i < n; i++) {
    count[i] = share_quota(nblk, share_weight(est[i]), W, lo, hi, &rem[i]);
    left -= count[i];
  }
  for (int pass = 0; pass < kSharePasses && left != 0; pass++) {
    const bool up = left > 0;
    const uint64_t want = (uint64_t)(up ? left : -left);
    for (uint32_t i = 0; i < n; i++) key[i] = share_key(up, count[i], rem[i], W, lo, hi);
    for (uint32_t i = 0; i < n; i++)
      if (key[i] && share_rank(up, key, n, i) < want) {
        count[i] += up ? 1 : -1;
        left += up ? -1 : 1;
      }
  }
  return left == 0 ? 0 : -1;
}
