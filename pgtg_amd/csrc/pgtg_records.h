// pgtg_amd/csrc/pgtg_records.h -- the packed words of an env's state in HBM: the one definition of each
// bit layout, shared by the kernels and by the host side of the C ABI (pgtg_env.hip).  Plain C++17 with
// no HIP header, so that a host-only program can pin the layouts (tests/test_records_cpu.py).
// A field that widens or a flag that moves changes here, and kStateVersion (pgtg_env.hip) with it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PGTG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PGTG_HD inline
#endif

namespace pgtg {

// Four words moved as one 16-byte access.  Device code keeps HIP's own uint4 (the includer brings
// hip_runtime.h), so that the kernels' loads and stores compile as they always did; a plain C++ build
// gets a struct of the same layout.
#ifdef __HIPCC__
using Quad = uint4;
#else
struct alignas(16) Quad {
  uint32_t x, y, z, w;
};
#endif
static_assert(sizeof(Quad) == 16 && alignof(Quad) == 16, "Quad is one 16-byte access");
static_assert(__builtin_offsetof(Quad, x) == 0 && __builtin_offsetof(Quad, y) == 4 && __builtin_offsetof(Quad, z) == 8 &&
                  __builtin_offsetof(Quad, w) == 12,
              "both spellings of Quad are the words x, y, z, w in order");

// ---- EnvRec: the agent record (32 B, one quad pair per env) ------------------------------------------
//  w0 = px | py<<16 (int16)   w1 = vx | vy<<16 (int16)   w2 = phase | flags<<16 (4 bits) | path_len<<20
//  w3 = elapsed steps         w4 = start/goal word (sg_word)
//  w5 = spawn counter (SeedSequence children spawned)   w6,w7 = used-subgoal tile mask (u64; maps of <= 64
//  tiles, larger maps mark the plan words, kPlanUsed)
struct EnvRec {
  Quad a, b;
};
static_assert(sizeof(EnvRec) == 32, "EnvRec is a quad pair");

// agent flags (EnvView::flags)
constexpr uint32_t kFlagTerminated = 1u << 0;
constexpr uint32_t kFlagFlatTire = 1u << 1;
constexpr uint32_t kFlagBraking = 1u << 2;
constexpr uint32_t kFlagTruncated = 1u << 3;

struct EnvView {
  int px, py, vx, vy;
  uint32_t phase, flags, path_len, elapsed;
  uint32_t sg, spawn;
  uint64_t used;
};

PGTG_HD EnvView rec_view(const EnvRec& e) {
  EnvView v;
  v.px = (int)(int16_t)(e.a.x & 0xffffu);
  v.py = (int)(int16_t)(e.a.x >> 16);
  v.vx = (int)(int16_t)(e.a.y & 0xffffu);
  v.vy = (int)(int16_t)(e.a.y >> 16);
  v.phase = e.a.z & 0xffffu;
  v.flags = (e.a.z >> 16) & 0xfu;
  v.path_len = e.a.z >> 20;
  v.elapsed = e.a.w;
  v.sg = e.b.x;
  v.spawn = e.b.y;
  v.used = (uint64_t)e.b.z | ((uint64_t)e.b.w << 32);
  return v;
}
PGTG_HD EnvRec rec_pack(const EnvView& v) {
  EnvRec e;
  e.a.x = ((uint32_t)v.px & 0xffffu) | ((uint32_t)v.py << 16);
  e.a.y = ((uint32_t)v.vx & 0xffffu) | ((uint32_t)v.vy << 16);
  e.a.z = (v.phase & 0xffffu) | ((v.flags & 0xfu) << 16) | (v.path_len << 20);
  e.a.w = v.elapsed;
  e.b.x = v.sg;
  e.b.y = v.spawn;
  e.b.z = (uint32_t)v.used;
  e.b.w = (uint32_t)(v.used >> 32);
  return e;
}
// the spawn counter alone (the fill kernels read nothing else of the record)
PGTG_HD uint32_t rec_spawn(const EnvRec& e) { return e.b.y; }

// ---- sg: the start/goal word of a map (EnvView::sg, DevCfg::fixed_sg, a map-ring entry's meta) --------
// start tile | start direction << 8 | goal tile << 16 | goal direction << 24
PGTG_HD uint32_t sg_word(int st_t, int st_d, int gl_t, int gl_d) {
  return (uint32_t)st_t | (uint32_t)st_d << 8 | (uint32_t)gl_t << 16 | (uint32_t)gl_d << 24;
}
// The field accessors of this header (int results) are macros, not functions: the step kernels test them
// inside short-circuit conditions (square_flags, the observation builders, the car loops), where a call --
// even an always-inline one -- is inlined only after the first control-flow simplification.  As functions
// the sg_* ones changed the schedule of k_envq, k_envb and k_env and cost the 5 x 5 workload 0.5 %
// (profiles/records_codec/).  Each evaluates its argument once.
#define sg_start_tile(sg) ((int)((sg) & 0xffu))
#define sg_start_dir(sg) ((int)(((sg) >> 8) & 0xffu))
#define sg_goal_tile(sg) ((int)(((sg) >> 16) & 0xffu))
#define sg_goal_dir(sg) ((int)((sg) >> 24))

// ---- car word w0 of a car slot (DevState::car_w0, an env's staging block) ---------------------------
// x | y<<8 | route<<16 (5 bits) | profile<<21 (3 bits) | delay<<24 (2 bits); bit 31: the slot holds no car
// (a despawned car's).  An empty slot reads as a car at (0, 0): every slot holds valid coordinates.
constexpr uint32_t kCarEmpty = 1u << 31;
PGTG_HD uint32_t car_pack(int x, int y, int route, int profile, int delay) {
  return (uint32_t)x | (uint32_t)y << 8 | (uint32_t)route << 16 | (uint32_t)profile << 21 | (uint32_t)delay << 24;
}
#define car_empty(w0) (((w0) & pgtg::kCarEmpty) != 0u)
#define car_x(w0) ((int)((w0) & 255u))
#define car_y(w0) ((int)(((w0) >> 8) & 255u))
#define car_route(w0) ((int)(((w0) >> 16) & 31u))
#define car_profile(w0) ((int)(((w0) >> 21) & 7u))
#define car_delay(w0) ((int)(((w0) >> 24) & 3u))

// ---- traffic record (DevState::traf, one quad per env) ----------------------------------------------
// {n_cars | n_spawners<<16, next car id, tail, flags}
struct TrafState {
  uint32_t n_cars, n_spawners, next_id, tail;  // tail: car slots in use (cars and empty slots)
  uint32_t fresh;  // the cars (and their counters) are still in the env's staging block (DevState::fresh)
};
// the flag word: the persisted occupancy counters are exact for the env's current cars (else k_env
// rebuilds them from the car slots); TrafState::fresh
constexpr uint32_t kTrafOccValid = 1u, kTrafFresh = 2u;
PGTG_HD Quad traf_words(uint32_t counts, uint32_t next_id, uint32_t tail, uint32_t flags) {
  return Quad{counts, next_id, tail, flags};
}
// (a macro so that the flag expression is evaluated after the counts word, as the kernels always did)
#define traf_pack(ts, flags) pgtg::traf_words((ts).n_cars | (ts).n_spawners << 16, (ts).next_id, (ts).tail, (flags))
PGTG_HD uint32_t traf_flags(const Quad& t) { return t.w; }
PGTG_HD TrafState traf_unpack(const Quad& t) {
  return TrafState{t.x & 0xffffu, t.x >> 16, t.y, t.z, (traf_flags(t) & kTrafFresh) ? 1u : 0u};
}
// the step kernel's form: into its live TrafState, field by field, with the counters' flag (as a value
// returned through a temporary the traffic instances of k_env were scheduled differently)
PGTG_HD void traf_unpack(const Quad& t, TrafState& ts, bool& occ_valid) {
  ts.n_cars = t.x & 0xffffu;
  ts.n_spawners = t.x >> 16;
  ts.next_id = t.y;
  ts.tail = t.z;
  ts.fresh = (t.w & kTrafFresh) ? 1u : 0u;
  occ_valid = (t.w & kTrafOccValid) != 0u;
}

// ---- qstate: one byte per env of a handle with a map queue (DevState::qstate) -----------------------
constexpr uint32_t kQueueStale = 0x80u;  // the ring's entries are not this env's (k_qfill regenerates them)
// k_envq: cur slot | head slot << 2 (| kQueueStale); the third slot of the ring is the spare
// (two bits as a slot index: never outside the ring, whatever the byte holds)
PGTG_HD uint32_t queue_slot(uint32_t bits) { return (bits & 3u) < 2u ? (bits & 3u) : 2u; }
PGTG_HD uint32_t queue_cur(uint32_t qs) { return queue_slot(qs); }
PGTG_HD uint32_t queue_head(uint32_t qs) { return queue_slot(qs >> 2); }
PGTG_HD bool queue_head_bad(uint32_t qs) { return ((qs >> 2) & 3u) == 3u; }  // head bits that name no slot
// the spare of a ring whose cur and head differ (else cur's successor's successor: still a slot)
PGTG_HD uint32_t queue_spare(uint32_t qc, uint32_t qh) { return qc != qh ? 3u - qc - qh : (qc + 2u) % 3u; }
PGTG_HD uint8_t queue_state(uint32_t cur, uint32_t head) { return (uint8_t)(cur | head << 2); }
// k_envb: entries held (0 .. 3) | head slot << 2 (kQueueStale: none held)
PGTG_HD uint32_t blockq_held(uint32_t qs) { return qs & 3u; }
PGTG_HD uint32_t blockq_head(uint32_t qs) { return (qs >> 2) & 3u; }
PGTG_HD uint8_t blockq_state(uint32_t held, uint32_t head) { return (uint8_t)(held | head << 2); }

}  // namespace pgtg
