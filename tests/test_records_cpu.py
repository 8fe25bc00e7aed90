"""pgtg_amd/csrc/pgtg_records.h without a GPU: a stand-alone C++ program compiled with plain g++ against the
header alone pins every packed state word (EnvRec, car word, traffic record, start/goal word, qstate) to
literal words worked out by hand from the layouts, and checks that unpack(pack) is the identity over the
corner values of every field.  A later edit of the header cannot move a field silently: the kernels and
the host side of the C ABI share these definitions, and state blobs (kStateVersion) store the words."""
import os
import subprocess
import tempfile

import helpers

HEADER_DIR = os.path.join(helpers.ROOT, "pgtg_amd", "csrc")

PROBE = r'''
#include <stdint.h>
#include <stdio.h>
#include "pgtg_records.h"
using namespace pgtg;

static int bad = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); bad++; } } while (0)
#define WORD(got, want) do { uint32_t g_ = (got); if (g_ != (want)) { \
    printf("FAILED line %d: %s = 0x%08x, want 0x%08x\n", __LINE__, #got, g_, (uint32_t)(want)); bad++; } } while (0)

static bool same(const EnvView& a, const EnvView& b) {
  return a.px == b.px && a.py == b.py && a.vx == b.vx && a.vy == b.vy && a.phase == b.phase && a.flags == b.flags &&
         a.path_len == b.path_len && a.elapsed == b.elapsed && a.sg == b.sg && a.spawn == b.spawn && a.used == b.used;
}

int main() {
  // ---- EnvRec: literal words ----
  static_assert(sizeof(EnvRec) == 32 && alignof(EnvRec) == 16, "EnvRec");
  static_assert(kFlagTerminated == 1 && kFlagFlatTire == 2 && kFlagBraking == 4 && kFlagTruncated == 8, "flags");
  EnvView v{};
  v.px = -3; v.py = 5; v.vx = -30000; v.vy = 30000;
  v.phase = 0xffffu; v.flags = kFlagTruncated | kFlagFlatTire; v.path_len = 4095u; v.elapsed = 0xffffffffu;
  v.sg = sg_word(0x12, 3, 0xfe, 1); v.spawn = 0xdeadbeefu; v.used = (1ull << 63) | 1ull;
  const EnvRec r = rec_pack(v);
  WORD(r.a.x, 0x0005fffdu);  // px | py << 16
  WORD(r.a.y, 0x75308ad0u);  // vx | vy << 16
  WORD(r.a.z, 0xfffaffffu);  // phase | flags << 16 | path_len << 20
  WORD(r.a.w, 0xffffffffu);  // elapsed
  WORD(r.b.x, 0x01fe0312u);  // sg
  WORD(r.b.y, 0xdeadbeefu);  // spawn counter
  WORD(r.b.z, 0x00000001u);  // used, low
  WORD(r.b.w, 0x80000000u);  // used, high
  WORD(rec_spawn(r), 0xdeadbeefu);
  CHECK(same(rec_view(r), v));
  // ---- EnvRec: rec_view(rec_pack(v)) == v over the corners of every field ----
  const int s16[4] = {-32768, -1, 0, 32767};
  const uint32_t ph[2] = {0u, 0xffffu}, fl[3] = {0u, 0xfu, kFlagBraking}, pl[2] = {0u, 4095u}, u32[2] = {0u, 0xffffffffu};
  const uint64_t us[3] = {0ull, ~0ull, (1ull << 63) | 1ull};
  long n = 0;
  for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) for (int c = 0; c < 4; c++) for (int d = 0; d < 4; d++)
  for (int e = 0; e < 2; e++) for (int f = 0; f < 3; f++) for (int g = 0; g < 2; g++) for (int h = 0; h < 2; h++)
  for (int i = 0; i < 2; i++) for (int j = 0; j < 2; j++) for (int k = 0; k < 3; k++) {
    EnvView w{s16[a], s16[b], s16[c], s16[d], ph[e], fl[f], pl[g], u32[h], u32[i], u32[j], us[k]};
    const EnvRec q = rec_pack(w);
    if (!same(rec_view(q), w)) { bad++; printf("FAILED EnvRec round trip %d %d %d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, i, j, k); }
    // each field lands in its own bits: the word of the other fields is untouched by this one
    if (q.a.x != (((uint32_t)s16[a] & 0xffffu) | (uint32_t)s16[b] << 16) || q.a.w != u32[h] || q.b.x != u32[i] || q.b.y != u32[j]) bad++;
    n++;
  }
  CHECK(n == 4 * 4 * 4 * 4 * 2 * 3 * 2 * 2 * 2 * 2 * 3);

  // ---- car word ----
  static_assert(kCarEmpty == 0x80000000u, "empty slot");
  WORD(car_pack(255, 0, 19, 4, 3), 0x039300ffu);  // x | y << 8 | route << 16 | profile << 21 | delay << 24
  WORD(car_pack(0, 255, 0, 0, 0), 0x0000ff00u);
  CHECK(car_empty(kCarEmpty) && car_x(kCarEmpty) == 0 && car_y(kCarEmpty) == 0);  // reads as a car at (0, 0)
  CHECK(!car_empty(0x7fffffffu));
  const int xy[2] = {0, 255}, ro[3] = {0, 19, 31}, pr[3] = {0, 4, 7}, de[2] = {0, 3};
  for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) for (int c = 0; c < 3; c++) for (int d = 0; d < 3; d++)
  for (int e = 0; e < 2; e++) {
    const uint32_t w0 = car_pack(xy[a], xy[b], ro[c], pr[d], de[e]);
    CHECK(!car_empty(w0) && car_x(w0) == xy[a] && car_y(w0) == xy[b] && car_route(w0) == ro[c] &&
          car_profile(w0) == pr[d] && car_delay(w0) == de[e]);
    CHECK(car_pack(car_x(w0), car_y(w0), car_route(w0), car_profile(w0), car_delay(w0)) == w0);
  }

  // ---- traffic record ----
  static_assert(kTrafOccValid == 1u && kTrafFresh == 2u, "traffic flags");
  {
    const TrafState ts{0xffffu, 1u, 7u, 9u, 0u};
    const Quad q = traf_pack(ts, kTrafOccValid);
    WORD(q.x, 0x0001ffffu);  // n_cars | n_spawners << 16
    WORD(q.y, 7u);
    WORD(q.z, 9u);
    WORD(q.w, 1u);
    const TrafState u = traf_unpack(q);
    CHECK(u.n_cars == 0xffffu && u.n_spawners == 1u && u.next_id == 7u && u.tail == 9u && u.fresh == 0u);
    CHECK(traf_flags(q) == kTrafOccValid);
    TrafState u2{};
    bool occ = false;
    traf_unpack(q, u2, occ);  // the step kernel's form
    CHECK(occ && u2.n_cars == 0xffffu && u2.n_spawners == 1u && u2.next_id == 7u && u2.tail == 9u && u2.fresh == 0u);
    const Quad f = traf_pack(ts, kTrafFresh);
    WORD(f.w, 2u);
    CHECK(traf_unpack(f).fresh == 1u && !(traf_flags(f) & kTrafOccValid));
  }
  for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) for (int c = 0; c < 2; c++) for (int d = 0; d < 2; d++)
  for (uint32_t fg = 0; fg < 4u; fg++) {
    const TrafState ts{ph[a], ph[b], u32[c], u32[d], (fg & kTrafFresh) ? 1u : 0u};
    const Quad q = traf_pack(ts, fg);
    const TrafState u = traf_unpack(q);
    CHECK(u.n_cars == ts.n_cars && u.n_spawners == ts.n_spawners && u.next_id == ts.next_id && u.tail == ts.tail &&
          u.fresh == ts.fresh && traf_flags(q) == fg);
    TrafState u2{};
    bool occ = false;
    traf_unpack(q, u2, occ);
    CHECK(occ == ((fg & kTrafOccValid) != 0u) && u2.n_cars == u.n_cars && u2.n_spawners == u.n_spawners &&
          u2.next_id == u.next_id && u2.tail == u.tail && u2.fresh == u.fresh);
    const Quad q2 = traf_pack(u, traf_flags(q));
    CHECK(q2.x == q.x && q2.y == q.y && q2.z == q.z && q2.w == q.w);
  }

  // ---- start/goal word ----
  WORD(sg_word(0x12, 3, 0xfe, 1), 0x01fe0312u);  // start tile | start dir << 8 | goal tile << 16 | goal dir << 24
  CHECK(sg_start_tile(0x01fe0312u) == 0x12 && sg_start_dir(0x01fe0312u) == 3 && sg_goal_tile(0x01fe0312u) == 0xfe &&
        sg_goal_dir(0x01fe0312u) == 1);
  const int ti[2] = {0, 255}, di[2] = {0, 3};
  for (int a = 0; a < 2; a++) for (int b = 0; b < 2; b++) for (int c = 0; c < 2; c++) for (int d = 0; d < 2; d++) {
    const uint32_t sg = sg_word(ti[a], di[b], ti[c], di[d]);
    CHECK(sg_start_tile(sg) == ti[a] && sg_start_dir(sg) == di[b] && sg_goal_tile(sg) == ti[c] && sg_goal_dir(sg) == di[d]);
  }

  // ---- qstate ----
  static_assert(kQueueStale == 0x80u, "stale flag");
  const uint8_t want[3][3] = {{0, 4, 8}, {1, 5, 9}, {2, 6, 10}};  // [held][head] = held | head << 2
  for (uint32_t held = 0; held < 3u; held++) for (uint32_t head = 0; head < 3u; head++) {
    const uint8_t qs = blockq_state(held, head);
    WORD(qs, want[held][head]);
    CHECK(blockq_held(qs) == held && blockq_head(qs) == head);
    const uint8_t qq = queue_state(held, head);  // k_envq: cur | head << 2, the same bits
    WORD(qq, want[held][head]);
    CHECK(queue_cur(qq) == held && queue_head(qq) == head && !queue_head_bad(qq));
    if (held != head) CHECK(queue_spare(held, head) == 3u - held - head);
    CHECK(queue_spare(held, head) < 3u);
    CHECK(queue_cur(qq | kQueueStale) == held);
  }
  WORD(blockq_state(3u, 2u), 11u);  // a full ring
  CHECK(blockq_held(11u) == 3u && blockq_head(11u) == 2u);
  CHECK(queue_cur(3u) == 2u && queue_head(0xcu) == 2u && queue_head_bad(0xcu));  // two bits as a slot: never outside the ring
  if (bad) { printf("%d checks failed\n", bad); return 1; }
  printf("records OK %ld\n", n);
  return 0;
}
'''


def test_packed_state_words_are_pinned_and_round_trip():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "records_probe.cc"), os.path.join(d, "records_probe")
        with open(src, "w") as f:
            f.write(PROBE)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", HEADER_DIR, "-o", exe, src], check=True)
        p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("records OK 73728"), p.stdout


def test_header_is_plain_cxx_without_hip():
    """The header compiles on its own under plain g++ (no HIP header, no hipcc) and includes nothing but stdint."""
    text = open(os.path.join(HEADER_DIR, "pgtg_records.h")).read()
    includes = [ln.split()[1] for ln in text.splitlines() if ln.startswith("#include")]
    assert includes == ["<stdint.h>"], includes
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                    os.path.join(HEADER_DIR, "pgtg_records.h"), os.devnull], check=True)
