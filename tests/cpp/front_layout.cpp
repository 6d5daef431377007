// The degree passes' scratch layouts (sheep_amd/csrc/front_layout.h) over a grid of shapes:
// every table inside [0, total), no two tables of a layout overlapping, u64 tables at even
// words, u16 entry arrays at multiples of 4 words with 8 entries of room behind their last
// entry, and every offset and total equal to what the size formulas and the launchers' pointer
// arithmetic gave before the layouts existed (frozen below, base address 0).  The radix sort's
// layout (rsort_layout) the same way, over record counts n.  Prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <cmath>
#include <random>
#include <vector>

#include "front_layout.h"

using namespace sheep;

static int fails = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++fails <= 40) {                             \
        fprintf(stderr, "FAIL %s: ", #c);              \
        fprintf(stderr, __VA_ARGS__);                  \
        fprintf(stderr, "\n");                         \
      }                                                \
    }                                                  \
  } while (0)

// ---- the former formulas, frozen (their own constants, nothing from the header) -------------
namespace ref {
constexpr uint64_t CHUNK = 32768, NBMAX = 1024, TMG = 256, FSMAX = 8192, STRIDE = 256, CLS = 64,
                   SCANT = 4096;
static bool params(uint32_t n_ids, int* SH_out, uint32_t* NB_out) {
  int bits = 0;
  for (uint64_t v = n_ids ? n_ids - 1 : 0; v; v >>= 1) ++bits;
  int SH = bits - 10;
  if (SH < 0) SH = 0;
  if (SH > 16) return false;
  *SH_out = SH;
  *NB_out = (uint32_t)(((uint64_t)n_ids + (1u << SH) - 1) >> SH);
  return true;
}
static size_t scan_words(uint64_t n) {
  size_t words = 0;
  while (n > SCANT) {
    n = (n + SCANT - 1) / SCANT;
    words += n;
  }
  return words + 1;
}
static uint64_t room(uint64_t items, uint32_t n_regions) {
  const double e = (double)items + 2.0 * STRIDE;
  return (uint64_t)(e + 5.0 * std::sqrt((double)STRIDE * n_regions * e)) + 2049ull * n_regions + 64;
}
static size_t cur_words(uint32_t n) { return 2 * (size_t)((n + 7) / 8) * CLS; }
static size_t degb_scan_words(uint64_t cw, uint64_t nchunks, uint32_t NB) {
  return std::max<size_t>(scan_words(cw), NB * ((nchunks + TMG - 1) / TMG) + 2 * (NB + 1) + 4);
}
static size_t degb_tmp_words(uint64_t m, uint32_t n_ids) {
  int SH = 0;
  uint32_t NB = 0;
  if (!params(n_ids, &SH, &NB)) return 1;
  uint64_t nchunks = (m + CHUNK - 1) / CHUNK;
  uint64_t cw = (uint64_t)NB * nchunks;
  return 2 * cw + degb_scan_words(cw, nchunks, NB) + (2 * m + 1) / 2 + 16;
}
static size_t degs_tmp_words(uint64_t m, uint32_t n_ids) {
  int SH = 0;
  uint32_t NB = 0;
  if (!params(n_ids, &SH, &NB)) return 1;
  const uint64_t ep = std::max<uint64_t>(room(2 * m, NB), room(m, FSMAX));
  return 2 * FSMAX + 2 * 2 * ((size_t)FSMAX + 1) + cur_words(FSMAX) + 2 + (ep + 1) / 2 + 16;
}
static size_t fh_tmp_words(uint64_t m, uint32_t n_ids) {
  int SH = 0;
  uint32_t NB = 0;
  if (!params(n_ids, &SH, &NB)) return 1;
  const uint64_t nchunks = (m + CHUNK - 1) / CHUNK;
  const uint64_t cw = (uint64_t)NB * nchunks;
  const uint64_t gw = (uint64_t)NB * ((nchunks + TMG - 1) / TMG);
  return 4 * cw + 2 * (gw + 2 * (NB + 1) + 8) + (m + 16) / 2 + 16;
}
// The carvings: byte addresses from base 0 (u32* arithmetic = 4 bytes a step, u64* = 8).
static uint64_t up(uint64_t bytes, uint64_t a) { return (bytes + a - 1) & ~(a - 1); }
struct Degb { uint64_t counts, offsets, gsum, bstart, ep; };
static Degb carve_degb(uint64_t m, uint32_t NB) {
  const uint32_t nchunks = (uint32_t)((m + CHUNK - 1) / CHUNK);
  const uint64_t cw = (uint64_t)NB * nchunks;
  Degb r;
  r.counts = 0;
  r.offsets = 4 * cw;
  const uint64_t stmp = r.offsets + 4 * cw;
  r.ep = up(stmp + 4 * degb_scan_words(cw, nchunks, NB), 16);
  r.gsum = stmp;
  r.bstart = up(r.gsum + 4 * (uint64_t)(NB * ((nchunks + (uint32_t)TMG - 1) / (uint32_t)TMG)), 8);
  return r;
}
struct Degs { uint64_t scnt, bst, bcur, bcap, ep; };
static Degs carve_sampled() {
  Degs r;
  r.scnt = 0;
  r.bst = 4 * (2 * NBMAX);
  r.bcur = r.bst + 8 * (NBMAX + 1);
  r.bcap = r.bcur + 8 * NBMAX;
  r.ep = up(r.bcap + 8 * (NBMAX + 1), 16);
  return r;
}
static Degs carve_fused() {
  Degs r;
  r.scnt = 0;
  r.bst = 4 * (2 * FSMAX);
  r.bcur = r.bst + 8 * (FSMAX + 1);
  r.bcap = r.bcur + 8 * (cur_words(FSMAX) / 2 + 1);
  r.ep = up(r.bcap + 8 * (FSMAX + 1), 16);
  return r;
}
struct Fh { uint64_t cy, cx, oy, ox, gy, by, gx, bx, epx; };
static Fh carve_fh(uint64_t m, uint32_t NB) {
  const uint32_t nchunks = (uint32_t)((m + CHUNK - 1) / CHUNK);
  const uint64_t cw = (uint64_t)NB * nchunks;
  const uint64_t gw = (uint64_t)NB * ((nchunks + TMG - 1) / TMG);
  Fh r;
  r.cy = 0;
  r.cx = r.cy + 4 * cw;
  r.oy = r.cx + 4 * cw;
  r.ox = r.oy + 4 * cw;
  r.gy = r.ox + 4 * cw;
  r.by = up(r.gy + 4 * gw, 8);
  r.gx = r.by + 8 * ((uint64_t)NB + 2);
  r.bx = up(r.gx + 4 * gw, 8);
  r.epx = up(r.bx + 8 * ((uint64_t)NB + 2), 16);
  return r;
}
// The radix sort's tmp: the size formula (its flat-scan term included), and the sort's carving
// from an 8-byte-aligned base (uintptr_t arithmetic on base + 4 * words).
constexpr uint64_t RSTILE = 8192;
static size_t rsort_tmp_words(uint64_t n) {
  uint64_t nt = (n + RSTILE - 1) / RSTILE;
  return 512 * nt + std::max<size_t>(scan_words(512 * nt), 512 * ((nt + TMG - 1) / TMG) + 1030);
}
struct Rsort { uint64_t counts, gsum, dstart; };
static Rsort carve_rsort(uint64_t n, uint64_t base) {
  uint64_t nt = (n + RSTILE - 1) / RSTILE;
  Rsort r;
  r.counts = 0;
  r.gsum = 4 * (512 * nt);
  r.dstart = ((base + r.gsum + 4 * (512 * ((nt + TMG - 1) / TMG)) + 7) & ~(uint64_t)7) - base;
  return r;
}
}  // namespace ref

// A table of a layout: [off, off + len) words; kind 1: u32, 2: u64, 3: u16 entries (len covers
// the entries and the 8 entries of room behind them).
struct Arr { const char* name; uint64_t off, len; int kind; };

static void check_arrays(const char* layout, uint64_t m, uint32_t n, std::vector<Arr> a, uint64_t total) {
  for (const Arr& x : a) {
    CHECK(x.off + x.len <= total, "%s.%s [%llu, +%llu) past total %llu (m=%llu n=%u)", layout, x.name,
          (unsigned long long)x.off, (unsigned long long)x.len, (unsigned long long)total,
          (unsigned long long)m, n);
    if (x.kind == 2) CHECK(x.off % 2 == 0, "%s.%s u64 at odd word (m=%llu n=%u)", layout, x.name, (unsigned long long)m, n);
    if (x.kind == 3) CHECK(x.off % 4 == 0, "%s.%s u16 not 16-B aligned (m=%llu n=%u)", layout, x.name, (unsigned long long)m, n);
  }
  std::sort(a.begin(), a.end(), [](const Arr& p, const Arr& q) { return p.off < q.off; });
  for (size_t i = 0; i + 1 < a.size(); ++i)
    CHECK(a[i].off + a[i].len <= a[i + 1].off, "%s: %s overlaps %s (m=%llu n=%u)", layout, a[i].name,
          a[i + 1].name, (unsigned long long)m, n);
}
// words of `entries` u16 entries plus 8 entries of room
static uint64_t ep_words(uint64_t entries) { return (entries + 8 + 1) / 2; }

#define SAME(field, refbytes)                                                                  \
  CHECK((uint64_t)(field) * 4 == (refbytes), #field " %llu words, before %llu bytes (m=%llu n=%u)", \
        (unsigned long long)(field), (unsigned long long)(refbytes), (unsigned long long)m, n)

// rsort_layout(n) against the former size formula and carving; containment, order, alignment.
static void check_rsort(uint64_t m) {
  const uint32_t n = 0;  // (the messages' id count: none here)
  const RsortLayout L = rsort_layout(m);
  const uint64_t nt = (m + ref::RSTILE - 1) / ref::RSTILE, ng = (nt + ref::TMG - 1) / ref::TMG;
  CHECK(L.ntiles == nt, "rsort ntiles %llu (n=%llu)", (unsigned long long)L.ntiles, (unsigned long long)m);
  CHECK(L.total == ref::rsort_tmp_words(m), "rsort total %zu, before %zu (n=%llu)", L.total,
        ref::rsort_tmp_words(m), (unsigned long long)m);
  for (uint64_t base : {0ull, 256ull, 0x7f0000000008ull}) {
    const ref::Rsort r = ref::carve_rsort(m, base);
    SAME(L.counts, r.counts);
    SAME(L.gsum, r.gsum);
    SAME(L.dstart, r.dstart);
  }
  check_arrays("rsort", m, n,
               {{"counts", L.counts, 512 * nt, 1}, {"gsum", L.gsum, 512 * ng, 1},
                {"dstart", L.dstart, 2 * 513, 2}},
               L.total);
}

int main() {
  const uint32_t ns[] = {1, 2, 1023, 1024, 1025, 1u << 20, 3000017, 1u << 25, (1u << 25) + 1,
                         40000003, (1u << 26) - 5, 1u << 26, (1u << 26) + 1};
  const uint64_t ms[] = {1, 32767, 32768, 32769, (1ull << 22) + 12345, (1ull << 25) + 999,
                         (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 1};
  CHECK(!degb_ok((1u << 26) + 1), "2^26 + 1 ids: not applicable");
  CHECK(degb_ok(1u << 26) && degb_ok(1), "applicable up to 2^26 ids");
  for (uint32_t n : ns)
    for (uint64_t m : ms) {
      int SH = 0, rSH = 0;
      uint32_t NB = 0, rNB = 0;
      const bool ok = ref::params(n, &rSH, &rNB);
      CHECK(degb_ok(n) == ok, "degb_ok(%u)", n);
      CHECK(degb_params(n, &SH, &NB) == ok && (!ok || (SH == rSH && NB == rNB)), "degb_params(%u)", n);
      CHECK(fs_room(m, NB ? NB : 1) == ref::room(m, NB ? NB : 1), "fs_room(%llu)", (unsigned long long)m);
      CHECK(scan_tmp_words(m) == ref::scan_words(m), "scan_tmp_words(%llu)", (unsigned long long)m);
      const DegbLayout B = degb_layout(m, n);
      const DegsLayout S = degs_layout(m, n);
      const FhLayout F = fh_layout(m, n);
      CHECK(B.total == ref::degb_tmp_words(m, n), "degb total %zu (m=%llu n=%u)", B.total, (unsigned long long)m, n);
      CHECK(S.total == ref::degs_tmp_words(m, n), "degs total %zu (m=%llu n=%u)", S.total, (unsigned long long)m, n);
      CHECK(F.total == ref::fh_tmp_words(m, n), "fh total %zu (m=%llu n=%u)", F.total, (unsigned long long)m, n);
      if (!ok) {
        CHECK(n == (1u << 26) + 1, "only 2^26 + 1 ids are beyond the passes (n=%u)", n);
        CHECK(B.total == 1 && S.total == 1 && F.total == 1, "not applicable: 1 word");
        continue;
      }
      const uint64_t nchunks = (m + ref::CHUNK - 1) / ref::CHUNK, cw = NB * nchunks;
      const uint64_t gw = (uint64_t)NB * ((nchunks + ref::TMG - 1) / ref::TMG);
      {  // the bucketed pass: ep holds both endpoints of every record at most
        const ref::Degb r = ref::carve_degb(m, NB);
        SAME(B.counts, r.counts);
        SAME(B.offsets, r.offsets);
        SAME(B.gsum, r.gsum);
        SAME(B.bstart, r.bstart);
        SAME(B.ep, r.ep);
        check_arrays("degb", m, n,
                     {{"counts", B.counts, cw, 1}, {"offsets", B.offsets, cw, 1}, {"gsum", B.gsum, gw, 1},
                      {"bstart", B.bstart, 2 * ((uint64_t)NB + 1), 2}, {"ep", B.ep, ep_words(2 * m), 3}},
                     B.total);
      }
      {  // the sampled view: DEGB_NB strides, plain cursors, fs_room(2m, NB) entries
        const ref::Degs r = ref::carve_sampled();
        const DegsView& V = S.sampled;
        CHECK(V.stride == 1024 && !V.spread, "sampled view: stride %u", V.stride);
        CHECK(V.ep_slots == ref::room(2 * m, NB), "sampled ep_slots");
        SAME(V.scnt, r.scnt);
        SAME(V.bst, r.bst);
        SAME(V.bcur, r.bcur);
        SAME(V.bcap, r.bcap);
        SAME(V.ep, r.ep);
        check_arrays("degs.sampled", m, n,
                     {{"scnt", V.scnt, 2 * 1024, 1}, {"bst", V.bst, 2 * 1025, 2}, {"bcur", V.bcur, 2 * 1024, 2},
                      {"bcap", V.bcap, 2 * 1024, 2}, {"ep", V.ep, ep_words(V.ep_slots), 3}},
                     S.total);
      }
      {  // the fused view: FS_MAX strides, spread cursors, fs_room(m, NB * G) <= ep_slots entries
        const ref::Degs r = ref::carve_fused();
        const DegsView& V = S.fused;
        CHECK(V.stride == 8192 && V.spread, "fused view: stride %u", V.stride);
        CHECK(V.ep_slots == ref::room(m, 8192), "fused ep_slots");
        for (uint32_t G = 1; G <= 8; ++G)
          CHECK(ref::room(m, NB * G) <= V.ep_slots, "fused regions of %u groups fit", G);
        SAME(V.scnt, r.scnt);
        SAME(V.bst, r.bst);
        SAME(V.bcur, r.bcur);
        SAME(V.bcap, r.bcap);
        SAME(V.ep, r.ep);
        check_arrays("degs.fused", m, n,
                     {{"scnt", V.scnt, 2 * 8192, 1}, {"bst", V.bst, 2 * 8193, 2},
                      {"bcur", V.bcur, ref::cur_words(8192), 2}, {"bcap", V.bcap, 2 * 8192, 2},
                      {"ep", V.ep, ep_words(V.ep_slots), 3}},
                     S.total);
      }
      {  // the counted-fused pass: epx holds one x id per record at most
        const ref::Fh r = ref::carve_fh(m, NB);
        SAME(F.cy, r.cy);
        SAME(F.cx, r.cx);
        SAME(F.oy, r.oy);
        SAME(F.ox, r.ox);
        SAME(F.gy, r.gy);
        SAME(F.by, r.by);
        SAME(F.gx, r.gx);
        SAME(F.bx, r.bx);
        SAME(F.epx, r.epx);
        check_arrays("fh", m, n,
                     {{"cy", F.cy, cw, 1}, {"cx", F.cx, cw, 1}, {"oy", F.oy, cw, 1}, {"ox", F.ox, cw, 1},
                      {"gy", F.gy, gw, 1}, {"by", F.by, 2 * ((uint64_t)NB + 1), 2}, {"gx", F.gx, gw, 1},
                      {"bx", F.bx, 2 * ((uint64_t)NB + 1), 2}, {"epx", F.epx, ep_words(m), 3}},
                     F.total);
      }
    }
  {  // the sort: n = 0 and 1, around every multiple of RS_TILE and of RS_TILE * TM_G up to
     // 2^32 - 1 records, the largest n, and random n (uniform, and uniform in magnitude)
    static_assert(RS_TILE == ref::RSTILE && TM_G == ref::TMG, "frozen constants");
    const uint64_t NMAX = (1ull << 32) - 1, T = ref::RSTILE, GT = ref::RSTILE * ref::TMG;
    auto around = [&](uint64_t c) {
      for (int d = -2; d <= 2; ++d)
        if ((d >= 0 || c >= (uint64_t)-d) && c + d <= NMAX) check_rsort(c + d);
    };
    check_rsort(0);
    check_rsort(1);
    for (uint64_t c = T; c <= NMAX; c += T) around(c);
    for (uint64_t c = GT; c <= NMAX; c += GT) around(c);
    around(NMAX);
    std::mt19937_64 rng(12345);
    for (int i = 0; i < 4000; ++i) check_rsort(rng() % (NMAX + 1));
    for (int i = 0; i < 1000; ++i) check_rsort(rng() % (1ull << (10 + i % 22)));
  }
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
