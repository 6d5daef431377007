// Scratch layouts of the degree passes and the radix sort (sheep_kernels.hip): where each table
// of a pass's `tmp` buffer lies, in u32 words from its start, and how many words it takes.  The
// size functions (*_tmp_words) return `total` and the launchers take their pointers from the
// same struct, so a table cannot grow in one and not in the other.  Host code only, no HIP:
// plain C++17 (tests/cpp/front_layout.cpp compiles it with g++).
// Alignment is a property of the offsets: the buffers come from hipMalloc (256-byte aligned at
// least), u64 tables start at even words, u16 entry arrays at multiples of 4 words (16-byte
// loads).  Every entry array keeps at least 8 entries of room behind its last entry: the
// histograms read 16-byte groups from the 8-aligned entry below a run and may run 7 entries
// past its end.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace sheep {

constexpr int DEGB_THREADS = 1024;
constexpr int DEGB_CHUNK = 32768;  // edges per chunk (<= 65536 endpoints -> 128 KB LDS)
constexpr uint32_t DEGB_NB = 1024;
constexpr uint32_t TM_G = 256;  // tiles per group of the tile-major scan (tm_offsets)
constexpr uint32_t PD_Y = 1024;  // y digits of the first partition pass of the rank gathers
// The fused front pass's tile groups (k_front_fused), and the subregions they make of the regions.
constexpr uint32_t FF_GMAX = 8, FS_MAX = DEGB_NB * FF_GMAX;
constexpr uint32_t FS_STRIDE = 256;  // the sampled capacities count every FS_STRIDE-th record
constexpr int SCAN_TILE = 4096;      // keys per tile of launch_scan_exclusive

// The fused front pass's region cursors are spread over memory (sheep_internal.h, fs_cix):
// eight to a 64-B line, consecutive lines SHEEP_FS_CLS u64 apart (8: contiguous).
#ifndef SHEEP_FS_CLS
#define SHEEP_FS_CLS 64
#endif
constexpr uint32_t FS_CLS = SHEEP_FS_CLS;
constexpr size_t fs_cur_words(uint32_t n) { return 2 * (size_t)((n + 7) / 8) * FS_CLS; }

// SH: local-id bits, NB buckets; false when n_ids is beyond the bucketed passes (> 2^26).
inline bool degb_params(uint32_t n_ids, int* SH_out, uint32_t* NB_out) {
  int bits = 0;
  for (uint64_t v = n_ids ? n_ids - 1 : 0; v; v >>= 1) ++bits;
  int SH = bits - 10;
  if (SH < 0) SH = 0;
  if (SH > 16) return false;
  *SH_out = SH;
  *NB_out = (uint32_t)(((uint64_t)n_ids + (1u << SH) - 1) >> SH);
  return true;
}
// The bucketed, sampled and counted-fused passes apply to these ids (their *_tmp_words are 1
// word otherwise: launch_degree_bucketed then takes the global-atomic pass).
inline bool degb_ok(uint32_t n_ids) {
  int SH;
  uint32_t NB;
  return degb_params(n_ids, &SH, &NB);
}

// The most slots the sampled capacity regions of `items` items over n_regions can take (the
// first pass's packed records: fs_room(m, 1024) slots of 6 bytes; see fs_cap, sheep_kernels.hip).
inline uint64_t fs_room(uint64_t items, uint32_t n_regions) {
  const double e = (double)items + 2.0 * FS_STRIDE;
  return (uint64_t)(e + 5.0 * std::sqrt((double)FS_STRIDE * n_regions * e)) + 2049ull * n_regions + 64;
}

// Exclusive scan of n u32 (launch_scan_exclusive): the words of its tmp.
inline size_t scan_tmp_words(uint64_t n) {
  size_t words = 0;
  while (n > (uint64_t)SCAN_TILE) {
    n = (n + SCAN_TILE - 1) / SCAN_TILE;
    words += n;
  }
  return words + 1;
}

constexpr size_t lay_up(size_t w, size_t a) { return (w + a - 1) / a * a; }  // a: a power of two

struct DegChunks {  // 32K-record chunks, and the tile-major count matrix of NB columns over them
  uint64_t nchunks, cw /* NB * nchunks */, gw /* the scan's group sums: NB * groups */;
  DegChunks(uint64_t m, uint32_t NB)
      : nchunks((m + DEGB_CHUNK - 1) / DEGB_CHUNK), cw(NB * nchunks),
        gw((uint64_t)NB * ((nchunks + TM_G - 1) / TM_G)) {}
};

// launch_degree_bucketed ("degb_tmp"): the chunks' bucket counts and offsets (cw each), the scan
// area (group sums, then NB + 1 u64 bucket starts; sized for a flat scan of the counts as well,
// which no longer runs: the size is kept), and the u16 endpoints (2m at most).
struct DegbLayout {
  size_t counts = 0, offsets = 0, gsum = 0, bstart = 0, ep = 0, total = 1;
};
inline DegbLayout degb_layout(uint64_t m, uint32_t n_ids) {
  DegbLayout L;
  int SH;
  uint32_t NB;
  if (!degb_params(n_ids, &SH, &NB)) return L;
  const DegChunks c(m, NB);
  L.offsets = c.cw;
  L.gsum = 2 * c.cw;
  L.bstart = lay_up(L.gsum + c.gw, 2);
  const size_t scan = std::max<size_t>(scan_tmp_words(c.cw), c.gw + 2 * (NB + 1) + 4);
  L.ep = lay_up(L.gsum + scan, 4);
  L.total = L.gsum + scan + (2 * m + 1) / 2 + 16;
  return L;
}

// "degs_tmp", one slot carved in two ways.  Both views hold the sample counts (2 * stride
// words: stride bucket counts per group, then y digit counts), u64 region starts (stride + 1),
// cursors, ends (stride + 1) and the u16 entries; they differ in the stride of the tables and
// in how the cursors lie:
//   sampled (launch_degree_sampled): stride DEGB_NB, cursor q at u64 index q;
//   fused (launch_front_fused): stride FS_MAX (FF_GMAX subregions per bucket), cursor q at u64
//     index fs_cix(q), fs_cur_words(FS_MAX) words (+ 2).
// The slot is sized for the fused view's tables and for the larger of the two entry arrays:
// both endpoints of every record in the sampled view, the x endpoints over FS_MAX regions at
// most in the fused one.
struct DegsView {
  uint32_t stride = 0;
  bool spread = false;  // cursors at fs_cix(q)
  size_t scnt = 0, bst = 0, bcur = 0, bcap = 0, ep = 0;
  uint64_t ep_slots = 0;  // u16 entries the view's capacity regions may take
};
struct DegsLayout {
  DegsView sampled, fused;
  size_t total = 1;
};
inline DegsLayout degs_layout(uint64_t m, uint32_t n_ids) {
  DegsLayout L;
  int SH;
  uint32_t NB;
  if (!degb_params(n_ids, &SH, &NB)) return L;
  auto view = [](uint32_t stride, bool spread, uint64_t ep_slots) {
    DegsView v;
    v.stride = stride;
    v.spread = spread;
    v.bst = 2 * (size_t)stride;
    v.bcur = v.bst + 2 * ((size_t)stride + 1);
    v.bcap = v.bcur + (spread ? fs_cur_words(stride) + 2 : 2 * (size_t)stride);
    v.ep = lay_up(v.bcap + 2 * ((size_t)stride + 1), 4);
    v.ep_slots = ep_slots;
    return v;
  };
  L.sampled = view(DEGB_NB, false, fs_room(2 * m, NB));
  L.fused = view(FS_MAX, true, fs_room(m, FS_MAX));
  const uint64_t ep = std::max(L.sampled.ep_slots, L.fused.ep_slots);
  L.total = L.fused.bcap + 2 * ((size_t)FS_MAX + 1) + (ep + 1) / 2 + 16;
  return L;
}

// launch_fh_front ("degb_tmp"): the y and x count matrices and their offsets (cw each), each
// scan's group sums (gw) and u64 bucket starts (NB + 2), and the u16 x ids (m at most).
struct FhLayout {
  size_t cy = 0, cx = 0, oy = 0, ox = 0, gy = 0, by = 0, gx = 0, bx = 0, epx = 0, total = 1;
};
inline FhLayout fh_layout(uint64_t m, uint32_t n_ids) {
  FhLayout L;
  int SH;
  uint32_t NB;
  if (!degb_params(n_ids, &SH, &NB)) return L;
  const DegChunks c(m, NB);
  L.cx = c.cw;
  L.oy = 2 * c.cw;
  L.ox = 3 * c.cw;
  L.gy = 4 * c.cw;
  L.by = lay_up(L.gy + c.gw, 2);
  L.gx = L.by + 2 * ((size_t)NB + 2);
  L.bx = lay_up(L.gx + c.gw, 2);
  L.epx = lay_up(L.bx + 2 * ((size_t)NB + 2), 4);
  L.total = 4 * c.cw + 2 * (c.gw + 2 * (NB + 1) + 8) + (m + 16) / 2 + 16;
  return L;
}

// radix_sort_u64 and group_by_bins ("rsort_tmp"): 512 digit or bin counts per tile of RS_TILE
// items (turned into offsets in place), the tile-major scan's group sums, and 513 u64 column
// starts (512 columns and the total).
constexpr int RS_TILE = 8192;
struct RsortLayout {
  uint64_t ntiles = 0;
  size_t counts = 0, gsum = 0, dstart = 0, total = 0;
};
inline RsortLayout rsort_layout(uint64_t n) {
  RsortLayout L;
  L.ntiles = (n + RS_TILE - 1) / RS_TILE;
  const size_t gw = 512 * (size_t)((L.ntiles + TM_G - 1) / TM_G);
  L.gsum = 512 * (size_t)L.ntiles;
  L.dstart = lay_up(L.gsum + gw, 2);
  L.total = L.gsum + gw + 2 * 513 + 4;
  return L;
}

}  // namespace sheep
