// Internal declarations shared by the HIP kernels (sheep_kernels.hip) and the C-ABI
// (sheep_capi.cpp).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <deque>
#include <mutex>
#include <string>
#include <vector>

#include "front_layout.h"

namespace sheep {

constexpr uint32_t INV = 0xFFFFFFFFu;

// Bits of the device error word (OR-ed by kernels, read by the host after a sync).
constexpr uint32_t ERR_RANGE = 1u;      // an id >= n_ids, or index.at(nbr) out of range
constexpr uint32_t ERR_DUP_SEQ = 2u;    // an id repeated in seq

// The current device's walk-guard word (sheep_kernels.hip): non-zero after a zipper or
// union-find walk met corrupt data and stopped; check_err reports it as -EIO and clears it.
uint32_t* fault_word();

// Growable device scratch.  One instance per device; slots are named so that the hot path
// reuses its buffers across calls (allocation only happens on the first / a larger call).
struct Scratch {
  struct Slot { void* p = nullptr; size_t bytes = 0; };
  std::vector<std::pair<std::string, Slot>> slots;
  void* get(const char* name, size_t bytes);  // throws std::runtime_error on hipMalloc failure
  size_t bytes_of(const char* name) const;    // current size of a slot (0: none)
  void release();
};

// Tuning options.  Every setting gives the same results (the etree is unique); they move work
// between kernels.  Read from SHEEP_<NAME> environment variables once, when the library first
// initialises a device, and changeable afterwards through sheep_set_option (include/
// sheep_amd.h) — never re-read per call.
struct Knobs {
  int degree = 0;        // SHEEP_DEGREE: 0 auto (bucketed from 2^18 records), 1 atomic, 2 bucketed
  int edge_part = -1;    // SHEEP_EDGE_PART: partitioned rank gathers; -1 auto (m >= 2^22), 0, 1
  int part_overlap = 4;  // SHEEP_PART_OVERLAP: one read for the degrees and the first partition
                         //   pass into sampled regions (4, from 2^25 records of the graph or of
                         //   a rank's shard; else 2), the first pass beside the degree pass (2:
                         //   both into sampled regions from 2^25 records), after it (1),
                         //   in line (0), fused into a counted degree scatter (3; taken anyway
                         //   from 2^31 records)
  int kb_buckets = 0;    // SHEEP_KB_BUCKETS: kb buckets cut at edge quantiles (0 = auto)
  int kb_rankb = 0;      // SHEEP_KB_RANKB: kb buckets cut at rank quantiles (0 = auto)
  int kb_pipe = 1;       // SHEEP_KB_PIPE: map of bucket k+1 beside the apply of bucket k
  int tree_stats = 0;    // SHEEP_TREE_STATS: 1 totals, 2 per bucket (stderr; diagnostics)
  int bin_direct = 1;    // SHEEP_BIN_DIRECT: the edge pass fills the hi bins directly (no scatter)
  int bin_slack = 50;    // SHEEP_BIN_SLACK: bin capacity = estimate x (1 + slack / 1000) + 8192
  int kb_gsum = -1;      // SHEEP_KB_GSUM: the map tests 64-rank "all in the giant" blocks in LDS
                         //   first; -1 auto (from 2^27 records), 0, 1
  int ls_seq = 1;        // SHEEP_LS_SEQ: with P > 1 ranks each sorts the ids of its 1/P of the id
                         //   space (degrees reduce-scattered; 0: all-reduced, every rank sorts all)
  int ls_split = 1;      // SHEEP_LS_SPLIT: with P > 1 ranks each bucket's zipper runs on one owner
                         //   rank (0: every rank applies every bucket's zipper)
  int kb_merge = 35;     // SHEEP_KB_MERGE: merge adjacent kb buckets while together they hold at
                         //   most kb_merge / 10000 of the records (0: off;
                         //   the lockstep loop: 20 unless off)
  int kb_fresh_lo = 50;  // SHEEP_KB_FRESH_LO / _HI: the kb loop's birth window, in hundredths of
  int kb_fresh_hi = 100; //   the mean degree 2E/B below a bucket's end (tree_from_sorted)
  int ff_groups = 1;     // SHEEP_FF_GROUPS: tile groups of the fused front pass (1..8): group g's
                         //   tiles write their own subregion of every region, so a subregion's
                         //   runs come from one XCD's blocks and merge in its L2 (round 6)
  int kb_rlink = 1;      // SHEEP_KB_RLINK: the refresh makes the zipper's first step of pairs from
                         //   pre-bucket roots (CAS INVALID -> b), leaving the rest to the zipper
  int eval_pass = 31;    // SHEEP_EVAL_PASS: at most 2^eval_pass adjacency entries sorted per pass
                         //   of the partition evaluation (more: passes over id ranges)
  int net_chunk = 32 << 20;  // SHEEP_NET_CHUNK: bytes of text per chunk of the .net ingest, kept
                         //   in [4096, 2^30] and a multiple of 16 (net_layout.h net_chunk_clamp)
};
Knobs& knobs();  // the process-wide options (sheep_capi.cpp)

struct Ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;     // second stream of the pipelined kb loop (the maps)
  hipEvent_t kb_ev[5] = {};       // kb loop: [0,1] map done, [2,3] apply done (by parity), [4] start
  hipEvent_t part_ev[2] = {};     // graph2tree: [0] degree done, [1] first partition pass done
  hipEvent_t bins_ev = nullptr;   // the chunk degree sums reached the pinned host buffer
  uint64_t* h_chunks = nullptr;   // pinned host buffer for them (grown on demand)
  unsigned long long* h_bstart = nullptr;  // pinned: the 513 bin starts of the scatter
  size_t h_chunks_n = 0;
  Scratch scratch;
  uint32_t* d_err = nullptr;     // device error word
  uint32_t* h_pinned = nullptr;  // pinned host words for small readbacks
  std::vector<std::pair<const char*, double>> timings;
  std::deque<std::string> span_names;  // storage for the "<name>#" timing labels
  std::vector<hipEvent_t> ev_pool;     // timing events of finished calls (Timer), reused
  std::mutex ev_mu;                    // guards ev_pool (the rest of a context is one caller's at
                                       // a time: include/sheep_amd.h "Threads")
  int ls_live = 0;                     // live lockstep sessions (sheep_ls_*) on this device
  struct Comm* comm = nullptr;         // this rank's communicator (sheep_comm_init), if any
  // host record ranges declared immutable (sheep_records_register / sheep_records_load_dat)
  // and their device copies: host-pointer calls on them upload nothing
  struct Registered { const uint32_t* host; uint64_t m; uint32_t* dev; };
  std::vector<Registered> registered;
  void* h_part = nullptr;  // pinned: the heavy ranks and the deltas of sheep_partition_dev
  size_t h_part_bytes = 0;
};

Ctx& ctx();  // this thread's context for the current device (sheep_gpu_init)

// ---- launchers (sheep_kernels.hip); all enqueue on `s` -------------------------------------
void launch_degree(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode, uint32_t* deg,
                   uint32_t* selfc, uint32_t* err, hipStream_t s);
// Bucketed LDS degree histogram for large m (same result as launch_degree); selfc nullable.
// (tmp: degb_layout, front_layout.h; applicable where degb_ok(n_ids), else 1 word and the
// global-atomic pass)
size_t degb_tmp_words(uint64_t m, uint32_t n_ids);
// yhist (nullable, 1024 words): also counts the y digits of launch_part_gather's first pass
// (n_rank = n_ids), so that pass needs no counting read; returns true when it did.
bool launch_degree_bucketed(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                            uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                            hipStream_t s, uint32_t* yhist = nullptr,
                            hipEvent_t counted = nullptr /* recorded once yhist is complete */,
                            uint32_t* stats = nullptr /* [0] max degree, [1] zero-degree ids */);
// Fused front half (graph2tree_dev): degrees (deg, selfc, stats as launch_degree_bucketed)
// and the records (x, y) grouped by y bucket into recs (m u64), the x digits of
// launch_part_second counted into part_ws (spread, xh_ix) — what launch_part_first produced.  tmp:
// fh_tmp_words (fh_layout, front_layout.h).  False when not applicable (degb_ok(n_ids)).
size_t fh_tmp_words(uint64_t m, uint32_t n_ids);
bool launch_fh_front(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode, uint32_t* deg,
                     uint32_t* selfc, uint32_t* err, uint32_t* tmp, uint64_t* recs,
                     uint32_t* part_ws, uint32_t* stats, hipStream_t s,
                     void (*mark)(void*, const char*) = nullptr /* phase marks (timing) */,
                     void* mark_arg = nullptr);
void launch_deg_stats(const uint32_t* deg, uint32_t n, uint32_t* stats /*[0]=max,[1]=zeros*/,
                      hipStream_t s);
// Exclusive scan of n u32 (n < 2^32); tmp needs scan_tmp_words(n) u32 (front_layout.h).
void launch_scan_exclusive(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* tmp,
                           hipStream_t s);
size_t rsort_tmp_words(uint64_t n);  // rsort_layout(n).total (front_layout.h)
int rsort_first_width(int bits);
uint64_t* radix_sort_u64(const uint64_t* in, uint64_t* a, uint64_t* b, uint64_t n, int bit_lo,
                         int bit_hi, uint32_t* tmp, hipStream_t s, bool counted0 = false);
// (deg << 32 | id) of the ids with deg > 0 only, in id order; tmp: pack_nz_tmp_words(n) u32.
size_t pack_nz_tmp_words(uint32_t n);
void launch_pack_nonzero(const uint32_t* deg, uint32_t n, uint64_t* items, uint32_t* tmp,
                         hipStream_t s);
void launch_unpack_seq(const uint64_t* items, uint32_t zeros, uint32_t n_seq, uint32_t* seq,
                       uint32_t* rank, hipStream_t s, uint32_t* nsd = nullptr,
                       const uint32_t* selfc = nullptr, int file_mode = 0,
                       uint32_t base = 0 /* first sequence position written */);
// Counting-sort sequence (k_seqc_*): seq/rank/nsd of every id of degree 1 .. seqc_threshold()-1,
// rank INVALID for degree 0; the ids of higher degree go to big as (deg << 32 | id) in id order,
// to be sorted and unpacked from the position the returned device word (u64) holds.
size_t seqc_tmp_words(uint32_t n);
uint32_t seqc_threshold();
// selfc (nullable): nsd = deg - w * selfc (w = 2 in FILE mode).
uint32_t* launch_seqc_place(const uint32_t* deg, uint32_t n, uint32_t* seq, uint32_t* rank,
                            uint32_t* nsd, uint64_t* big, uint32_t* tmp, hipStream_t s,
                            const uint32_t* selfc, int file_mode);
void launch_fill(uint32_t* p, uint32_t value, uint64_t n, hipStream_t s);
void launch_rank_scatter(const uint32_t* seq, uint32_t n_seq, uint32_t* rank, uint32_t* err,
                         hipStream_t s);
// edge pass + the first radix pass's tile histograms (sort bits from `shift`, DB wide)
void launch_edge_pass_tiles(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                            uint32_t* pst, uint64_t* items, uint32_t* err, int shift, int DB,
                            uint32_t* tmp, hipStream_t s, bool pre = false);
// Hi bins (one-pass grouping, see sheep_kernels.hip): chunk degree sums (256 ranks per chunk).
void launch_chunk_degsum(const uint32_t* seq, const uint32_t* deg, uint32_t n_seq, uint64_t* out,
                         hipStream_t s, const uint32_t* nsd = nullptr);
// Records (uv, or k_part's pre records) -> items (hi << 32 | lo) grouped by hi bin: the edge
// pass counting bins (no pst; nb <= 512 bounds, bounds[0] = 0, bounds[nb-1] = n_seq so that
// INVALID his fall in the last bin; items, each item's bin into digits (m u16), tile bin counts
// into tmp: rsort_tmp_words(m)), then the scatter by bin.
// Returns the buffer holding the result (items_b; items is then free); uv may be items_b.
// bin_start: nb + 1 u64; h_start (pinned, nullable): bin_start, copied out before the scatter
// runs; started: recorded once h_start is written.
uint64_t* group_by_bins(const uint32_t* uv, bool pre, uint64_t m, const uint32_t* rank,
                        uint32_t n_rank, uint32_t* err, const uint32_t* bins, uint32_t nb,
                        uint64_t* items, uint64_t* items_b, uint32_t* tmp, uint16_t* digits,
                        unsigned long long* bin_start, hipStream_t s,
                        unsigned long long* h_start = nullptr, hipEvent_t started = nullptr);
// Partitioned rank gathers: uv (x, y) -> pre (x, rank[y] | sentinel) in x-digit order (mid:
// m u64 scratch, ws: PART_WS_WORDS u32 scratch); then launch_edge_pass_tiles(pre, ..., pre = true).
// ws: y / x digit counts, the first pass's u64 cursors, the u32 region starts of both passes'
// outputs, the second pass's cursors, the first pass's capacity region ends (sheep_kernels.hip).
// The fused front pass's region cursors (k_front_fused: one device-scope atomic per region and
// tile, ~134 M a call at RMAT-26, performed at the memory side) are spread over memory: cursor
// q sits at u64 index fs_cix(q) = (q / 8) * SHEEP_FS_CLS + q % 8, eight to a 64-B line and
// consecutive lines SHEEP_FS_CLS u64 apart (8: contiguous).
// (FS_CLS and fs_cur_words, the cursors' words: front_layout.h)
__host__ __device__ inline uint32_t fs_cix(uint32_t q) { return (q >> 3) * FS_CLS + (q & 7u); }
// (+ the fused front pass's subregion tables: 8192 u64 starts + 2, cursors (spread), ends, u32
// tile map)
// The second partition pass's x-digit counts (256 u32, added to by every tile of the first pass
// or the fused pass) are spread the same way: digit i at xh_ix(i) = (i / 16) * XH_CLS + i % 16.
constexpr uint32_t XH_CLS = 128;
__host__ __device__ inline uint32_t xh_ix(uint32_t i) { return (i >> 4) * XH_CLS + (i & 15u); }
constexpr size_t XH_WORDS = (256 / 16) * XH_CLS;
constexpr size_t PART_WS_WORDS = 1280 + 2 * 1024 + 1025 + 257 + 2 * 256 + 2 * 1024 +
                                 2 * (8192 + 2) + fs_cur_words(8192) + 2 * 8192 + 8192 + 1 +
                                 1 + XH_WORDS;
// p6: the second pass's records are packed to 6 bytes (sheep_kernels.hip "packed 6-byte
// records"; only where part_p6_ok(n_rank) and an id >= n_rank fails the call).
bool part_p6_ok(uint32_t n_rank);
void launch_part_gather(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                        uint64_t* mid, uint64_t* pre, uint32_t* ws, hipStream_t s,
                        bool yhist_ready = false, bool p6 = false);
// The two passes of launch_part_gather separately (the first needs no ranks, so it can run
// while the sequence is sorted): uv -> mid (y-digit order), then mid -> pre (x-digit order).
void launch_part_first(const uint32_t* uv, uint64_t m, uint32_t n_rank, uint64_t* mid,
                       uint32_t* ws, hipStream_t s, bool yhist_ready);
// out6: pre is written packed; caps: mid holds launch_part_first_caps's regions (mid_slots);
// in6 (with caps): ... launch_front_fused's packed ones.
// (in6: the tiles follow the fused pass's subregions, G per y digit: launch_front_fused's G.)
void launch_part_second(const uint64_t* mid, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                        uint64_t* pre, uint32_t* ws, hipStream_t s, bool out6 = false,
                        uint64_t mid_slots = 0, bool caps = false, bool in6 = false,
                        uint32_t G = 1);
// Sampled capacities (sheep_kernels.hip, "sampled capacities"): the degree pass without a
// counting read — a 1/256 sample sizes each bucket's and each y digit's capacity region; the
// y regions go to part_ws for launch_part_first_caps (mid_slots records; the event caps_done
// marks them written).  *ovf is set when a run outgrew its region: the degrees
// are then invalid and the caller runs the exact pass.  False when not applicable.
// tmp: degs_tmp_words (degs_layout, front_layout.h: the sampled view; the fused pass below takes
// the same slot by its fused view).
size_t degs_tmp_words(uint64_t m, uint32_t n_ids);
bool launch_degree_sampled(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                           uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                           uint32_t* part_ws, uint64_t mid_slots, uint32_t* stats, uint32_t* ovf,
                           hipStream_t s, hipEvent_t caps_done);
// The fused front pass (sheep_kernels.hip k_front_fused): degrees and the first partition from
// ONE read of the records, into sampled capacity regions (mid_slots, a multiple of 8, packed
// records in mid).  *ovf_x: the degrees need the exact pass; *ovf_y: the partition must be
// redone from uv, and the degrees too (the histogram counts y's ids from the packed records).  False when not applicable (front_fused_ok).
// G (option ff_groups, 1..8): tile groups, each writing its own subregion of every region
// (sheep_kernels.hip k_front_fused); front_fused_slots: the mid_slots these regions need.
bool front_fused_ok(uint64_t m, uint32_t n_ids);
uint64_t front_fused_slots(uint64_t m, uint32_t n_ids, uint32_t G);
bool launch_front_fused(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                        uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                        uint32_t* part_ws, uint64_t* mid, uint64_t mid_slots, uint32_t* stats,
                        uint32_t* ovf_x, uint32_t* ovf_y, hipStream_t s,
                        void (*mark)(void*, const char*) = nullptr, void* mark_arg = nullptr,
                        uint32_t G = 1);
void launch_part_first_caps(const uint32_t* uv, uint64_t m, uint32_t n_rank, uint64_t* mid,
                            uint64_t mid_slots, uint32_t* ws, uint32_t* ovf, hipStream_t s);
void launch_pst_from_count(const uint32_t* seq, uint32_t n_seq, const uint32_t* deg,
                           const uint32_t* selfc, int file_mode, const uint32_t* cnt, uint32_t* pst,
                           hipStream_t s,
                           const uint32_t* nsd = nullptr);
void launch_kb_bounds(const uint64_t* items, uint64_t n, uint32_t K_e, uint32_t K_r,
                      uint32_t n_seq, int gshift, unsigned long long* out, hipStream_t s);
// The records of a kb bucket when they were binned directly (launch_edge_bin): bins [i0, i1),
// bin i's items at [start[i], min(cur[i], cap[i])) (device arrays).
struct KbSegs {
  const unsigned long long* start;
  const unsigned long long* cur;
  const unsigned long long* cap;
  uint32_t i0, i1;
};
// Direct binning (sheep_kernels.hip): records (uv, or k_part's pre records) -> items grouped by
// hi bin, each bin in its capacity region [cursor[b] at entry, cap_end[b]); cursor[b] ends at
// the bin's fill.  *ovf is set (and the run dropped) when a bin overflows its capacity.
// part_ws (non-null only with pre): the records are launch_part_second's packed output, whose
// x-digit regions part_ws holds.
void launch_edge_bin(const uint32_t* uv, bool pre, uint64_t m, const uint32_t* rank,
                     uint32_t n_rank, uint32_t* err, const uint32_t* bins, uint32_t nb,
                     unsigned long long* cursor, const unsigned long long* cap_end, uint64_t* out,
                     uint32_t* ovf, hipStream_t s, const uint32_t* part_ws = nullptr);
// The device state of one kb loop (the bucket-synchronous tree loop of tree_from_sorted and of
// the lockstep sessions; kb_state_init in sheep_capi.cpp allocates and initialises it).  Which
// set or slot a bucket uses is written once, in the accessors.
struct KbState {
  uint32_t n_seq = 0;
  size_t bm_words = 0;   // words of one mark bitmap and of the giant bitmap (n_seq / 32 + 2)
  size_t spq_words = 0;  // words of one spine queue (n_seq / 32 + 64)
  // Parent and hint interleaved (pj[2v], pj[2v + 1]; launch_pj_init): a zipper step loads one
  // line.  The parents are copied out after the loop (launch_pj_parents).
  uint32_t* pj = nullptr;
  uint32_t* parent() const { return pj; }
  uint32_t* uf = nullptr;      // union-find over the ranks (iota)
  uint32_t* label = nullptr;   // a root's component's elimination-tree root (iota)
  uint32_t* linked = nullptr;  // the pre-bucket roots a zipper linked, for the bucket's union
  // 16 words per set, zero before the first bucket: [1] n_linked, [2] n_spine, [3] n_kept (each
  // bucket's label kernel resets its set)
  uint32_t* counters = nullptr;
  uint32_t* bitmap = nullptr;  // the marks (the giant's records into a bucket): bm_words per set
  uint32_t* spq = nullptr;     // the spine queues: spq_words per set
  uint32_t* gbits = nullptr;  // giant bitmap (k_kb_map): bit v = v is in its reference vertex's
  uint32_t* gx = nullptr;     //   component; that vertex, in two slots (INV: none yet)
  // Giant summary the maps test first (bit q: ranks [64q, 64q + 64) all set in gbits; n_seq /
  // 2048 + 1 words), rewritten by each rebase.  Nullable: it pays on large inputs only.
  uint32_t* gsum = nullptr;
  // The giant's anchor of each map, picked on the device (launch_kb_rebase), in two slots; the
  // kernels take the slot's rank unless the host's anchor rank is INV (no giant yet).
  uint32_t* anc = nullptr;
  unsigned long long* st = nullptr;  // 16 stats words (diagnostics; the zipper's from st + 8)
  uint32_t* hcnt = nullptr;          // nullable: the maps add each hi's run length (for pst)
  // Counters, marks and spine queues alternate between two sets by bucket parity, so that map
  // k + 1 may run beside apply k (false: one set, a loop that never overlaps them).
  bool two_sets = true;
  size_t set_of(size_t k) const { return two_sets ? (k & 1) : 0; }
  uint32_t* cnt_of(size_t k) const { return counters + set_of(k) * 16; }
  uint32_t* bm_of(size_t k) const { return bitmap + set_of(k) * bm_words; }
  uint32_t* spq_of(size_t k) const { return spq + set_of(k) * spq_words; }
  // Map j reads its anchor and the bitmap's reference vertex from slot j & 1.  The rebase for
  // map j (launch_kb_rebase) reads slot (j - 1) & 1, what map j - 1 used, and writes slot j & 1,
  // at a point where nothing else touches the union-find (map j - 1 and apply j - 1 complete);
  // an apply passes the j of the latest rebase on its stream.
  uint32_t* gx_of(size_t j) const { return gx + (j & 1); }
  uint32_t* anc_of(size_t j) const { return anc + (j & 1); }
};
// One kb bucket in two halves (sheep_kernels.hip): the map (records -> kept pairs + giant marks
// + hi counts) and the apply (spine, zipper, union-find fold, labels).
// anchor: a rank whose component is taken as the giant (INV: none; sheep_kernels.hip).  segs
// (nullable): the records were binned directly, e_begin / e_end bound its bins' capacity.
// kept_cap: the u64 slots kept holds (a reservation past it raises the fault word, -EIO).
// gshift, bins / nb (nullable): how the items are grouped by hi.  defer: 1: misses kept as
// (b, a) for launch_kb_apply's refresh; 2: as (b, root of a) (split lockstep); 0: as (b, label).
void launch_kb_map(const KbState& S, size_t k, const uint64_t* items, uint64_t e_begin,
                   uint64_t e_end, const KbSegs* segs, uint32_t B0, uint32_t anchor,
                   uint64_t* kept, uint64_t kept_cap, int gshift, const uint32_t* bins,
                   uint32_t nb, int defer, bool stats, hipStream_t s);
// Before map j (j >= 1), with nothing else running on the union-find: the giant's anchor for
// map j, picked on the device among ranks [0, B0lim) (the component holding most of an even
// sample; INV when B0lim = 0), the giant bitmap rebased on it, and the giant summary (if any)
// of the rebased bitmap.
void launch_kb_rebase(const KbState& S, size_t j, uint32_t B0lim, hipStream_t s);
// Giant sweep (sheep_kernels.hip k_gb_sweep): the giant bits of every rank v < B0lim in the
// component of the bitmap's reference vertex (slot gx_slot, as launch_kb_apply), with nothing
// that may move that vertex running beside it.
void launch_gb_sweep(const KbState& S, uint32_t B0lim, size_t gx_slot, hipStream_t s);
// Apply of bucket k = ranks [B0, B1) over its kept pairs, whose starts it first re-resolves
// against the current union-find (the map ran beside an earlier apply).  gx_slot: the j
// of the latest rebase on this stream.  The union keeps the root of map k + 1's anchor on top.
void launch_kb_apply(const KbState& S, size_t k, uint32_t B0, uint32_t B1, uint32_t anchor,
                     bool nonempty, uint64_t* kept, bool stats, size_t gx_slot, hipStream_t s);
// Lockstep exchange of one bucket (sheep_ls_*): pack this rank's mark words [w0, w1] (ms u64
// slots) and kept pairs (padded to cap) for an all-gather; unpack P such blocks into the
// bitmap (OR) and a contiguous kept array, setting *n_kept = P * cap (kept and n_kept
// nullable: the marks only).
void launch_ls_pack(const uint32_t* bitmap, uint32_t w0, uint32_t w1, uint32_t ms, uint64_t* send,
                    const uint32_t* n_kept /* device */, uint32_t cap, hipStream_t s);
void launch_ls_count(const uint32_t* n_kept, long long* out, hipStream_t s);
void launch_ls_unpack(const uint64_t* recv, uint32_t P, uint32_t ms, uint32_t cap, uint32_t* bitmap,
                      uint32_t w0, uint32_t w1, uint64_t* kept, uint32_t* n_kept, hipStream_t s);
// Split lockstep apply of bucket k (P > 1; see sheep_kernels.hip): the refresh alone, over the
// owner's copies of the pairs (kept, *n_kept) and marks (bitmap); G of the bucket's giant into
// *gslot; every rank's union-find part (fold, union of the kept pairs in recv, labels; counters
// reset); the owner's spine + zipper over its copies (zn: n_kept, n_spine, G).
void launch_kb_refresh(const KbState& S, size_t k, uint64_t* kept, const uint32_t* n_kept,
                       uint32_t* bitmap, uint32_t B0, uint32_t anchor, size_t gx_slot,
                       hipStream_t s);
void launch_ls_gslot(const KbState& S, size_t k, uint32_t anchor, uint32_t* gslot, hipStream_t s);
void launch_ls_fold_union_label(const KbState& S, size_t k, uint32_t B0, uint32_t B1,
                                uint32_t anchor, bool nonempty, const uint64_t* recv, uint32_t P,
                                uint32_t ms, uint32_t cap, size_t gx_slot, hipStream_t s);
void launch_ls_zip(const uint64_t* zkept, uint32_t* zn, const uint32_t* zbm, uint32_t* zspq,
                   uint32_t B0, uint32_t B1, bool has_anchor, uint32_t* parent, hipStream_t s);
void launch_add_u32(uint32_t* p, uint64_t n, uint32_t d, hipStream_t s);  // p[i] += d (wraps)
// Sharded degree sequence (P > 1, sheep_capi.cpp sequence_sharded; see sheep_kernels.hip).
void launch_seq_runs(const uint64_t* sorted, uint32_t n, uint32_t* lst, uint32_t* H, hipStream_t s);
void launch_seq_base(const uint32_t* hall, uint32_t P, uint32_t r, uint32_t D, uint32_t Dp,
                     uint32_t* tot, uint32_t* pre, hipStream_t s);
void launch_seq_rank(const uint64_t* sorted, uint32_t n, const uint32_t* S, const uint32_t* pre,
                     const uint32_t* lst, uint32_t* rank_slice, hipStream_t s);
void launch_seq_from_rank(const uint32_t* rank, uint32_t n_ids, uint32_t* seq, hipStream_t s);
void launch_deg_of_rank(const uint32_t* S, uint32_t D, uint32_t n_seq, uint32_t* out, hipStream_t s);
void launch_seq_stats64(const uint32_t* stats, uint32_t c, long long* out, hipStream_t s);
void launch_iota(uint32_t* p, uint32_t n, hipStream_t s);
void launch_forest_items(const uint32_t* parent, uint32_t n, uint64_t* items, hipStream_t s);
// The kb loop's parents and hints, interleaved (pj[2v] = parent, pj[2v + 1] = hint; 2n words):
// (INVALID, 0) for every rank; the parents out to parent[0, n).
void launch_pj_init(uint32_t* pj, uint32_t n, hipStream_t s);

void launch_pj_parents(const uint32_t* pj, uint32_t n, uint32_t* parent, hipStream_t s);
// Partition quality (sheep_eval.hip).  ws: 4k + 8 u64: [0,3k) hash/down/up balances, [3k,4k)
// vertex balance, then cut, self-loop records, nodes, and the distinct keys of vcom, hash,
// down, up.  keys/keys_b: 2m u64; rtmp: rsort_tmp_words(2m) u32; deg: LLAMA degrees.
// passes (nullable / empty: one pass over the 2m entries): (first id, keys bound) of
// consecutive id ranges; each pass sorts only the entries X -> Y with X in its range (keys /
// keys_b then need the largest bound, not 2m).  ws[4k + 7] is the passes' append counter.
void launch_evaluate(const uint32_t* uv, uint64_t m, const int16_t* parts, const uint32_t* pos,
                     const uint32_t* deg, uint32_t n_ids, uint32_t k, uint64_t* keys,
                     uint64_t* keys_b, uint32_t* rtmp, unsigned long long* ws, uint32_t* err,
                     hipStream_t s,
                     const std::vector<std::pair<uint32_t, uint64_t>>* passes = nullptr);
// graph2tree -p K -o OUT (sheep_eval.hip): the non-self-loop records as (min, max) pairs,
// grouped by the part of their lower-sequence endpoint, each part in (min, record) order.
// items / items_b: m u64; rtmp: rsort_tmp_words(m); out: 2m u32; pstart: n_parts + 1 u64.
void launch_partition_edges(const uint32_t* uv, uint64_t m, const int16_t* parts, const uint32_t* pos,
                            uint32_t n_ids, uint32_t n_parts, uint64_t* items, uint64_t* items_b,
                            uint32_t* rtmp, uint32_t* out, unsigned long long* pstart, uint32_t* err,
                            hipStream_t s);
// Tree certificate and tree facts (sheep_verify.hip; index arithmetic in verify_layout.h).
// The counter words (ws: VF_WS_WORDS u64, reset by launch_vf_heap): violation counts, the
// smallest rank in any violation (low word; INV: none), then the facts' reductions.
enum { VF_HEAP = 0, VF_A, VF_B, VF_PST, VF_MIN, VF_ROOTS, VF_WIDTH, VF_EDGES, VF_HALO, VF_VH, VF_EH,
       VF_WS_WORDS = 16 };
// Children lists and Euler tour of a heap-ordered forest over n ranks (n < 2^31: 2n arcs).
struct VfTour {
  uint32_t n = 0;
  uint64_t* kids = nullptr;     // n: (parent << 32 | v) sorted by parent (roots under parent n)
  uint32_t* kfirst = nullptr;   // n + 1: first slot of a parent's children (INV: none)
  uint32_t* klast = nullptr;    // n + 1: their last slot
  uint64_t* cells_a = nullptr;  // 2n each: the list ranking's double buffer
  uint64_t* cells_b = nullptr;
  uint2* tt = nullptr;          // n: (tin, tout) tour positions per rank
  uint32_t* ktin = nullptr;     // n: tin of the child in each slot
};
// Wave reductions of the verifier's and the widths' counters (the result in lane 0).
__device__ __forceinline__ unsigned long long vf_wave_sum(unsigned long long c) {
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  return c;
}
__device__ __forceinline__ uint32_t vf_wave_min(uint32_t c) {
  for (int o = 32; o > 0; o >>= 1) c = min(c, (uint32_t)__shfl_down(c, o));
  return c;
}
__device__ __forceinline__ unsigned long long vf_wave_max(unsigned long long c) {
  for (int o = 32; o > 0; o >>= 1) c = max(c, (unsigned long long)__shfl_down(c, o));
  return c;
}
// Resets ws, then counts heap-order violations (VF_HEAP, VF_MIN) and roots (VF_ROOTS).
void launch_vf_heap(const uint32_t* parent, uint32_t n, unsigned long long* ws, hipStream_t s);
void launch_vf_items(const uint32_t* parent, uint32_t n, uint64_t* items, hipStream_t s);
// From T.kids (sorted): everything else of T.  Only for a forest that passed launch_vf_heap.
void launch_vf_tour(const VfTour& T, hipStream_t s);
// Per record: the pst recount into cnt (nullable; n zeroed words), (A) into VF_A / VF_MIN, the
// witness bytes (n, zeroed).  ERR_RANGE as the edge pass, and for a rank >= n.
void launch_vf_records(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_ids,
                       const uint32_t* parent, const VfTour& T, uint32_t* cnt, uint8_t* witness,
                       unsigned long long* ws, uint32_t* err, hipStream_t s);
// Per rank: non-roots without witness (VF_B), pst != cnt (VF_PST; pst nullable), VF_MIN.
void launch_vf_final(const uint32_t* parent, const uint32_t* pst, const uint32_t* cnt,
                     const uint8_t* witness, uint32_t n, unsigned long long* ws, hipStream_t s);
// VF_WIDTH .. VF_EH from the tour and pst.  wv / we: 2n i64 each (T.cells_a / cells_b are free
// once launch_vf_tour is done); sums: vf_scan_tiles(n) i64.
size_t vf_scan_tiles(uint32_t n);
void launch_vf_facts(const VfTour& T, const uint32_t* pst, long long* wv, long long* we,
                     long long* sums, unsigned long long* ws, hipStream_t s);
// In-place inclusive scan of the 2n i64 values of a tour (sums: vf_scan_tiles(n) i64).
void launch_vf_scan(long long* io, uint32_t n, long long* sums, hipStream_t s);
// Exact tree widths (sheep_width.hip; index arithmetic in width_layout.h).  The counter words
// (ws: TW_WS_WORDS u64, reset by launch_tw_rmq): records violating (A), then the reductions.
enum { TW_A = 0, TW_WIDTH, TW_FILL, TW_HALO, TW_WS_WORDS = 8 };
struct TwBufs {
  uint32_t* depth = nullptr;    // 2n: depth after the arc at each tour position
  uint64_t* pre = nullptr;      // 2n each: in-block prefix / suffix minima (depth << 32 | pos)
  uint64_t* suf = nullptr;
  uint64_t* tab = nullptr;      // tw_levels(nb) * nb: the sparse table over the block minima
  uint32_t* lca_tin = nullptr;  // 2n: tin of the rank a minimum at this position names (INV: none)
  uint8_t* has_lower = nullptr;  // n: the rank is some record's upper end
};
// The range-minimum structure from the depths sv (launch_vf_facts's first scan) of a toured forest.
void launch_tw_rmq(const VfTour& T, const uint32_t* parent, const long long* sv, const TwBufs& B,
                   unsigned long long* ws, hipStream_t s);
// keys[i] (m u64) of every record: (hi << 32 | tin lo), TW_SKIP for one that counts nothing;
// (A) violations into ws[TW_A]; ERR_RANGE as launch_vf_records.
void launch_tw_keys(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_ids,
                    const VfTour& T, uint64_t* keys, unsigned long long* ws, uint32_t* err,
                    hipStream_t s);
// From the sorted keys: the weights wt (2n i64, zeroed here) at tin positions.
void launch_tw_weights(const uint64_t* keys, uint64_t m, const VfTour& T, const TwBufs& B,
                       long long* wt, hipStream_t s);
// From the scanned weights S: width_out (n, nullable), ws[TW_WIDTH .. TW_HALO].
void launch_tw_final(const VfTour& T, const uint32_t* pst, const long long* S, uint32_t* width_out,
                     unsigned long long* ws, hipStream_t s);
// Forward partition of a tree in HBM (sheep_part.hip; the host half in part_layout.h).  The
// counter words (ws: PT_WS_WORDS u64, reset by launch_pt_reduce): sum and maximum of pst, maximum
// of seq.
enum { PT_TOTAL = 0, PT_WMAX, PT_SEQMAX, PT_WS_WORDS = 8 };
struct PtHeavy;  // part_layout.h
struct PtDelta;
void launch_pt_reduce(const uint32_t* pst, const uint32_t* seq, uint32_t n, unsigned long long* ws,
                      hipStream_t s);
// s0 (n u64): the subtree sum of pst per rank; ks0 (n u64): the same in children-list slot order
// (ks0[i] belongs to the kid in T.kids[i]).  wt: 2n i64 scratch; sums: vf_scan_tiles(n) i64.
void launch_pt_sums(const VfTour& T, const uint32_t* pst, long long* wt, long long* sums,
                    unsigned long long* s0, unsigned long long* ks0, hipStream_t s);
// flag / idx (n + 1 u32 each): s0[v] > max_component and its exclusive scan, idx[n] = |H|; tmp:
// scan_tmp_words(n + 1) u32.
void launch_pt_flag(const unsigned long long* s0, uint32_t n, uint64_t max_component, uint32_t* flag,
                    uint32_t* idx, uint32_t* tmp, hipStream_t s);
// out (nh records): the heavy ranks ascending, each with its parent's index in H.
void launch_pt_heavy(const uint32_t* flag, const uint32_t* idx, const uint32_t* parent,
                     const unsigned long long* s0, const VfTour& T, uint32_t nh, PtHeavy* out,
                     hipStream_t s);
// row (n_vid int16) = -1, then row[seq[v]] = the part of v's nearest packed ancestor-or-self from
// the nd deltas (wt: 2n i64 scratch).  ERR_RANGE for a seq id >= n_vid (nothing is stored for it).
void launch_pt_push(const PtDelta* deltas, uint32_t nd, const VfTour& T, long long* wt, long long* sums,
                    const uint32_t* seq, uint32_t n_vid, int16_t* row, uint32_t* err, hipStream_t s);
// XS1 records {u32 tail, u32 head, f32 weight} -> (tail, head) pairs; max id + 1 into *max_id.
void launch_strip_xs1(const uint32_t* raw, uint64_t n, uint32_t* uv, uint32_t* max_id, hipStream_t s);
// One chunk of SNAP text (sheep_ingest.hip; net_layout.h): n bytes at text (allocated up to a
// multiple of 16), the chunk's first byte at file_off; tiles: net_tiles(n) u32 scratch; state:
// the pass's NET_WORDS u64.  uv null: the count pass (token count and stop pair only); else the
// values of the tokens in [lo2, hi2) go to uv[t - lo2] and their max id + 1 to NET_MAX.
void launch_net_chunk(const uint8_t* text, uint32_t n, uint64_t file_off, uint32_t* tiles,
                      unsigned long long* state, uint32_t* uv, uint64_t lo2, uint64_t hi2,
                      hipStream_t s);
void launch_merge(uint32_t* parent_a, uint32_t* pst_a, const uint32_t* parent_b,
                  const uint32_t* pst_b, uint32_t n, uint32_t* jump, hipStream_t s);
void launch_rmat(uint32_t* uv, int scale, uint64_t seed, uint64_t e_begin, uint64_t e_end,
                 hipStream_t s);
void launch_powerlaw(uint32_t* uv, uint32_t n, double gamma, double i0, uint64_t seed,
                     uint64_t e_begin, uint64_t e_end, hipStream_t s);

}  // namespace sheep
