// HIP kernels for gfx950 (MI355X) — Sheep's tree-construction hot path.
//
// All arithmetic is u32 integer work bound by HBM traffic, random gathers and atomics; nothing
// here is GEMM-shaped, so there is no MFMA.  Wave = 64 lanes throughout (ballots are 64-bit).
//
//   k_degree        per-vertex degree (sequence.h:101-107 / graph_wrapper.h:87-89)
//   k_degb_*        LDS-bucketed degree histogram (large inputs)
//   k_rsort_*       stable LSD radix sort of packed u64 items, LDS-ranked and LDS-staged
//                   8192-item tiles (degree sequence: sequence.h:55-61; edges by max(rank))
//   k_scan_*        exclusive scan (radix offsets)
//   k_edge_pass_tiles / k_edge_bin
//                   rank translation, pst_weight (jtree.cpp:84-87), (lo,hi) tree edges
//   k_tree_insert   lock-free elimination-tree insertion ("zipper"), replacing the
//                   union-find loop jtree.cpp:73-83 + unionfind.h:46-102
//   k_merge         associative tree union (jnode.cpp:174-201) with the same insertion
//   k_rmat          synthetic input generator (rmat.h)
// The s_waitcnt immediates below are gfx9 encodings (vmcnt bits [3:0] and [15:14], lgkmcnt
// [11:8]); on another target they would silently mean a different wait.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sheep_amd kernels are written for gfx950 only"
#endif
#include <atomic>
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <algorithm>

#include "powerlaw.h"
#include "rmat.h"
#include "sheep_comm.h"
#include "sheep_internal.h"

namespace sheep {

static constexpr int BLOCK = 256;
static constexpr int ITEMS = 16;
static constexpr int TILE = BLOCK * ITEMS;  // keys per radix/scan tile
static constexpr int MAX_GRID = 256 * 8;    // 8 blocks of 256 per CU over 256 CUs

// Compute units of the current device.
static unsigned device_cus() {
  static thread_local int cached_dev = -1;
  static thread_local unsigned cached = 0;
  int dev = 0, n = 0;
  (void)hipGetDevice(&dev);
  if (dev != cached_dev) {
    (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    cached = n > 0 ? (unsigned)n : 256u;
    cached_dev = dev;
  }
  return cached;
}

// Device fault word.  The tree kernels trust what earlier kernels wrote (ranks, offsets, the
// forest), and a corrupt input could turn a walk into an endless loop (a lab variant that left
// the degree scatter's output unwritten once hung a later kernel).  So every unbounded walk is
// guarded: a zipper walk that meets a parent not above its child, or a union-find walk longer
// than FAULT_STEPS, stops and raises the fault; the host reports it as -EIO after the call.
__device__ uint32_t g_fault;
static constexpr uint32_t FAULT_STEPS = 1u << 26;
__device__ __forceinline__ void raise_fault(uint32_t bit) { atomicOr(&g_fault, bit); }
constexpr uint32_t FAULT_FOREST = 1u, FAULT_UF = 2u, FAULT_KEPT = 4u;

// The address is looked up once per device and cached (a runtime symbol lookup per
// synchronising call otherwise).  (Round 6 first took the ~0.3-0.4 ms idle gaps at the end of
// the traces' last step for this lookup; they are bench.py's own readbacks after its timed
// loop, and the cache changed no step time: profiles/r06/c_edge_tilemap/.)
uint32_t* fault_word() {
  static std::atomic<uint32_t*> cache[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
  uint32_t* p = cache[d].load(std::memory_order_acquire);
  if (p) return p;
  void* q = nullptr;
  if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_fault)) != hipSuccess) return nullptr;
  cache[d].store((uint32_t*)q, std::memory_order_release);
  return (uint32_t*)q;
}

static inline unsigned grid_for(uint64_t n, int per_block = BLOCK) {
  uint64_t g = (n + per_block - 1) / per_block;
  if (g < 1) g = 1;
  if (g > MAX_GRID) g = MAX_GRID;
  return (unsigned)g;
}

// ---------------------------------------------------------------------------------------
// Degree.  LLAMA mode: deg[t]++, deg[h]++ unless t == h (a self-loop is one adjacency entry,
// graph_wrapper.h:43-63 as loaded LL_L_UNDIRECTED_DOUBLE).  FILE mode: deg[t]++, deg[h]++
// always (sequence.h:105-106).
// ---------------------------------------------------------------------------------------
__global__ void k_degree(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode,
                         uint32_t* __restrict__ deg, uint32_t* __restrict__ selfc, uint32_t* err) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += stride) {
    uint2 e = uv[i];
    if (e.x >= n_ids || e.y >= n_ids) { atomicOr(err, ERR_RANGE); continue; }
    atomicAdd(&deg[e.x], 1u);
    if (file_mode || e.x != e.y) atomicAdd(&deg[e.y], 1u);
    if (selfc && e.x == e.y) atomicAdd(&selfc[e.x], 1u);
  }
}

void launch_degree(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode, uint32_t* deg,
                   uint32_t* selfc, uint32_t* err, hipStream_t s) {
  if (n_ids) (void)hipMemsetAsync(deg, 0, (size_t)n_ids * 4, s);
  if (n_ids && selfc) (void)hipMemsetAsync(selfc, 0, (size_t)n_ids * 4, s);
  if (m == 0) return;
  hipLaunchKernelGGL(k_degree, dim3(grid_for(m)), dim3(BLOCK), 0, s, (const uint2*)uv, m, n_ids,
                     file_mode, deg, selfc, err);
}

// pst_weight without per-edge atomics.  For the jnid r of vertex v = seq[r], the records at v
// that are not self-loops are either PREORDER (other endpoint earlier in seq: r is their hi)
// or POSTORDER (other endpoint later, or not in seq): jtree.cpp:78-87.  So
//     pst[r] = nsdeg[v] - |{records with hi == r}|,   nsdeg[v] = deg[v] - w * selfloops[v]
// (w = 1 for LLAMA degrees, 2 for FILE degrees), and the second term cnt[r] is counted by
// k_kb_map.
// nsd (nullable): nsdeg already in rank order (k_unpack_seq), read instead of two gathers.
__global__ void k_pst_from_count(const uint32_t* __restrict__ seq, uint32_t n_seq,
                                 const uint32_t* __restrict__ deg, const uint32_t* __restrict__ selfc,
                                 uint32_t w, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ pst,
                                 const uint32_t* __restrict__ nsd) {
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_seq; r += gridDim.x * blockDim.x) {
    if (nsd) {
      pst[r] = nsd[r] - cnt[r];
    } else {
      uint32_t v = seq[r];
      pst[r] = deg[v] - w * selfc[v] - cnt[r];
    }
  }
}

void launch_pst_from_count(const uint32_t* seq, uint32_t n_seq, const uint32_t* deg,
                           const uint32_t* selfc, int file_mode, const uint32_t* cnt, uint32_t* pst,
                           hipStream_t s, const uint32_t* nsd) {
  if (n_seq == 0) return;
  hipLaunchKernelGGL(k_pst_from_count, dim3(grid_for(n_seq)), dim3(BLOCK), 0, s, seq, n_seq, deg,
                     selfc, file_mode ? 2u : 1u, cnt, pst, nsd);
}

// stats[0] = max degree, stats[1] = number of zero-degree ids, stats[2] = number of ids of
// degree >= SEQ_BIG (the sequence's radix-sorted tail: its size is then known with the other
// two, and the sequence needs no readback of where the tail starts).
static constexpr uint32_t SEQ_BIG = 1024;
__device__ __forceinline__ void block_sync();
// Max degree and zero-degree count: 16-B loads when deg is 16-B aligned (V4; else one word per
// load), one pair of atomics per workgroup.
template <bool V4>
__global__ void k_deg_stats(const uint32_t* __restrict__ deg, uint32_t n, uint32_t* stats) {
  __shared__ uint32_t smx[BLOCK / 64], szr[BLOCK / 64], sbg[BLOCK / 64];
  uint32_t mx = 0, zeros = 0, big = 0;
  const uint32_t n4 = V4 ? n / 4 : 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
    const uint4 q = ((const uint4*)deg)[i];
    mx = max(max(mx, max(q.x, q.y)), max(q.z, q.w));
    zeros += (q.x == 0) + (q.y == 0) + (q.z == 0) + (q.w == 0);
    big += (q.x >= SEQ_BIG) + (q.y >= SEQ_BIG) + (q.z >= SEQ_BIG) + (q.w >= SEQ_BIG);
  }
  for (uint32_t i = 4 * n4 + blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    const uint32_t d = deg[i];
    mx = max(mx, d);
    zeros += d == 0;
    big += d >= SEQ_BIG;
  }
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    zeros += (uint32_t)__shfl_xor((int)zeros, o);
    big += (uint32_t)__shfl_xor((int)big, o);
  }
  if ((threadIdx.x & 63) == 0) {
    smx[threadIdx.x >> 6] = mx;
    szr[threadIdx.x >> 6] = zeros;
    sbg[threadIdx.x >> 6] = big;
  }
  block_sync();
  if (threadIdx.x == 0) {
    for (int i = 1; i < BLOCK / 64; ++i) { mx = max(mx, smx[i]); zeros += szr[i]; big += sbg[i]; }
    if (mx) atomicMax(&stats[0], mx);
    if (zeros) atomicAdd(&stats[1], zeros);
    if (big) atomicAdd(&stats[2], big);
  }
}

void launch_deg_stats(const uint32_t* deg, uint32_t n, uint32_t* stats, hipStream_t s) {
  (void)hipMemsetAsync(stats, 0, 12, s);
  if (n == 0) return;
  const bool v4 = ((uintptr_t)deg & 15) == 0;
  hipLaunchKernelGGL(v4 ? k_deg_stats<true> : k_deg_stats<false>,
                     dim3(std::min<unsigned>(grid_for(v4 ? n / 4 + 1 : n), 1024)), dim3(BLOCK), 0, s,
                     deg, n, stats);
}

__global__ void k_fill(uint32_t* p, uint32_t v, uint64_t n) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}

void launch_fill(uint32_t* p, uint32_t value, uint64_t n, hipStream_t s) {
  if (n == 0) return;
  if (value == 0 || value == INV) {
    (void)hipMemsetAsync(p, value ? 0xFF : 0, n * 4, s);
    return;
  }
  hipLaunchKernelGGL(k_fill, dim3(grid_for(n)), dim3(BLOCK), 0, s, p, value, n);
}

// ---------------------------------------------------------------------------------------
// Exclusive scan (u32), TILE elements per block: reduce -> scan of block sums -> downsweep.
// ---------------------------------------------------------------------------------------
// Workgroup barrier that first drains the wave's LDS operations.  __syncthreads() alone was
// once compiled without that wait on a loop exit (k_degb_hist16: the last no-return ds_add of
// the counting loop could land after another wave's read behind the barrier, which lost or
// moved counts run to run — measured on the twitter shape), so every barrier here waits.
__device__ __forceinline__ void block_sync() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0); vmcnt and expcnt left at their maxima
  __syncthreads();
}

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  int lane = threadIdx.x & 63;
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = (uint32_t)__shfl_up((int)v, o);
    if (lane >= o) v += t;
  }
  return v;
}

// Exclusive scan of one TILE held in LDS (tile[0..TILE)); returns the tile total.
__device__ uint32_t block_scan_tile(uint32_t* tile, uint32_t* wsum) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint32_t local[ITEMS];
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) { local[i] = tile[t * ITEMS + i]; sum += local[i]; }
  uint32_t incl = wave_incl_scan(sum);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t wbase = 0, total = 0;
#pragma unroll
  for (int i = 0; i < BLOCK / 64; ++i) { if (i < w) wbase += wsum[i]; total += wsum[i]; }
  uint32_t run = wbase + incl - sum;
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) { tile[t * ITEMS + i] = run; run += local[i]; }
  block_sync();
  return total;
}

__global__ void k_scan_reduce(const uint32_t* __restrict__ in, uint64_t n, uint32_t* sums) {
  uint64_t base = (uint64_t)blockIdx.x * TILE;
  uint32_t s = 0;
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t idx = base + (uint64_t)i * BLOCK + threadIdx.x;
    if (idx < n) s += in[idx];
  }
  for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o);
  __shared__ uint32_t ws[BLOCK / 64];
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  block_sync();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int i = 0; i < BLOCK / 64; ++i) t += ws[i];
    sums[blockIdx.x] = t;
  }
}

__global__ void k_scan_down(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                            uint64_t n, const uint32_t* __restrict__ offsets) {
  __shared__ uint32_t tile[TILE];
  __shared__ uint32_t wsum[BLOCK / 64];
  uint64_t base = (uint64_t)blockIdx.x * TILE;
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t idx = base + (uint64_t)i * BLOCK + threadIdx.x;
    tile[i * BLOCK + threadIdx.x] = idx < n ? in[idx] : 0;
  }
  block_sync();
  block_scan_tile(tile, wsum);
  uint32_t off = offsets ? offsets[blockIdx.x] : 0;
  for (int i = 0; i < ITEMS; ++i) {
    uint64_t idx = base + (uint64_t)i * BLOCK + threadIdx.x;
    if (idx < n) out[idx] = tile[i * BLOCK + threadIdx.x] + off;
  }
}

static_assert(TILE == SCAN_TILE, "scan_tmp_words (front_layout.h) counts this scan's tiles");

void launch_scan_exclusive(const uint32_t* in, uint32_t* out, uint64_t n, uint32_t* tmp,
                           hipStream_t s) {
  if (n == 0) return;
  if (n <= (uint64_t)TILE) {
    hipLaunchKernelGGL(k_scan_down, dim3(1), dim3(BLOCK), 0, s, in, out, n, (const uint32_t*)nullptr);
    return;
  }
  uint64_t nb = (n + TILE - 1) / TILE;
  uint32_t* sums = tmp;
  hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(BLOCK), 0, s, in, n, sums);
  launch_scan_exclusive(sums, sums, nb, tmp + nb, s);  // in-place: each tile is read before written
  hipLaunchKernelGGL(k_scan_down, dim3((unsigned)nb), dim3(BLOCK), 0, s, in, out, n,
                     (const uint32_t*)sums);
}

// ---------------------------------------------------------------------------------------
// Bucketed degree histogram (the path for large m).  Random global atomics run at ~22 G/s on
// MI355X (k_degree above: 95 ms for RMAT-26's 2.1 G endpoints), so endpoints are first
// partitioned by id range into NB <= 1024 buckets of 2^SH <= 65536 ids, written as 16-bit
// local ids, then counted in LDS:
//   k_degb_count    per-chunk bucket counts -> counts[chunk][bucket] (tile-major, tm_offsets)
//   k_degb_scatter  block-local counting sort of the chunk in LDS (its counts come from
//                   k_degb_count), then each wave writes whole bucket runs (~128 B at RMAT-26);
//                   self-loop records also bump selfc[v] (global atomics: self-loops are rare)
//   k_degb_hist     one workgroup per bucket (<= 32768 ids; k_degb_hist16 for 65536): LDS
//                   counters, wave-level aggregation of repeated ids (hubs), coalesced write
// LLAMA mode emits t, and h only when t != h; FILE mode emits both.
// Supports n_ids <= 2^26 (launch_degree_bucketed falls back to k_degree above that).
// The constants the passes' scratch layouts depend on (DEGB_THREADS, DEGB_CHUNK, DEGB_NB, TM_G,
// PD_Y, FF_GMAX, FS_MAX, FS_STRIDE) and the layouts themselves: front_layout.h.
// ---------------------------------------------------------------------------------------
// A record streamed once (non-temporal: it should not evict what the other kernels keep).
__device__ __forceinline__ uint2 ld_rec_nt(const uint2* p) {
  const uint64_t v = __builtin_nontemporal_load((const uint64_t*)p);
  return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
}
// k_deg_stats folded into the histogram kernels: the block's max degree and zero-degree ids,
// two global atomics per block (called by every thread of a DEGB_THREADS block).
__device__ __forceinline__ void deg_stats_flush(uint32_t* stats, uint32_t mx, uint32_t zeros,
                                                uint32_t big) {
  __shared__ uint32_t smx[DEGB_THREADS / 64], szr[DEGB_THREADS / 64], sbg[DEGB_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) {
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    zeros += (uint32_t)__shfl_xor((int)zeros, o);
    big += (uint32_t)__shfl_xor((int)big, o);
  }
  if ((threadIdx.x & 63) == 0) {
    smx[threadIdx.x >> 6] = mx;
    szr[threadIdx.x >> 6] = zeros;
    sbg[threadIdx.x >> 6] = big;
  }
  block_sync();
  if (threadIdx.x == 0) {
    for (int i = 1; i < DEGB_THREADS / 64; ++i) { mx = max(mx, smx[i]); zeros += szr[i]; big += sbg[i]; }
    if (mx) atomicMax(&stats[0], mx);
    if (zeros) atomicAdd(&stats[1], zeros);
    if (big) atomicAdd(&stats[2], big);
  }
}
// Tile-major count matrices and their scan (defined with the hi bins below).
static void tm_offsets(const uint32_t* counts, uint32_t* offsets, uint32_t ntiles, uint32_t NC,
                       uint32_t nb, uint32_t* gsum, unsigned long long* bin_start, hipStream_t s,
                       uint32_t G = TM_G);

// Digits of the partition passes of the rank gathers (launch_part_gather): the first pass
// (by y) cuts the ids into 1024 ranges (256 KB rank slices for the second pass's gathers), the
// second (by x) into 256 (1 MB slices for the edge pass's: 1024 x digits made the edge pass
// 8.2 -> 7.7 ms but the second pass 5.6 -> 8.0 ms, its 8K-record tiles then writing 64-B
// runs).  part_ws layout (PART_WS_WORDS u32): y-digit counts [0, 1024), (unused to 1280), u64
// cursors from word 1280; the x-digit counts are spread at PW_XH (below).
static constexpr uint32_t PD_X = 256, PW_CUR = 1280;  // (PD_Y = 1024; words 1024-1279: unused)
// ...then the u32 region starts of both passes' outputs, the second pass's u64 cursors (the
// first pass's stay: they are its regions' fill) and the first pass's capacity region ends.
static constexpr uint32_t PW_YST = 1280 + 2 * 1024, PW_XST = PW_YST + PD_Y + 1;
static constexpr uint32_t PW_XCUR = PW_XST + PD_X + 1, PW_YCAP = PW_XCUR + 2 * PD_X;
static_assert(PW_XCUR % 2 == 0 && PW_YCAP % 2 == 0, "u64 arrays");
// ...then the fused front pass's y subregions (k_front_fused, FF_GMAX tile groups at most): u64
// starts (FS_MAX + 1), cursors and ends (FS_MAX each), and the u32 first tile of each subregion
// in the second pass's tile map (FS_MAX + 1; k_fs_tile_scan).
static constexpr uint32_t PW_FST = PW_YCAP + 2 * PD_Y, PW_FCUR = PW_FST + 2 * (FS_MAX + 2),
                          PW_FCAP = PW_FCUR + (uint32_t)fs_cur_words(FS_MAX),
                          PW_FTOFF = PW_FCAP + 2 * FS_MAX;
static_assert(PW_FST % 2 == 0 && PW_FCUR % 2 == 0 && PW_FCAP % 2 == 0, "u64 arrays");
// ...and the x-digit counts, spread (xh_ix, sheep_internal.h): word PW_XH.  (Words 1024-1279,
// where they used to be, stay unused.)
static constexpr uint32_t PW_XH = (PW_FTOFF + FS_MAX + 1 + 1) & ~1u;
static_assert(PW_XH + XH_WORDS <= PART_WS_WORDS, "part_ws holds the fused pass's tables");
// Second-pass records (x, ry): ry's sentinels.
constexpr uint32_t RY_SELF = 0xFFFFFFFDu;  // the record is a self-loop
constexpr uint32_t RY_OUT = 0xFFFFFFFEu;   // y >= n_rank (outside the rank table)
template <uint32_t ND>
__device__ __forceinline__ uint32_t part_digit(uint32_t id, int sh) { return min(id >> sh, ND - 1); }
static int part_shift(uint32_t n_rank, uint32_t nd) {  // id >> shift < nd for ids < n_rank
  int bits = 0, db = 0;
  for (uint64_t v = n_rank ? n_rank - 1 : 0; v; v >>= 1) ++bits;
  for (uint32_t v = nd - 1; v; v >>= 1) ++db;
  return bits > db ? bits - db : 0;
}

// ---- packed 6-byte records (P6) ------------------------------------------------------------
// Inside one digit region of the second partition pass's output the x digit's bits are
// implied, so with every id below n_rank <= 2^26 a record (x, ry) needs 43-45 bits: shx <= 18
// low bits of x and ry:  a = ry' << XH | x_lo >> 16,  b = x_lo & 0xFFFF,  XH = shx - 16, with
// ry' = ry, or a sentinel (RY_SELF / RY_OUT / INV) folded into the top of its 32 - XH bits.
// A buffer of m records holds the u32 array a (4m bytes) then the u16 array b (2m bytes): the
// second pass writes and the edge pass reads 6 bytes per record instead of 8.  The edge pass
// takes the digit from its tile (k_xd_tile_desc over the region starts of k_part_cursor; the
// descriptors live in the spare 2 B per record behind the two arrays).  Only for
// callers where an id >= n_rank fails the call anyway (graph2tree_dev, the multi-rank driver:
// the degree pass raises ERR_RANGE): such an id loses its high bits here.
struct P6Ref {
  const uint32_t* a;
  const uint16_t* b;
};
__device__ __forceinline__ P6Ref p6_in(const void* base, uint64_t m) {
  return {(const uint32_t*)base, (const uint16_t*)((const char*)base + 4 * m)};
}
__device__ __forceinline__ uint32_t p6_ry_enc(uint32_t ry, int xh) {
  return ry >= RY_SELF ? ry & (~0u >> xh) : ry;  // sentinels to the top 3 values of 32 - xh bits
}
__device__ __forceinline__ uint32_t p6_ry_dec(uint32_t v, int xh) {
  const uint32_t lim = (~0u >> xh) - 2u;
  return v >= lim ? v | ~(~0u >> xh) : v;
}

// The digit of input position pos: the last region (of ND) whose start is <= pos (empty
// regions share their start with the next one).  One full wave, two dependent loads: lane i
// tests region i * (ND / 64), then lane i the i-th region of the segment found.
template <uint32_t ND>
__device__ __forceinline__ uint32_t wave_find_digit(const uint32_t* __restrict__ starts, uint64_t pos) {
  constexpr uint32_t STEP = ND / 64;
  const uint32_t lane = threadIdx.x & 63;
  const bool ok1 = starts[lane * STEP] <= pos;
  const uint64_t b1 = __ballot(ok1);
  const uint32_t seg = 63 - __clzll((long long)(b1 | 1ull)) ;
  const uint32_t i2 = seg * STEP + (lane < STEP ? lane : 0u);  // (in bounds for every lane)
  const bool ok2 = lane < STEP && starts[i2] <= pos;
  const uint64_t b2 = __ballot(ok2) | 1ull;
  return seg * STEP + (63 - __clzll((long long)b2));
}

// A tile's regions [d0, d1] (the digits of its first and last input positions) in LDS: sst[0] =
// d0, sst[1] = d1, sst[2 ..] = starts[d0 + 1 .. d1].  Called by every thread; ends in a barrier.
template <uint32_t ND>
__device__ __forceinline__ void tile_regions(const uint32_t* __restrict__ starts, uint64_t tb,
                                             uint32_t tn, uint32_t* sst) {
  if (threadIdx.x < 64) {
    const uint32_t d0 = wave_find_digit<ND>(starts, tb);
    const uint32_t d1 = wave_find_digit<ND>(starts, tb + tn - 1);
    if (threadIdx.x == 0) { sst[0] = d0; sst[1] = d1; }
  }
  block_sync();
  const uint32_t d0 = sst[0], d1 = sst[1];
  for (uint32_t i = threadIdx.x; i < d1 - d0; i += blockDim.x) sst[2 + i] = starts[d0 + 1 + i];
  block_sync();
}
// The digit of position pos of the tile (tile_regions above).
__device__ __forceinline__ uint32_t tile_digit(const uint32_t* sst, uint64_t pos) {
  uint32_t d = sst[0];
  const uint32_t n = sst[1] - d;
  if (n == 0) return d;
  uint32_t lo = 0, cnt = n;  // entries sst[2 .. 2 + n) <= pos
  while (cnt > 0) {
    const uint32_t h = cnt >> 1;
    if (sst[2 + lo + h] <= pos) { lo += h + 1; cnt -= h + 1; } else cnt = h;
  }
  return d + lo;
}

__global__ void __launch_bounds__(DEGB_THREADS)
k_degb_count(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
             uint32_t NB, uint32_t* __restrict__ counts /* tile-major: [chunk][bucket] */,
             uint32_t* err, int psh, uint32_t* __restrict__ yhist) {
  __shared__ uint32_t hist[DEGB_NB];
  __shared__ uint32_t yh[PD_Y];  // y digits of the later rank-gather partition (nullable yhist)
  for (uint32_t i = threadIdx.x; i < NB; i += blockDim.x) hist[i] = 0;
  for (uint32_t i = threadIdx.x; i < PD_Y; i += blockDim.x) yh[i] = 0;
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * DEGB_CHUNK;
  const uint32_t cn = (uint32_t)min((uint64_t)DEGB_CHUNK, m - base);
  constexpr int U = 8;  // records loaded per thread before use (bytes in flight)
  for (int r = 0; r < DEGB_CHUNK / (DEGB_THREADS * U); ++r) {
    uint2 e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + threadIdx.x;
      e[u] = i < cn ? uv[base + i] : make_uint2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + threadIdx.x;
      if (i >= cn) continue;
      if (e[u].x >= n_ids || e[u].y >= n_ids) { atomicOr(err, ERR_RANGE); continue; }
      atomicAdd(&hist[e[u].x >> SH], 1u);
      if (file_mode || e[u].x != e[u].y) atomicAdd(&hist[e[u].y >> SH], 1u);
      if (yhist) atomicAdd(&yh[part_digit<PD_Y>(e[u].y, psh)], 1u);
    }
  }
  block_sync();
  if (yhist)
    for (uint32_t i = threadIdx.x; i < PD_Y; i += blockDim.x)
      if (yh[i]) atomicAdd(&yhist[i], yh[i]);
  for (uint32_t i = threadIdx.x; i < NB; i += blockDim.x)
    counts[(uint64_t)blockIdx.x * NB + i] = hist[i];
}

__global__ void __launch_bounds__(DEGB_THREADS)
k_degb_scatter(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
               uint32_t NB, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
               uint16_t* __restrict__ ep, uint32_t* __restrict__ selfc) {
  __shared__ uint32_t cur[DEGB_NB], start[DEGB_NB], goff[DEGB_NB], wsum[DEGB_THREADS / 64];
  __shared__ uint16_t buf[2 * DEGB_CHUNK];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t lmask = (1u << SH) - 1u;
  // this chunk's bucket counts and global run offsets (one scattered read per thread)
  uint32_t cnt = 0;
  if (t < (int)NB) {
    const uint64_t at = (uint64_t)blockIdx.x * NB + t;
    cnt = counts[at];
    goff[t] = offsets[at];
  }
  uint32_t incl = wave_incl_scan(cnt);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  if (t < (int)NB) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    start[t] = add + incl - cnt;
    cur[t] = add + incl - cnt;
  }
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * DEGB_CHUNK;
  const uint32_t cn = (uint32_t)min((uint64_t)DEGB_CHUNK, m - base);
  constexpr int U = 8;
  for (int r = 0; r < DEGB_CHUNK / (DEGB_THREADS * U); ++r) {
    uint2 ee[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + t;
      ee[u] = i < cn ? uv[base + i] : make_uint2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + t;
      uint2 e = ee[u];
      if (i >= cn || e.x >= n_ids || e.y >= n_ids) continue;
      bool loop = e.x == e.y;
      buf[atomicAdd(&cur[e.x >> SH], 1u)] = (uint16_t)(e.x & lmask);
      if (file_mode || !loop) buf[atomicAdd(&cur[e.y >> SH], 1u)] = (uint16_t)(e.y & lmask);
      if (loop && selfc) atomicAdd(&selfc[e.x], 1u);
    }
  }
  block_sync();
  // each wave writes whole bucket runs
  for (uint32_t b = w; b < NB; b += DEGB_THREADS / 64) {
    uint32_t s0 = start[b], n = cur[b] - s0;
    uint64_t g = goff[b];
    for (uint32_t j = lane; j < n; j += 64) ep[g + j] = buf[s0 + j];
  }
}

// ---- sampled capacities (large inputs): no counting read of the records ------------------
// The degree scatter and the first partition pass above need, before they write, where each
// bucket's (y digit's) runs go: k_degb_count reads every record once for that (8 B per record,
// 1.6 ms at RMAT-26, on the critical path: both chains wait for it).  Instead, every FS_STRIDE-th
// record is counted (k_front_sample: 1/FS_STRIDE of the records), and each bucket / digit gets
// a capacity region of its estimate plus six standard deviations of it plus a margin
// (k_front_caps).  The scatter counts its chunk in LDS and reserves its runs with one atomic per
// bucket (k_degb_scatter_cap); the histogram reads each region up to its fill; the partition
// pass reserves on the digit cursors (k_part, cap_end).  A run that would cross its region's
// end is dropped and a flag set: the caller then runs the exact (counted) pass instead.  The
// regions and the fill are all the readers see, so any capacities give the same degrees.

// FF_G (k_front_fused): the groups of tiles whose runs of one region go to a subregion of
// their own (group = tile % G; see k_front_fused).  The sample counts each group's records
// apart: block b samples group b % G only (gridDim a multiple of G), sample k lies in sample
// tile k / SPT (SPT samples per fused tile), so group g's samples are those of tiles g, g + G, ...
// scnt: G x NB bucket counts, then G x PD_Y digit counts.  G = 1: every FS_STRIDE-th record.
__global__ void __launch_bounds__(DEGB_THREADS)
k_front_sample(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
               uint32_t NB, int psh, uint32_t* __restrict__ scnt /* G x NB, then G x PD_Y */,
               int xonly /* the fused pass: x endpoints only in the buckets */, uint32_t G,
               uint32_t SPT) {
  __shared__ uint32_t hb[DEGB_NB], hy[PD_Y];
  for (uint32_t i = threadIdx.x; i < DEGB_NB; i += DEGB_THREADS) { hb[i] = 0; hy[i] = 0; }
  block_sync();
  const uint32_t g = blockIdx.x % G, bi = blockIdx.x / G, nbg = gridDim.x / G;
  const uint64_t ns = (m + FS_STRIDE - 1) / FS_STRIDE;
  const uint64_t ntl = (ns + SPT - 1) / SPT;                // sample tiles
  const uint64_t nq = (ntl + G - 1 - g) / G * SPT;          // ... of group g, as samples
  for (uint64_t q = (uint64_t)bi * DEGB_THREADS + threadIdx.x; q < nq;
       q += (uint64_t)nbg * DEGB_THREADS) {
    const uint64_t k = ((q / SPT) * G + g) * SPT + q % SPT;
    if (k >= ns) continue;
    const uint2 e = uv[k * FS_STRIDE];
    if (e.x >= n_ids || e.y >= n_ids) continue;  // the scatter reports it
    if (!xonly) atomicAdd(&hb[e.x >> SH], 1u);
    if (file_mode || e.x != e.y) atomicAdd(&hb[(xonly ? e.x : e.y) >> SH], 1u);
    atomicAdd(&hy[part_digit<PD_Y>(e.y, psh)], 1u);
  }
  block_sync();
  for (uint32_t i = threadIdx.x; i < NB; i += DEGB_THREADS)
    if (hb[i]) atomicAdd(&scnt[g * DEGB_NB + i], hb[i]);
  for (uint32_t i = threadIdx.x; i < PD_Y; i += DEGB_THREADS)
    if (hy[i]) atomicAdd(&scnt[G * DEGB_NB + g * PD_Y + i], hy[i]);
}

// Capacity of a region estimated at est items from c samples (est = c * FS_STRIDE): est + 5
// sigma (sigma = sqrt(FS_STRIDE * est), the sampling error) + 2048, at most lim.  A region
// outgrows it with probability ~3e-7 on an unordered stream.  Over n regions the capacities
// sum to at most E + 5 sqrt(FS_STRIDE n E) + 2048 n (Cauchy-Schwarz), E = the sampled total
// <= 2 (m + FS_STRIDE) endpoints or m + FS_STRIDE records: fs_room (front_layout.h) sizes the
// buffers by it.
__device__ __forceinline__ unsigned long long fs_cap(uint32_t c, unsigned long long lim) {
  const double est = (double)c * FS_STRIDE;
  const double cap = est + 5.0 * sqrt((double)FS_STRIDE * est) + 2048.0;
  return cap < (double)lim ? (unsigned long long)cap : lim;
}

// One block of 1024 threads: bucket regions (bst: NB + 1 starts, bcur: cursors = starts, bcap:
// region ends) within ep_slots u16 entries, and the y-digit regions (ystart: PD_Y + 1 u32,
// ycur: cursors, ycap: ends) within mid_slots records.  Regions that do not fit get capacity 0
// (every run then overflows: the caller's exact pass takes over).
// G > 1 (k_front_fused's tile groups): each region is G subregions s = region * G + group,
// adjacent in memory, each sized from its group's own samples; every table above is then per
// subregion (NB * G + 1 starts), and ystart (u32) is not written (nullable).
__global__ void __launch_bounds__(1024)
k_front_caps(const uint32_t* __restrict__ scnt, uint32_t NB, uint64_t m, uint64_t ep_slots,
             uint64_t mid_slots, unsigned long long* bst, unsigned long long* bcur,
             unsigned long long* bcap, uint32_t* ystart, unsigned long long* ycur,
             unsigned long long* ycap, unsigned long long* ys64 /* nullable: ystart as u64 */,
             uint32_t G, int spread /* cursors at fs_cix(q) (k_front_fused), else at q */) {
  __shared__ unsigned long long ws[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int pass = 0; pass < 2; ++pass) {
    const uint32_t n = pass ? PD_Y : NB;
    const unsigned long long lim = pass ? m : 2 * m, room = pass ? mid_slots : ep_slots;
    const uint32_t* sc = scnt + (pass ? G * DEGB_NB : 0);
    unsigned long long cg[8], c = 0;  // (G <= 8)
#pragma unroll
    for (uint32_t g = 0; g < 8; ++g) {
      cg[g] = ((uint32_t)t < n && g < G) ? fs_cap(sc[g * (pass ? PD_Y : DEGB_NB) + t], lim) : 0ull;
      c += cg[g];
    }
    unsigned long long incl = c;  // inclusive wave scan (u64)
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) ws[w] = incl;
    block_sync();
    unsigned long long add = 0, total = 0;
    for (int i = 0; i < 16; ++i) { if (i < w) add += ws[i]; total += ws[i]; }
    const bool fits = total <= room;
    unsigned long long st = fits ? add + incl - c : 0ull;
    if ((uint32_t)t < n) {
      for (uint32_t g = 0; g < G; ++g) {
        const unsigned long long end = fits ? st + cg[g] : 0ull;
        const uint32_t q = t * G + g;
        if (pass) {
          if (ystart) ystart[q] = (uint32_t)st;
          if (ys64) ys64[q] = st;
          ycur[spread ? fs_cix(q) : q] = st;
          ycap[q] = end;
        } else {
          bst[q] = st;
          bcur[spread ? fs_cix(q) : q] = st;
          bcap[q] = end;
        }
        st = end;
      }
    }
    if (t == 0) {
      if (pass) {
        if (ystart) ystart[n * G] = (uint32_t)(fits ? total : 0ull);
        if (ys64) ys64[n * G] = fits ? total : 0ull;
      }
      else bst[n * G] = fits ? total : 0ull;
    }
    block_sync();
  }
}

// k_degb_scatter on capacity regions: the chunk's bucket counts from LDS, its runs reserved on
// the bucket cursors (bcur), dropped past the region end (bcap) with *ovf set.
__global__ void __launch_bounds__(DEGB_THREADS)
k_degb_scatter_cap(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
                   uint32_t NB, unsigned long long* bcur, const unsigned long long* __restrict__ bcap,
                   uint16_t* __restrict__ ep, uint32_t* __restrict__ selfc, uint32_t* ovf,
                   uint32_t* err) {
  __shared__ uint32_t cur[DEGB_NB], start[DEGB_NB], wsum[DEGB_THREADS / 64];
  __shared__ unsigned long long goff[DEGB_NB];
  __shared__ uint16_t buf[2 * DEGB_CHUNK];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t lmask = (1u << SH) - 1u;
  constexpr int U = 8, RND = DEGB_CHUNK / (DEGB_THREADS * U);
  for (uint32_t i = t; i < DEGB_NB; i += DEGB_THREADS) cur[i] = 0;
  const uint64_t base = (uint64_t)blockIdx.x * DEGB_CHUNK;
  const uint32_t cn = (uint32_t)min((uint64_t)DEGB_CHUNK, m - base);
  uint2 ee[RND * U];  // the chunk stays in registers between the count and the placement
#pragma unroll
  for (int q = 0; q < RND * U; ++q) {
    const uint32_t i = (uint32_t)q * DEGB_THREADS + t;
    ee[q] = i < cn ? ld_rec_nt(uv + base + i) : make_uint2(INV, INV);
  }
  block_sync();
#pragma unroll
  for (int q = 0; q < RND * U; ++q) {
    const uint2 e = ee[q];
    if (e.x >= n_ids || e.y >= n_ids) {
      if ((uint32_t)q * DEGB_THREADS + t < cn) atomicOr(err, ERR_RANGE);
      continue;
    }
    atomicAdd(&cur[e.x >> SH], 1u);
    if (file_mode || e.x != e.y) atomicAdd(&cur[e.y >> SH], 1u);
  }
  block_sync();
  const uint32_t cnt = (uint32_t)t < NB ? cur[t] : 0u;
  const uint32_t incl = wave_incl_scan(cnt);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  if ((uint32_t)t < NB) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    start[t] = add + incl - cnt;
    cur[t] = add + incl - cnt;
    unsigned long long g = ~0ull;
    if (cnt) {
      g = atomicAdd(&bcur[t], (unsigned long long)cnt);
      if (g + cnt > bcap[t]) {
        atomicOr(ovf, 1u);
        g = ~0ull;
      }
    }
    goff[t] = g;
  }
  block_sync();
#pragma unroll
  for (int q = 0; q < RND * U; ++q) {
    const uint2 e = ee[q];
    if (e.x >= n_ids || e.y >= n_ids) continue;
    const bool loop = e.x == e.y;
    buf[atomicAdd(&cur[e.x >> SH], 1u)] = (uint16_t)(e.x & lmask);
    if (file_mode || !loop) buf[atomicAdd(&cur[e.y >> SH], 1u)] = (uint16_t)(e.y & lmask);
    if (loop && selfc) atomicAdd(&selfc[e.x], 1u);
  }
  block_sync();
  for (uint32_t b = w; b < NB; b += DEGB_THREADS / 64) {
    const unsigned long long g = goff[b];
    if (g == ~0ull) continue;
    const uint32_t s0 = start[b], n = cur[b] - s0;
    for (uint32_t j = lane; j < n; j += 64) ep[g + j] = buf[s0 + j];
  }
}

// The fused front pass (graph2tree_dev, part_overlap 4): ONE read of the records does the
// degree scatter's x half and the first partition pass, into the sampled capacity regions of
// k_front_caps:
//   the records go out grouped by y digit, packed (P6F): x as a u32 array oa, y's low bits
//     (y - digit << SH, < 2^16) as a u16 array ob, both indexed by the record's position;
//   the x endpoints (LLAMA: x != y only, a self-loop counts once) go out as u16 by x bucket.
// The histogram then counts y from ob and x from ep (SH == the y-digit shift: the buckets ARE
// the y digits), and k_part<1> reads (oa, ob) and restores y's digit from the region starts.
// Bytes per record: 8 read + 4 + 2 (records) + 2 (x endpoint) written, against 8 + 4 (degree
// scatter) and 8 + 8 (first pass) before; the histogram reads the same 4.
// Tile: FF_NT x FF_IT records.  LDS: the tile staged twice 64 KB (x; digit << 16 | y_lo), the x
// endpoints restaged into the first half, and the run tables of both sorts.
static constexpr int FF_NT = 1024, FF_IT = 16;
// Tile groups (G = FF_G, round 6): every region is G adjacent subregions, and tile t reserves its
// runs in subregion t % G.  With gridDim a multiple of G, block b's tiles all belong to group
// b % G, and blocks b, b + 8, ... share an XCD (round-robin dispatch: for speed only, correctness
// never depends on it).  So consecutive runs of a subregion come from one XCD and meet in its L2,
// which writes whole lines instead of each XCD writing its own partial lines of a 32-64 B run
// (the pass wrote 14.9 GB for its 8.6 GB: profiles/r05/ev6/pmc_table.md).
// Persistent: gridDim blocks (one per CU) walk the tiles blockIdx.x, + gridDim.x, ...  The x runs are
// staged and written first, then the y runs staged; the next tile's records are loaded right
// after that (the last use of this tile's records in registers) so that their HBM latency
// overlaps the y write-out instead of opening the next tile with an idle CU (one block per CU:
// the two 64 KB stages fill the LDS).  No uncounted wait lies between the loads and their use:
// the y write-out holds stores only, and the barriers wait for LDS operations alone.  (RMAT-26
// 8.04 -> 7.79 ms on one box, profiles/r05/q_fused_pipe_et/; the capacity check of the y runs
// moved from a global load per record of the write-out to an LDS table, yfit.)
__global__ void __launch_bounds__(FF_NT)
k_front_fused(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
              uint32_t NB, uint32_t* __restrict__ oa, uint16_t* __restrict__ ob,
              unsigned long long* ycur, const unsigned long long* __restrict__ ycap,
              unsigned long long* bcur, const unsigned long long* __restrict__ bcap,
              uint16_t* __restrict__ ep, uint32_t* __restrict__ selfc, uint32_t* ovf_y,
              uint32_t* ovf_x, uint32_t* err, uint32_t* __restrict__ xhist, int shx,
              int xdd /* shx == SH + 2: the x digits come from the x runs */, uint32_t G) {
  constexpr int TILE = FF_NT * FF_IT;
  __shared__ uint32_t sa[TILE], sb[TILE];
  __shared__ uint32_t ty[DEGB_NB + 1], tx[DEGB_NB + 1], hxd[PD_X], wsum[2 * (FF_NT / 64)];
  __shared__ unsigned long long gy[DEGB_NB], gx[DEGB_NB];
  __shared__ uint32_t yfit[DEGB_NB];  // the part of a y run that fits its capacity region
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t lmask = (1u << SH) - 1u;
  const uint64_t ntiles = (m + TILE - 1) / TILE;
  uint2 e[FF_IT];
  auto load = [&](uint64_t tile) {  // unpredicated (clamped to the tile's last record)
    const uint2* p = uv + tile * TILE;
    const uint32_t last = (uint32_t)min((uint64_t)TILE, m - tile * TILE) - 1u;
    uint32_t o = t;
    asm volatile("" : "+v"(o));  // (keeps the 16 offsets from being hoisted out of the tile loop)
#pragma unroll
    for (int k = 0; k < FF_IT; ++k) e[k] = ld_rec_nt(p + min((uint32_t)k * FF_NT + o, last));
  };
  uint64_t tile = blockIdx.x;
  load(tile);
  for (; tile < ntiles; tile += gridDim.x) {
  const uint32_t grp = (uint32_t)(tile % G);  // this tile's subregion of every region
  for (uint32_t i = t; i < DEGB_NB; i += FF_NT) { ty[i] = 0; tx[i] = 0; }
  for (uint32_t i = t; i < PD_X; i += FF_NT) hxd[i] = 0;
  const uint64_t base = tile * TILE;
  const uint32_t cn = (uint32_t)min((uint64_t)TILE, m - base);
  // the records have arrived (one wait here: the compiler then counts none of the loads as
  // pending behind the x write-out's stores, which a later wait would otherwise drain)
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  block_sync();
  uint32_t ly[FF_IT], lx[FF_IT];  // rank within the tile's y run / x run (INV: none)
#pragma unroll
  for (int k = 0; k < FF_IT; ++k) {
    ly[k] = INV;
    lx[k] = INV;
    const uint2 r = e[k];
    if ((uint32_t)k * FF_NT + t >= cn) continue;
    if (r.x >= n_ids || r.y >= n_ids) {
      atomicOr(err, ERR_RANGE);
      continue;
    }
    ly[k] = atomicAdd(&ty[r.y >> SH], 1u);
    const bool loop = r.x == r.y;
    if (file_mode || !loop) lx[k] = atomicAdd(&tx[r.x >> SH], 1u);
    if (loop && selfc) atomicAdd(&selfc[r.x], 1u);
    // x digits of k_part<1> (shx == SH + 2: 4 x buckets per digit, taken from the x runs
    // below; only the records no x run holds are counted here)
    if (!xdd || lx[k] == INV) atomicAdd(&hxd[part_digit<PD_X>(r.x, shx)], 1u);
  }
  block_sync();
  // both run tables: exclusive starts in the tile, and the global runs (capacity regions: a y
  // run keeps the part that fits; an x run that does not fit is dropped — either sets its flag)
  {
    const uint32_t c1 = (uint32_t)t < NB ? ty[t] : 0u, c2 = (uint32_t)t < NB ? tx[t] : 0u;
    if (xdd && c2) atomicAdd(&hxd[t >> 2], c2);
    const uint32_t i1 = wave_incl_scan(c1), i2 = wave_incl_scan(c2);
    if (lane == 63) { wsum[w] = i1; wsum[FF_NT / 64 + w] = i2; }
    unsigned long long g1 = 0, g2 = ~0ull;
    if ((uint32_t)t < NB) {
      const uint32_t q = t * G + grp;  // region t's subregion of this tile's group
      uint32_t fit = 0;
      if (c1) {
        g1 = atomicAdd(&ycur[fs_cix(q)], (unsigned long long)c1);
        const unsigned long long cap = ycap[q];
        fit = g1 + c1 <= cap ? c1 : g1 < cap ? (uint32_t)(cap - g1) : 0u;
        if (fit < c1) atomicOr(ovf_y, 1u);
      }
      yfit[t] = fit;
      if (c2) {
        g2 = atomicAdd(&bcur[fs_cix(q)], (unsigned long long)c2);
        if (g2 + c2 > bcap[q]) {
          atomicOr(ovf_x, 1u);
          g2 = ~0ull;
        }
      }
      gy[t] = g1;
      gx[t] = g2;
    }
    block_sync();
    uint32_t a1 = 0, a2 = 0;
    for (int i = 0; i < w; ++i) { a1 += wsum[i]; a2 += wsum[FF_NT / 64 + i]; }
    if ((uint32_t)t < NB) { ty[t] = a1 + i1 - c1; tx[t] = a2 + i2 - c2; }
    if (t == FF_NT - 1) {
      uint32_t s1 = 0, s2 = 0;
      for (int i = 0; i < FF_NT / 64; ++i) { s1 += wsum[i]; s2 += wsum[FF_NT / 64 + i]; }
      ty[NB] = s1;
      tx[NB] = s2;
    }
  }
  for (uint32_t i = t; i < PD_X; i += FF_NT)
    if (hxd[i]) atomicAdd(&xhist[xh_ix(i)], hxd[i]);
  block_sync();
#pragma unroll
  for (int k = 0; k < FF_IT; ++k)
    if (lx[k] != INV) {
      const uint32_t b = e[k].x >> SH;
      sa[tx[b] + lx[k]] = (b << 16) | (e[k].x & lmask);
    }
  block_sync();
  const uint32_t nx = tx[NB];
  for (uint32_t j = t; j < nx; j += FF_NT) {
    const uint32_t v = sa[j], b = v >> 16;
    const unsigned long long g = gx[b];
    if (g != ~0ull) ep[g + (j - tx[b])] = (uint16_t)(v & 0xFFFFu);
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < FF_IT; ++k)
    if (ly[k] != INV) {
      const uint32_t d = e[k].y >> SH, j = ty[d] + ly[k];
      sa[j] = e[k].x;
      sb[j] = (d << 16) | (e[k].y & lmask);
    }
  load(min(tile + gridDim.x, ntiles - 1));  // (past the last tile: re-read, unused)
  block_sync();
  const uint32_t ny = ty[NB];
  for (uint32_t j = t; j < ny; j += FF_NT) {  // flat: every lane busy
    const uint32_t v = sb[j], d = v >> 16;
    const uint32_t i = j - ty[d];
    if (i < yfit[d]) {
      const unsigned long long pos = gy[d] + i;
      oa[pos] = sa[j];
      ob[pos] = (uint16_t)(v & 0xFFFFu);
    }
  }
  block_sync();  // (the tables and stages are reset / rewritten by the next tile)
  }
}

__global__ void __launch_bounds__(DEGB_THREADS, 8)  // (8 waves per SIMD, two blocks per CU: <= 64 VGPRs)
k_degb_hist(const uint16_t* __restrict__ ep, int SH, uint32_t n_ids, uint32_t* __restrict__ deg,
            const unsigned long long* __restrict__ bstart, uint32_t* __restrict__ stats,
            const uint16_t* __restrict__ ep2, const unsigned long long* __restrict__ bstart2,
            const uint64_t* __restrict__ rec0,
            const unsigned long long* __restrict__ bend /* nullable: capacity regions' fill */,
            const unsigned long long* __restrict__ bend2 /* ... of ep2's regions */, uint32_t G,
            int spread /* bend / bend2 at fs_cix (k_front_fused's cursors) */) {
  // span words of dynamic LDS (degb_hist_lds): 16 KB for R-MAT-22's 4096-id buckets, where a
  // fixed 128 KB array held the CU to one block
  extern __shared__ uint32_t cnt[];
  const uint32_t b = blockIdx.x;
  const uint32_t span = 1u << SH;
  for (uint32_t i = threadIdx.x; i < span; i += blockDim.x) cnt[i] = 0;
  block_sync();
  const int lane = threadIdx.x & 63;
  // ep2 (nullable, bstart2): a second endpoint array (the fused front half's x ids)
  // G > 1: the bucket's entries lie in G subregions (k_front_fused's groups)
  for (uint32_t sq = 0; sq < (ep2 ? 2u : 1u) * G; ++sq) {
  const int sg = (int)(sq / G);
  const uint32_t bq = b * G + sq % G;  // the bucket's subregion (G = 1: the bucket)
  const uint16_t* __restrict__ ep_s = sg ? ep2 : ep;
  // bucket (subregion) starts, then the total
  uint64_t s0 = sg ? bstart2[bq] : bstart[bq];
  uint64_t s1 = sg ? bstart2[bq + 1] : bstart[bq + 1];
  const uint32_t cq = spread ? fs_cix(bq) : bq;
  if (bend && sg == 0) s1 = min(s1, (uint64_t)bend[cq]);  // (a region's fill past its end: dropped)
  if (bend2 && sg == 1) s1 = min(s1, (uint64_t)bend2[cq]);
  if (sg == 0 && rec0) {  // the fused front half's records (x, y) of y bucket b: y's id
    const uint32_t lm = (1u << SH) - 1u;
    for (uint64_t i0 = s0; i0 < s1; i0 += 8 * DEGB_THREADS) {
      uint2 q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint64_t i = i0 + (uint64_t)u * DEGB_THREADS + threadIdx.x;
        q[u] = i < s1 ? ld_rec_nt((const uint2*)rec0 + i) : make_uint2(0, INV);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (q[u].y != INV) atomicAdd(&cnt[q[u].y & lm], 1u);
    }
    continue;
  }
  // 32 entries (four 16-B loads, all issued before use: the loop is latency-bound otherwise)
  // per thread per iteration, from the 8-aligned entry below s0 (ep is padded: the loads may
  // run up to 7 entries past the end)
  // The next iteration's loads are issued before this one's entries are counted (registers
  // double-buffered; clamped to the last 8-entry group, used only below s1).
  constexpr int V = 4;
  const uint64_t ilast = s1 > s0 ? (s1 - 1) & ~7ull : 0;
  uint4 nq[V];
  auto load_it = [&](uint64_t i0) {
    uint32_t tt = threadIdx.x;
    asm volatile("" : "+v"(tt));  // (not hoisted: registers for two blocks per CU)
#pragma unroll
    for (int u = 0; u < V; ++u)
      nq[u] = *(const uint4*)(ep_s + min(i0 + 8 * ((uint64_t)u * DEGB_THREADS + tt), ilast));
  };
  if (s0 < s1) load_it(s0 & ~7ull);
  for (uint64_t i0 = s0 & ~7ull; i0 < s1; i0 += 8 * V * DEGB_THREADS) {
    uint4 q[V];
#pragma unroll
    for (int u = 0; u < V; ++u) q[u] = nq[u];
    if (i0 + 8 * V * DEGB_THREADS < s1) load_it(i0 + 8 * V * DEGB_THREADS);
#pragma unroll
    for (int u = 0; u < V; ++u) {
      uint64_t i = i0 + 8 * ((uint64_t)u * DEGB_THREADS + threadIdx.x);
      uint32_t wv[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint64_t ik = i + k;
        uint32_t e = (wv[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        bool done = !(ik >= s0 && ik < s1);
        // (masked: a capacity region's unwritten hole, read only on the way to the exact pass)
        uint32_t v = e & (span - 1);
        // one round of leader matching folds a hub's repeated id into one LDS add
        uint64_t act = __ballot(!done);
        if (act) {
          int leader = __ffsll((unsigned long long)act) - 1;
          uint32_t lv = __builtin_amdgcn_readlane(v, leader);
          uint64_t same = __ballot(!done && v == lv);
          if (lane == leader) atomicAdd(&cnt[lv], (uint32_t)__popcll(same));
          if ((same >> lane) & 1) done = true;
          if (!done) atomicAdd(&cnt[v], 1u);
        }
      }
    }
  }
  }  // segments
  block_sync();
  uint64_t g0 = (uint64_t)b << SH;
  uint32_t mx = 0, zeros = 0, big = 0;
  for (uint32_t i = threadIdx.x; i < span; i += blockDim.x)
    if (g0 + i < n_ids) {
      const uint32_t d = cnt[i];
      deg[g0 + i] = d;
      mx = max(mx, d);
      zeros += d == 0;
      big += d >= SEQ_BIG;
    }
  if (stats) deg_stats_flush(stats, mx, zeros, big);
}

// Dynamic LDS of k_degb_hist: its counters, one word per id of a bucket.
static size_t degb_hist_lds(int SH) { return (size_t)(1u << SH) * 4; }

// Buckets of 65536 ids (n_ids > 2^25): one workgroup per bucket (u32 counters for them all
// would not fit the LDS: k_degb_hist once ran two workgroups there, each reading the whole run
// for its half of the ids).  The
// 65536 counters are u16 halves of 32768 LDS words; the run is counted in segments of at most
// 65535 entries, so no half can carry into its neighbour, and after each segment every thread
// folds its 64 ids into u32 registers.
__global__ void __launch_bounds__(DEGB_THREADS)
k_degb_hist16(const uint16_t* __restrict__ ep, uint32_t n_ids, uint32_t* __restrict__ deg,
              const unsigned long long* __restrict__ bstart, uint32_t* __restrict__ stats,
              const uint16_t* __restrict__ ep2, const unsigned long long* __restrict__ bstart2,
              const uint64_t* __restrict__ rec0,
              const unsigned long long* __restrict__ bend /* nullable: capacity regions' fill */) {
  __shared__ uint32_t pk[32768];
  const uint32_t b = blockIdx.x;
  uint32_t acc[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) acc[k] = 0;
  constexpr int V = 4;
  // ep2 (nullable, bstart2): a second endpoint array (the fused front half's x ids)
  for (int sg = 0; sg < (ep2 ? 2 : 1); ++sg) {
  const uint16_t* __restrict__ ep_s = sg ? ep2 : ep;
  const uint64_t s0 = sg ? bstart2[b] : bstart[b];
  uint64_t s1 = sg ? bstart2[b + 1] : bstart[b + 1];
  if (bend && sg == 0) s1 = min(s1, (uint64_t)bend[b]);
  for (uint64_t g0 = s0; g0 < s1; g0 += 65535) {
    const uint64_t g1 = min(g0 + 65535, s1);
    for (uint32_t i = threadIdx.x; i < 32768; i += DEGB_THREADS) pk[i] = 0;
    block_sync();
    if (sg == 0 && rec0) {  // the fused front half's records (x, y) of y bucket b: y's id
      for (uint64_t i0 = g0; i0 < g1; i0 += 8 * DEGB_THREADS) {
        uint2 q[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const uint64_t i = i0 + (uint64_t)u * DEGB_THREADS + threadIdx.x;
          q[u] = i < g1 ? ld_rec_nt((const uint2*)rec0 + i) : make_uint2(0, INV);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (q[u].y != INV) {
            const uint32_t v = q[u].y & 0xFFFFu;
            atomicAdd(&pk[v >> 1], 1u << (16 * (v & 1)));
          }
      }
    } else
    for (uint64_t i0 = g0 & ~7ull; i0 < g1; i0 += 8 * V * DEGB_THREADS) {
      uint4 q[V];
#pragma unroll
      for (int u = 0; u < V; ++u) {
        uint64_t i = i0 + 8 * ((uint64_t)u * DEGB_THREADS + threadIdx.x);
        q[u] = i < g1 ? *(const uint4*)(ep_s + i) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < V; ++u) {
        uint64_t i = i0 + 8 * ((uint64_t)u * DEGB_THREADS + threadIdx.x);
        uint32_t wv[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          uint64_t ik = i + k;
          uint32_t v = (wv[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
          // no matching: repeated ids of a wave serialise in the LDS atomic unit
          if (ik >= g0 && ik < g1) atomicAdd(&pk[v >> 1], 1u << (16 * (v & 1)));
        }
      }
    }
    block_sync();
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const uint32_t id = (uint32_t)k * DEGB_THREADS + threadIdx.x;
      acc[k] += (pk[id >> 1] >> (16 * (id & 1))) & 0xFFFFu;
    }
    block_sync();
  }
  }  // segments
  const uint64_t base = (uint64_t)b << 16;
  uint32_t mx = 0, zeros = 0, big = 0;
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const uint64_t id = base + (uint64_t)k * DEGB_THREADS + threadIdx.x;
    if (id < n_ids) {
      deg[id] = acc[k];
      mx = max(mx, acc[k]);
      zeros += acc[k] == 0;
      big += acc[k] >= SEQ_BIG;
    }
  }
  if (stats) deg_stats_flush(stats, mx, zeros, big);
}

// k_degb_hist16 in slices (the fused front pass's histogram): bucket b's entries, x endpoints
// [xs[b], min(xs[b + 1], xf[b])) then y ids [ys[b], min(ys[b + 1], yf[b])), are cut into
// ceil(count / CH) slices of CH entries, one workgroup each (block i finds its bucket and slice
// from a block-wide scan of the slice counts; blocks past the last slice return).  A bucket of
// one slice stores its degrees; the slices of a split bucket add theirs to deg, which the
// caller zeroed.  One workgroup per bucket left the step waiting on the buckets of the hub ids
// and on the last round of buckets over the CUs.  Counting as k_degb_hist16 (u16 halves of
// 32768 LDS words, segments of at most 65535 entries, u32 totals in registers).
// REQUIRES the fused front pass's cursor layout: xf / yf are k_front_fused's region cursors,
// spread over memory (cursor q at u64 index fs_cix(q), sheep_internal.h), while xs / ys are
// plain arrays of region starts.  Cursors laid out contiguously (the sampled degree pass's) would
// be read at the wrong words: only launch_front_fused may launch these.
// Slices of bucket t (thread t of a 1024-thread block, t < NB) and the first slice's block
// index (an exclusive scan over the buckets; wsum: DEGB_THREADS / 64 words of LDS).
__device__ __forceinline__ void hist16s_slices(const unsigned long long* __restrict__ xs,
                                               const unsigned long long* __restrict__ xf,
                                               const unsigned long long* __restrict__ ys,
                                               const unsigned long long* __restrict__ yf,
                                               uint32_t NB, uint64_t CH, uint32_t* wsum,
                                               uint32_t& ns, uint32_t& p0, uint32_t G) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  ns = 0;
  if ((uint32_t)t < NB) {
    uint64_t n = 0;
    for (uint32_t q = t * G; q < (t + 1) * G; ++q) {  // the bucket's G subregions
      const unsigned long long xq = xf[fs_cix(q)], yq = yf[fs_cix(q)];
      n += min(xs[q + 1], xq) - min(xs[q], min(xs[q + 1], xq));
      n += min(ys[q + 1], yq) - min(ys[q], min(ys[q + 1], yq));
    }
    ns = (uint32_t)max((uint64_t)1, (n + CH - 1) / CH);
  }
  const uint32_t incl = wave_incl_scan(ns);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t add = 0;
  for (int i = 0; i < w; ++i) add += wsum[i];
  p0 = add + incl - ns;
}

// (Partial counts of a split bucket's later slices stored to a buffer and added by a second
// kernel, instead of the atomics here, measured no faster: RMAT-26 hist 2.00 -> 2.04 ms.)
__global__ void __launch_bounds__(DEGB_THREADS)
k_degb_hist16s(const uint16_t* __restrict__ ex, const unsigned long long* __restrict__ xs,
               const unsigned long long* __restrict__ xf, const uint16_t* __restrict__ ey,
               const unsigned long long* __restrict__ ys, const unsigned long long* __restrict__ yf,
               uint32_t NB, uint32_t n_ids, uint64_t CH, uint32_t* __restrict__ deg,
               uint32_t G /* subregions per bucket (k_front_fused's groups) */) {
  __shared__ uint32_t pk[32768];
  __shared__ uint32_t wsum[DEGB_THREADS / 64], s_b, s_s, s_n;
  const int t = threadIdx.x;
  // slice table: thread t = bucket t
  if (t == 0) s_b = INV;
  uint32_t ns, p0;
  hist16s_slices(xs, xf, ys, yf, NB, CH, wsum, ns, p0, G);
  if ((uint32_t)t < NB && blockIdx.x >= p0 && blockIdx.x < p0 + ns) {
    s_b = t;
    s_s = blockIdx.x - p0;
    s_n = ns;
  }
  block_sync();
  const uint32_t b = s_b;
  if (b == INV) return;  // (uniform: past the last slice)
  const uint32_t sl = s_s, nsl = s_n;
  // the slice [v0, v1) of the bucket's entries: its x subregions, then its y subregions, as one
  // sequence (vend: its length)
  uint64_t vend = 0;
  for (uint32_t q = b * G; q < (b + 1) * G; ++q)
    vend += (max(xs[q], min(xs[q + 1], xf[fs_cix(q)])) - xs[q]) +
            (max(ys[q], min(ys[q + 1], yf[fs_cix(q)])) - ys[q]);
  const uint64_t v0 = (uint64_t)sl * CH, v1 = min(v0 + CH, vend);
  // Rounds of RW = 65528 entries (8191 16-B loads: thread 1023 skips its eighth, so a round
  // counts at most 65528 < 65536 of one id into a u16 half) from the 8-aligned entry below the
  // segment's start, in two halves of four loads per thread.  The next round's first half is
  // loaded right after this round's counting, so that it is in flight during the fold (which
  // reads and clears each counter word once: ids 2w and 2w + 1 of word w) — the zeroing pass
  // and one barrier per round are gone too.  RMAT-26 histogram 2.03 -> 1.72 ms, twitter shape
  // 3.31 -> 2.84 ms (profiles/r05/t_hist_rounds/; 65535-entry segments with a zeroing pass, a
  // separate fold and the loads issued only inside the count before).
  constexpr uint64_t RW = 65528;
  uint32_t lo[32], hi[32];
#pragma unroll
  for (int k = 0; k < 32; ++k) { lo[k] = 0; hi[k] = 0; }
  for (uint32_t i = t; i < 32768; i += DEGB_THREADS) pk[i] = 0;
  block_sync();
  uint64_t off = 0;
  for (uint32_t sq = 0; sq < 2 * G; ++sq) {
    const int sg = (int)(sq / G);
    const uint32_t bq = b * G + sq % G;
    const unsigned long long* __restrict__ st = sg ? ys : xs;
    const unsigned long long* __restrict__ fl = sg ? yf : xf;
    const uint64_t z0 = st[bq], len = max(z0, min(st[bq + 1], fl[fs_cix(bq)])) - z0;
    const uint64_t a = min(max(v0, off), off + len) - off, e = min(max(v1, off), off + len) - off;
    off += len;
    if (a >= e) continue;  // (uniform)
    const uint16_t* __restrict__ src = sg ? ey : ex;
    const uint64_t s0 = z0 + a, s1 = z0 + e;
    const uint64_t A = s0 & ~7ull, last = (s1 - 1) & ~7ull;
    const uint64_t nr = (s1 - A + RW - 1) / RW;
    uint4 q[4];
    // (offsets within a round in u32, from the round's uniform base pointer; half h of a
    // round = loads u = 4h .. 4h + 3)
    auto load_half = [&](uint64_t r, int h) {  // unpredicated: clamped to the last 8-entry group
      const uint64_t rb = A + r * RW;
      const uint16_t* rp = src + rb;
      const uint32_t lim = (uint32_t)(last - rb);
      uint32_t tt = t;
      asm volatile("" : "+v"(tt));
#pragma unroll
      for (int u = 0; u < 4; ++u)
        q[u] = *(const uint4*)(rp + min(8u * ((uint32_t)(4 * h + u) * DEGB_THREADS + tt), lim));
    };
    auto count_half = [&](uint32_t r0, uint32_t r1, int h) {
      uint32_t tt = t;
      asm volatile("" : "+v"(tt));  // (keeps the 32 positions from being hoisted and spilled)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t i = 8u * ((uint32_t)(4 * h + u) * DEGB_THREADS + tt);
        const bool inr = h == 0 || u < 3 || t < DEGB_THREADS - 1;
        const uint32_t wv[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t ik = i + k;
          const uint32_t v = (wv[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
          if (inr && ik >= r0 && ik < r1) atomicAdd(&pk[v >> 1], 1u << (16 * (v & 1)));
        }
      }
    };
    load_half(0, 0);
    for (uint64_t r = 0; r < nr; ++r) {
      const uint64_t rb = A + r * RW;
      const uint32_t r0 = (uint32_t)(max(s0, rb) - rb), r1 = (uint32_t)(min(s1, rb + RW) - rb);
      count_half(r0, r1, 0);
      if (r1 > 32768) {  // (uniform)
        load_half(r, 1);
        count_half(r0, r1, 1);
      }
      if (r + 1 < nr) load_half(r + 1, 0);  // in flight during the fold
      block_sync();
#pragma unroll
      for (int k = 0; k < 32; ++k) {
        const uint32_t wd = (uint32_t)k * DEGB_THREADS + t;
        const uint32_t v = pk[wd];
        pk[wd] = 0;
        lo[k] += v & 0xFFFFu;
        hi[k] += v >> 16;
        // (batches of 8 reads: all 32 in flight beside the prefetched loads would spill)
        if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
      }
      block_sync();
    }
  }
  const uint64_t base = (uint64_t)b << 16;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    const uint64_t id = base + 2 * ((uint64_t)k * DEGB_THREADS + t);
    if (id + 1 < n_ids) {
      if (nsl == 1) {
        *(uint2*)(deg + id) = make_uint2(lo[k], hi[k]);
      } else {
        if (lo[k]) atomicAdd(&deg[id], lo[k]);
        if (hi[k]) atomicAdd(&deg[id + 1], hi[k]);
      }
    } else if (id < n_ids) {
      if (nsl == 1) deg[id] = lo[k];
      else if (lo[k]) atomicAdd(&deg[id], lo[k]);
    }
  }
}

// The scratch of the passes below: their layouts' totals (front_layout.h), 1 word where the
// pass does not apply (!degb_ok(n_ids)).
size_t degb_tmp_words(uint64_t m, uint32_t n_ids) { return degb_layout(m, n_ids).total; }
size_t degs_tmp_words(uint64_t m, uint32_t n_ids) { return degs_layout(m, n_ids).total; }
size_t fh_tmp_words(uint64_t m, uint32_t n_ids) { return fh_layout(m, n_ids).total; }
static_assert(PD_Y == DEGB_NB, "degs_tmp's sample counts: as many y digits as buckets");

// What a bucket histogram counts, bucket by bucket: the ids of `ids` (or the y ids of the
// records `recs` in its place) and, where given, of a second array `ids2`.  Bucket b's entries
// of an array lie at [start[b], start[b + 1]), cut at fill[b] where the regions are capacity
// regions (k_front_caps) filled up to their cursors; with G > 1 a bucket is G adjacent
// subregions b * G .. b * G + G - 1, and `spread` fills are k_front_fused's cursors (fill of
// region q at u64 index fs_cix(q)).
struct HistSrc {
  const uint16_t* ids = nullptr;
  const uint64_t* recs = nullptr;
  const unsigned long long* start = nullptr;
  const unsigned long long* fill = nullptr;
  const uint16_t* ids2 = nullptr;
  const unsigned long long* start2 = nullptr;
  const unsigned long long* fill2 = nullptr;
  uint32_t G = 1;
  bool spread = false;
  uint32_t* stats = nullptr;  // nullable: max degree, zero-degree ids, ids of degree >= SEQ_BIG
};
// k_degb_hist16 for buckets of 65536 ids, else k_degb_hist.  (k_degb_hist16 knows one region per
// bucket and plain fills: the fused front pass, whose fills are spread, has its own kernel
// there, k_degb_hist16s.)
// Each kernel has one way of adding, the one that measured faster for it; both once took either
// as a run-time mode, and the losing modes are removed.  k_degb_hist16 adds without the per-wave
// leader matching of repeated ids: ids are spread over 65536 counters per bucket, so a wave
// rarely repeats one, and the match cost more than the serialised hub adds it saves (RMAT-26
// hist 11.7 -> 10.7 ms of degree phase, twitter-shape 15.6 -> 14.1 ms).  The small-bucket
// histogram (k_degb_hist) matches: RMAT-22's 4096-id buckets repeat hub ids within a wave
// (degree 0.88 -> 0.94 ms with plain adds); the LJ shape would have gained from plain adds
// (0.81 -> 0.72 ms).  Gone with them: k_degb_hist over halves of a 65536-id bucket (two
// workgroups, each reading the whole run; k_degb_hist16 replaced it), and the digit-major count
// matrix with its flat scan, which every kernel here could still index (the tile-major matrix
// and tm_offsets replaced it).
static void launch_degb_hist(const HistSrc& h, int SH, uint32_t NB, uint32_t n_ids, uint32_t* deg,
                             hipStream_t s) {
  if (SH > 15)
    hipLaunchKernelGGL(k_degb_hist16, dim3(NB), dim3(DEGB_THREADS), 0, s, h.ids, n_ids, deg, h.start,
                       h.stats, h.ids2, h.start2, h.recs, h.fill);
  else
    hipLaunchKernelGGL(k_degb_hist, dim3(NB), dim3(DEGB_THREADS), degb_hist_lds(SH), s, h.ids, SH,
                       n_ids, deg, h.start, h.stats, h.ids2, h.start2, h.recs, h.fill, h.fill2, h.G,
                       (int)h.spread);
}

// deg (and selfc if non-null) for n_ids ids; tmp: degb_layout.
bool launch_degree_bucketed(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                            uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                            hipStream_t s, uint32_t* yhist, hipEvent_t counted, uint32_t* stats) {
  int SH;
  uint32_t NB;
  if (!degb_params(n_ids, &SH, &NB)) {
    launch_degree(uv, m, n_ids, file_mode, deg, selfc, err, s);
    if (stats) launch_deg_stats(deg, n_ids, stats, s);
    return false;
  }
  if (selfc) (void)hipMemsetAsync(selfc, 0, (size_t)n_ids * 4, s);
  if (n_ids == 0) {
    if (stats) (void)hipMemsetAsync(stats, 0, 12, s);
    return false;
  }
  if (m == 0) {
    (void)hipMemsetAsync(deg, 0, (size_t)n_ids * 4, s);
    if (stats) launch_deg_stats(deg, n_ids, stats, s);
    return false;
  }
  const int psh = part_shift(n_ids, PD_Y);  // as launch_part_gather with n_rank = n_ids
  if (yhist) (void)hipMemsetAsync(yhist, 0, PD_Y * 4, s);
  if (stats) (void)hipMemsetAsync(stats, 0, 12, s);
  const uint32_t nchunks = (uint32_t)((m + DEGB_CHUNK - 1) / DEGB_CHUNK);
  const DegbLayout L = degb_layout(m, n_ids);
  uint32_t* counts = tmp + L.counts;
  uint32_t* offsets = tmp + L.offsets;
  unsigned long long* bstart = (unsigned long long*)(tmp + L.bstart);
  uint16_t* ep = (uint16_t*)(tmp + L.ep);
  // tile-major counts (as the hi bins): bucket starts come from the scan
  hipLaunchKernelGGL(k_degb_count, dim3(nchunks), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m,
                     n_ids, file_mode, SH, NB, counts, err, psh, yhist);
  if (counted) (void)hipEventRecord(counted, s);
  tm_offsets(counts, offsets, nchunks, NB, NB, tmp + L.gsum, bstart, s);
  hipLaunchKernelGGL(k_degb_scatter, dim3(nchunks), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m,
                     n_ids, file_mode, SH, NB, (const uint32_t*)counts, (const uint32_t*)offsets, ep,
                     selfc);
  HistSrc h;
  h.ids = ep;
  h.start = bstart;
  h.stats = stats;
  launch_degb_hist(h, SH, NB, n_ids, deg, s);
  return yhist != nullptr;
}

// The sampled-capacity degree pass (see k_front_sample); tmp: degs_layout's sampled view.
bool launch_degree_sampled(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                           uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                           uint32_t* part_ws, uint64_t mid_slots, uint32_t* stats, uint32_t* ovf,
                           hipStream_t s, hipEvent_t caps_done) {
  int SH;
  uint32_t NB;
  if (m == 0 || n_ids == 0 || !degb_params(n_ids, &SH, &NB) || 2 * m >= (1ull << 32)) return false;
  const DegsView L = degs_layout(m, n_ids).sampled;  // (stride DEGB_NB, plain cursors)
  uint32_t* scnt = tmp + L.scnt;
  unsigned long long* bst = (unsigned long long*)(tmp + L.bst);
  unsigned long long* bcur = (unsigned long long*)(tmp + L.bcur);
  unsigned long long* bcap = (unsigned long long*)(tmp + L.bcap);
  uint16_t* ep = (uint16_t*)(tmp + L.ep);
  if (selfc) (void)hipMemsetAsync(selfc, 0, (size_t)n_ids * 4, s);
  if (stats) (void)hipMemsetAsync(stats, 0, 12, s);
  (void)hipMemsetAsync(scnt, 0, 2 * L.stride * 4, s);
  const int psh = part_shift(n_ids, PD_Y);  // the first partition pass's y digits
  const uint64_t ns = (m + FS_STRIDE - 1) / FS_STRIDE;
  const unsigned sg = (unsigned)std::min<uint64_t>((ns + DEGB_THREADS - 1) / DEGB_THREADS, 512);
  hipLaunchKernelGGL(k_front_sample, dim3(sg), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m, n_ids,
                     file_mode, SH, NB, psh, scnt, 0, 1u, 1u);
  hipLaunchKernelGGL(k_front_caps, dim3(1), dim3(1024), 0, s, (const uint32_t*)scnt, NB, m,
                     L.ep_slots, mid_slots, bst, bcur, bcap, part_ws + PW_YST,
                     (unsigned long long*)(part_ws + PW_CUR), (unsigned long long*)(part_ws + PW_YCAP),
                     (unsigned long long*)nullptr, 1u, 0);
  if (caps_done) (void)hipEventRecord(caps_done, s);
  const uint32_t nchunks = (uint32_t)((m + DEGB_CHUNK - 1) / DEGB_CHUNK);
  hipLaunchKernelGGL(k_degb_scatter_cap, dim3(nchunks), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m,
                     n_ids, file_mode, SH, NB, bcur, (const unsigned long long*)bcap, ep, selfc, ovf, err);
  HistSrc h;
  h.ids = ep;
  h.start = bst;
  h.fill = bcur;
  h.stats = stats;
  launch_degb_hist(h, SH, NB, n_ids, deg, s);
  return true;
}

// The fused front pass (k_front_fused) and its histogram: degrees (deg, selfc), the first
// partition's packed records in mid (mid_slots positions: u32 x array, then u16 y_lo array) and
// its region tables in part_ws (PW_FST / PW_FCUR / PW_FCAP, the x digits at PW_XH).  tmp:
// degs_tmp_words.  ovf_x: an x bucket outgrew its region (the degrees are then incomplete: the
// caller runs the exact pass); ovf_y: a y region (the histogram's y ids are then incomplete too:
// the caller runs the exact pass, and partitions again from uv).
bool front_fused_ok(uint64_t m, uint32_t n_ids) {
  int SH;
  uint32_t NB;
  return m > 0 && n_ids > 0 && degb_params(n_ids, &SH, &NB) && 2 * m < (1ull << 32) &&
         part_shift(n_ids, PD_Y) == SH && SH <= 16 && NB <= DEGB_NB;
}

// the histogram's slice length: about 2m / 1024 entries (at least 2^20), 4 slices per CU
static uint64_t hist16s_ch(uint64_t m) { return std::max<uint64_t>(1ull << 20, (2 * m + 1023) / 1024); }
// The packed first-pass records' slots (mid_slots) with G tile groups: the capacities of the
// PD_Y * G y subregions (k_front_caps sizes every digit, used or not) sum to at most this
// (fs_room), a multiple of 8.
uint64_t front_fused_slots(uint64_t m, uint32_t n_ids, uint32_t G) {
  (void)n_ids;
  return (fs_room(m, PD_Y * std::max<uint32_t>(1, std::min(G, FF_GMAX))) + 7) & ~7ull;
}

bool launch_front_fused(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode,
                        uint32_t* deg, uint32_t* selfc, uint32_t* err, uint32_t* tmp,
                        uint32_t* part_ws, uint64_t* mid, uint64_t mid_slots, uint32_t* stats,
                        uint32_t* ovf_x, uint32_t* ovf_y, hipStream_t s,
                        void (*mark)(void*, const char*), void* mark_arg, uint32_t G) {
  int SH;
  uint32_t NB;
  if (!front_fused_ok(m, n_ids) || mid_slots % 8 != 0) return false;
  degb_params(n_ids, &SH, &NB);
  G = std::max<uint32_t>(1, std::min(G, FF_GMAX));
  const unsigned nt = (unsigned)((m + FF_NT * FF_IT - 1) / (FF_NT * FF_IT));
  // persistent grid, one block per CU; with G groups a multiple of G (block b's tiles are then
  // all of group b % G)
  unsigned grid = std::min(nt, device_cus());
  if (G > 1 && grid >= G) grid -= grid % G;
  const DegsView L = degs_layout(m, n_ids).fused;  // (stride FS_MAX, cursors spread: fs_cix)
  uint32_t* scnt = tmp + L.scnt;
  unsigned long long* bst = (unsigned long long*)(tmp + L.bst);
  unsigned long long* bcur = (unsigned long long*)(tmp + L.bcur);
  unsigned long long* bcap = (unsigned long long*)(tmp + L.bcap);
  uint16_t* ep = (uint16_t*)(tmp + L.ep);
  unsigned long long* ys64 = (unsigned long long*)(part_ws + PW_FST);
  unsigned long long* ycur = (unsigned long long*)(part_ws + PW_FCUR);
  unsigned long long* ycap = (unsigned long long*)(part_ws + PW_FCAP);
  if (selfc) (void)hipMemsetAsync(selfc, 0, (size_t)n_ids * 4, s);
  if (stats) (void)hipMemsetAsync(stats, 0, 12, s);
  (void)hipMemsetAsync(scnt, 0, 2 * G * DEGB_NB * 4, s);
  (void)hipMemsetAsync(part_ws + PW_XH, 0, XH_WORDS * 4, s);  // the x digits of k_part<1>
  const uint64_t ns = (m + FS_STRIDE - 1) / FS_STRIDE;
  unsigned sg = (unsigned)std::min<uint64_t>((ns + DEGB_THREADS - 1) / DEGB_THREADS, 512);
  sg = (sg + G - 1) / G * G;
  hipLaunchKernelGGL(k_front_sample, dim3(sg), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m, n_ids,
                     file_mode, SH, NB, SH, scnt, 1, G, (uint32_t)(FF_NT * FF_IT / FS_STRIDE));
  hipLaunchKernelGGL(k_front_caps, dim3(1), dim3(1024), 0, s, (const uint32_t*)scnt, NB, m,
                     fs_room(m, NB * G), mid_slots, bst, bcur, bcap, (uint32_t*)nullptr, ycur, ycap,
                     ys64, G, (int)L.spread);
  if (mark) mark(mark_arg, "degree_sample");
  uint32_t* oa = (uint32_t*)mid;
  uint16_t* ob = (uint16_t*)(oa + mid_slots);
  hipLaunchKernelGGL(k_front_fused, dim3(grid), dim3(FF_NT), 0, s,
                     (const uint2*)uv, m, n_ids,
                     file_mode, SH, NB, oa, ob, ycur, (const unsigned long long*)ycap, bcur,
                     (const unsigned long long*)bcap, ep, selfc, ovf_y, ovf_x, err,
                     part_ws + PW_XH, part_shift(n_ids, PD_X),
                     (int)(part_shift(n_ids, PD_X) == SH + 2), G);
  if (mark) mark(mark_arg, "front_fused");
  // the x endpoints, then the y ids (the region of y digit b is x bucket b's id range)
  if (SH > 15) {
    // k_degb_hist16s REQUIRES spread cursors (it reads fill q at fs_cix(q)): bcur and ycur are,
    // by this pass's view of degs_tmp (degs_layout's fused view) and by part_ws's PW_FCUR
    const uint64_t CH = hist16s_ch(m);
    const unsigned hgrid = (unsigned)(NB + (2 * m + CH - 1) / CH + 1);
    (void)hipMemsetAsync(deg, 0, (size_t)n_ids * 4, s);
    hipLaunchKernelGGL(k_degb_hist16s, dim3(hgrid), dim3(DEGB_THREADS), 0, s, (const uint16_t*)ep,
                       (const unsigned long long*)bst, (const unsigned long long*)bcur,
                       (const uint16_t*)ob, (const unsigned long long*)ys64,
                       (const unsigned long long*)ycur, NB, n_ids, CH, deg, G);
    if (stats) launch_deg_stats(deg, n_ids, stats, s);
  } else {
    HistSrc h;
    h.ids = ep;
    h.start = bst;
    h.fill = bcur;
    h.ids2 = ob;
    h.start2 = ys64;
    h.fill2 = ycur;
    h.G = G;
    h.spread = L.spread;
    h.stats = stats;
    launch_degb_hist(h, SH, NB, n_ids, deg, s);
  }
  return true;
}

// ---------------------------------------------------------------------------------------
// Fused front half (graph2tree_dev, large inputs): the degree pass also performs the first
// partition of the rank gathers.  One counting read and one scattering read of the records:
//   k_fh_count    per 32K-record chunk: records per y bucket (2^SH ids), x endpoints per x
//                 bucket (LLAMA: x != y only; a self-loop counts once), and the x digits of the
//                 second partition pass (global, 256 counters) -> two tile-major count rows
//   k_fh_scatter  LDS counting sorts: the chunk's x ids (u16) by x bucket, and in four
//                 8K-record parts the RECORDS by y bucket
//   k_degb_hist16 / k_degb_hist  one workgroup per bucket over its records' y ids, then its
//                 x ids.
// The records come out grouped by y bucket — what the first pass of launch_part_gather
// produced from a second read — so the second pass (k_part<1>) gathers rank[y] from 256 KB
// slices.  Bytes per record: 8 (count) + 8 + 8 + 2 (scatter) + 8 + 2 (histogram) = 36,
// against 8 + 12 + 4 for the degree pass and 16 for the partition pass before.
// Chunks are dealt to blocks XCD-contiguously (xcd_chunk): the blocks of one XCD scatter
// consecutive chunks, whose runs of a bucket are adjacent in memory, so the short runs of the
// u16 arrays merge into whole lines in that XCD's L2.
// ---------------------------------------------------------------------------------------


// Block b -> chunk: blocks b and b + 8 share an XCD (round-robin dispatch; for speed only), so
// each group of blocks b % 8 takes one contiguous range of the n chunks (a bijection).
__device__ __forceinline__ uint32_t xcd_chunk(uint32_t b, uint32_t n) {
  const uint32_t q = n / 8, r = n % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

__global__ void __launch_bounds__(DEGB_THREADS)
k_fh_count(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
           uint32_t NB, uint32_t* __restrict__ cy, uint32_t* __restrict__ cx, uint32_t* err,
           int psh, uint32_t* __restrict__ xdig) {
  __shared__ uint32_t hy[DEGB_NB], hx[DEGB_NB], xd[PD_X];
  for (uint32_t i = threadIdx.x; i < NB; i += blockDim.x) { hy[i] = 0; hx[i] = 0; }
  for (uint32_t i = threadIdx.x; i < PD_X; i += blockDim.x) xd[i] = 0;
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * DEGB_CHUNK;
  const uint32_t cn = (uint32_t)min((uint64_t)DEGB_CHUNK, m - base);
  constexpr int U = 8;
  for (int r = 0; r < DEGB_CHUNK / (DEGB_THREADS * U); ++r) {
    uint2 e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + threadIdx.x;
      e[u] = i < cn ? ld_rec_nt(uv + base + i) : make_uint2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t i = (uint32_t)(r * U + u) * DEGB_THREADS + threadIdx.x;
      if (i >= cn) continue;
      if (e[u].x >= n_ids || e[u].y >= n_ids) { atomicOr(err, ERR_RANGE); continue; }
      atomicAdd(&hy[e[u].y >> SH], 1u);
      if (file_mode || e[u].x != e[u].y) atomicAdd(&hx[e[u].x >> SH], 1u);
      atomicAdd(&xd[part_digit<PD_X>(e[u].x, psh)], 1u);
    }
  }
  block_sync();
  for (uint32_t i = threadIdx.x; i < PD_X; i += blockDim.x)
    if (xd[i]) atomicAdd(&xdig[xh_ix(i)], xd[i]);
  for (uint32_t i = threadIdx.x; i < NB; i += blockDim.x) {
    cy[(uint64_t)blockIdx.x * NB + i] = hy[i];
    cx[(uint64_t)blockIdx.x * NB + i] = hx[i];
  }
}

// The chunk's x ids are staged whole (64 KB of u16, one run per x bucket as in k_degb_scatter:
// ~64-B runs) — staged per part, their 16-B runs would each cost a 64-B HBM write (measured:
// 26.5 GB written for 12.9 GB of data).  The records go out per 8K-record part (64-B runs).
// The y ids are not written separately: the histogram reads them from the records.
static constexpr int FH_PART = 8192, FH_PARTS = DEGB_CHUNK / FH_PART;

__global__ void __launch_bounds__(DEGB_THREADS)
k_fh_scatter(const uint2* __restrict__ uv, uint64_t m, uint32_t n_ids, int file_mode, int SH,
             uint32_t NB, const uint32_t* __restrict__ cx, const uint32_t* __restrict__ offy,
             const uint32_t* __restrict__ offx, uint64_t* __restrict__ recs,
             uint16_t* __restrict__ epx, uint32_t* __restrict__ selfc) {
  __shared__ uint16_t xbuf[DEGB_CHUNK];  // 64 KB: the chunk's x ids by x bucket
  __shared__ uint64_t stage[FH_PART];    // 64 KB: a part's records by y bucket
  __shared__ uint32_t sy[DEGB_NB + 1], xs[DEGB_NB], xcur[DEGB_NB], goy[DEGB_NB], gox[DEGB_NB];
  __shared__ uint32_t wsum[DEGB_THREADS / 64];
  constexpr int IT = FH_PART / DEGB_THREADS;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t lmask = (1u << SH) - 1u;
  const uint32_t c = xcd_chunk(blockIdx.x, gridDim.x);
  // the chunk's x runs: exclusive scan of its x count row (k_fh_count)
  {
    const uint32_t v = t < (int)NB ? cx[(uint64_t)c * NB + t] : 0u;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    if (t < (int)NB) {
      goy[t] = offy[(uint64_t)c * NB + t];
      gox[t] = offx[(uint64_t)c * NB + t];
    }
    block_sync();
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    if (t < (int)NB) { xs[t] = add + inc - v; xcur[t] = add + inc - v; }
  }
  const uint64_t base = (uint64_t)c * DEGB_CHUNK;
  const uint32_t cn = (uint32_t)min((uint64_t)DEGB_CHUNK, m - base);
  uint2 e[IT], en[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const uint32_t j = (uint32_t)(k * DEGB_THREADS + t);
    e[k] = j < cn ? ld_rec_nt(uv + base + j) : make_uint2(INV, INV);
  }
  for (int h = 0; h < FH_PARTS; ++h) {
    if (t < (int)NB) sy[t] = 0;
    block_sync();
    uint32_t ky[IT];  // rank inside the part's y run (INV: not stored)
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      ky[k] = INV;
      if (e[k].x >= n_ids || e[k].y >= n_ids) continue;  // padding, or ERR_RANGE (k_fh_count)
      const bool loop = e[k].x == e[k].y;
      ky[k] = atomicAdd(&sy[e[k].y >> SH], 1u);
      if (file_mode || !loop) xbuf[atomicAdd(&xcur[e[k].x >> SH], 1u)] = (uint16_t)(e[k].x & lmask);
      if (loop && selfc) atomicAdd(&selfc[e[k].x], 1u);
    }
    block_sync();
    const uint32_t v = t < (int)NB ? sy[t] : 0u;
    const uint32_t inc = wave_incl_scan(v);
    if (lane == 63) wsum[w] = inc;
    block_sync();
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    if (t < (int)NB) sy[t] = add + inc - v;
    if (t == DEGB_THREADS - 1) sy[NB] = add + inc;
    block_sync();
#pragma unroll
    for (int k = 0; k < IT; ++k)
      if (ky[k] != INV) stage[sy[e[k].y >> SH] + ky[k]] = ((uint64_t)e[k].y << 32) | e[k].x;
    if (h + 1 < FH_PARTS) {  // the next part's records, in flight during this part's writes
#pragma unroll
      for (int k = 0; k < IT; ++k) {
        const uint32_t j = (uint32_t)((h + 1) * FH_PART + k * DEGB_THREADS + t);
        en[k] = j < cn ? ld_rec_nt(uv + base + j) : make_uint2(INV, INV);
      }
    }
    block_sync();
    // written flat: thread j stores staged record j at its run's position (full waves even
    // where the runs are short; a run continues the previous part's, chunk after chunk)
    const uint32_t ny = sy[NB];
    for (uint32_t j = t; j < ny; j += DEGB_THREADS) {
      const uint64_t r = stage[j];
      const uint32_t b = (uint32_t)(r >> 32) >> SH;
      recs[(uint64_t)goy[b] + (j - sy[b])] = r;
    }
    block_sync();
    if (t < (int)NB) goy[t] += sy[t + 1] - sy[t];  // the next part continues each run
#pragma unroll
    for (int k = 0; k < IT; ++k) e[k] = en[k];
  }
  block_sync();
  // each wave writes whole x runs
  for (uint32_t b = w; b < NB; b += DEGB_THREADS / 64) {
    const uint32_t s0 = xs[b], n = xcur[b] - s0, g = gox[b];
    for (uint32_t j = lane; j < n; j += 64) epx[(uint64_t)g + j] = xbuf[s0 + j];
  }
}

// tmp: fh_layout.
bool launch_fh_front(const uint32_t* uv, uint64_t m, uint32_t n_ids, int file_mode, uint32_t* deg,
                     uint32_t* selfc, uint32_t* err, uint32_t* tmp, uint64_t* recs,
                     uint32_t* part_ws, uint32_t* stats, hipStream_t s,
                     void (*mark)(void*, const char*), void* mark_arg) {
  int SH;
  uint32_t NB;
  if (m == 0 || n_ids == 0 || !degb_params(n_ids, &SH, &NB)) return false;
  const uint32_t nchunks = (uint32_t)((m + DEGB_CHUNK - 1) / DEGB_CHUNK);
  const FhLayout L = fh_layout(m, n_ids);
  uint32_t *cy = tmp + L.cy, *cx = tmp + L.cx, *oy = tmp + L.oy, *ox = tmp + L.ox;
  uint32_t *gy = tmp + L.gy, *gx = tmp + L.gx;
  unsigned long long* by = (unsigned long long*)(tmp + L.by);
  unsigned long long* bx = (unsigned long long*)(tmp + L.bx);
  uint16_t* epx = (uint16_t*)(tmp + L.epx);
  if (selfc) (void)hipMemsetAsync(selfc, 0, (size_t)n_ids * 4, s);
  if (stats) (void)hipMemsetAsync(stats, 0, 12, s);
  (void)hipMemsetAsync(part_ws + PW_XH, 0, XH_WORDS * 4, s);  // the x digits of k_part<1>
  const int psh = part_shift(n_ids, PD_X);  // as launch_part_second with n_rank = n_ids
  hipLaunchKernelGGL(k_fh_count, dim3(nchunks), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m,
                     n_ids, file_mode, SH, NB, cy, cx, err, psh, part_ws + PW_XH);
  tm_offsets(cy, oy, nchunks, NB, NB, gy, by, s);
  tm_offsets(cx, ox, nchunks, NB, NB, gx, bx, s);
  if (mark) mark(mark_arg, "degree_count");
  hipLaunchKernelGGL(k_fh_scatter, dim3(nchunks), dim3(DEGB_THREADS), 0, s, (const uint2*)uv, m,
                     n_ids, file_mode, SH, NB, (const uint32_t*)cx, (const uint32_t*)oy,
                     (const uint32_t*)ox, recs, epx, selfc);
  if (mark) mark(mark_arg, "degree_scatter");
  HistSrc h;
  h.recs = recs;
  h.start = by;
  h.ids2 = epx;
  h.start2 = bx;
  h.stats = stats;
  launch_degb_hist(h, SH, NB, n_ids, deg, s);
  return true;
}

// ---------------------------------------------------------------------------------------
// Stable LSD radix sort of packed u64 items (key = upper 32 bits), 8- or 9-bit digits.
// Tile = 1024 threads x 8 items; wave w owns tile items [512 w, 512 w + 512), read in 8
// rounds of 64 consecutive items (coalesced).  Per pass: k_rsort_count (tile digit
// histograms, tile-major: counts[tile * NBIN + digit]) -> tm_offsets -> k_rsort_scatter.
// Ranking is wave-private: in each round the lanes holding one digit find each other with a
// ballot match, and a per-wave LDS counter per digit gives the stable rank inside the wave —
// no block barrier per round.  Then one pass over the digits turns the per-wave counts into
// per-wave offsets, the tile is staged in LDS in digit order, and written so that
// consecutive lanes store consecutive addresses of one digit run.
// ---------------------------------------------------------------------------------------
// bin of hi: the largest i with bounds[i] <= hi (bounds[0] = 0; INVALID his: the last bin)
__device__ __forceinline__ uint32_t bin_of(const uint32_t* bounds, uint32_t nb, uint32_t hi) {
  uint32_t lo = 0, n = nb;
  while (n > 1) {
    uint32_t half = n >> 1;
    if (bounds[lo + half] <= hi) lo += half;
    n -= half;
  }
  return lo;
}

static constexpr int RS_THREADS = 1024;
static constexpr int RS_ITEMS = 8;
static_assert(RS_TILE == RS_THREADS * RS_ITEMS, "rsort_layout (front_layout.h) counts these tiles");
static constexpr int RS_WAVES = RS_THREADS / 64;

// Lanes of the wave (among `valid` ones) whose digit equals this lane's d.
template <int DB>
__device__ __forceinline__ uint64_t digit_match(uint32_t d, bool valid) {
  uint64_t match = __ballot(valid);
#pragma unroll
  for (int b = 0; b < DB; ++b) {
    bool bit = (d >> b) & 1u;
    uint64_t bal = __ballot(bit);
    match &= bit ? bal : ~bal;
  }
  return match;
}

template <int DB>  // digit bits: 8 or 9
__global__ void __launch_bounds__(RS_THREADS)
k_rsort_count(const uint64_t* __restrict__ in, uint64_t n, int shift, uint32_t* __restrict__ counts) {
  constexpr uint32_t NBIN = 1u << DB;
  __shared__ uint32_t hist[NBIN];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t i = t; i < NBIN; i += RS_THREADS) hist[i] = 0;
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE + (uint64_t)w * (64 * RS_ITEMS) + lane;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint64_t it[RS_ITEMS];
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    uint64_t idx = base + (uint64_t)k * 64;
    it[k] = idx < n ? in[idx] : 0ull;
  }
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    bool valid = base + (uint64_t)k * 64 < n;
    uint32_t d = (uint32_t)(it[k] >> (32 + shift)) & (NBIN - 1);
    uint64_t match = digit_match<DB>(d, valid);  // one LDS add per distinct digit (skewed keys)
    if (valid && (match & lt) == 0) atomicAdd(&hist[d], (uint32_t)__popcll(match));
  }
  block_sync();
  for (uint32_t i = t; i < NBIN; i += RS_THREADS) counts[(uint64_t)blockIdx.x * NBIN + i] = hist[i];
}

// offsets are tile-major (offsets[tile * NBIN + digit], see k_tm_rows): the tile reads its NBIN
// offsets as one contiguous run.
template <int DB>
__global__ void __launch_bounds__(RS_THREADS)
k_rsort_scatter(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n, int shift,
                const uint32_t* __restrict__ offsets) {
  constexpr uint32_t NBIN = 1u << DB;
  __shared__ uint64_t stage[RS_TILE];
  __shared__ uint32_t whist[RS_WAVES][NBIN];
  __shared__ uint32_t tstart[NBIN], goff[NBIN], wsum[RS_WAVES];
  auto digit = [&](uint64_t it) -> uint32_t { return (uint32_t)(it >> (32 + shift)) & (NBIN - 1); };
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * RS_TILE;
  const uint32_t tile_n = (uint32_t)((n - tbase) < (uint64_t)RS_TILE ? (n - tbase) : RS_TILE);
  const uint32_t wbase = (uint32_t)w * (64 * RS_ITEMS) + lane;  // tile index of round 0
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (uint32_t i = t; i < NBIN; i += RS_THREADS) goff[i] = offsets[(uint64_t)blockIdx.x * NBIN + i];
  for (uint32_t i = lane; i < NBIN; i += 64) whist[w][i] = 0;
  uint32_t dg[RS_ITEMS];
  uint64_t item[RS_ITEMS];
  uint32_t rk[RS_ITEMS];
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    uint32_t li = wbase + (uint32_t)k * 64;
    item[k] = li < tile_n ? in[tbase + li] : 0ull;
  }
  // stable rank inside the wave: rounds in item order, lanes in item order within a round
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    bool valid = wbase + (uint32_t)k * 64 < tile_n;
    uint32_t d = digit(item[k]);
    dg[k] = d;
    uint64_t match = digit_match<DB>(d, valid);
    uint32_t before = (uint32_t)__popcll(match & lt);
    uint32_t prev = whist[w][d];
    rk[k] = prev + before;
    if (valid && before == 0) whist[w][d] = prev + (uint32_t)__popcll(match);
  }
  block_sync();
  // per-wave counts -> per-wave exclusive offsets inside each digit; tile digit totals -> tstart
  for (uint32_t dd = t; dd < NBIN; dd += RS_THREADS) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < RS_WAVES; ++i) { uint32_t v = whist[i][dd]; whist[i][dd] = s; s += v; }
    uint32_t incl = wave_incl_scan(s);
    if (lane == 63) wsum[w] = incl;
    tstart[dd] = incl - s;
  }
  block_sync();
  if (t < (int)NBIN) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    tstart[t] += add;
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    if (wbase + (uint32_t)k * 64 < tile_n) {
      uint32_t d = dg[k];
      stage[tstart[d] + whist[w][d] + rk[k]] = item[k];
    }
  }
  block_sync();
  for (uint32_t j = t; j < tile_n; j += RS_THREADS) {
    uint64_t it = stage[j];
    uint32_t d = digit(it);
    out[(uint64_t)goff[d] + (j - tstart[d])] = it;
  }
}

// Tile-major bin counts (counts[tile * 512 + bin], written by k_edge_pass_tiles) ->
// tile-major global offsets, in three coalesced passes over groups of TM_G tiles:
//   k_tm_colsum       gsum[g][bin] = records of the bin in group g;
//   k_tm_scan_groups  gsum[g][bin] <- exclusive prefix over groups; bin_start = exclusive
//                     prefix of the bin totals (and n at [nb]);
//   k_tm_rows         counts[t][bin] <- bin_start[bin] + gsum[g][bin] + earlier tiles of g.
// The digit-major layout had every tile write (edge pass) and read (scatter) 512 words that
// lie ntiles words apart: 131 K tiles x 512 x a 64-B sector each way at RMAT-26.
// NC columns (bins) per tile row; launched with blockDim.x >= NC (threads beyond NC idle).

__global__ void __launch_bounds__(1024)
k_tm_colsum(const uint32_t* __restrict__ counts, uint32_t ntiles, uint32_t NC,
            uint32_t* __restrict__ gsum, uint32_t G) {
  const uint32_t d = threadIdx.x, t0 = blockIdx.x * G, t1 = min(t0 + G, ntiles);
  if (d >= NC) return;
  uint32_t sum = 0;
  for (uint32_t t = t0; t < t1; t += 8) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = t + u < t1 ? counts[(uint64_t)(t + u) * NC + d] : 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += v[u];
  }
  gsum[(uint64_t)blockIdx.x * NC + d] = sum;
}

// One block.  bin_start[d] (d < nb) = exclusive prefix of the column totals; bin_start[nb] =
// the grand total (columns nb..NC-1 must be empty).
__global__ void __launch_bounds__(1024)
k_tm_scan_groups(uint32_t* __restrict__ gsum, uint32_t ngroups, uint32_t NC, uint32_t nb,
                 unsigned long long* __restrict__ bin_start) {
  __shared__ uint32_t wsum[16];
  const uint32_t d = threadIdx.x, lane = d & 63, w = d >> 6;
  uint32_t run = 0;
  if (d < NC)
    for (uint32_t g = 0; g < ngroups; g += 8) {
      uint32_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = g + u < ngroups ? gsum[(uint64_t)(g + u) * NC + d] : 0u;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (g + u < ngroups) gsum[(uint64_t)(g + u) * NC + d] = run;
        run += v[u];
      }
    }
  const uint32_t incl = wave_incl_scan(run);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t add = 0;
  for (uint32_t i = 0; i < w; ++i) add += wsum[i];
  if (d < nb) bin_start[d] = add + incl - run;
  if (d == blockDim.x - 1) bin_start[nb] = add + incl;
}

// out[t][d] = bin_start[d] + gsum[g][d] + in[t'][d] summed over the earlier tiles t' of g
// (out may alias in).
__global__ void __launch_bounds__(1024)
k_tm_rows(const uint32_t* in, uint32_t* out, uint32_t ntiles, uint32_t NC,
          const uint32_t* __restrict__ gsum, const unsigned long long* __restrict__ bin_start,
          uint32_t nb, uint32_t G) {
  const uint32_t d = threadIdx.x, t0 = blockIdx.x * G, t1 = min(t0 + G, ntiles);
  if (d >= NC) return;
  uint32_t run = (d < nb ? (uint32_t)bin_start[d] : 0u) + gsum[(uint64_t)blockIdx.x * NC + d];
  for (uint32_t t = t0; t < t1; t += 8) {
    uint32_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = t + u < t1 ? in[(uint64_t)(t + u) * NC + d] : 0u;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (t + u < t1) out[(uint64_t)(t + u) * NC + d] = run;
      run += v[u];
    }
  }
}

// Tile-major exclusive offsets of an ntiles x NC count matrix (gsum: NC * ceil(ntiles / G)
// words of scratch); bin_start: nb + 1 u64 (column starts, then the total).  G: tiles per
// group (the column and row passes run one block per group).
static void tm_offsets(const uint32_t* counts, uint32_t* offsets, uint32_t ntiles, uint32_t NC,
                       uint32_t nb, uint32_t* gsum, unsigned long long* bin_start, hipStream_t s,
                       uint32_t G) {
  const uint32_t ng = (ntiles + G - 1) / G;
  const unsigned th = NC <= 512 ? 512 : 1024;
  hipLaunchKernelGGL(k_tm_colsum, dim3(ng), dim3(th), 0, s, counts, ntiles, NC, gsum, G);
  hipLaunchKernelGGL(k_tm_scan_groups, dim3(1), dim3(th), 0, s, gsum, ng, NC, nb, bin_start);
  hipLaunchKernelGGL(k_tm_rows, dim3(ng), dim3(th), 0, s, counts, offsets, ntiles, NC,
                     (const uint32_t*)gsum, (const unsigned long long*)bin_start, nb, G);
}

// The hi-bin scatter without stability (the order inside a bin is free: the kb loop and pst
// never depend on it): 16384-item tiles — two of the edge pass's 8192-item count tiles, whose
// runs of a bin are adjacent in the output, so the tile's base for bin d is the first one's
// tile-major offset — ranked by LDS atomics, staged in bin order, and written as whole runs
// per wave (runs twice as long as the stable scatter's, without its 9-ballot rank).
static constexpr int BS_TILE = 2 * RS_TILE;

__global__ void __launch_bounds__(1024)
k_bin_scatter(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n,
              const uint32_t* __restrict__ offsets, const uint16_t* __restrict__ digits) {
  constexpr int NT = 1024, IT = BS_TILE / NT;
  __shared__ uint64_t stage[BS_TILE];
  __shared__ uint32_t hist[512], tstart[512], goff[512], wsum[NT / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t tbase = (uint64_t)blockIdx.x * BS_TILE;
  const uint32_t tile_n = (uint32_t)min((uint64_t)BS_TILE, n - tbase);
  if (t < 512) {
    hist[t] = 0;
    goff[t] = offsets[(uint64_t)(2 * blockIdx.x) * 512 + t];
  }
  uint64_t it[IT];
  uint32_t dg[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const uint32_t j = (uint32_t)k * NT + t;
    it[k] = j < tile_n ? in[tbase + j] : 0ull;
    dg[k] = j < tile_n ? digits[tbase + j] : 0u;
  }
  block_sync();
  uint32_t li[IT];
#pragma unroll
  for (int k = 0; k < IT; ++k)
    if ((uint32_t)k * NT + t < tile_n) li[k] = atomicAdd(&hist[dg[k]], 1u);
  block_sync();
  if (t < 512) {
    const uint32_t c = hist[t];
    const uint32_t incl = wave_incl_scan(c);
    if (lane == 63) wsum[w] = incl;
    tstart[t] = incl - c;
  }
  block_sync();
  if (t < 512) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    tstart[t] += add;
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < IT; ++k)
    if ((uint32_t)k * NT + t < tile_n) stage[tstart[dg[k]] + li[k]] = it[k];
  block_sync();
  for (uint32_t d = w; d < 512; d += NT / 64) {
    const uint32_t s0 = tstart[d], c = hist[d];
    const uint64_t g = goff[d];
    for (uint32_t j = lane; j < c; j += 64) out[g + j] = stage[s0 + j];
  }
}

// The scatter by bin: tmp holds launch_edge_pass_bins's tile counts (rsort_layout(n)), digits
// each item's bin; bin_start: nb + 1 u64; h_start (pinned, nullable): bin_start copied out before
// the scatter, `started` recorded once it is written.
static void bin_sort_u64(const uint64_t* in, uint64_t* out, uint64_t n, uint32_t nb, uint32_t* tmp,
                         unsigned long long* bin_start, const uint16_t* digits, hipStream_t s,
                         unsigned long long* h_start, hipEvent_t started) {
  // the bin starts are known before the scatter: the caller may read them while it runs
  auto publish = [&]() {
    if (h_start) {
      (void)hipMemcpyAsync(h_start, bin_start, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, s);
      (void)hipEventRecord(started, s);
    }
  };
  const RsortLayout L = rsort_layout(n);
  uint32_t* counts = tmp + L.counts;
  if (n == 0) return;
  tm_offsets(counts, counts, (uint32_t)L.ntiles, 512, nb, tmp + L.gsum, bin_start, s);
  publish();
  hipLaunchKernelGGL(k_bin_scatter, dim3((unsigned)((n + BS_TILE - 1) / BS_TILE)), dim3(1024), 0, s,
                     in, out, n, (const uint32_t*)counts, digits);
}

size_t rsort_tmp_words(uint64_t n) { return rsort_layout(n).total; }

// Digit width of the first pass when `bits` are sorted in passes of <= 9 bits (even split,
// wider first): 25 bits -> 9+8+8, 18 -> 9+9.
int rsort_first_width(int bits) {
  if (bits <= 0) return 0;
  int passes = (bits + 8) / 9;
  return bits / passes + (bits % passes ? 1 : 0);
}

// Sorts n items on bits [bit_lo, bit_hi) of their upper word with passes of <= 9 bits;
// returns the buffer holding the result (in, a or b).  `in` is only read by the first pass.
// counted0: the first pass's tile histograms are already in tmp (k_edge_pass_tiles).
uint64_t* radix_sort_u64(const uint64_t* in, uint64_t* a, uint64_t* b, uint64_t n, int bit_lo,
                         int bit_hi, uint32_t* tmp, hipStream_t s, bool counted0) {
  const RsortLayout L = rsort_layout(n);
  const uint64_t nt = L.ntiles;
  uint32_t *counts = tmp + L.counts, *stmp = tmp + L.gsum;
  unsigned long long* dstart = (unsigned long long*)(tmp + L.dstart);
  const uint64_t* src = in;
  uint64_t* dst = a;
  for (int shift = bit_lo, p = 0; shift < bit_hi; ++p) {
    int width = rsort_first_width(bit_hi - shift);
    if (n) {
      bool count = !(p == 0 && counted0);
      const dim3 g((unsigned)nt), bl(RS_THREADS);
      if (width > 8) {
        if (count) hipLaunchKernelGGL(k_rsort_count<9>, g, bl, 0, s, src, n, shift, counts);
        tm_offsets(counts, counts, (uint32_t)nt, 512, 512, stmp, dstart, s);
        hipLaunchKernelGGL(k_rsort_scatter<9>, g, bl, 0, s, src, dst, n, shift, (const uint32_t*)counts);
      } else {
        if (count) hipLaunchKernelGGL(k_rsort_count<8>, g, bl, 0, s, src, n, shift, counts);
        tm_offsets(counts, counts, (uint32_t)nt, 256, 256, stmp, dstart, s);
        hipLaunchKernelGGL(k_rsort_scatter<8>, g, bl, 0, s, src, dst, n, shift, (const uint32_t*)counts);
      }
    }
    shift += width;
    src = dst;
    dst = (dst == a) ? b : a;
  }
  return (uint64_t*)src;
}

// Degree sequence helpers: items = (deg << 32 | id); after the sort, seq = ids past the
// zero-degree prefix and rank[seq[i]] = i (jtree.h:165-168) in the same pass.
// nsd (nullable): nsd[i] = degree of seq[i] in rank order (the sorted item's key), less
// w * selfc[seq[i]] when selfc is given.
__global__ void k_unpack_seq(const uint64_t* __restrict__ items, uint32_t zeros, uint32_t n_seq,
                             uint32_t* __restrict__ seq, uint32_t* __restrict__ rank,
                             uint32_t* __restrict__ nsd, const uint32_t* __restrict__ selfc,
                             uint32_t w, uint32_t base) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += gridDim.x * blockDim.x) {
    const uint64_t it = items[zeros + i];
    uint32_t v = (uint32_t)it;
    seq[base + i] = v;
    if (rank) rank[v] = base + i;
    if (nsd) nsd[base + i] = (uint32_t)(it >> 32) - (selfc ? w * selfc[v] : 0u);
  }
}

// The sequence holds only the ids with deg > 0 (sequence.h:55-61): pack just those, in id
// order (a stable compaction: per-block counts, a scan, a block-local scan), so the radix
// passes sort n_seq items instead of n_ids (half of them at RMAT-26).
static constexpr uint32_t NZ_BLOCK = 4096;  // ids per block: 1024 threads x 4

__global__ void __launch_bounds__(1024)
k_nz_count(const uint32_t* __restrict__ deg, uint32_t n, uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t wsum[16];
  const uint32_t t = threadIdx.x, base = blockIdx.x * NZ_BLOCK + 4 * t;
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c += (base + k < n && deg[base + k] != 0);
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((t & 63) == 0) wsum[t >> 6] = c;
  block_sync();
  if (t == 0) {
    uint32_t sum = 0;
    for (int i = 0; i < 16; ++i) sum += wsum[i];
    bcnt[blockIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(1024)
k_pack_nz(const uint32_t* __restrict__ deg, uint32_t n, const uint32_t* __restrict__ bofs,
          uint64_t* __restrict__ items) {
  __shared__ uint32_t wsum[16];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6, base = blockIdx.x * NZ_BLOCK + 4 * t;
  uint32_t d[4], c = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    d[k] = base + k < n ? deg[base + k] : 0u;
    c += d[k] != 0;
  }
  const uint32_t incl = wave_incl_scan(c);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t pos = bofs[blockIdx.x] + incl - c;
  for (uint32_t i = 0; i < w; ++i) pos += wsum[i];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (d[k]) items[pos++] = ((uint64_t)d[k] << 32) | (base + k);
}

size_t pack_nz_tmp_words(uint32_t n) {
  const uint64_t nb = ((uint64_t)n + NZ_BLOCK - 1) / NZ_BLOCK;
  return 2 * nb + scan_tmp_words(nb) + 2;
}

void launch_pack_nonzero(const uint32_t* deg, uint32_t n, uint64_t* items, uint32_t* tmp,
                         hipStream_t s) {
  if (n == 0) return;
  const uint32_t nb = (uint32_t)(((uint64_t)n + NZ_BLOCK - 1) / NZ_BLOCK);
  uint32_t* bcnt = tmp;
  uint32_t* bofs = tmp + nb;
  hipLaunchKernelGGL(k_nz_count, dim3(nb), dim3(1024), 0, s, deg, n, bcnt);
  launch_scan_exclusive(bcnt, bofs, nb, bofs + nb, s);
  hipLaunchKernelGGL(k_pack_nz, dim3(nb), dim3(1024), 0, s, deg, n, (const uint32_t*)bofs, items);
}

void launch_unpack_seq(const uint64_t* items, uint32_t zeros, uint32_t n_seq, uint32_t* seq,
                       uint32_t* rank, hipStream_t s, uint32_t* nsd, const uint32_t* selfc,
                       int file_mode, uint32_t base) {
  if (n_seq)
    hipLaunchKernelGGL(k_unpack_seq, dim3(grid_for(n_seq)), dim3(BLOCK), 0, s, items, zeros, n_seq,
                       seq, rank, nsd, selfc, file_mode ? 2u : 1u, base);
}

// ---------------------------------------------------------------------------------------
// Degree sequence by counting (sequence.h:55-61: the ids with deg > 0 by degree, ties in id
// order).  Degrees 1 .. SQ_T-1 are classes of a counting sort straight from deg[] — no items,
// no radix passes; the few ids of degree >= SQ_T share the last class and are radix-sorted
// among themselves behind the others.  A chunk is 16 waves x SQ_IT rounds of 64 consecutive
// ids, wave w owning ids [w 64 SQ_IT, (w + 1) 64 SQ_IT) of it: the per-wave stable rank of
// k_rsort_scatter then gives id order inside each class.
//   k_seqc_count   per-chunk class counts (tile-major), then tm_offsets: each chunk's first
//                  position of every class;
//   k_seqc_place   seq[pos] = id, rank[id] = pos, nsd[pos] = deg for the counted classes,
//                  rank[id] = INVALID for degree 0, (deg << 32 | id) for the last class.
// ---------------------------------------------------------------------------------------
static constexpr int SQ_DB = 10;
static constexpr uint32_t SQ_T = 1u << SQ_DB;  // == the block size: one class per thread
static_assert(SQ_T == SEQ_BIG, "the degree stats count the radix-sorted tail's ids");
static constexpr int SQ_IT = 16;
static constexpr uint32_t SQ_CHUNK = 1024u * SQ_IT;
static constexpr uint32_t SQ_G = 16;  // chunks per group of tm_offsets' column and row passes

__device__ __forceinline__ uint32_t seqc_class(uint32_t d) { return (min(d, SQ_T) - 1) & (SQ_T - 1); }

__global__ void __launch_bounds__(1024)
k_seqc_count(const uint32_t* __restrict__ deg, uint32_t n, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[SQ_T];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  hist[t] = 0;
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * SQ_CHUNK + (uint64_t)w * (64 * SQ_IT) + lane;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t d[SQ_IT];
#pragma unroll
  for (int k = 0; k < SQ_IT; ++k) {
    const uint64_t id = base + (uint64_t)k * 64;
    d[k] = id < n ? deg[id] : 0u;
  }
#pragma unroll
  for (int k = 0; k < SQ_IT; ++k) {
    const uint32_t c = seqc_class(d[k]);
    const uint64_t match = digit_match<SQ_DB>(c, d[k] != 0);  // one LDS add per class and round
    if (d[k] && (match & lt) == 0) atomicAdd(&hist[c], (uint32_t)__popcll(match));
  }
  block_sync();
  counts[(uint64_t)blockIdx.x * SQ_T + t] = hist[t];
}

__global__ void __launch_bounds__(1024)
k_seqc_place(const uint32_t* __restrict__ deg, uint32_t n, const uint32_t* __restrict__ offsets,
             const unsigned long long* __restrict__ cstart, uint32_t* __restrict__ seq,
             uint32_t* __restrict__ rank, uint32_t* __restrict__ nsd, uint64_t* __restrict__ big,
             const uint32_t* __restrict__ selfc, uint32_t sw) {
  __shared__ uint32_t whist[16][SQ_T];  // per-wave class counts, then per-wave offsets
  __shared__ uint32_t goff[SQ_T];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  goff[t] = offsets[(uint64_t)blockIdx.x * SQ_T + t];
  for (uint32_t i = lane; i < SQ_T; i += 64) whist[w][i] = 0;
  const uint32_t big0 = (uint32_t)cstart[SQ_T - 1];
  block_sync();
  const uint64_t base = (uint64_t)blockIdx.x * SQ_CHUNK + (uint64_t)w * (64 * SQ_IT) + lane;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t d[SQ_IT], rk[SQ_IT];
#pragma unroll
  for (int k = 0; k < SQ_IT; ++k) {
    const uint64_t id = base + (uint64_t)k * 64;
    d[k] = id < n ? deg[id] : 0u;
  }
#pragma unroll
  for (int k = 0; k < SQ_IT; ++k) {  // rounds in id order, lanes in id order within a round
    const uint32_t c = seqc_class(d[k]);
    const uint64_t match = digit_match<SQ_DB>(c, d[k] != 0);
    const uint32_t before = (uint32_t)__popcll(match & lt);
    const uint32_t prev = whist[w][c];
    rk[k] = prev + before;
    if (d[k] && before == 0) whist[w][c] = prev + (uint32_t)__popcll(match);
  }
  block_sync();
  {  // thread t = class t: the waves' exclusive offsets inside the chunk's run of the class
    uint32_t run = goff[t];
#pragma unroll
    for (int i = 0; i < 16; ++i) { const uint32_t v = whist[i][t]; whist[i][t] = run; run += v; }
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < SQ_IT; ++k) {
    const uint64_t id = base + (uint64_t)k * 64;
    if (id >= n) continue;
    if (d[k] == 0) {
      if (rank) rank[id] = INV;
    } else if (d[k] < SQ_T) {
      const uint32_t pos = whist[w][d[k] - 1] + rk[k];
      seq[pos] = (uint32_t)id;
      if (rank) rank[id] = pos;
      if (nsd) nsd[pos] = d[k] - (selfc ? sw * selfc[id] : 0u);
    } else {
      big[whist[w][SQ_T - 1] + rk[k] - big0] = ((uint64_t)d[k] << 32) | id;
    }
  }
}

size_t seqc_tmp_words(uint32_t n) {
  const uint64_t nc = ((uint64_t)n + SQ_CHUNK - 1) / SQ_CHUNK;
  return SQ_T * nc + SQ_T * ((nc + SQ_G - 1) / SQ_G) + 2 * (SQ_T + 1) + 2;
}

uint32_t* launch_seqc_place(const uint32_t* deg, uint32_t n, uint32_t* seq, uint32_t* rank,
                            uint32_t* nsd, uint64_t* big, uint32_t* tmp, hipStream_t s,
                            const uint32_t* selfc, int file_mode) {
  const uint32_t nc = (uint32_t)(((uint64_t)n + SQ_CHUNK - 1) / SQ_CHUNK);
  uint32_t* counts = tmp;
  uint32_t* gsum = counts + (size_t)SQ_T * nc;
  unsigned long long* cstart = (unsigned long long*)(((uintptr_t)(gsum + (size_t)SQ_T *
                                ((nc + SQ_G - 1) / SQ_G)) + 7) & ~(uintptr_t)7);
  if (n == 0) return nullptr;
  hipLaunchKernelGGL(k_seqc_count, dim3(nc), dim3(1024), 0, s, deg, n, counts);
  tm_offsets(counts, counts, nc, SQ_T, SQ_T, gsum, cstart, s, SQ_G);
  hipLaunchKernelGGL(k_seqc_place, dim3(nc), dim3(1024), 0, s, deg, n, (const uint32_t*)counts,
                     (const unsigned long long*)cstart, seq, rank, nsd, big, selfc,
                     file_mode ? 2u : 1u);
  return (uint32_t*)(cstart + (SQ_T - 1));  // the first position of the last class (u64)
}

uint32_t seqc_threshold() { return SQ_T; }

// ---------------------------------------------------------------------------------------
// rank[seq[i]] = i (JTree::insert(X, id), jtree.h:165-168).  A repeated id trips the
// reference's assert; here it sets ERR_DUP_SEQ.
// ---------------------------------------------------------------------------------------
__global__ void k_rank_scatter(const uint32_t* __restrict__ seq, uint32_t n_seq,
                               uint32_t* __restrict__ rank, uint32_t* err) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += gridDim.x * blockDim.x) {
    if (atomicCAS(&rank[seq[i]], INV, i) != INV) atomicOr(err, ERR_DUP_SEQ);
  }
}

void launch_rank_scatter(const uint32_t* seq, uint32_t n_seq, uint32_t* rank, uint32_t* err,
                         hipStream_t s) {
  if (n_seq == 0) return;
  hipLaunchKernelGGL(k_rank_scatter, dim3(grid_for(n_seq)), dim3(BLOCK), 0, s, seq, n_seq, rank, err);
}

// ---------------------------------------------------------------------------------------
// Edge pass (JTree::insert's edge loop, jtree.cpp:73-90, edge-parallel): for record (t,h),
// t != h, in jnid space lo = min(rank), hi = max(rank) with INVALID = +inf:
//   lo valid           -> pst_weight[lo] += 1        (the POSTORDER edge seen from lo)
//   lo, hi both valid  -> tree edge (lo, hi)         (the PREORDER edge seen from hi)
// Ids >= n_rank are outside the reference's index vector: if the other endpoint is in seq the
// reference's index.at() throws (jtree.cpp:75) -> ERR_RANGE; otherwise neither endpoint is
// ever visited and the record is ignored.  (k_edge_pass_tiles and k_edge_bin below.)
// ---------------------------------------------------------------------------------------
// Hi bins: one radix-style pass instead of the two 9-bit passes.  The kb loop needs the
// records grouped by hi only down to 256-rank groups, and only where they are dense; the bins
// are runs of 256-rank chunks cut from an estimate of the records per hi rank taken from the
// degrees alone (a vertex of degree d at rank r is the hi end of about d * D(r) / 2m records,
// D(r) the degree mass below r), so they exist before the edge pass computes a single hi.
// The estimate only shapes the work; any bins give the same tree.
// ---------------------------------------------------------------------------------------
// out[c] = sum of deg[seq[r]] over r in [256 c, 256 c + 256) (one wave per chunk).
// nsd (nullable): rank-ordered degrees (k_unpack_seq's non-self-loop degrees: the bins are only
// an estimate) read instead of gathering deg[seq[r]].
__global__ void k_chunk_degsum(const uint32_t* __restrict__ seq, const uint32_t* __restrict__ deg,
                               uint32_t n_seq, uint64_t* __restrict__ out,
                               const uint32_t* __restrict__ nsd) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t nch = (n_seq + 255) / 256;
  for (uint32_t ch = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; ch < nch;
       ch += (gridDim.x * blockDim.x) >> 6) {
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint32_t r = ch * 256 + k * 64 + lane;
      if (r < n_seq) sum += nsd ? nsd[r] : deg[seq[r]];
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if (lane == 0) out[ch] = sum;
  }
}

void launch_chunk_degsum(const uint32_t* seq, const uint32_t* deg, uint32_t n_seq, uint64_t* out,
                         hipStream_t s, const uint32_t* nsd) {
  if (n_seq) hipLaunchKernelGGL(k_chunk_degsum, dim3(grid_for((uint64_t)(n_seq + 255) / 256 * 64)),
                                dim3(BLOCK), 0, s, seq, deg, n_seq, out, nsd);
}


// The edge pass fused with the first radix pass's tile histograms (digit = bits
// [shift, shift + DB) of hi): one block per RS_TILE records, wave-striped like
// k_rsort_count; each thread loads its 8 records and issues their rank gathers before using
// any (keep many gathers in flight).  pst (nullable): pst_weight[lo] += 1 per record (above).
// PRE: the records are k_part's output (x, ry): rank[y] was gathered already (or is one of the
// sentinels RY_SELF / RY_OUT), only rank[x] is gathered here.
// BINS: the digit is the hi bin (bin_of over the nb bounds in bins), also written to digits.
// The tile histograms are written tile-major (tm_offsets).
// plain (1 exactly where BINS): count by plain LDS atomics, no ballot match.  It stays a run-time
// argument: as a compile-time test the BINS kernels take 46 / 52 VGPRs instead of 34.
template <int DB, bool PRE, bool BINS = false>
__global__ void __launch_bounds__(RS_THREADS)
k_edge_pass_tiles(const uint2* __restrict__ uv, uint64_t m, const uint32_t* __restrict__ rank,
                  uint32_t n_rank, uint32_t* __restrict__ pst, uint64_t* __restrict__ items,
                  uint32_t* err, int shift, uint32_t* __restrict__ counts,
                  const uint32_t* __restrict__ bins = nullptr, uint32_t nb = 0,
                  uint16_t* __restrict__ digits = nullptr, int plain = 0) {
  constexpr uint32_t NBIN = 1u << DB;
  __shared__ uint32_t hist[NBIN];
  __shared__ uint32_t sb[BINS ? NBIN : 1];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t i = t; i < NBIN; i += RS_THREADS) hist[i] = 0;
  if (BINS)
    for (uint32_t i = t; i < nb; i += RS_THREADS) sb[i] = bins[i];
  const uint64_t base = (uint64_t)blockIdx.x * RS_TILE + (uint64_t)w * (64 * RS_ITEMS) + lane;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint2 e[RS_ITEMS];
  uint32_t rx[RS_ITEMS], ry[RS_ITEMS];
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    uint64_t idx = base + (uint64_t)k * 64;
    e[k] = idx < m ? uv[idx] : make_uint2(0, PRE ? RY_SELF : 0u);
  }
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    if (PRE) {
      rx[k] = (e[k].y != RY_SELF && e[k].x < n_rank) ? rank[e[k].x] : INV;
    } else {
      bool g = e[k].x != e[k].y;  // self-loops (and padding) gather nothing
      rx[k] = (g && e[k].x < n_rank) ? rank[e[k].x] : INV;
      ry[k] = (g && e[k].y < n_rank) ? rank[e[k].y] : INV;
    }
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < RS_ITEMS; ++k) {
    uint64_t idx = base + (uint64_t)k * 64;
    bool valid = idx < m;
    uint32_t hi = INV, lo = INV;
    bool loop = PRE ? e[k].y == RY_SELF : e[k].x == e[k].y;
    if (valid && !loop) {
      bool ox = e[k].x >= n_rank, oy;
      uint32_t r_y;
      if (PRE) { oy = e[k].y == RY_OUT; r_y = oy ? INV : e[k].y; }
      else { oy = e[k].y >= n_rank; r_y = ry[k]; }
      if ((ox && r_y != INV) || (oy && rx[k] != INV)) {
        atomicOr(err, ERR_RANGE);
      } else {
        lo = min(rx[k], r_y);
        hi = max(rx[k], r_y);
        if (lo != INV && pst) atomicAdd(&pst[lo], 1u);
      }
    }
    if (valid) items[idx] = ((uint64_t)hi << 32) | lo;
    uint32_t d = BINS ? bin_of(sb, nb, hi) : (hi >> shift) & (NBIN - 1);
    if (BINS && valid) digits[idx] = (uint16_t)d;  // the scatter pass reads it back
    if (plain) {  // hi bins are cut to similar record counts: few same-bin lanes per wave
      if (valid) atomicAdd(&hist[d], 1u);
    } else {
      uint64_t match = digit_match<DB>(d, valid);
      if (valid && (match & lt) == 0) atomicAdd(&hist[d], (uint32_t)__popcll(match));
    }
  }
  block_sync();
  for (uint32_t i = t; i < NBIN; i += RS_THREADS) counts[(uint64_t)blockIdx.x * NBIN + i] = hist[i];
}

// The edge pass counting hi bins (no pst; nb <= 512 bounds) into tmp (rsort_layout(m)'s counts:
// every tile writes all 512 of its counts); digits: m u16, each item's bin for bin_sort_u64.
// pre: uv holds k_part's (x, ry) records.
static void launch_edge_pass_bins(const uint32_t* uv, uint64_t m, const uint32_t* rank,
                                  uint32_t n_rank, uint64_t* items, uint32_t* err,
                                  const uint32_t* bins, uint32_t nb, uint32_t* tmp,
                                  uint16_t* digits, hipStream_t s, bool pre) {
  if (m == 0) return;
  const RsortLayout L = rsort_layout(m);
  auto k = pre ? k_edge_pass_tiles<9, true, true> : k_edge_pass_tiles<9, false, true>;
  hipLaunchKernelGGL(k, dim3((unsigned)L.ntiles), dim3(RS_THREADS), 0, s, (const uint2*)uv, m, rank,
                     n_rank, (uint32_t*)nullptr, items, err, 0, tmp + L.counts, bins, nb, digits, 1);
}

// Edge pass whose output feeds radix_sort_u64(..., bit_lo = shift, counted0 = true): tmp is
// that sort's tmp (rsort_tmp_words(m)); DB = rsort_first_width of the sorted bit range.
// pre: uv holds k_part's (x, ry) records.
void launch_edge_pass_tiles(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                            uint32_t* pst, uint64_t* items, uint32_t* err, int shift, int DB,
                            uint32_t* tmp, hipStream_t s, bool pre) {
  if (m == 0) return;
  const RsortLayout L = rsort_layout(m);
  auto k = DB > 8 ? (pre ? k_edge_pass_tiles<9, true> : k_edge_pass_tiles<9, false>)
                  : (pre ? k_edge_pass_tiles<8, true> : k_edge_pass_tiles<8, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)L.ntiles), dim3(RS_THREADS), 0, s, (const uint2*)uv, m, rank,
                     n_rank, pst, items, err, shift, tmp + L.counts, (const uint32_t*)nullptr, 0u,
                     (uint16_t*)nullptr, 0);
}

uint64_t* group_by_bins(const uint32_t* uv, bool pre, uint64_t m, const uint32_t* rank,
                        uint32_t n_rank, uint32_t* err, const uint32_t* bins, uint32_t nb,
                        uint64_t* items, uint64_t* items_b, uint32_t* tmp, uint16_t* digits,
                        unsigned long long* bin_start, hipStream_t s,
                        unsigned long long* h_start, hipEvent_t started) {
  launch_edge_pass_bins(uv, m, rank, n_rank, items, err, bins, nb, tmp, digits, s, pre);
  bin_sort_u64(items, items_b, m, nb, tmp, bin_start, digits, s, h_start, started);
  return items_b;
}

// ---------------------------------------------------------------------------------------
// Direct binning: the edge pass stores its items straight into their hi bins, so the items
// are written once and there is no scatter pass (no digits array, no tile count matrix).
// Bin b owns the capacity region [cursor0[b], cap_end[b]) of `out`, sized by the host from the
// degree estimate of its records (make_bins; the estimate is within a few % on R-MAT and
// Chung-Lu inputs); a tile reserves its run of bin b with one atomic on cursor[b] (which then
// ends at the bin's fill).  A run that would cross cap_end[b] is dropped and *ovf set: the
// caller then groups the records again through the scatter path.  Records without a tree
// item (self-loops, INVALID hi) are not stored.  Tile = NT threads x IT records, staged in LDS
// in bin order and written as whole runs per wave (as k_bin_scatter).
// ---------------------------------------------------------------------------------------
// Largest i with tb[i] <= v over a 512-entry table (entries past the used ones hold INV, and
// v < INV): nine halvings with a fixed trip count, so the searches of a thread's N values
// interleave (N LDS loads in flight per step, not one dependent chain per value).
template <int N>
__device__ __forceinline__ void search512(const uint32_t* tb, const uint32_t* v, uint32_t* idx) {
  uint32_t lo[N];
#pragma unroll
  for (int k = 0; k < N; ++k) lo[k] = 0;
#pragma unroll
  for (uint32_t half = 256; half; half >>= 1) {
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (tb[lo[k] + half] <= v[k]) lo[k] += half;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) idx[k] = lo[k];
}

// The same search over the table in Eytzinger order (et[n] = tb[probe of node n], n = 1..511;
// et_of gives the entry): the nodes probed at one depth are contiguous, so the lanes of a wave
// read distinct banks, where the sorted layout's probes at one depth lie a power of two apart
// (one bank) — k_edge_bin's bank-conflict fraction was 0.69 (round 4 counters); RMAT-26 edge
// pass 7.50 -> 6.83 ms (profiles/r05/q_fused_pipe_et/).
__device__ __forceinline__ uint32_t et_index(uint32_t n) {  // node n >= 1 -> sorted index
  const uint32_t d = 31u - __builtin_clz(n);
  return ((n - (1u << d)) << (9u - d)) + (256u >> d);
}
template <int N>
__device__ __forceinline__ void search512_et(const uint32_t* et, const uint32_t* v, uint32_t* idx) {
  uint32_t n[N];
#pragma unroll
  for (int k = 0; k < N; ++k) n[k] = 1;
#pragma unroll
  for (int d = 0; d < 9; ++d) {
#pragma unroll
    for (int k = 0; k < N; ++k) n[k] = 2 * n[k] + (et[n[k]] <= v[k] ? 1u : 0u);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) idx[k] = n[k] - 512u;
}

// The edge pass's tile map over k_part<1>'s x-digit regions [xst[d], xst[d + 1]) (exact): tiles
// of TILE records that never cross a region, so a tile knows its digit and searches nothing
// (as the second pass's map over the fused pass's regions, k_fs_tile_desc).  Each block scans
// the ND + 1 starts itself (cheap) and writes the descriptors (first position, digit << 16 |
// records) of its 256 tile slots; records 0 past the last tile.
template <uint32_t ND>
__global__ void __launch_bounds__(ND)
k_xd_tile_desc(const uint32_t* __restrict__ xst, uint32_t TILE, uint64_t nt, uint2* __restrict__ desc) {
  static_assert(ND == 256, "one thread per digit");
  __shared__ uint32_t toff[ND + 1], wsum[ND / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint32_t n = xst[t + 1] - xst[t], c = (n + TILE - 1) / TILE;
  const uint32_t incl = wave_incl_scan(c);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t add = 0, tot = 0;
  for (int i = 0; i < (int)(ND / 64); ++i) { if (i < w) add += wsum[i]; tot += wsum[i]; }
  toff[t] = add + incl - c;
  if (t == 0) toff[ND] = tot;
  block_sync();
  const uint64_t j = (uint64_t)blockIdx.x * ND + t;
  if (j >= nt) return;
  if (j >= tot) {
    desc[j] = make_uint2(0u, 0u);
    return;
  }
  uint32_t lo = 0, cnt = ND;  // the last d with toff[d] <= j
  while (cnt > 0) {
    const uint32_t h = cnt >> 1;
    if (toff[lo + h] <= (uint32_t)j) { lo += h + 1; cnt -= h + 1; } else cnt = h;
  }
  const uint32_t d = lo - 1, k = (uint32_t)j - toff[d];
  const uint32_t p0 = xst[d] + k * TILE;
  desc[j] = make_uint2(p0, (d << 16) | min(TILE, xst[d + 1] - p0));
}

// IN6 (with PRE): the records are k_part<1>'s packed output; x's digit comes from the tile map
// (tdesc, k_xd_tile_desc over the x-digit region starts; shx: the digit shift).
// PK (every rank < 2^26): a staged slot holds bin << 52 | hi << 26 | lo, so the write-out reads
// its bin instead of searching the tile's run starts for it.
template <bool PRE, int NT, int IT, bool IN6 = false, bool PK = false>
__global__ void __launch_bounds__(NT)
k_edge_bin(const uint2* __restrict__ uv, uint64_t m, const uint32_t* __restrict__ rank,
           uint32_t n_rank, uint32_t* err, const uint32_t* __restrict__ bins, uint32_t nb,
           unsigned long long* cursor, const unsigned long long* __restrict__ cap_end,
           uint64_t* __restrict__ out, uint32_t* ovf, const uint2* __restrict__ tdesc, int shx) {
  static_assert(NT >= 512, "one thread per bin in the scan");
  static_assert(!IN6 || PRE, "packed records are second-pass records");
  constexpr int TILE = NT * IT;
  __shared__ uint64_t stage[TILE];
  __shared__ uint32_t hist[512], tstart[512], sb[512], wsum[NT / 64];
  __shared__ unsigned long long gbase[512];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint64_t tbase;
  uint32_t tile_n, tdig = 0;
  if (IN6) {  // one x-digit region's tile
    const uint2 dsc = tdesc[blockIdx.x];
    tbase = dsc.x;
    tile_n = dsc.y & 0xFFFFu;
    tdig = dsc.y >> 16;
    if (tile_n == 0) return;  // (the grid covers the largest tile count)
  } else {
    tbase = (uint64_t)blockIdx.x * TILE;
    tile_n = (uint32_t)min((uint64_t)TILE, m - tbase);
  }
  if (t < 512) {
    hist[t] = 0;
    const uint32_t i = t ? et_index(t) : 0u;  // Eytzinger order (search512_et; sb[0] unused)
    sb[t] = i < nb ? bins[i] : INV;            // padded
  }
  uint2 e[IT];
  uint32_t rx[IT], ry[IT];
  if (IN6) {
    const P6Ref pin = p6_in(uv, m);
    const int xh = shx > 16 ? shx - 16 : 0;
    uint32_t ea[IT];
    uint16_t eb[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      ea[k] = j < tile_n ? pin.a[tbase + j] : 0u;
      eb[k] = j < tile_n ? pin.b[tbase + j] : (uint16_t)0;
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      const uint32_t xlo = ((ea[k] & ((1u << xh) - 1u)) << 16) | eb[k];
      const uint32_t x = (tdig << shx) | xlo;
      e[k] = j < tile_n ? make_uint2(x, p6_ry_dec(ea[k] >> xh, xh)) : make_uint2(0, RY_SELF);
    }
  } else {
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      e[k] = j < tile_n ? uv[tbase + j] : make_uint2(0, PRE ? RY_SELF : 0u);
    }
  }
#pragma unroll
  for (int k = 0; k < IT; ++k) {  // every gather issued before any is used
    if (PRE) {
      rx[k] = (e[k].y != RY_SELF && e[k].x < n_rank) ? rank[e[k].x] : INV;
    } else {
      const bool g = e[k].x != e[k].y;
      rx[k] = (g && e[k].x < n_rank) ? rank[e[k].x] : INV;
      ry[k] = (g && e[k].y < n_rank) ? rank[e[k].y] : INV;
    }
  }
  block_sync();
  uint64_t item[IT];
  uint32_t hiv[IT], pk[IT];  // pk: bin << 16 | index within the tile's run of the bin; ~0u: not stored
#pragma unroll
  for (int k = 0; k < IT; ++k) {
    const bool loop = PRE ? e[k].y == RY_SELF : e[k].x == e[k].y;
    uint32_t hi = INV, lo = INV;
    if ((uint32_t)k * NT + t < tile_n && !loop) {  // insert's edge loop, jtree.cpp:73-90
      const bool ox = e[k].x >= n_rank;
      bool oy;
      uint32_t r_y;
      if (PRE) { oy = e[k].y == RY_OUT; r_y = oy ? INV : e[k].y; }
      else { oy = e[k].y >= n_rank; r_y = ry[k]; }
      if ((ox && r_y != INV) || (oy && rx[k] != INV)) {
        atomicOr(err, ERR_RANGE);
      } else {
        lo = min(rx[k], r_y);
        hi = max(rx[k], r_y);
      }
    }
    item[k] = ((uint64_t)hi << 32) | lo;
    hiv[k] = hi == INV ? 0u : hi;  // searched anyway (no divergence), not stored
  }
  search512_et<IT>(sb, hiv, pk);
#pragma unroll
  for (int k = 0; k < IT; ++k)
    pk[k] = (uint32_t)(item[k] >> 32) != INV ? (pk[k] << 16) | atomicAdd(&hist[pk[k]], 1u) : ~0u;
  block_sync();
  if (t < 512) {
    const uint32_t c = hist[t];
    const uint32_t incl = wave_incl_scan(c);
    if (lane == 63) wsum[w] = incl;
    tstart[t] = incl - c;
    unsigned long long g = ~0ull;
    if (c) {
      g = atomicAdd(&cursor[t], (unsigned long long)c);
      if (g + c > cap_end[t]) {
        atomicOr(ovf, 1u);
        g = ~0ull;
      }
    }
    gbase[t] = g;
  }
  block_sync();
  if (t < 512) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
    tstart[t] += add;
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < IT; ++k)
    if (pk[k] != ~0u) {
      const uint64_t v = PK ? ((uint64_t)(pk[k] >> 16) << 52) | ((item[k] >> 32) << 26) |
                                  (uint32_t)item[k]
                            : item[k];
      stage[tstart[pk[k] >> 16] + (pk[k] & 0xFFFFu)] = v;
    }
  block_sync();
  // The staged tile in bin order, written with every lane busy: slot j belongs to the last bin
  // whose start is <= j (empty bins share their start with the next one).  (One wave per bin
  // run left 3/4 of the lanes idle on ~16-item runs: 2x the LDS and store instructions.)
  const uint32_t n_st = tstart[511] + hist[511];
  for (uint32_t j = t; j < n_st; j += NT) {
    uint32_t d;
    uint64_t v = stage[j];
    if (PK) {
      d = (uint32_t)(v >> 52);
      v = (((v >> 26) & 0x3FFFFFFull) << 32) | (v & 0x3FFFFFFull);
    } else {
      search512<1>(tstart, &j, &d);
    }
    const unsigned long long g = gbase[d];
    if (g != ~0ull) out[g + (j - tstart[d])] = v;
  }
}

void launch_edge_bin(const uint32_t* uv, bool pre, uint64_t m, const uint32_t* rank,
                     uint32_t n_rank, uint32_t* err, const uint32_t* bins, uint32_t nb,
                     unsigned long long* cursor, const unsigned long long* cap_end, uint64_t* out,
                     uint32_t* ovf, hipStream_t s, const uint32_t* part_ws) {
  if (m == 0) return;
  // 8192-record tiles, 64 KB stage: two blocks of 16 waves per CU (RMAT-26 edge phase: 512 x
  // 16 -> 8.9 ms, 1024 x 16 -> 10.8, 512 x 8 -> 8.5, 1024 x 8 -> 7.8)
  constexpr int NT = 1024, IT = 8;
  unsigned nt = (unsigned)((m + NT * IT - 1) / (NT * IT));
  const bool in6 = pre && part_ws;
  const bool pk = n_rank <= (1u << 26);  // ranks < n_seq <= n_rank
  uint2* desc = nullptr;
  if (in6) {
    // the tile map over the x-digit regions (round 6: a tile no longer searches its digits),
    // its descriptors in the spare 2 B per record behind the packed records (uv holds 8 B each)
    nt += PD_X;  // >= the tiles (one partial tile per region)
    desc = (uint2*)((char*)uv + 6 * ((m + 3) & ~3ull));
    hipLaunchKernelGGL(k_xd_tile_desc<PD_X>, dim3((nt + PD_X - 1) / PD_X), dim3(PD_X), 0, s,
                       (const uint32_t*)(part_ws + PW_XST), (uint32_t)(NT * IT), (uint64_t)nt, desc);
  }
  auto k = in6 ? (pk ? k_edge_bin<true, NT, IT, true, true> : k_edge_bin<true, NT, IT, true>)
       : pre   ? (pk ? k_edge_bin<true, NT, IT, false, true> : k_edge_bin<true, NT, IT>)
               : (pk ? k_edge_bin<false, NT, IT, false, true> : k_edge_bin<false, NT, IT>);
  hipLaunchKernelGGL(k, dim3(nt), dim3(NT), 0, s, (const uint2*)uv, m, rank, n_rank, err, bins, nb,
                     cursor, cap_end, out, ovf, (const uint2*)desc, part_shift(n_rank, PD_X));
}

// ---------------------------------------------------------------------------------------
// Partitioned rank gathers.  rank[] (4 B per id, 268 MB at RMAT-26) is far beyond L2 and the
// stream evicts it from the Infinity Cache: gathered in stream order, every lookup is a 64-B
// HBM access (~60 G lookups/s, 2 per record).  Partitioned by the looked-up id's top 8 bits,
// the records of one tile look up one 1 MB slice: 3x faster per lookup (measured), for one
// partition pass (8 B read + 8 B written per record).  So:
//   k_part<0>: records (x, y) partitioned by y's digit;                 (x-digit histogram)
//   k_part<1>: ... gather ry = rank[y] and partition (x, ry) by x's digit;
//   k_edge_pass_tiles<PRE>: gather rank[x] in x-digit order.
// Order inside a digit is not kept (tiles reserve their runs with one atomic per digit):
// nothing downstream depends on record order.  Digit = min(id >> sh, 255).
// ---------------------------------------------------------------------------------------
static constexpr int PT_THREADS = 1024;
static constexpr int PT_ITEMS = 16;
// k_part<MODE, NT> tiles are NT * PT_ITEMS records (8 B each staged in LDS): the first pass
// uses 1024 threads (16384 records, 128 KB: one block per CU, which leaves room beside it for
// the degree kernels it overlaps); the second runs alone and uses 512 (8192 records, 64 KB:
// two blocks per CU, so one streams while the other is between barriers; RMAT-26 7.7 -> 6.3 ms).
static constexpr int PT0_THREADS = 1024, PT1_THREADS = 512;
static constexpr int PT0_ITEMS = PT_ITEMS, PT1_ITEMS = PT_ITEMS;


// Global histogram of the y digits (the first partition's run sizes).
__global__ void __launch_bounds__(PT_THREADS)
k_part_count(const uint2* __restrict__ uv, uint64_t m, int sh, uint32_t* __restrict__ ghist) {
  __shared__ uint32_t hist[PD_Y];
  for (uint32_t i = threadIdx.x; i < PD_Y; i += PT_THREADS) hist[i] = 0;
  block_sync();
  for (uint64_t i = (uint64_t)blockIdx.x * PT_THREADS + threadIdx.x; i < m;
       i += (uint64_t)gridDim.x * PT_THREADS)
    atomicAdd(&hist[part_digit<PD_Y>(uv[i].y, sh)], 1u);
  block_sync();
  for (uint32_t i = threadIdx.x; i < PD_Y; i += PT_THREADS)
    if (hist[i]) atomicAdd(&ghist[i], hist[i]);
}

// cursor[d] = exclusive prefix of hist (one block of ND threads); hist is then cleared.
// starts (nullable): the same prefix as u32, ND + 1 entries (the last = the total) — the digit
// regions of this pass's output, which a packed (P6) reader needs to restore the digit bits.
template <uint32_t ND, bool XH = false /* hist spread as the x-digit counts (xh_ix) */>
__global__ void k_part_cursor(uint32_t* hist, unsigned long long* cursor, uint32_t* starts) {
  __shared__ unsigned long long s[ND + 1];
  uint32_t t = threadIdx.x;
  const uint32_t ht = XH ? xh_ix(t) : t;
  s[t] = hist[ht];
  block_sync();
  if (t == 0) {
    unsigned long long run = 0;
    for (uint32_t i = 0; i < ND; ++i) { unsigned long long v = s[i]; s[i] = run; run += v; }
    s[ND] = run;
  }
  block_sync();
  cursor[t] = s[t];
  if (starts) {
    starts[t] = (uint32_t)s[t];
    if (t == 0) starts[ND] = (uint32_t)s[ND];
  }
  hist[ht] = 0;
}

// The second pass's tile map over the fused front pass's y subregions (k_front_fused): the
// filled part of subregion q, [st[q], min(cur[q], cap[q])), is cut into tiles of TILE records,
// so that no tile crosses a subregion (the unwritten slack between subregions is never read,
// and a tile's y digit is its subregion's, q / G).  k_fs_tile_scan (one block): toff[q] = the
// first tile of subregion q, toff[S] = the tiles.  k_fs_tile_desc (one thread per tile slot of
// the launch, nt of them): desc[j] = (first position, digit << 16 | records), records 0 past
// the last tile.
__global__ void __launch_bounds__(1024)
k_fs_tile_scan(const unsigned long long* __restrict__ st, const unsigned long long* __restrict__ cur,
               const unsigned long long* __restrict__ cap, uint32_t S, uint32_t TILE,
               uint32_t* __restrict__ toff) {
  __shared__ uint32_t wsum[16];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  constexpr uint32_t PER = FS_MAX / 1024;  // subregions per thread
  uint32_t nt[PER], sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < PER; ++i) {
    const uint32_t q = t * PER + i;
    nt[i] = 0;
    if (q < S) {
      const unsigned long long f = min(cur[fs_cix(q)], cap[q]);
      const uint64_t n = f > st[q] ? f - st[q] : 0;
      nt[i] = (uint32_t)((n + TILE - 1) / TILE);
    }
    sum += nt[i];
  }
  const uint32_t incl = wave_incl_scan(sum);
  if (lane == 63) wsum[w] = incl;
  block_sync();
  uint32_t run = incl - sum, tot = 0;
  for (int i = 0; i < 16; ++i) { if (i < w) run += wsum[i]; tot += wsum[i]; }
#pragma unroll
  for (uint32_t i = 0; i < PER; ++i) {
    const uint32_t q = t * PER + i;
    if (q < S) toff[q] = run;
    run += nt[i];
  }
  if (t == 0) toff[S] = tot;
}

__global__ void __launch_bounds__(256)
k_fs_tile_desc(const unsigned long long* __restrict__ st, const unsigned long long* __restrict__ cur,
               const unsigned long long* __restrict__ cap, const uint32_t* __restrict__ toff,
               uint32_t S, uint32_t G, uint32_t TILE, uint64_t nt, uint2* __restrict__ desc) {
  const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= nt) return;
  if (j >= toff[S]) {
    desc[j] = make_uint2(0u, 0u);
    return;
  }
  uint32_t lo = 0, cnt = S;  // the last q with toff[q] <= j (toff[0] = 0)
  while (cnt > 0) {
    const uint32_t h = cnt >> 1;
    if (toff[lo + h] <= (uint32_t)j) { lo += h + 1; cnt -= h + 1; } else cnt = h;
  }
  const uint32_t q = lo - 1;
  const uint64_t k = j - toff[q], p0 = st[q] + k * TILE, f = min(cur[fs_cix(q)], cap[q]);
  const uint32_t n = (uint32_t)min((uint64_t)TILE, f - p0);
  desc[j] = make_uint2((uint32_t)p0, ((q / G) << 16) | n);
}

// ND: digits of this pass (PD_Y for MODE 0, PD_X for MODE 1), ND / NT per thread in the scan.
// MODE 0 also counts the x digits (PD_X) of the second pass into xhist.
// in, m: the input and its positions.  REG (MODE 1): the input lies in the first pass's
// capacity regions (starts in_starts, which end at in_starts[PD_Y]); a position counts only
// below its region's fill (in_fill, capped at in_cap).  OUT6 (MODE 1): the output is written
// as packed 6-byte records, m_out of them.  cap_end / ovf (nullable, MODE 0): capacity regions —
// a run past its digit's end keeps the part that fits and sets *ovf.
// (Packing the first pass's records too measured no faster: 44.96 vs 44.99 ms at RMAT-26 —
// its 16-record runs became 64- and 32-byte runs, written at 1.6x their bytes.)
template <int MODE, int NT, int IT, uint32_t ND, bool OUT6 = false, bool REG = false,
          bool IN6 = false>
__global__ void __launch_bounds__(NT)
k_part(const uint64_t* __restrict__ in, uint64_t m, uint64_t* __restrict__ out, uint64_t m_out,
       unsigned long long* __restrict__ cursor, uint32_t* __restrict__ xhist, int sh, int shx,
       const uint32_t* __restrict__ rank, uint32_t n_rank, int ysh,
       const uint32_t* __restrict__ in_starts, int ish,
       const unsigned long long* __restrict__ in_fill, const unsigned long long* __restrict__ in_cap,
       const unsigned long long* __restrict__ cap_end, uint32_t* ovf,
       const uint2* __restrict__ tdesc = nullptr /* IN6: the tile map (k_fs_tile_desc) */) {
  static_assert(ND % NT == 0 || NT % ND == 0, "digits per thread");
  static_assert(!REG || MODE == 1, "capacity-region input: the second pass only");
  static_assert(!OUT6 || MODE == 1, "packed output: the second pass only");
  static_assert(IT <= 32, "validity mask");
  static_assert(!IN6 || REG, "packed input: the fused pass's capacity regions");
  constexpr bool RG = REG;
  constexpr int R = ND > (uint32_t)NT ? (int)ND / NT : 1;  // digits per thread in the scan
  constexpr int PT_ITEMS = IT;
  constexpr int TILE = NT * PT_ITEMS;
  __shared__ uint64_t stage[TILE];
  __shared__ uint32_t hist[ND], tstart[ND], hx[MODE == 0 ? PD_X : 1], wsum[NT / 64];
  __shared__ unsigned long long gbase[ND], gcap[MODE == 0 ? ND : 1];
  __shared__ uint32_t sst[RG && !IN6 ? PD_Y + 2 : 1], sfill[RG && !IN6 ? PD_Y : 1], s_nv;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint64_t tbase;
  uint32_t tile_n, tdig = 0;
  if constexpr (IN6) {  // one subregion's tile: (first position, y digit << 16 | records)
    const uint2 dsc = tdesc[blockIdx.x];
    tbase = dsc.x;
    tile_n = dsc.y & 0xFFFFu;
    tdig = dsc.y >> 16;
    if (tile_n == 0) return;  // (the grid covers the largest tile count)
  } else {
    tbase = (uint64_t)blockIdx.x * TILE;
    const uint64_t lim = RG ? min(m, (uint64_t)in_starts[PD_Y]) : m;
    if (tbase >= lim) return;  // (the grid covers m slots; the regions may end earlier)
    tile_n = (uint32_t)min((uint64_t)TILE, lim - tbase);
  }
  for (uint32_t i = t; i < ND; i += NT) hist[i] = 0;
  if (MODE == 0)
    for (uint32_t i = t; i < PD_X; i += NT) hx[i] = 0;
  uint64_t rec[PT_ITEMS];
  uint32_t li[PT_ITEMS];
  uint32_t vm = 0;  // bit k: item k is a record
  if constexpr (IN6) {
    // the fused front pass's packed records (k_front_fused): x from the u32 array, y's low bits
    // from the u16 array after it (m positions each), y's digit from the tile's subregion
    const uint32_t* ia = (const uint32_t*)in;
    const uint16_t* ib = (const uint16_t*)(ia + m);
    uint16_t yb[PT_ITEMS];
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      rec[k] = j < tile_n ? ia[tbase + j] : 0u;
      yb[k] = j < tile_n ? ib[tbase + j] : (uint16_t)0;
    }
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      vm |= (uint32_t)(j < tile_n) << k;
      rec[k] |= (uint64_t)((tdig << ish) | yb[k]) << 32;
    }
  } else if constexpr (REG) {
    // the first pass's capacity regions (launch_part_first_caps): y's digit from the region
    // starts, positions past a region's fill masked
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      rec[k] = j < tile_n ? in[tbase + j] : 0ull;
    }
    tile_regions<PD_Y>(in_starts, tbase, tile_n, sst);  // (the loads above are in flight)
    const uint32_t d0 = sst[0];
    for (uint32_t i = t; i <= sst[1] - d0; i += NT) {
      const unsigned long long f = in_fill[d0 + i], c = in_cap ? in_cap[d0 + i] : f;
      sfill[i] = (uint32_t)min(f, c);
    }
    block_sync();
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      const uint64_t pos = tbase + min(j, tile_n - 1);
      const uint32_t d = tile_digit(sst, pos);
      vm |= (uint32_t)(j < tile_n && pos < sfill[d - d0]) << k;
    }
  } else {
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      uint32_t j = (uint32_t)k * NT + t;
      rec[k] = j < tile_n ? in[tbase + j] : 0ull;
      vm |= (uint32_t)(j < tile_n) << k;
    }
  }
  if (MODE == 1 && ysh >= 0) {
    // The tile in y order first, by 256 sub-ranges of its y digit (counting sort in LDS): the
    // 64 gathers of a wave then fall in a few 256-id sub-ranges and share cache lines, where
    // in stream order each is an L2 request of its own (the pass is bound by those requests).
    static_assert(MODE != 1 || ND == 256, "sub-ranges use the x-digit arrays");
    block_sync();
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k)
      if ((vm >> k) & 1) li[k] = atomicAdd(&hist[(uint32_t)(rec[k] >> (32 + ysh)) & 255u], 1u);
    block_sync();
    if (t < 256) {
      const uint32_t c = hist[t], incl = wave_incl_scan(c);
      if (lane == 63) wsum[w] = incl;
      tstart[t] = incl - c;
    }
    block_sync();
    if (t < 256) {
      uint32_t add = 0;
      for (int i = 0; i < w; ++i) add += wsum[i];
      tstart[t] += add;
      if (t == 255) s_nv = tstart[t] + hist[t];
      hist[t] = 0;
    }
    block_sync();
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k)
      if ((vm >> k) & 1)
        stage[tstart[(uint32_t)(rec[k] >> (32 + ysh)) & 255u] + li[k]] = rec[k];
    block_sync();
    const uint32_t n_valid = s_nv;
    vm = 0;
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      const uint32_t j = (uint32_t)k * NT + t;
      rec[k] = j < n_valid ? stage[j] : 0ull;
      vm |= (uint32_t)(j < n_valid) << k;
    }
  }
  if (MODE == 1) {  // (x, y) -> (x, ry)
    uint32_t ry[PT_ITEMS];
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      uint32_t x = (uint32_t)rec[k], y = (uint32_t)(rec[k] >> 32);
      ry[k] = (x != y && y < n_rank) ? rank[y] : INV;
    }
#pragma unroll
    for (int k = 0; k < PT_ITEMS; ++k) {
      uint32_t x = (uint32_t)rec[k], y = (uint32_t)(rec[k] >> 32);
      uint32_t v = x == y ? RY_SELF : (y >= n_rank ? RY_OUT : ry[k]);
      rec[k] = ((uint64_t)v << 32) | x;
    }
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < PT_ITEMS; ++k) {
    if ((vm >> k) & 1) {
      uint32_t key = MODE == 0 ? (uint32_t)(rec[k] >> 32) : (uint32_t)rec[k];
      li[k] = atomicAdd(&hist[part_digit<ND>(key, sh)], 1u);
      if (MODE == 0) atomicAdd(&hx[part_digit<PD_X>((uint32_t)rec[k], shx)], 1u);
    }
  }
  block_sync();
  if (t * R < (int)ND) {  // digits [t R, t R + R): exclusive starts in the tile, global runs
    uint32_t c[R], sum = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) { c[r] = hist[t * R + r]; sum += c[r]; }
    const uint32_t incl = wave_incl_scan(sum);
    if (lane == 63) wsum[w] = incl;
    uint32_t run = incl - sum;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t d = t * R + r;
      tstart[d] = run;
      run += c[r];
      const unsigned long long g = c[r] ? atomicAdd(&cursor[d], (unsigned long long)c[r]) : 0ull;
      if (MODE == 0) {
        // capacity regions: a run past its digit's end keeps the part that fits (no unwritten
        // hole below the region's end, which the second pass reads up to) and flags the pass
        const unsigned long long ce = cap_end ? cap_end[d] : ~0ull;
        if (c[r] && g + c[r] > ce) atomicOr(ovf, 1u);
        gcap[d] = ce;
      }
      gbase[d] = g;
    }
  }
  if (MODE == 0)
    for (uint32_t i = t; i < PD_X; i += NT)
      if (hx[i]) atomicAdd(&xhist[xh_ix(i)], hx[i]);
  block_sync();
  if (t * R < (int)ND) {
    uint32_t add = 0;
    for (int i = 0; i < w; ++i) add += wsum[i];
#pragma unroll
    for (int r = 0; r < R; ++r) tstart[t * R + r] += add;
  }
  block_sync();
#pragma unroll
  for (int k = 0; k < PT_ITEMS; ++k) {
    if ((vm >> k) & 1) {
      uint32_t key = MODE == 0 ? (uint32_t)(rec[k] >> 32) : (uint32_t)rec[k];
      stage[tstart[part_digit<ND>(key, sh)] + li[k]] = rec[k];
    }
  }
  block_sync();
  uint32_t* oa = (uint32_t*)out;
  uint16_t* ob = (uint16_t*)((char*)out + 4 * m_out);
  const int xh = shx > 16 ? shx - 16 : 0;  // MODE 1, OUT6: x bits above the u16 half
  const uint32_t n_st = tstart[ND - 1] + hist[ND - 1];  // the staged records
  for (uint32_t j = t; j < n_st; j += NT) {
    uint64_t r = stage[j];
    uint32_t d = part_digit<ND>(MODE == 0 ? (uint32_t)(r >> 32) : (uint32_t)r, sh);
    const uint64_t pos = gbase[d] + (j - tstart[d]);
    if (MODE == 0 && pos >= gcap[d]) continue;  // past the capacity region (flagged above)
    if (!OUT6) {
      out[pos] = r;
    } else {  // a = ry' << xh | x_lo >> 16, b = x_lo & 0xFFFF
      // (masked: an id >= n_rank, clamped to the last digit, must not spill into ry's bits)
      const uint32_t xlo = ((uint32_t)r - (d << sh)) & ((1u << sh) - 1u);
      oa[pos] = (p6_ry_enc((uint32_t)(r >> 32), xh) << xh) | (xlo >> 16);
      ob[pos] = (uint16_t)(xlo & 0xFFFFu);
    }
  }
}

// Whether the partition passes may use packed records: every digit region's low bits fit.
bool part_p6_ok(uint32_t n_rank) {
  return n_rank > 0 && part_shift(n_rank, PD_Y) <= 16 && part_shift(n_rank, PD_X) <= 18;
}

// uv (x, y) -> pre (x, ry) in x-digit order, via mid (y-digit order).  ws: PART_WS_WORDS.
void launch_part_first(const uint32_t* uv, uint64_t m, uint32_t n_rank, uint64_t* mid,
                       uint32_t* ws, hipStream_t s, bool yhist_ready) {
  if (m == 0) return;
  const int sh = part_shift(n_rank, PD_Y), shx = part_shift(n_rank, PD_X);
  uint32_t* yhist = ws;
  uint32_t* xhist = ws + PW_XH;
  unsigned long long* cursor = (unsigned long long*)(ws + PW_CUR);
  (void)hipMemsetAsync(xhist, 0, XH_WORDS * 4, s);
  if (!yhist_ready) {  // (else counted by the degree pass, launch_degree_bucketed)
    (void)hipMemsetAsync(ws, 0, PD_Y * 4, s);
    hipLaunchKernelGGL(k_part_count, dim3(1024), dim3(PT_THREADS), 0, s, (const uint2*)uv, m, sh, yhist);
  }
  hipLaunchKernelGGL(k_part_cursor<PD_Y>, dim3(1), dim3(PD_Y), 0, s, yhist, cursor, ws + PW_YST);
  uint64_t nt = (m + PT0_THREADS * PT0_ITEMS - 1) / (PT0_THREADS * PT0_ITEMS);
  hipLaunchKernelGGL((k_part<0, PT0_THREADS, PT0_ITEMS, PD_Y>), dim3((unsigned)nt), dim3(PT0_THREADS),
                     0, s, (const uint64_t*)uv, m, mid, m,
                     cursor, xhist, sh, shx, (const uint32_t*)nullptr, n_rank, -1,
                     (const uint32_t*)nullptr, 0, (const unsigned long long*)nullptr,
                     (const unsigned long long*)nullptr, (const unsigned long long*)nullptr,
                     (uint32_t*)nullptr);
}

// The first pass into the capacity regions launch_degree_sampled left in ws (mid_slots records
// in mid); a run past its region's end keeps what fits and sets *ovf.
void launch_part_first_caps(const uint32_t* uv, uint64_t m, uint32_t n_rank, uint64_t* mid,
                            uint64_t mid_slots, uint32_t* ws, uint32_t* ovf, hipStream_t s) {
  if (m == 0) return;
  const int sh = part_shift(n_rank, PD_Y), shx = part_shift(n_rank, PD_X);
  (void)hipMemsetAsync(ws + PW_XH, 0, XH_WORDS * 4, s);
  uint64_t nt = (m + PT0_THREADS * PT0_ITEMS - 1) / (PT0_THREADS * PT0_ITEMS);
  hipLaunchKernelGGL((k_part<0, PT0_THREADS, PT0_ITEMS, PD_Y>), dim3((unsigned)nt),
                     dim3(PT0_THREADS), 0, s, (const uint64_t*)uv, m, mid, mid_slots,
                     (unsigned long long*)(ws + PW_CUR), ws + PW_XH, sh, shx, (const uint32_t*)nullptr,
                     n_rank, -1, (const uint32_t*)nullptr, 0, (const unsigned long long*)nullptr,
                     (const unsigned long long*)nullptr,
                     (const unsigned long long*)(ws + PW_YCAP), ovf);
}

// caps: mid holds the first pass's capacity regions (mid_slots positions); out6: pre is written
// packed.
void launch_part_second(const uint64_t* mid, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                        uint64_t* pre, uint32_t* ws, hipStream_t s, bool out6, uint64_t mid_slots,
                        bool caps, bool in6, uint32_t G) {
  if (m == 0) return;
  const int sh = part_shift(n_rank, PD_Y), shx = part_shift(n_rank, PD_X);
  const int ysh = std::max(sh - 8, 0);
  uint32_t* xhist = ws + PW_XH;
  unsigned long long* cursor = (unsigned long long*)(ws + PW_XCUR);
  hipLaunchKernelGGL((k_part_cursor<PD_X, true>), dim3(1), dim3(PD_X), 0, s, xhist, cursor, ws + PW_XST);
  constexpr uint32_t TILE = PT1_THREADS * PT1_ITEMS;
  if (caps && in6) {
    // the fused pass's subregions (launch_front_fused: ws's PW_F* tables, G per y digit): the
    // tile map, its descriptors in the spare 2 B per slot behind the packed records
    int SH;
    uint32_t NB;
    if (!degb_params(n_rank, &SH, &NB)) NB = DEGB_NB;
    G = std::max<uint32_t>(1, std::min(G, FF_GMAX));
    const uint32_t S = NB * G;
    const unsigned long long* fst = (const unsigned long long*)(ws + PW_FST);
    const unsigned long long* fcur = (const unsigned long long*)(ws + PW_FCUR);
    const unsigned long long* fcap = (const unsigned long long*)(ws + PW_FCAP);
    uint32_t* toff = ws + PW_FTOFF;
    const uint64_t nt = mid_slots / TILE + S + 1;  // >= the tiles (one partial tile per subregion)
    uint2* desc = (uint2*)((char*)mid + 6 * mid_slots);  // (mid holds 8 B per slot)
    hipLaunchKernelGGL(k_fs_tile_scan, dim3(1), dim3(1024), 0, s, fst, fcur, fcap, S, TILE, toff);
    hipLaunchKernelGGL(k_fs_tile_desc, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, fst, fcur,
                       fcap, (const uint32_t*)toff, S, G, TILE, nt, desc);
    auto k = out6 ? k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, true, true, true>
                  : k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, false, true, true>;
    hipLaunchKernelGGL(k, dim3((unsigned)nt), dim3(PT1_THREADS), 0, s, mid, mid_slots, pre, m, cursor,
                       xhist, shx, shx, rank, n_rank, ysh, (const uint32_t*)nullptr, sh,
                       (const unsigned long long*)nullptr, (const unsigned long long*)nullptr,
                       (const unsigned long long*)nullptr, (uint32_t*)nullptr, (const uint2*)desc);
    return;
  }
  const uint64_t pos = caps && mid_slots ? mid_slots : m;
  uint64_t nt = (pos + TILE - 1) / TILE;
  auto k = caps ? (out6 ? k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, true, true>
                        : k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, false, true>)
                : (out6 ? k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, true>
                        : k_part<1, PT1_THREADS, PT1_ITEMS, PD_X, false>);
  hipLaunchKernelGGL(k, dim3((unsigned)nt), dim3(PT1_THREADS), 0, s, mid, pos, pre, m, cursor, xhist,
                     shx, shx, rank, n_rank, ysh, (const uint32_t*)(ws + PW_YST), sh,
                     (const unsigned long long*)(ws + PW_CUR),
                     caps ? (const unsigned long long*)(ws + PW_YCAP) : (const unsigned long long*)nullptr,
                     (const unsigned long long*)nullptr, (uint32_t*)nullptr, (const uint2*)nullptr);
}

void launch_part_gather(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_rank,
                        uint64_t* mid, uint64_t* pre, uint32_t* ws, hipStream_t s,
                        bool yhist_ready, bool p6) {
  launch_part_first(uv, m, n_rank, mid, ws, s, yhist_ready);
  launch_part_second(mid, m, rank, n_rank, pre, ws, s, p6, m, false, false);
}

// ---------------------------------------------------------------------------------------
// Lock-free elimination-tree insertion.
//
// State: parent[] is a heap-ordered forest (parent > child, INVALID = root) and a set of
// pending edges.  Invariant: etree(parent-forest ∪ pending) = etree(all edges inserted so
// far).  Inserting pending edge (a, b), a < b:
//   walk up from a to a vertex x < b whose parent p is >= b (or INVALID);
//     p == b       -> a already hangs below b: drop the edge;
//     p == INVALID -> CAS parent[x]: INVALID -> b, done;
//     p >  b       -> CAS parent[x]: p -> b, then insert pending (b, p)  ("zipper" step).
// Each step is one CAS on one word and preserves the threshold-connectivity of the graph at
// every rank, hence the etree (SURVEY §7 "Hard parts" fact 3).  A failed CAS returns the
// current value and the walk resumes from it.  parent values only ever decrease, so a stale
// (L2-cached) read is always a former ancestor: walking to it is still valid, and CASing on it
// fails and refreshes.  jump[] is a hint array of former ancestors (path splitting) that only
// accelerates the walk.  When no edge is pending the forest is the etree of every inserted
// edge — the same unique result as Liu's sequential union-find (jtree.cpp:73-83,
// unionfind.h:46-102), independent of insertion order and interleaving.
// ---------------------------------------------------------------------------------------
// Parent loads: relaxed agent-scope atomic loads (global_load sc1: bypasses L1, L2 served).
// Staleness never breaks correctness (see above), only costs extra CAS round trips.  (System-scope
// loads and a returning atomic OR 0, performed at memory and always fresh, were the alternatives.)
__device__ __forceinline__ uint32_t ld_parent(uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct ZState {
  uint32_t a, b, x, prev, p;
  uint32_t flags;  // ZF_* (kb spine mode only)
  bool fresh;
};

// ZState flags.  ZF_KEEP: the pending edge may carry a marked rank's connection to G — a
// giant-path edge (G, b) from the spine queue, or any zipper continuation (b, p), which takes
// over the forest edge (x, p) it displaced — so the redundancy rule below must not drop it
// (only edges that have not yet changed the forest are dropped).  ZF_SPINE: the walk of the
// current pending edge has reached the spine (checked once per pending edge).
constexpr uint32_t ZF_KEEP = 1u, ZF_SPINE = 2u, ZF_LINKED = 4u;
// A kept pair written as (hi, lo) = (r, b) with r < b is finished: k_kb_refresh linked the
// pre-bucket root of union-find root r below the bucket rank b (every real pair has its hi end
// above its lo end: the zipper skips these, k_kb_union unions r with b).  INVALID hi: dropped.

struct ZCount {
  uint32_t steps = 0, cas = 0, fail = 0;
  uint32_t root = 0, one = 0;  // (STATS) edges starting below B0; edges done in one step
};

// One step of the insertion of pending edge (s.a, s.b); returns true when it is finished.
struct ZRec {  // where to record pre-bucket roots (x < B0) that a CAS links for the first time
  uint32_t B0 = 0;
  uint32_t* linked = nullptr;
  uint32_t* n_linked = nullptr;
  // block-local staging (LDS): appends reserve here with LDS atomics and the block
  // flushes once at its end (zip_flush_linked) — one global counter hit by every wave at
  // every step serialises (~88 returning atomics per microsecond on one word)
  uint32_t* lbuf = nullptr;
  uint32_t* lcnt = nullptr;
  uint32_t lcap = 0;

};

// The giant's spine inside a kb bucket [B0, B1).  G is the elimination-tree root of the
// component of rank B0 - 1 (in a degree-ordered sequence: the giant); bitmap marks the ranks
// of the bucket that have an edge to G's component.  The ancestors of G in the final etree
// (its spine) form one chain and contain G and every marked rank.  Two facts follow, both
// used by zip_step (see k_kb_spine for how the marks become forest edges):
//   * a walk at a spine vertex x for pending edge (x, b) with b marked can stop: b is
//     already an etree ancestor of x through other edges, so the edge adds nothing;
//   * a walk at a spine vertex x may jump to the highest marked y < b: y is an etree
//     ancestor of x, and any walk may move to an etree ancestor below b (the pending edge
//     (x, b) and (y, b) give the same threshold connectivity).
struct SpineInfo {
  const uint32_t* bitmap = nullptr;
  uint32_t B0 = 0, B1 = 0, G = INV;
};
constexpr uint32_t KB_SCAN_LIMIT = 64;  // spine scans (sp_pred, k_kb_spine): bitmap words per search
// The stride of the kb loop's parent[]: interleaved with the hints (ld_pj below, k_pj_init).
constexpr uint32_t KB_PS = 2;

__device__ __forceinline__ bool sp_marked(const SpineInfo& sp, uint32_t v) {
  return v >= sp.B0 && v < sp.B1 && ((sp.bitmap[v >> 5] >> (v & 31)) & 1u);
}

// Bits of bitmap word w restricted to ranks [lo, hi).
__device__ __forceinline__ uint32_t word_in(const uint32_t* bitmap, uint32_t w, uint32_t lo,
                                            uint32_t hi) {
  uint32_t bits = bitmap[w];
  if (w == (lo >> 5)) bits &= ~0u << (lo & 31);
  if (w == ((hi - 1) >> 5) && (hi & 31)) bits &= ~(~0u << (hi & 31));
  return bits;
}

// Highest marked y with x < y < b (scans at most KB_SCAN_LIMIT words below b's); INV if none.
__device__ __forceinline__ uint32_t sp_pred(const SpineInfo& sp, uint32_t b, uint32_t x) {
  uint32_t lo = max(x + 1, sp.B0);
  if (b <= lo) return INV;
  uint32_t w = (b - 1) >> 5, wl = lo >> 5;
  for (uint32_t k = 0; k <= KB_SCAN_LIMIT; ++k) {
    uint32_t bits = word_in(sp.bitmap, w, lo, b);
    if (bits) return (w << 5) + 31 - __clz(bits);
    if (w == wl) break;
    --w;
  }
  return INV;
}

// Parent and hint of rank v.  S = 1: two arrays (parent[v], jump[v]); S = 2: one interleaved
// array, parent at pj[2v] and the hint at pj[2v + 1] (the kb loop): a step then loads both with
// one 8-byte relaxed agent-scope load — one cache line per step, not two.  (The hint half is
// written with plain stores and the parent half only by CAS: write-back L2s merge dirty bytes
// only, so neither half overwrites the other.)
template <int S>
__device__ __forceinline__ void ld_pj(uint32_t* parent, uint32_t* jump, uint32_t x, uint32_t& p,
                                      uint32_t& j) {
  if (S == 2) {
    const uint64_t w = __hip_atomic_load((uint64_t*)(parent + 2 * (size_t)x), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    p = (uint32_t)w;
    j = (uint32_t)(w >> 32);
  } else {
    p = ld_parent(&parent[x]);
    j = jump ? jump[x] : 0u;
  }
}

// jump: the hint array (S = 1 only; S = 2 takes the hints from parent + 1).
template <bool STATS, bool REC = false, bool SPINE = false, int S = 1>
__device__ __forceinline__ bool zip_step(uint32_t* parent, uint32_t* jump, ZState& s, ZCount& c,
                                         const ZRec& rec = ZRec(),
                                         const SpineInfo& sp = SpineInfo()) {
  uint32_t* const jp = S == 2 ? parent + 1 : jump;  // jp[S * v]: the hint of v
  if (STATS) c.steps++;
  if (!s.fresh) {
    // the parent, the hint and (until the walk reaches the spine) x's mark word are loaded
    // together: one memory latency per step, not two.  When the hint is taken the parent read
    // is dropped; when the spine moves x, both are loaded again (once per pending edge).
    const bool chk = SPINE && !(s.flags & ZF_SPINE);
    const uint32_t mw = (chk && s.x >= sp.B0 && s.x < sp.B1) ? sp.bitmap[s.x >> 5] : 0u;
    uint32_t pj, j;
    ld_pj<S>(parent, jump, s.x, pj, j);
    if (chk && (s.x == sp.G || ((mw >> (s.x & 31)) & 1u))) {
      s.flags |= ZF_SPINE;
      if (!(s.flags & ZF_KEEP) && sp_marked(sp, s.b)) return true;
      uint32_t y = sp_pred(sp, s.b, s.x);
      if (y != INV) {
        s.prev = INV;
        s.x = y;
        ld_pj<S>(parent, jump, s.x, pj, j);
      }
    }
    if (j > s.x && j < s.b) {
      if (s.prev != INV) jp[(size_t)S * s.prev] = j;
      s.prev = s.x;
      s.x = j;
      return false;
    }
    s.p = pj;
  }
  s.fresh = false;
  if (s.p < s.b) {  // INVALID is never < b
    if (s.p <= s.x) {  // not heap-ordered: corrupt input; stop the walk (fault_word)
      raise_fault(FAULT_FOREST);
      return true;
    }
    if (s.prev != INV) jp[(size_t)S * s.prev] = s.p;
    s.prev = s.x;
    s.x = s.p;
    return false;
  }
  if (s.x != s.a) jp[(size_t)S * s.a] = s.x;
  if (s.p == s.b) return true;
  if (STATS) c.cas++;
  uint32_t old = atomicCAS(&parent[(size_t)S * s.x], s.p, s.b);
  if (old != s.p) {
    if (STATS) c.fail++;
    s.p = old;
    s.fresh = true;
    return false;
  }
  if (s.p == INV) {
    if (REC && s.x < rec.B0) s.flags |= ZF_LINKED;  // appended by the caller, per wave
    return true;
  }
  s.a = s.b;  // zipper: continue with pending edge (b, old parent)
  s.b = s.p;
  s.x = s.a;
  s.prev = INV;
  s.flags = ZF_KEEP;
  return false;
}

__device__ __forceinline__ void zstart(ZState& s, uint32_t a, uint32_t b, uint32_t flags = 0) {
  s.a = a;
  s.b = b;
  s.x = a;
  s.prev = INV;
  s.flags = flags;
  s.fresh = false;
}

template <bool STATS>
__device__ __forceinline__ void flush_stats(unsigned long long* stats, uint64_t edges, const ZCount& c,
                                            uint32_t maxsteps) {
  if (!STATS) return;
  atomicAdd(&stats[0], (unsigned long long)edges);
  atomicAdd(&stats[1], (unsigned long long)c.steps);
  atomicAdd(&stats[2], (unsigned long long)c.cas);
  atomicAdd(&stats[3], (unsigned long long)c.fail);
  atomicMax(&stats[4], (unsigned long long)maxsteps);
  atomicAdd(&stats[5], (unsigned long long)c.root);
  atomicAdd(&stats[6], (unsigned long long)c.one);
}

// Lane-level work queue.  Each wave pulls chunks of edges in increasing order and
// every lane that finishes an edge takes the next one at the following step, so a wave never
// idles behind its slowest lane.
// Edge source of the queue: packed u64 items (hi << 32 | lo), or (kb) the spine queue
// followed by the kept (b, g) pairs of a bucket.
struct EdgeSrc {
  const uint64_t* items;  // packed (hi << 32 | lo)
  // kb bucket mode (spq != nullptr): indices [0, np) are giant-path edges (G, spq[i]), then
  // [np, n) the kept pairs items[i - np].
  const uint32_t* spq = nullptr;
  uint32_t G = INV;
  uint64_t np = 0;
  __device__ __forceinline__ void get(uint64_t i, uint32_t& b, uint32_t& a, uint32_t& fl) const {
    fl = 0;
    if (i < np) { b = spq[i]; a = G; fl = ZF_KEEP; return; }
    uint64_t it = items[i - np];
    b = (uint32_t)(it >> 32);
    a = (uint32_t)it;
  }
};

// Queue chunk (edges per wave refill): all waves sweep the list together, so about
// nwaves * chunk edges are in flight — the concurrency window that the zipper's rework grows
// with (tree phase, RMAT-26: 26.3 / 25.6 / 25.3 / 25.8 ms at 64 / 256 / 512 / 1024;
// twitter-shape: 37.7 / 37.6 / 38.9 ms at 64 / 256 / 512; LJ-shape within noise).
constexpr uint32_t KB_QCHUNK = 256;

// pj: the kb loop's interleaved parents and hints (ld_pj, S = 2).  With REC, rec.lbuf is the
// block's LDS buffer.
template <bool STATS, bool REC, bool SPINE>
__device__ __forceinline__ void tree_queue_body(EdgeSrc src, uint64_t n, uint32_t* pj,
                                                unsigned long long* stats, const ZRec& rec,
                                                const SpineInfo& sp = SpineInfo()) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint64_t cbase = 0, cend = 0;  // wave-uniform chunk cursor
  const uint64_t wave_id = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  uint64_t chunk_k = 0;
  bool active = false, exhausted = false;
  ZState s;
  ZCount c;
  uint64_t edges = 0;
  uint32_t maxsteps = 0, st0 = 0;
  for (;;) {
    uint64_t freem = __ballot(!active);
    while (freem && !exhausted) {
      if (cbase >= cend) {
        // the wave's next chunk: static stride over the grid, so all waves sweep the edge
        // list together in increasing order with no shared counter (a single global cursor
        // serialises: one same-address atomic per chunk)
        uint64_t st = (wave_id + chunk_k * nwaves) * (uint64_t)KB_QCHUNK;
        ++chunk_k;
        if (st >= n) { exhausted = true; break; }
        cbase = st;
        cend = st + KB_QCHUNK < n ? st + KB_QCHUNK : n;
      }
      uint32_t k = (uint32_t)__popcll(freem & lt);
      uint64_t cnt = (uint64_t)__popcll(freem);
      uint64_t avail = cend - cbase;
      if (!active && k < avail) {
        uint64_t idx = cbase + k;
        uint32_t b, a, fl;
        src.get(idx, b, a, fl);
        if (b != INV && a < b) {  // (INVALID: dropped; a > b: linked by k_kb_refresh)
          zstart(s, a, b, fl);
          active = true;
          if (STATS) { edges++; st0 = c.steps; c.root += a < rec.B0; }
        }
      }
      cbase += cnt < avail ? cnt : avail;
      freem = __ballot(!active);
    }
    if (__ballot(active) == 0) break;
    bool linked = false;
    if (active && zip_step<STATS, REC, SPINE, 2>(pj, nullptr, s, c, rec, sp)) {
      active = false;
      linked = REC && (s.flags & ZF_LINKED);
      if (STATS) { maxsteps = max(maxsteps, c.steps - st0); c.one += c.steps - st0 == 1; }
    }
    if (REC) {  // the pre-bucket roots linked in this step: one append reservation per wave
      const uint64_t bal = __ballot(linked);
      if (bal) {
        const int leader = __ffsll((unsigned long long)bal) - 1;
        const uint32_t cnt = (uint32_t)__popcll(bal), r = (uint32_t)__popcll(bal & lt);
        // into the block's LDS buffer; what does not fit goes straight out
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(rec.lcnt, cnt);
        base = __builtin_amdgcn_readlane(base, leader);
        const uint32_t over0 = base > rec.lcap ? base : rec.lcap;
        const uint32_t nover = base + cnt > over0 ? base + cnt - over0 : 0u;
        uint32_t g = 0;
        if (nover && lane == leader) g = atomicAdd(rec.n_linked, nover);
        g = __builtin_amdgcn_readlane(g, leader);
        if (linked) {
          const uint32_t slot = base + r;
          if (slot < rec.lcap) rec.lbuf[slot] = s.x;
          else rec.linked[g + (slot - over0)] = s.x;
        }
      }
    }
  }
  flush_stats<STATS>(stats, edges, c, maxsteps);
}

__device__ void zip_insert(uint32_t* parent, uint32_t* jump, uint32_t a, uint32_t b) {
  ZState s;
  ZCount c;
  zstart(s, a, b);
  while (!zip_step<false>(parent, jump, s, c)) {
  }
}

// ---------------------------------------------------------------------------------------
// Bucket-synchronous Kruskal ("kb"): Liu's algorithm run over rank buckets [B0, B1) in order.
//
// Between buckets the connectivity of every edge with hi < B0 is held in a union-find uf[]
// (random-priority linking, path halving) whose roots carry label[] = the component's max
// jnid = its elimination-tree root.  Both are frozen (and coherent: kernel boundary) while a
// bucket runs, so for a tree edge (a, b) with a < B0 the walk of Liu's find is replaced by
//     g = label[find(a)]     (exact: g < B0 <= b and a ~ g through vertices <= g)
// (a >= B0: g = a).  Inside a wave the 64 consecutive edges (sorted by b) are deduplicated on
// (g, b) — a hub's thousands of edges from the giant component collapse to one — and the
// survivors are inserted with the lock-free zipper, whose walks now stay inside the bucket.
// After the bucket: union(x, parent[x]) for every link the bucket created (pre-bucket roots
// that were linked are recorded by the zipper), then label[find(v)] = v for every in-bucket
// etree root v.  The result is the unique etree, as for the plain zipper.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t uf_prio(uint32_t x) {  // a bijection on u32: no ties
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// find with path halving.  ATOMIC: loads with relaxed agent atomics (during concurrent unions).
// (A walk longer than FAULT_STEPS means a cycle — corrupt input: it stops at x, fault_word.)
template <bool ATOMIC>
__device__ __forceinline__ uint32_t uf_find(uint32_t* uf, uint32_t x) {
  for (uint32_t k = 0;; ++k) {
    uint32_t p = ATOMIC ? __hip_atomic_load(&uf[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : uf[x];
    if (p == x) return x;
    uint32_t gp = ATOMIC ? __hip_atomic_load(&uf[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : uf[p];
    if (gp == p) return p;
    if (k == FAULT_STEPS) {
      raise_fault(FAULT_UF);
      return x;
    }
    uf[x] = gp;  // x is a non-root forever; any ancestor is a valid pointer
    x = gp;
  }
}

// find without path compression, for values every thread of a launch asks for (G): a
// compressing find would have all of them write the same words.
__device__ __forceinline__ uint32_t uf_find_ro(const uint32_t* uf, uint32_t x) {
  uint32_t k = 0;
  for (uint32_t p = uf[x]; p != x; p = uf[x]) {
    if (++k == FAULT_STEPS) {
      raise_fault(FAULT_UF);
      break;
    }
    x = p;
  }
  return x;
}

// Link order: R (the giant's root, see k_kb_union) above everything, then uf_prio — a strict
// total order, so concurrent links never close a cycle.  Each retry follows a link another
// thread made; more than FAULT_STEPS of them (or a find that gave up) means corrupt input.
__device__ __forceinline__ void uf_union(uint32_t* uf, uint32_t u, uint32_t v, uint32_t R) {
  for (uint32_t k = 0; k < FAULT_STEPS; ++k) {
    uint32_t ru = uf_find<true>(uf, u), rv = uf_find<true>(uf, v);
    if (ru == rv) return;
    if (ru == R || (rv != R && uf_prio(ru) > uf_prio(rv))) { uint32_t t = ru; ru = rv; rv = t; }
    if (atomicCAS(&uf[ru], ru, rv) == ru) return;
  }
  raise_fault(FAULT_UF);
}

// The kb map pass over one bucket's records (sorted by hi down to groups of 2^gshift ranks,
// in stream order inside a group).  Per record (b = hi, a = lo):
//   g = a (a >= B0) or label[find(a)] (a < B0: a's pre-bucket etree root, exact);
//   g == G (the giant, see SpineInfo): b is marked in the bucket's rank bitmap;
//   otherwise (g, b) is kept for the zipper;
//   cnt[b] += 1 (nullable: the run length of b that pst needs).
// Giant membership without the union-find: gbits (nullable) holds one bit per rank, set only
// for ranks known to lie in the component of the reference vertex X = *gx; the rebase before
// this launch (k_kb_pick) made X a member of the anchor's component, so a set bit means
// g = G with no find at all.  Only the other records (non-giant components, and giant members
// whose bit is not set yet) run the find, and those finds are batched: every lane first loads
// its KM_R records and their bitmap words, then walks all of its misses' chains together (the
// loads of different records interleave), and a miss that reaches the giant sets its bit for
// the records that follow.  Bits are set by this map, by k_kb_spine (the bucket's marked ranks)
// and by k_kb_label (the bucket's ranks that ended in X's component); they are only ever
// cleared by k_kb_pick when X moves to another component (before the giant has formed).
// A block takes chunks of KM_CHUNK records; marks and counts of ranks within KM_WIN of the
// chunk's first group go to LDS (bitmap + packed 16-bit counts) and reach global memory once
// per word per chunk — a hub's records span many waves, and same-word atomics from every
// wave serialise.  Ranks beyond the window use global atomics directly.
// The anchor a kernel works with: the device-picked one (anc, k_kb_pick) when the host says
// there is one, else the host's.
__device__ __forceinline__ uint32_t anchor_rank(uint32_t anchor, const uint32_t* anc) {
  return (anc && anchor != INV) ? *anc : anchor;
}

static constexpr int KM_THREADS = 1024;
static constexpr int KM_CHUNK = 8192;       // < 65536: the packed 16-bit counts cannot carry
static constexpr uint32_t KM_WIN = 32768;   // ranks
static constexpr int KM_R = KM_CHUNK / KM_THREADS;  // records per lane per chunk
static constexpr uint32_t KM_FLUSH = 65535 / KM_CHUNK;  // chunks per window flush at most
// Giant summary words in the map's LDS (64 KB: ranks below 2^25).  The map's static LDS is
// ~80 KB, so map + summary stays one block per CU and leaves ~16 KB beside it for the zipper.
static constexpr uint32_t KM_GSUM = 16384;

template <bool STATS, bool HUB = false, int DF = -1>
__global__ void __launch_bounds__(KM_THREADS)
k_kb_map(const uint64_t* __restrict__ items, uint64_t e_begin, uint64_t e_end, KbSegs sg,
         uint32_t B0, int gshift, uint32_t* uf, const uint32_t* __restrict__ label, uint64_t* kept,
         uint32_t* n_kept, uint32_t* bitmap, uint32_t* cnt, unsigned long long* stats,
         uint32_t anchor, const uint32_t* __restrict__ bins, uint32_t nb, uint32_t* gbits,
         const uint32_t* __restrict__ gx, int defer, const uint32_t* __restrict__ anc,
         const uint32_t* __restrict__ gsum, uint32_t gs_words, uint32_t gs_w0, uint32_t kept_cap) {
  extern __shared__ uint32_t s_gsum[];  // gs_words words of the giant summary (dynamic LDS)
  if (DF >= 0) defer = DF;  // (compile-time for the deferred misses)
  __shared__ uint32_t wbits[KM_WIN / 32];
  __shared__ uint32_t wcnt[KM_WIN / 2];
  __shared__ uint32_t woff[KM_THREADS / 64 + 1];
  __shared__ uint32_t sbins[512];
  __shared__ unsigned long long s_s0[512];  // the bucket's segments [s0, s0 + len)
  __shared__ uint32_t s_len[512];
  __shared__ uint32_t s_cp[513];                        // chunks before each segment
  constexpr int R = KM_R;
  // RG: the giant's union-find root, found from the anchor rank (see launch_kb_map); it does
  // not move while this map runs (k_kb_union links everything else below it).  Membership is
  // tested on the root, not on the label, which the apply of the previous bucket may be
  // rewriting meanwhile.
  anchor = anchor_rank(anchor, anc);
  const uint32_t RG = anchor != INV ? uf_find_ro(uf, anchor) : INV;
  const bool use_bm = gbits != nullptr && RG != INV && *gx != INV;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint64_t edges = 0, kept_n = 0, inb = 0, misses = 0;
  // The LDS window starts zero and every flush re-zeroes the words it read, so a chunk never
  // clears it; the bin bounds are searched in LDS.
  for (uint32_t i = t; i < KM_WIN / 32; i += KM_THREADS) wbits[i] = 0;
  if (cnt)
    for (uint32_t i = t; i < KM_WIN / 2; i += KM_THREADS) wcnt[i] = 0;
  if (bins)
    for (uint32_t i = t; i < nb; i += KM_THREADS) sbins[i] = bins[i];
  // the summary covers ranks [gs_lo, gs_hi), the KM_GSUM words below B0 (all of them when
  // B0 <= 2^25): bit q set = ranks [64q, 64q + 64) all have their giant bit (k_gb_sum, a
  // snapshot taken before this map: bits are only ever added)
  const uint32_t gs_lo = gs_w0 * 2048u, gs_hi = use_bm ? gs_lo + gs_words * 2048u : 0u;
  for (uint32_t i = t; i < (use_bm ? gs_words : 0u); i += KM_THREADS) s_gsum[i] = gsum[gs_w0 + i];
  block_sync();
  // Each block maps a contiguous run of chunks, so that consecutive chunks mostly share one
  // window (a bin): the window is flushed to global memory only when the next chunk's differs,
  // after KM_FLUSH chunks (the packed 16-bit counts must not carry), and at the end.
  // The bucket's records: one range [e_begin, e_end), or the filled part of each of its
  // directly binned bins (launch_edge_bin) — chunks never cross a segment end.
  uint32_t nseg = 1;
  if (sg.start) {
    nseg = sg.i1 - sg.i0;
    for (uint32_t i = t; i < nseg; i += KM_THREADS) {
      s_s0[i] = sg.start[sg.i0 + i];
      s_len[i] = (uint32_t)(min(sg.cur[sg.i0 + i], sg.cap[sg.i0 + i]) - s_s0[i]);
    }
  } else if (t == 0) {
    s_s0[0] = e_begin;
    s_len[0] = (uint32_t)(e_end - e_begin);
  }
  block_sync();
  if (w == 0) {
    uint32_t run = 0;
    for (uint32_t b0 = 0; b0 < nseg; b0 += 64) {
      const uint32_t i = b0 + lane;
      const uint32_t c = i < nseg ? (uint32_t)(((uint64_t)s_len[i] + KM_CHUNK - 1) / KM_CHUNK) : 0u;
      const uint32_t incl = wave_incl_scan(c);
      if (i < nseg) s_cp[i] = run + incl - c;
      run += (uint32_t)__shfl((int)incl, 63);
    }
    if (lane == 0) s_cp[nseg] = run;
  }
  block_sync();
  const uint32_t total = s_cp[nseg];
  const uint32_t per = (total + gridDim.x - 1) / gridDim.x;
  const uint32_t j0 = min(blockIdx.x * per, total), j1 = min(j0 + per, total);
  uint32_t si = 0;  // segment of the chunk fetched last (chunks are visited in order)
  auto window = [&](uint32_t h0, uint32_t blast, uint32_t& bbase, uint32_t& gend) {
    if (bins) {
      bbase = sbins[bin_of(sbins, nb, h0)] & ~31u;
      gend = (uint32_t)min((uint64_t)sbins[min(bin_of(sbins, nb, blast) + 1, nb - 1)],
                           (uint64_t)bbase + KM_WIN);
      if (gend <= bbase) gend = bbase + 1;
    } else {
      bbase = ((h0 >> gshift) << gshift) & ~31u;
      gend = (uint32_t)min((((uint64_t)(blast >> gshift)) + 1) << gshift, (uint64_t)bbase + KM_WIN);
    }
  };
  // Prefetch.  Chunk j + 1's records are loaded during chunk j.  Where the loads are issued
  // matters: a wave's loads return in order, and a wait for a load that the compiler cannot
  // count (a predicated one, a returning atomic) waits for everything issued before it.  With
  // the prefetch issued right after the giant-bit loads (rounds 1-4), the classification's wait
  // drained it within the same chunk (ISA: s_waitcnt vmcnt(0) before the bit tests).  So the
  // records are loaded after the chunk's last uncounted wait (the classification and the
  // out-of-window mark tests), right after the kept pairs' reservation: every record load is
  // unpredicated (clamped to the chunk, masked later) and the reservation's result is then a
  // counted wait; the prefetch overlaps the flush, the kept-pair stores and the next chunk's
  // start.  A chunk's window needs no load either: in segment mode (directly binned records)
  // a chunk lies in one bin, whose bounds are in LDS; otherwise its first and last hi are
  // loaded a chunk ahead, before the classification.  (Past the block's last chunk the
  // prefetch re-reads the last one: valid addresses, never used.)
  uint64_t nx[R];
  auto bounds_of = [&](uint32_t j, uint64_t& b0, uint64_t& b1, uint32_t& sj) {
    while (s_cp[si + 1] <= j) ++si;  // (j only grows over the calls)
    b0 = s_s0[si] + (uint64_t)(j - s_cp[si]) * KM_CHUNK;
    b1 = min(b0 + (uint64_t)KM_CHUNK, s_s0[si] + s_len[si]);
    sj = si;
  };
  auto fetch = [&](uint64_t b0, uint64_t b1) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t idx = b0 + (uint64_t)r * KM_THREADS + (uint64_t)w * 64 + lane;
      nx[r] = __builtin_nontemporal_load(&items[min(idx, b1 - 1)]);  // streamed once
    }
  };
  const bool segw = sg.start != nullptr && bins != nullptr;  // windows from the segments' bins
  auto seg_window = [&](uint32_t sj, uint32_t& bbase, uint32_t& gend) {
    const uint32_t b = sg.i0 + sj;
    bbase = sbins[b] & ~31u;
    gend = (uint32_t)min((uint64_t)sbins[min(b + 1, nb - 1)], (uint64_t)bbase + KM_WIN);
    if (gend <= bbase) gend = bbase + 1;
  };
  uint64_t nc0 = 0, nc1 = 0, pc0 = 0, pc1 = 0;  // chunk j's and chunk j + 1's records
  uint32_t ns = 0, ps = 0;                      // ... their segments
  uint32_t nh0 = 0, nbl = 0;                    // (not segment mode) chunk j's first, last hi
  if (j0 < j1) {
    bounds_of(j0, nc0, nc1, ns);
    fetch(nc0, nc1);
    if (!segw) {
      nh0 = (uint32_t)(items[nc0] >> 32);
      nbl = (uint32_t)(items[nc1 - 1] >> 32);
    }
    if (j0 + 1 < j1) bounds_of(j0 + 1, pc0, pc1, ps);
    else { pc0 = nc0; pc1 = nc1; ps = ns; }
  }
  uint32_t since_flush = 0;
  for (uint32_t j = j0; j < j1; ++j) {
    const uint64_t c0 = nc0, c1 = nc1;
    uint64_t it[R];
    uint32_t vmask = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      it[r] = nx[r];
      const uint64_t idx = c0 + (uint64_t)r * KM_THREADS + (uint64_t)w * 64 + lane;
      vmask |= (uint32_t)(idx < c1) << r;
    }
    // the chunk's records lie in [group (or bin) of its first record, that of its last)
    uint32_t bbase, gend;
    if (segw) seg_window(ns, bbase, gend);
    else window(nh0, nbl, bbase, gend);
    uint32_t qh0 = 0, qbl = 0;  // (not segment mode) chunk j + 1's first and last hi
    if (!segw) {
      qh0 = (uint32_t)(items[pc0] >> 32);
      qbl = (uint32_t)(items[pc1 - 1] >> 32);
    }
    const uint32_t span = gend - bbase;  // ranks of the window that can hold records
    // Narrow windows (hub bins: few ranks, many records each) keep RF u32 copies of each
    // rank's count, lane l adding to copy l % RF: a hub's lanes in one wave then hit RF
    // addresses, not one (same-address LDS atomics of a wave serialise).  RF = 1: the packed
    // 16-bit counts.  (RF is fixed per window: the window, hence span, only changes at a flush.)
    // HUB: buckets of 2^25 records and more (launch_kb_map; the small configs keep the plain
    // counts: with the copies their tree took 0.1-0.15 ms longer).
    const uint32_t RF = !HUB ? 1u : span <= 512 ? 32u : span <= 1024 ? 16u : span <= 2048 ? 8u : 1u;
    uint32_t gw[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t a = (uint32_t)it[r];
      const bool t_ = use_bm && ((vmask >> r) & 1) && a < B0;
      // most lo ranks lie in 64-rank blocks that are all in the giant: answered from LDS
      const bool full = t_ && a >= gs_lo && a < gs_hi &&
                        ((s_gsum[(a - gs_lo) >> 11] >> ((a >> 6) & 31)) & 1u);
      gw[r] = full ? ~0u : (t_ ? gbits[a >> 5] : 0u);
    }
    const bool more = j + 1 < j1;
    uint32_t giant = 0, miss = 0, x[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t a = (uint32_t)it[r];
      x[r] = a;
      if (((vmask >> r) & 1) && a < B0) {
        if ((gw[r] >> (a & 31)) & 1) giant |= 1u << r;
        else miss |= 1u << r;
      }
    }
    if (STATS) misses += (uint64_t)__popc(miss);
    // 2. the misses' finds (path halving), all chains of the lane advanced together — unless
    // they are deferred: then a miss is kept as (b, a) and k_kb_refresh resolves it
    for (uint32_t act = defer == 1 ? 0u : miss; act;) {
      uint32_t p[R], gp[R];
#pragma unroll
      for (int r = 0; r < R; ++r) p[r] = ((act >> r) & 1) ? uf[x[r]] : 0u;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (((act >> r) & 1) && p[r] == x[r]) act &= ~(1u << r);
#pragma unroll
      for (int r = 0; r < R; ++r) gp[r] = ((act >> r) & 1) ? uf[p[r]] : 0u;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if ((act >> r) & 1) {
          if (gp[r] == p[r]) {
            x[r] = p[r];
            act &= ~(1u << r);
          } else {
            uf[x[r]] = gp[r];  // x is a non-root forever; any ancestor is a valid pointer
            x[r] = gp[r];
          }
        }
    }
    // 3. roots -> giant (and its bit) or the pre-bucket etree root g = label[root]
    uint32_t lab[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (defer != 1 && ((miss >> r) & 1) && x[r] == RG) {
        giant |= 1u << r;
        if (use_bm) {
          const uint32_t a = (uint32_t)it[r];
          atomicOr(&gbits[a >> 5], 1u << (a & 31));
        }
      }
      // defer 2 (split lockstep): the root itself — the ranks' unions need no more, and the
      // bucket's owner refreshes its pairs to the pre-bucket etree roots anyway
      lab[r] = (defer == 0 && ((miss & ~giant) >> r) & 1) ? label[x[r]]
               : (defer == 2 && ((miss & ~giant) >> r) & 1) ? x[r] : (uint32_t)it[r];
    }
    uint32_t nout = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool valid = (vmask >> r) & 1, gi = (giant >> r) & 1;
      const uint32_t b = (uint32_t)(it[r] >> 32), a = (uint32_t)it[r];
      const uint32_t g = ((miss >> r) & 1) ? lab[r] : a;
      if (STATS) { edges += valid; kept_n += valid && !gi; inb += valid && !gi && a >= B0; }
      const uint32_t o = b - bbase;
      if (valid && cnt) {
        if (o >= span) atomicAdd(&cnt[b], 1u);
        else if (RF > 1) atomicAdd(&wcnt[o * RF + (lane & (RF - 1))], 1u);
        else atomicAdd(&wcnt[o >> 1], 1u << (16 * (o & 1)));
      }
      if (gi) {  // a hub's records repeat its mark: test first (a read of one word is a
                 // broadcast, same-word atomics from a wave serialise)
        if (o < span) {
          if (!((wbits[o >> 5] >> (o & 31)) & 1u)) atomicOr(&wbits[o >> 5], 1u << (o & 31));
        } else if (!((bitmap[b >> 5] >> (b & 31)) & 1u)) {
          atomicOr(&bitmap[b >> 5], 1u << (b & 31));
        }
      }
      const bool k2 = valid && !gi;
      it[r] = k2 ? (((uint64_t)b << 32) | g) : ~0ull;
      nout += (uint32_t)__popcll(__ballot(k2));
    }
    if (lane == 0) woff[w] = nout;
    // flush the window unless the next chunk of this block keeps it (uniform decision)
    // (the packed 16-bit counts must not carry: flushed every KM_FLUSH chunks; the u32 copies
    // only when the window changes)
    bool flush = !more || (++since_flush >= KM_FLUSH && RF == 1);
    if (!flush) {
      uint32_t nbase, nend;
      if (segw) seg_window(ps, nbase, nend);
      else window(qh0, qbl, nbase, nend);
      flush = nbase != bbase || nend != gend;
    }
    block_sync();
    // compaction: one reservation per chunk for the kept pairs of all its waves (issued here,
    // before the prefetch, so that its result is a counted wait).  Guard: a chunk keeps at most
    // its records and the host sizes kept for the bucket's records, so a reservation past
    // kept_cap means corrupt counts; it raises the fault word (-EIO), nothing is written past
    // kept_cap, and n_kept is clamped to it (every later reservation is past it too and clamps
    // again), so the refresh and the zipper read only written slots.
    uint32_t kbase = 0, krun = 0;
    if (t == 0) {
      for (int i = 0; i < KM_THREADS / 64; ++i) { uint32_t v = woff[i]; woff[i] = krun; krun += v; }
      // (an address the compiler cannot prove uniform — mbcnt of an empty mask is 0 — keeps
      // the atomic optimizer from broadcasting the result with readfirstlane right away, which
      // waits for it, and for the prefetch behind it)
      if (krun) kbase = atomicAdd(n_kept + __builtin_amdgcn_mbcnt_lo(0u, 0u), krun);
    }
    // the prefetch: chunk j + 1's records (chunk j's again past the block's last)
    fetch(pc0, pc1);
    nc0 = pc0; nc1 = pc1; ns = ps; nh0 = qh0; nbl = qbl;
    if (j + 2 < j1) bounds_of(j + 2, pc0, pc1, ps);
    if (flush) {
      since_flush = 0;
      for (uint32_t i = t; i < (span + 31) / 32; i += KM_THREADS) {
        const uint32_t v = wbits[i];
        if (v) {
          atomicOr(&bitmap[(bbase >> 5) + i], v);
          wbits[i] = 0;
        }
      }
      if (cnt && RF > 1) {
        for (uint32_t i = t; i < span; i += KM_THREADS) {
          uint32_t v = 0;
          for (uint32_t r = 0; r < RF; ++r) {
            v += wcnt[i * RF + r];
            wcnt[i * RF + r] = 0;
          }
          if (v) atomicAdd(&cnt[bbase + i], v);
        }
      } else if (cnt) {
        for (uint32_t i = t; i < (span + 1) / 2; i += KM_THREADS) {
          const uint32_t v = wcnt[i];
          if (v) {
            if (v & 0xFFFFu) atomicAdd(&cnt[bbase + 2 * i], v & 0xFFFFu);
            if (v >> 16) atomicAdd(&cnt[bbase + 2 * i + 1], v >> 16);
            wcnt[i] = 0;
          }
        }
      }
    }
    if (t == 0) {
      if (krun && (uint64_t)kbase + krun > kept_cap) {
        raise_fault(FAULT_KEPT);
        atomicMin(n_kept, kept_cap);
      }
      woff[KM_THREADS / 64] = kbase;
    }
    block_sync();
    uint32_t pos = woff[KM_THREADS / 64] + woff[w];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      uint64_t bal = __ballot(it[r] != ~0ull);
      const uint32_t q = pos + (uint32_t)__popcll(bal & lt);
      if (it[r] != ~0ull && q < kept_cap) kept[q] = it[r];
      pos += (uint32_t)__popcll(bal);
    }
    // no barrier here: the next chunk writes LDS only after its own barrier has seen every
    // wave past this chunk's flush, and woff[w] is this wave's own slot
  }
  if (STATS) {
    atomicAdd(&stats[0], (unsigned long long)edges);
    atomicAdd(&stats[5], (unsigned long long)kept_n);
    atomicAdd(&stats[6], (unsigned long long)inb);
    atomicAdd(&stats[7], (unsigned long long)misses);
  }
}

// Before the map of a bucket, with nothing else running on the union-find (the previous map
// and the previous apply are complete): keep the bitmap's reference vertex X if it lies in the
// component of this map's anchor, else move X to the anchor and clear the bitmap.  X is read
// from one slot and written to the other (every block reads before block 0 writes).
// The giant summary: bit q of gsum = ranks [64q, 64q + 64) all have their giant bit (one lane
// per 64-rank block, ballot-assembled words).  Run with nothing writing gbits (before a map,
// after the rebase).
__global__ void k_gb_sum(const uint32_t* __restrict__ gbits, uint32_t nfull, uint32_t nwords,
                         uint32_t* gsum) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;  // one 64-rank block per lane
  bool full = false;
  if (q < nfull) {  // complete blocks only: a partial last block reads as not full
    const uint2 w = *(const uint2*)(gbits + 2 * (size_t)q);
    full = w.x == ~0u && w.y == ~0u;
  }
  const uint64_t bal = __ballot(full);
  const int lane = threadIdx.x & 63;
  if ((lane == 0 || lane == 32) && (q >> 5) < nwords)  // every word a map may read is written
    gsum[q >> 5] = lane ? (uint32_t)(bal >> 32) : (uint32_t)bal;
}

static void launch_gb_sum(const uint32_t* gbits, uint32_t n_seq, uint32_t* gsum, hipStream_t s) {
  const uint32_t nwords = (n_seq + 2047) / 2048;  // the words of ranks [0, n_seq)
  if (nwords == 0) return;
  const uint32_t lanes = nwords * 32;
  hipLaunchKernelGGL(k_gb_sum, dim3((lanes + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s, gbits, n_seq / 64,
                     nwords, gsum);
}

// Giant sweep: every applied rank v < B0lim whose giant bit is clear and whose component is
// that of the bitmap's reference vertex X = *gx gets its bit.  The bits are otherwise set only
// for the ranks of a bucket that end in X's component (k_kb_label) and for the lo ends the
// refresh finds in it, so the ranks of the small components that the giant swallows after
// their own bucket miss the bitmap until a refresh meets them: the maps keep their records as
// pairs for the refresh (RMAT-26: 102 M of the 179 M kept pairs resolved to the giant).  Safe
// beside the next map (bits are only added; a root RX that another union moves below a new root
// only loses matches) but not beside a pick that may move X (it runs on the picks' stream).
// One wave per 64 ranks (two bitmap words): a find for each clear bit, one atomicOr per word.
__global__ void k_gb_sweep(uint32_t* uf, uint32_t* gbits, uint32_t B0lim,
                           const uint32_t* __restrict__ gx) {
  const uint32_t X = *gx;
  if (X == INV || X >= B0lim) return;
  const uint32_t RX = uf_find_ro(uf, X);
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < B0lim; base += stride) {
    const uint32_t v = base + lane;
    bool in = false;
    if (v < B0lim && !((gbits[v >> 5] >> (v & 31)) & 1u)) in = uf_find<true>(uf, v) == RX;
    const uint64_t bal = __ballot(in);
    const uint32_t half = lane < 32 ? (uint32_t)bal : (uint32_t)(bal >> 32);
    if ((lane & 31) == 0 && half) atomicOr(&gbits[v >> 5], half);
  }
}

void launch_gb_sweep(const KbState& S, uint32_t B0lim, size_t gx_slot, hipStream_t s) {
  if (B0lim == 0) return;
  const uint32_t waves = (B0lim + 63) / 64;
  hipLaunchKernelGGL(k_gb_sweep, dim3(std::min<uint32_t>((waves + 3) / 4, 4096)), dim3(BLOCK), 0, s,
                     S.uf, S.gbits, B0lim, (const uint32_t*)S.gx_of(gx_slot));
}

// The giant's anchor, picked on the device before the map of a bucket, with nothing else
// running on the union-find.  The host's choice, rank B0lim - 1 (the highest degree among the
// applied ranks [0, B0lim)), can sit outside the giant: its bucket then sees no giant records
// and the zipper walks the giant's spine unaided (twitter shape, 40 + 40 cuts: tree 31.6 ->
// 47.8 ms).  So every block samples KP ranks spread evenly over [0, B0lim) (the last one is
// B0lim - 1) and finds the component holding the most samples; all blocks compute the same
// answer.  Two evenly spaced samples land in one component only if it spans about 1/KP of the
// ranks: beyond a couple of samples that is the giant.  The anchor is then
//   the previous anchor, if its component still holds >= 3 samples and at least the best
//     count minus 4 (a move clears the giant bitmap);
//   else a sampled rank of the best component, if it holds >= 3 samples;
//   else B0lim - 1 (no dominant component yet: the host's choice).
// Any applied rank is exact as an anchor (see launch_kb_map); the choice only shapes the work.
// B0lim = 0: no anchor (INV).  gbits (nullable): the bitmap is then rebased on the anchor:
// its reference vertex (*gx_rd) stays if it is in the anchor's component, else it moves to the
// anchor and the bitmap (n_seq / 32 + 2 words) is cleared; the result goes to *gx_wr.
static constexpr int KP = BLOCK;  // samples (one per thread of a block)
__global__ void __launch_bounds__(BLOCK)
k_kb_pick(const uint32_t* uf, uint32_t B0lim, const uint32_t* __restrict__ anc_prev,
          uint32_t* anc_out, uint32_t* gbits, uint32_t nwords, const uint32_t* __restrict__ gx_rd,
          uint32_t* gx_wr) {
  __shared__ uint32_t roots[KP], wkey[KP / 64], wcp[KP / 64];
  __shared__ uint32_t s_anchor;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  uint32_t anchor = INV;
  if (B0lim > 0) {  // uniform over the block
    const uint32_t smp = t == KP - 1 ? B0lim - 1 : (uint32_t)(((uint64_t)t * B0lim) / KP);
    const uint32_t r = uf_find_ro(uf, smp);
    roots[t] = r;
    const uint32_t prev = *anc_prev;
    const uint32_t rp = (prev != INV && prev < B0lim) ? uf_find_ro(uf, prev) : INV;
    block_sync();
    uint32_t cnt = 0;  // samples in this thread's component
    for (int u = 0; u < KP; ++u) cnt += roots[u] == r;
    uint32_t key = (cnt << 16) | (uint32_t)t;  // most samples, then the highest thread
    uint32_t cp = r == rp ? cnt : 0u;
    for (int o = 32; o > 0; o >>= 1) {
      key = max(key, (uint32_t)__shfl_xor((int)key, o));
      cp = max(cp, (uint32_t)__shfl_xor((int)cp, o));
    }
    if (lane == 0) { wkey[w] = key; wcp[w] = cp; }
    block_sync();
    if (t == 0) {
      uint32_t bk = 0, bp = 0;
      for (int i = 0; i < KP / 64; ++i) { bk = max(bk, wkey[i]); bp = max(bp, wcp[i]); }
      const uint32_t bc = bk >> 16, bt = bk & 0xFFFFu;
      const uint32_t bs = bt == KP - 1 ? B0lim - 1 : (uint32_t)(((uint64_t)bt * B0lim) / KP);
      s_anchor = (rp != INV && bp >= 3 && bp + 4 >= bc) ? prev : (bc >= 3 ? bs : B0lim - 1);
    }
    block_sync();
    anchor = s_anchor;
  }
  if (blockIdx.x == 0 && t == 0) *anc_out = anchor;
  if (!gbits) return;
  const uint32_t X = *gx_rd;
  const bool keep = anchor == INV || (X != INV && uf_find_ro(uf, X) == uf_find_ro(uf, anchor));
  if (blockIdx.x == 0 && t == 0) *gx_wr = anchor == INV ? INV : (keep ? X : anchor);
  if (!keep)
    for (uint32_t i = blockIdx.x * blockDim.x + t; i < nwords; i += gridDim.x * blockDim.x)
      gbits[i] = 0;
}

// Star -> path for the giant.  G's edges into the bucket go to the marked ranks b1 < b2 < ...;
// for the etree that star is equivalent to the path G-b1-b2-...: at every threshold both
// connect G with exactly the marked ranks present.  The path edges (b_i, b_i+1) are written
// straight into the forest (parent[] of every in-bucket rank is still INVALID here, so this
// is what the zipper would do, in one store).  A run of marks is cut where the next mark is
// more than KB_SCAN_LIMIT words away; each run's first mark b is queued as the edge (G, b), which
// the zipper inserts (walking G's chain).  One thread per bitmap word; the forward search of
// a word's last mark and the backward search of a word's first mark are symmetric, so every
// mark gets exactly one incoming connection.
// The same pass is the giant fold: every marked rank of the bucket ends in the anchor's
// component (the spine joins all of them to G), and its union-find slot is still its own
// (iota: nothing links an in-bucket rank before its bucket's union), so it is stored under
// that component's root R directly — no find, no CAS (nothing before the bucket's union
// reads in-bucket union-find slots).  k_kb_union then skips the links between two marked
// ranks (already in one tree).  gbits (nullable): the marked ranks are giant members; when
// the bitmap's reference vertex *gx lies in the anchor's component they are set there too
// (see k_kb_map).
// Split lockstep (P ranks, launch_ls_apply_split): CHAIN writes only the forest part (parent,
// spq: the bucket's zipper owner), FOLD only the union-find part (uf, gbits: every rank).
template <bool CHAIN, bool FOLD>
__global__ void k_kb_spine(const uint32_t* __restrict__ bitmap, uint32_t B0, uint32_t B1,
                           uint32_t* parent, uint32_t* spq, uint32_t* n_spine, uint32_t* uf,
                           uint32_t anchor, uint32_t* gbits, const uint32_t* __restrict__ gx,
                           const uint32_t* __restrict__ anc) {
  const uint32_t w0 = B0 >> 5, w1 = (B1 - 1) >> 5;
  const uint32_t R = FOLD ? uf_find_ro(uf, anchor_rank(anchor, anc)) : INV;
  const uint32_t X = (FOLD && gbits) ? *gx : INV;
  const bool set_g = FOLD && X != INV && uf_find_ro(uf, X) == R;
  // (The forward / backward searches below as wave ballots over 64-word windows, one load per
  // lane per window: RMAT-26 and RMAT-22 trees within noise, LJ tree +0.12 ms — the spine queue
  // comes out in another order, and the percolation bucket's zipper is sensitive to it;
  // profiles/r06/h_spine_fresh/)
  for (uint32_t w = w0 + blockIdx.x * blockDim.x + threadIdx.x; w <= w1;
       w += gridDim.x * blockDim.x) {
    uint32_t bits = word_in(bitmap, w, B0, B1);
    if (!bits) continue;
    if (set_g) atomicOr(&gbits[w], bits);
    uint32_t cur = (w << 5) + __ffs(bits) - 1;
    const uint32_t first = cur;
    if (FOLD) uf[cur] = R;
    bits &= bits - 1;
    while (bits) {
      uint32_t nx = (w << 5) + __ffs(bits) - 1;
      bits &= bits - 1;
      if (CHAIN) parent[(size_t)KB_PS * cur] = nx;
      if (FOLD) uf[nx] = R;
      cur = nx;
    }
    if (!CHAIN) continue;
    for (uint32_t v = w + 1, k = 0; v <= w1 && k < KB_SCAN_LIMIT; ++v, ++k) {
      uint32_t nb = word_in(bitmap, v, B0, B1);
      if (nb) { parent[(size_t)KB_PS * cur] = (v << 5) + __ffs(nb) - 1; break; }
    }
    bool has_pred = false;
    for (uint32_t v = w, k = 0; v > w0 && k < KB_SCAN_LIMIT; --v, ++k)
      if (word_in(bitmap, v - 1, B0, B1)) { has_pred = true; break; }
    if (!has_pred) spq[atomicAdd(n_spine, 1u)] = first;
  }
}

// Pipelined loop: the map of this bucket ran while the previous one was being applied, so its
// kept starts g may be stale — still exact, but from an old root the zipper walks up through
// everything the previous bucket linked.  With the union-find now current: g' = label[find(g)]
// (one thread per pair, all chains in flight together); a pair that turns out to reach the
// giant becomes b's mark (tested before the atomic: most hub words are marked already) and is
// dropped (b = INVALID, skipped by the zipper).  anchor: the map's and the spine's, so that
// every mark of the bucket is relative to one component.
// The map's deferred misses are kept pairs (b, a) with the raw lo a: this is where their finds
// run (every chain of the bucket in flight at once, against the current union-find), and a
// miss that reaches the giant sets its bit in gbits (nullable) when the bitmap's reference
// vertex *gx lies in the anchor's component.
// An in-bucket pair (a, b), B0 <= a < b, whose two ranks are both marked is dropped too:
// both are ancestors of G through their own edges to G's component, so b is already an ancestor
// of a without this edge (zip_step would stop it at its first step; here it costs two bitmap
// reads in a flat stream instead of a lane of the zipper's queue).  A mark this launch has not
// set yet only keeps a pair.
// pj (nullable; every launch_kb_apply — the one-GPU loop's and the lockstep loop's replicated,
// non-split apply — unless the option kb_rlink is 0; null in the split apply's
// launch_kb_refresh): the zipper's first step for a pair whose start is a
// pre-bucket root g' (every pair that reaches no giant): g' had no parent before this bucket
// (so no hint either), and zip_step's first move from it is exactly CAS(parent[g'], INVALID,
// b).  Done here, in this flat pass with the pair already in registers, instead of through the
// zipper's lane queue: the pair is then finished — rewritten as (rt, b), rt = the union-find
// root of g''s component (rt < B0 <= b: hi below lo, which no real pair has): the zipper skips
// it and k_kb_union unions rt with b straight from it (no parent load, a root to start from).  A CAS that fails
// leaves the pair to the zipper (another pair linked g' first; parent[g'] == b drops it, as
// zip_step does).  Zipper insertion is exact under any order of its steps, so running some
// first steps a kernel early changes nothing.
__global__ void k_kb_refresh(uint64_t* kept, const uint32_t* __restrict__ n_kept,
                             uint32_t* uf, const uint32_t* __restrict__ label, uint32_t* bitmap,
                             uint32_t B0, uint32_t anchor, uint32_t* gbits,
                             const uint32_t* __restrict__ gx, const uint32_t* __restrict__ anc,
                             uint32_t* pj = nullptr) {
  const uint32_t nk = *n_kept;
  anchor = anchor_rank(anchor, anc);
  const uint32_t RG = anchor != INV ? uf_find_ro(uf, anchor) : INV;
  const uint32_t X = gbits ? *gx : INV;
  const bool set_g = X != INV && RG != INV && uf_find_ro(uf, X) == RG;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) {
    const uint64_t it = kept[i];
    const uint32_t g = (uint32_t)it, b = (uint32_t)(it >> 32);
    if (g >= B0) {
      if (RG != INV && b != INV && ((bitmap[g >> 5] >> (g & 31)) & 1u) &&
          ((bitmap[b >> 5] >> (b & 31)) & 1u))
        kept[i] = ~0ull;
      continue;
    }
    const uint32_t rt = uf_find<false>(uf, g);
    if (rt == RG) {
      const uint32_t bit = 1u << (b & 31);
      if (!(bitmap[b >> 5] & bit)) atomicOr(&bitmap[b >> 5], bit);
      if (set_g) {
        const uint32_t gb = 1u << (g & 31);
        if (!(gbits[g >> 5] & gb)) atomicOr(&gbits[g >> 5], gb);
      }
      kept[i] = ~0ull;
    } else {
      const uint32_t g2 = label[rt];
      uint64_t nv = ((uint64_t)b << 32) | g2;
      if (pj && b != INV) {
        const uint32_t old = atomicCAS(&pj[2 * (size_t)g2], INV, b);
        if (old == INV) nv = ((uint64_t)rt << 32) | b;
        else if (old == b) nv = ~0ull;
      }
      if (nv != it) kept[i] = nv;
    }
  }
}

// The kb in-bucket pass: the spine queue, then the kept (b, g) pairs of the bucket, through
// the balanced lane queue with the spine rules (SpineInfo), recording pre-bucket roots it links.
// REC = false (split lockstep, the bucket's zipper owner): no linked roots are recorded (every
// rank unions the pairs themselves), and G comes from *gslot, captured before the bucket's
// union-find changed (anchor != INV means there is one).
template <bool STATS, bool REC = true>
__global__ void k_kb_zip(const uint64_t* __restrict__ kept, const uint32_t* __restrict__ n_kept,
                         const uint32_t* __restrict__ bitmap, const uint32_t* __restrict__ spq,
                         const uint32_t* __restrict__ n_spine, uint32_t B0, uint32_t B1,
                         uint32_t* uf, const uint32_t* __restrict__ label, uint32_t* pj,
                         unsigned long long* stats, uint32_t* linked, uint32_t* n_linked,
                         uint32_t anchor, const uint32_t* __restrict__ anc,
                         const uint32_t* __restrict__ gslot = nullptr) {
  constexpr uint32_t LCAP = REC ? 2048 : 1;
  __shared__ uint32_t lbuf[LCAP];
  __shared__ uint32_t lcnt, lbase;
  if (REC) {
    if (threadIdx.x == 0) lcnt = 0;
    block_sync();
  }
  ZRec rec;
  rec.B0 = B0;
  rec.linked = linked;
  rec.n_linked = n_linked;
  rec.lbuf = lbuf;
  rec.lcnt = &lcnt;
  rec.lcap = LCAP;
  EdgeSrc src{kept};
  const uint64_t nk = *n_kept;
  if (!gslot) anchor = anchor_rank(anchor, anc);
  if (anchor != INV) {
    SpineInfo sp;
    sp.bitmap = bitmap;
    sp.B0 = B0;
    sp.B1 = B1;
    sp.G = gslot ? *gslot : label[uf_find_ro(uf, anchor)];
    src.spq = spq;
    src.G = sp.G;
    src.np = *n_spine;
    tree_queue_body<STATS, REC, true>(src, src.np + nk, pj, stats, rec, sp);
  } else {
    tree_queue_body<STATS, REC, false>(src, nk, pj, stats, rec);
  }
  if (!REC) return;
  // the block's staged linked roots: one reservation, a coalesced copy
  block_sync();
  const uint32_t n = min(lcnt, LCAP);
  if (threadIdx.x == 0) lbase = n ? atomicAdd(n_linked, n) : 0u;
  block_sync();
  for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) linked[lbase + i] = lbuf[i];
}

// anchor: rank B0 - 1 (INV for the first bucket).  Its root R is never linked below another
// root here, so the giant keeps one root from bucket to bucket: the map of the next bucket,
// which runs concurrently in the pipelined loop, finds the same R from the same rank.  (All
// threads read the same R: no union of this launch can move it.)
// FOLD: the giant fold ran (k_kb_spine); links between two marked ranks are skipped, and the marks are cleared
// by k_kb_label instead (this launch reads them).
// linked / n_linked: the pre-bucket roots the zipper linked (k_kb_zip, REC).
// parent: the kb loop's, here and in k_kb_label (stride KB_PS; this kernel takes it as the
// argument ps, see profiles/sort_tree_modes/README.md).
template <bool FOLD>
__global__ void k_kb_union(const uint32_t* __restrict__ parent, uint32_t* uf, uint32_t B0,
                           uint32_t B1, uint32_t* bitmap, uint32_t anchor,
                           const uint32_t* __restrict__ anc, uint32_t ps,
                           const uint32_t* __restrict__ linked,
                           const uint32_t* __restrict__ n_linked,
                           const uint64_t* __restrict__ kept = nullptr,
                           const uint32_t* __restrict__ n_kept = nullptr) {
  anchor = anchor_rank(anchor, anc);
  const uint32_t R = anchor != INV ? uf_find_ro(uf, anchor) : INV;
  if (kept) {  // the pre-bucket roots k_kb_refresh linked: pairs (rt, b) with rt < b
    const uint32_t nk = *n_kept;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += gridDim.x * blockDim.x) {
      const uint64_t it = kept[i];
      const uint32_t r = (uint32_t)(it >> 32), b = (uint32_t)it;
      if (r < b) uf_union(uf, r, b, R);
    }
  }
  // the bucket's giant-path marks are consumed: clear them for the next bucket (words shared
  // with the next bucket hold no marks of it yet; the previous bucket cleared its own)
  if (!FOLD)
    for (uint32_t w = (B0 >> 5) + blockIdx.x * blockDim.x + threadIdx.x; w < ((B1 + 31) >> 5);
         w += gridDim.x * blockDim.x)
      bitmap[w] = 0;
  const uint32_t nl = *n_linked, width = B1 - B0;
  const uint64_t total = (uint64_t)width + nl;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t v = i < width ? B0 + (uint32_t)i : linked[i - width];
    uint32_t p = parent[(size_t)ps * v];
    if (p == INV) continue;
    if (FOLD && i < width && p < B1 && ((bitmap[v >> 5] >> (v & 31)) & 1) &&
        ((bitmap[p >> 5] >> (p & 31)) & 1))
      continue;
    uf_union(uf, v, p, R);
  }
}

// counters[1] = n_linked, [2] = n_spine, [3] = n_kept are reset here for the next bucket.
// clear_marks: the bucket's marks are cleared here (FOLD: k_kb_union read them).
// gbits (nullable): every rank of the bucket that ended in the component of the bitmap's
// reference vertex *gx gets its bit (one ballot-assembled word per 32 ranks).
__global__ void k_kb_label(const uint32_t* __restrict__ parent, uint32_t* uf, uint32_t* label,
                           uint32_t B0, uint32_t B1, uint32_t* counters, uint32_t* bitmap,
                           int clear_marks, uint32_t* gbits, const uint32_t* __restrict__ gx) {
  const uint32_t X = gbits ? *gx : INV;
  if (X == INV) {
    for (uint32_t v = B0 + blockIdx.x * blockDim.x + threadIdx.x; v < B1; v += gridDim.x * blockDim.x)
      if (parent[(size_t)KB_PS * v] == INV) label[uf_find<false>(uf, v)] = v;
  } else {
    const uint32_t RX = uf_find_ro(uf, X);
    const uint32_t v0 = B0 & ~63u;  // waves cover whole 64-rank (two-word) groups
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; v0 + (uint64_t)i < B1;
         i += gridDim.x * blockDim.x) {
      const uint32_t v = v0 + i;
      bool in = false;
      if (v >= B0) {
        const uint32_t rt = uf_find<false>(uf, v);
        if (parent[(size_t)KB_PS * v] == INV) label[rt] = v;
        in = rt == RX;
      }
      const uint64_t bal = __ballot(in);
      const int lane = threadIdx.x & 63;
      if (lane == 0 && (uint32_t)bal) atomicOr(&gbits[v >> 5], (uint32_t)bal);
      if (lane == 32 && (uint32_t)(bal >> 32)) atomicOr(&gbits[v >> 5], (uint32_t)(bal >> 32));
    }
  }
  if (clear_marks)
    for (uint32_t w = (B0 >> 5) + blockIdx.x * blockDim.x + threadIdx.x; w < ((B1 + 31) >> 5);
         w += gridDim.x * blockDim.x)
      bitmap[w] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) { counters[1] = 0; counters[2] = 0; counters[3] = 0; }
}

// Bucket boundaries by edge count: thread k finds m_valid (first INVALID hi), takes the rank at
// position k*m_valid/K and lower_bounds it.  out[2k] = B_k, out[2k+1] = first edge of bucket k.
__device__ __forceinline__ uint64_t lower_bound_hi(const uint64_t* a, uint64_t n, uint32_t key) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    uint64_t mid = (lo + hi) >> 1;
    if ((uint32_t)(a[mid] >> 32) < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Bucket boundaries: K_e by edge count (rank at edge quantile k/K_e) and K_r by rank
// (n_seq * k / K_r), so that no bucket is heavy in edges or wide in ranks (a wide bucket gets
// no union-find help: its in-bucket walks are long).  out[2i] = rank B, out[2i+1] = first
// edge with hi >= B; entry K_e + K_r carries (INVALID, m_valid).  The host merges and sorts.
__global__ void k_kb_bounds(const uint64_t* __restrict__ items, uint64_t n, uint32_t K_e,
                            uint32_t K_r, uint32_t n_seq, int gshift, unsigned long long* out) {
  uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t K = K_e + K_r;
  if (k > K) return;
  uint64_t mv = lower_bound_hi(items, n, INV);
  if (k == K) { out[2 * K] = INV; out[2 * K + 1] = mv; return; }
  uint32_t B;
  if (k < K_e) {
    uint64_t pos = mv * k / K_e;
    B = (k == 0 || mv == 0) ? 0u : (uint32_t)(items[pos] >> 32);
  } else {
    B = (uint32_t)((uint64_t)n_seq * (k - K_e) / K_r);
  }
  B = (B >> gshift) << gshift;  // items are sorted by hi down to groups of 2^gshift ranks
  out[2 * k] = B;
  out[2 * k + 1] = lower_bound_hi(items, mv, B);
}

void launch_kb_bounds(const uint64_t* items, uint64_t n, uint32_t K_e, uint32_t K_r,
                      uint32_t n_seq, int gshift, unsigned long long* out, hipStream_t s) {
  hipLaunchKernelGGL(k_kb_bounds, dim3((K_e + K_r + 1 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, s,
                     items, n, K_e, K_r, n_seq, gshift, out);
}

// kept: (e_end - e_begin) u64.
// The anchor is a rank whose component is taken as the giant: its elimination-tree root G is
// found when the map starts (marks) and again when the zipper starts (spine).  Any rank whose
// bucket has been applied before the map starts is exact: the two finds may see different
// roots while earlier buckets are still being folded into the union-find, but both lie in the
// anchor's component at rank B0, and an edge (a, b >= B0) may be moved to any vertex of a's
// component at B0.  (The pipelined loop maps bucket k+1 while bucket k is applied, so it
// anchors at the last rank of bucket k-1.)  INV: no giant (first buckets).
void launch_kb_map(const KbState& S, size_t k, const uint64_t* items, uint64_t e_begin,
                   uint64_t e_end, const KbSegs* segs, uint32_t B0, uint32_t anchor,
                   uint64_t* kept, uint64_t kept_cap, int gshift, const uint32_t* bins,
                   uint32_t nb, int defer, bool stats, hipStream_t s) {
  // segs: e_begin / e_end bound the bucket's records (the capacity of its bins)
  if (e_end <= e_begin) return;
  KbSegs sg{};
  if (segs) {
    sg = *segs;
    if (sg.i1 <= sg.i0 || sg.i1 - sg.i0 > 512) return;
  }
  uint64_t chunks = (e_end - e_begin + KM_CHUNK - 1) / KM_CHUNK;
  // One block per CU: the apply of the previous bucket (the loop's critical path) runs beside
  // this map, and more map blocks slow it down more than they speed the map up (RMAT-26 tree
  // phase 28.6 / 27.6 / 31.0 / 29.8 ms at 512 / 256 / 320 / 384 blocks; 192: 29.7).
  unsigned grid = (unsigned)std::min<uint64_t>(chunks, device_cus());
  const bool hub = e_end - e_begin >= (1ull << 25);
  auto mk = stats ? (hub ? k_kb_map<true, true> : k_kb_map<true, false>)
          : defer == 1 ? (hub ? k_kb_map<false, true, 1> : k_kb_map<false, false, 1>)
                       : (hub ? k_kb_map<false, true> : k_kb_map<false, false>);
  // the giant summary of the highest KM_GSUM words of ranks below B0 (the lo ends of most
  // records: a vertex is the lo end of its edges to higher-degree vertices) in dynamic LDS
  // (the first map has no summary yet: the first rebase, before map 1, writes it)
  const uint32_t* gsum = k >= 1 ? S.gsum : nullptr;
  const uint32_t w_end = (B0 + 2047) / 2048;
  const uint32_t gs_words = gsum ? std::min<uint32_t>(w_end, KM_GSUM) : 0u;
  const uint32_t gs_w0 = w_end - gs_words;
  hipLaunchKernelGGL(mk, dim3(grid), dim3(KM_THREADS), gs_words * 4, s, items, e_begin, e_end, sg,
                     B0, gshift, S.uf, (const uint32_t*)S.label, kept, S.cnt_of(k) + 3, S.bm_of(k),
                     S.hcnt, S.st, anchor, bins, nb, S.gbits, (const uint32_t*)S.gx_of(k), defer,
                     (const uint32_t*)S.anc_of(k), gsum, gs_words, gs_w0,
                     (uint32_t)std::min<uint64_t>(kept_cap, 0xFFFFFFFFull));
}

void launch_kb_rebase(const KbState& S, size_t j, uint32_t B0lim, hipStream_t s) {
  const uint32_t nwords = (uint32_t)S.bm_words;
  const unsigned grid = std::min<uint32_t>((nwords + BLOCK - 1) / BLOCK, 1024);
  // slot (j - 1) & 1 = (j + 1) & 1 holds what map j - 1 used
  hipLaunchKernelGGL(k_kb_pick, dim3(grid), dim3(BLOCK), 0, s, (const uint32_t*)S.uf, B0lim,
                     (const uint32_t*)S.anc_of(j + 1), S.anc_of(j), S.gbits, nwords,
                     (const uint32_t*)S.gx_of(j + 1), S.gx_of(j));
  if (S.gsum) launch_gb_sum(S.gbits, S.n_seq, S.gsum, s);
}

static bool kb_refresh_links() { return knobs().kb_rlink != 0; }

void launch_kb_apply(const KbState& S, size_t k, uint32_t B0, uint32_t B1, uint32_t anchor,
                     bool nonempty, uint64_t* kept, bool stats, size_t gx_slot, hipStream_t s) {
  uint32_t *uf = S.uf, *label = S.label, *parent = S.parent();
  uint32_t *linked = S.linked, *bitmap = S.bm_of(k), *spq = S.spq_of(k), *gbits = S.gbits;
  uint32_t* counters = S.cnt_of(k);
  uint32_t* n_linked = counters + 1;
  uint32_t* n_spine = counters + 2;
  uint32_t* n_kept = counters + 3;
  unsigned long long* st = S.st;
  const uint32_t* gx = S.gx_of(gx_slot);
  // this bucket's device anchor, and the next map's: the union keeps its root on top, so that
  // the map running beside it sees the giant's root unchanged
  const uint32_t *anc = S.anc_of(k), *anc_next = S.anc_of(k + 1);
  if (nonempty) {
    hipLaunchKernelGGL(k_kb_refresh, dim3(2048), dim3(BLOCK), 0, s, kept, (const uint32_t*)n_kept,
                       uf, (const uint32_t*)label, bitmap, B0, anchor, gbits, gx, anc,
                       kb_refresh_links() ? parent : (uint32_t*)nullptr);
    if (anchor != INV)  // the spine, and the giant fold of the marked ranks
      hipLaunchKernelGGL((k_kb_spine<true, true>), dim3(grid_for(((uint64_t)(B1 - B0) + 31) / 32 + 1)), dim3(BLOCK),
                         0, s, (const uint32_t*)bitmap, B0, B1, parent, spq, n_spine, uf, anchor,
                         gbits, gx, anc);
    // the zipper records the pre-bucket roots it links (LDS staging, one reservation per block)
    // for k_kb_union.  (Reading them back as the kept pairs' starts instead, with no recording:
    // tree phase +0.7 ms RMAT-26, +0.8 ms LJ-shape, +1.7 ms twitter-shape — DESIGN.md §9.)
    auto zk = stats ? k_kb_zip<true, true> : k_kb_zip<false, true>;
    // (a narrower window — 256 or 64 blocks sweeping the pairs in increasing order — made the
    // percolation bucket's walks longer, not shorter: LJ tree 3.19 -> 3.65 / 6.21 ms)
    hipLaunchKernelGGL(zk, dim3(MAX_GRID), dim3(BLOCK), 0, s, kept, (const uint32_t*)n_kept,
                       (const uint32_t*)bitmap, (const uint32_t*)spq, (const uint32_t*)n_spine, B0,
                       B1, uf, (const uint32_t*)label, parent, st + 8, linked, n_linked, anchor,
                       anc, (const uint32_t*)nullptr);
  }
  // giant fold: the marks are relative to the anchor's component; its root R_a may later be
  // linked below the union's R (pipelined: different anchors) — the folded ranks follow it
  const bool fold = nonempty && anchor != INV && B1 > B0;  // done by k_kb_spine
  // the linked pre-bucket roots (device count) can outnumber the bucket's ranks many times
  // over (hub buckets: ~500 ranks, ~0.3 M linked roots): a full grid, whatever the width
  unsigned ug = MAX_GRID;
  auto uk = fold ? k_kb_union<true> : k_kb_union<false>;
  const bool rl = nonempty && kb_refresh_links();
  hipLaunchKernelGGL(uk, dim3(ug), dim3(BLOCK), 0, s, (const uint32_t*)parent, uf, B0, B1,
                     bitmap, B0 > 0 ? B0 - 1 : INV, anc_next, KB_PS, (const uint32_t*)linked,
                     (const uint32_t*)n_linked, rl ? (const uint64_t*)kept : (const uint64_t*)nullptr,
                     rl ? (const uint32_t*)n_kept : (const uint32_t*)nullptr);
  hipLaunchKernelGGL(k_kb_label, dim3(grid_for((uint64_t)(B1 - B0) + 64)), dim3(BLOCK), 0, s,
                     (const uint32_t*)parent, uf, label, B0, B1, counters, bitmap, (int)fold,
                     gbits, gx);
}

void launch_kb_refresh(const KbState& S, size_t k, uint64_t* kept, const uint32_t* n_kept,
                       uint32_t* bitmap, uint32_t B0, uint32_t anchor, size_t gx_slot,
                       hipStream_t s) {
  hipLaunchKernelGGL(k_kb_refresh, dim3(2048), dim3(BLOCK), 0, s, kept, n_kept, S.uf,
                     (const uint32_t*)S.label, bitmap, B0, anchor, S.gbits,
                     (const uint32_t*)S.gx_of(gx_slot), (const uint32_t*)S.anc_of(k));
}

// ---- split lockstep apply (P ranks; sheep_capi.cpp ls_apply) ------------------------------
// The zipper of bucket [B0, B1) reads and writes parent[] / jump[] only at the pre-bucket roots
// its pairs start from (parent INVALID until this bucket) and at the bucket's own ranks (parent
// INVALID until this bucket); no other bucket's zipper touches those entries.  So with P ranks
// one owner rank runs a bucket's spine and zipper (on its own stream, off the loop's critical
// path), and every rank keeps only the union-find current: the fold of the marks, the union of
// the kept pairs themselves (not of the forest edges the zipper made) and the labels.  The
// owners' forests are disjoint and summed at the end (parent + 1, INVALID + 1 = 0).

// G for the owner's zipper: the giant's elimination-tree root at B0, before this bucket's union.
__global__ void k_ls_gslot(const uint32_t* uf, const uint32_t* __restrict__ label, uint32_t anchor,
                           const uint32_t* __restrict__ anc, uint32_t* gslot) {
  anchor = anchor_rank(anchor, anc);
  *gslot = anchor != INV ? label[uf_find_ro(uf, anchor)] : INV;
}

// union(g, b) for every kept pair of the P all-gathered contributions (recv, as k_ls_unpack
// reads it), straight from the exchange buffer.  g is the map's start — a vertex of the pair's
// component at B0, possibly stale, which the union does not mind (only the owner's zipper needs
// the refreshed pre-bucket root).  R (the next map's giant root) is never linked below another.
__global__ void k_ls_union_pairs(const uint64_t* __restrict__ recv, uint32_t P, uint32_t ms,
                                 uint32_t cap, uint32_t* uf, uint32_t anchor,
                                 const uint32_t* __restrict__ anc) {
  anchor = anchor_rank(anchor, anc);
  const uint32_t R = anchor != INV ? uf_find_ro(uf, anchor) : INV;
  const uint64_t stride = (uint64_t)ms + cap, total = (uint64_t)P * cap;
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
       j += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t r = j / cap, q = j - r * cap;
    const uint64_t it = recv[r * stride + ms + q];
    const uint32_t b = (uint32_t)(it >> 32);
    if (b != INV) uf_union(uf, (uint32_t)it, b, R);
  }
}

// Labels without the forest: every component this bucket touched holds one of its ranks, so its
// label (its maximum rank = its elimination-tree root) is the max over the bucket's ranks in it.
// One atomicMax per run of equal roots in consecutive lanes, and one per block for R (the giant:
// most ranks).  gbits / clearing / counters as k_kb_label.
__global__ void __launch_bounds__(BLOCK)
k_ls_label(uint32_t* uf, uint32_t* label, uint32_t B0, uint32_t B1, uint32_t* counters,
           uint32_t* bitmap, uint32_t* gbits, const uint32_t* __restrict__ gx, uint32_t anchor,
           const uint32_t* __restrict__ anc) {
  __shared__ uint32_t s_max;
  anchor = anchor_rank(anchor, anc);
  const uint32_t R = anchor != INV ? uf_find_ro(uf, anchor) : INV;
  const uint32_t X = gbits ? *gx : INV;
  const uint32_t RX = X != INV ? uf_find_ro(uf, X) : INV;
  if (threadIdx.x == 0) s_max = 0;
  block_sync();
  uint32_t rmax = 0;
  const int lane = threadIdx.x & 63;
  const uint32_t v0 = B0 & ~63u;  // waves cover whole 64-rank (two-word) groups
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; v0 + (uint64_t)i < B1 + 63;
       i += gridDim.x * blockDim.x) {
    const uint32_t v = v0 + i;
    const bool in_b = v >= B0 && v < B1;
    const uint32_t rt = in_b ? uf_find<false>(uf, v) : INV;
    const uint32_t nxt = (uint32_t)__shfl_down((int)rt, 1);
    if (in_b) {
      if (rt == R) rmax = max(rmax, v);
      else if (lane == 63 || nxt != rt) atomicMax(&label[rt], v);
    }
    if (X != INV) {
      const uint64_t bal = __ballot(in_b && rt == RX);
      if (lane == 0 && (uint32_t)bal) atomicOr(&gbits[v >> 5], (uint32_t)bal);
      if (lane == 32 && (uint32_t)(bal >> 32)) atomicOr(&gbits[v >> 5], (uint32_t)(bal >> 32));
    }
  }
  for (int o = 32; o > 0; o >>= 1) rmax = max(rmax, (uint32_t)__shfl_xor((int)rmax, o));
  if (lane == 0 && rmax) atomicMax(&s_max, rmax);
  block_sync();
  if (threadIdx.x == 0 && s_max) atomicMax(&label[R], s_max);
  for (uint32_t w = (B0 >> 5) + blockIdx.x * blockDim.x + threadIdx.x; w < ((B1 + 31) >> 5);
       w += gridDim.x * blockDim.x)
    bitmap[w] = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) { counters[1] = 0; counters[2] = 0; counters[3] = 0; }
}

void launch_ls_gslot(const KbState& S, size_t k, uint32_t anchor, uint32_t* gslot, hipStream_t s) {
  hipLaunchKernelGGL(k_ls_gslot, dim3(1), dim3(1), 0, s, (const uint32_t*)S.uf,
                     (const uint32_t*)S.label, anchor, (const uint32_t*)S.anc_of(k), gslot);
}

void launch_ls_fold_union_label(const KbState& S, size_t k, uint32_t B0, uint32_t B1,
                                uint32_t anchor, bool nonempty, const uint64_t* recv, uint32_t P,
                                uint32_t ms, uint32_t cap, size_t gx_slot, hipStream_t s) {
  uint32_t *uf = S.uf, *label = S.label, *bitmap = S.bm_of(k), *counters = S.cnt_of(k);
  uint32_t* gbits = S.gbits;
  const uint32_t *gx = S.gx_of(gx_slot), *anc = S.anc_of(k), *anc_next = S.anc_of(k + 1);
  const uint32_t anchor_next = B0 > 0 ? B0 - 1 : INV;
  if (nonempty) {
    if (anchor != INV && B1 > B0)  // the marked ranks go under the anchor's root (no forest)
      hipLaunchKernelGGL((k_kb_spine<false, true>), dim3(grid_for(((uint64_t)(B1 - B0) + 31) / 32 + 1)),
                         dim3(BLOCK), 0, s, (const uint32_t*)bitmap, B0, B1, nullptr, nullptr,
                         nullptr, uf, anchor, gbits, gx, anc);
    if (cap)
      hipLaunchKernelGGL(k_ls_union_pairs, dim3(MAX_GRID), dim3(BLOCK), 0, s, recv, P, ms, cap, uf,
                         anchor_next, anc_next);
  }
  if (B1 > B0)
    hipLaunchKernelGGL(k_ls_label, dim3(grid_for((uint64_t)(B1 - B0) + 128)), dim3(BLOCK), 0, s, uf,
                       label, B0, B1, counters, bitmap, gbits, gx, anchor_next, anc_next);
  else
    hipLaunchKernelGGL(k_kb_label, dim3(1), dim3(BLOCK), 0, s, (const uint32_t*)nullptr, uf, label, B0,
                       B1, counters, bitmap, 1, (uint32_t*)nullptr, (const uint32_t*)nullptr);
}

// The owner's half: spine (forest part) and zipper of one bucket over its copies of the kept
// pairs (zn[0] of them) and of the bucket's mark words; zn[1] = spine queue length (zeroed
// here), zn[2] = G (launch_ls_gslot; INV: no giant).
void launch_ls_zip(const uint64_t* zkept, uint32_t* zn, const uint32_t* zbm, uint32_t* zspq,
                   uint32_t B0, uint32_t B1, bool has_anchor, uint32_t* parent, hipStream_t s) {
  (void)hipMemsetAsync(zn + 1, 0, 4, s);
  if (has_anchor && B1 > B0)
    hipLaunchKernelGGL((k_kb_spine<true, false>), dim3(grid_for(((uint64_t)(B1 - B0) + 31) / 32 + 1)),
                       dim3(BLOCK), 0, s, zbm, B0, B1, parent, zspq, zn + 1, nullptr, 0u, nullptr,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr);
  hipLaunchKernelGGL((k_kb_zip<false, false>), dim3(MAX_GRID), dim3(BLOCK), 0, s, zkept,
                     (const uint32_t*)zn, zbm, (const uint32_t*)zspq, (const uint32_t*)(zn + 1), B0, B1,
                     nullptr, (const uint32_t*)nullptr, parent, nullptr, nullptr, nullptr,
                     has_anchor ? 0u : INV, (const uint32_t*)nullptr, (const uint32_t*)(zn + 2));
}

__global__ void k_add_u32(uint32_t* p, uint64_t n, uint32_t d) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    p[i] += d;
}

void launch_add_u32(uint32_t* p, uint64_t n, uint32_t d, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_add_u32, dim3(grid_for(n)), dim3(BLOCK), 0, s, p, n, d);
}

// ---- sharded degree sequence (multi-GPU, P > 1; sheep_capi.cpp sequence_sharded) ----------
// Rank r holds the global degrees of ids [r c, (r + 1) c) and sorts only those, stably by
// degree.  Ids of different ranks do not interleave, so the position in the global sequence of
// the i-th of r's items, of degree d, is
//   (ids of degree < d, all ranks) + (ids of degree d on ranks < r) + (i - first i of degree d)
// and every term comes from the ranks' histograms over degree values (all-gathered).

// Run bounds of each degree in the sorted local items: lst[d] = first index, H[d] = run length
// (H zeroed; absent degrees keep H = 0 and are never read in lst).
__global__ void k_seq_runs(const uint64_t* __restrict__ sorted, uint32_t n, uint32_t* lst,
                           uint32_t* H) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t d = (uint32_t)(sorted[i] >> 32);
    if (i == 0 || (uint32_t)(sorted[i - 1] >> 32) != d) {
      lst[d] = i;
      atomicSub(&H[d], i);
    }
    if (i + 1 == n || (uint32_t)(sorted[i + 1] >> 32) != d) atomicAdd(&H[d], i + 1);
  }
}

// hall: P rows of Dp words (rank q's H).  tot[d] = ids of degree d over all ranks, pre[d] =
// those on ranks < r.
__global__ void k_seq_base(const uint32_t* __restrict__ hall, uint32_t P, uint32_t r, uint32_t D,
                           uint32_t Dp, uint32_t* __restrict__ tot, uint32_t* __restrict__ pre) {
  for (uint32_t d = blockIdx.x * blockDim.x + threadIdx.x; d < D; d += gridDim.x * blockDim.x) {
    uint32_t t = 0, p = 0;
    for (uint32_t q = 0; q < P; ++q) {
      const uint32_t h = hall[(uint64_t)q * Dp + d];
      t += h;
      if (q < r) p += h;
    }
    tot[d] = t;
    pre[d] = p;
  }
}

// rank_slice[local id] = global position (S: exclusive prefix of tot).
__global__ void k_seq_rank(const uint64_t* __restrict__ sorted, uint32_t n, const uint32_t* __restrict__ S,
                           const uint32_t* __restrict__ pre, const uint32_t* __restrict__ lst,
                           uint32_t* __restrict__ rank_slice) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint64_t it = sorted[i];
    const uint32_t d = (uint32_t)(it >> 32);
    rank_slice[(uint32_t)it] = S[d] + pre[d] + (i - lst[d]);
  }
}

// seq[rank[v]] = v (jtree.h:165-168 the other way round).
__global__ void k_seq_from_rank(const uint32_t* __restrict__ rank, uint32_t n_ids,
                                uint32_t* __restrict__ seq) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n_ids; v += gridDim.x * blockDim.x) {
    const uint32_t r = rank[v];
    if (r != INV) seq[r] = v;
  }
}

// The global degree at every position of the sequence (non-decreasing): the largest d with
// S[d] <= p (an absent degree has S[d] = S[d + 1], so the largest such d is present).
__global__ void k_deg_of_rank(const uint32_t* __restrict__ S, uint32_t D, uint32_t n_seq,
                              uint32_t* __restrict__ out) {
  for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n_seq; p += gridDim.x * blockDim.x) {
    uint32_t lo = 1, hi = D - 1;  // S[1] = 0 <= p (degree 0 is never sorted: tot[0] = 0)
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (S[mid] <= p) lo = mid;
      else hi = mid - 1;
    }
    out[p] = lo;
  }
}

// [0] = this rank's max degree, [1] = its ids of degree > 0 (from k_deg_stats over c ids).
__global__ void k_seq_stats64(const uint32_t* __restrict__ stats, uint32_t c, long long* out) {
  out[0] = stats[0];
  out[1] = (long long)(c - stats[1]);
}

void launch_seq_runs(const uint64_t* sorted, uint32_t n, uint32_t* lst, uint32_t* H, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_seq_runs, dim3(grid_for(n)), dim3(BLOCK), 0, s, sorted, n, lst, H);
}
void launch_seq_base(const uint32_t* hall, uint32_t P, uint32_t r, uint32_t D, uint32_t Dp,
                     uint32_t* tot, uint32_t* pre, hipStream_t s) {
  if (D) hipLaunchKernelGGL(k_seq_base, dim3(grid_for(D)), dim3(BLOCK), 0, s, hall, P, r, D, Dp, tot, pre);
}
void launch_seq_rank(const uint64_t* sorted, uint32_t n, const uint32_t* S, const uint32_t* pre,
                     const uint32_t* lst, uint32_t* rank_slice, hipStream_t s) {
  if (n)
    hipLaunchKernelGGL(k_seq_rank, dim3(grid_for(n)), dim3(BLOCK), 0, s, sorted, n, S, pre, lst,
                       rank_slice);
}
void launch_seq_from_rank(const uint32_t* rank, uint32_t n_ids, uint32_t* seq, hipStream_t s) {
  if (n_ids) hipLaunchKernelGGL(k_seq_from_rank, dim3(grid_for(n_ids)), dim3(BLOCK), 0, s, rank, n_ids, seq);
}
void launch_deg_of_rank(const uint32_t* S, uint32_t D, uint32_t n_seq, uint32_t* out, hipStream_t s) {
  if (n_seq && D > 1)
    hipLaunchKernelGGL(k_deg_of_rank, dim3(grid_for(n_seq)), dim3(BLOCK), 0, s, S, D, n_seq, out);
}
void launch_seq_stats64(const uint32_t* stats, uint32_t c, long long* out, hipStream_t s) {
  hipLaunchKernelGGL(k_seq_stats64, dim3(1), dim3(1), 0, s, stats, c, out);
}

// ---- lockstep exchange (multi-GPU kb loop, sheep_ls_*) -----------------------------------
// One rank's contribution to a bucket, laid out for one all-gather: `ms` u64 slots holding the
// bucket's mark words [w0, w1] (two per slot, zero beyond w1), then `cap` kept pairs, padded
// past this rank's *d_kept (the map's count, cap >= it) with INVALID (b = INVALID: skipped by
// the zipper).
// The same rank's count as an int64 for the caller's MAX all-reduce.
__global__ void k_ls_count(const uint32_t* __restrict__ n_kept, long long* out) { *out = *n_kept; }

void launch_ls_count(const uint32_t* n_kept, long long* out, hipStream_t s) {
  hipLaunchKernelGGL(k_ls_count, dim3(1), dim3(1), 0, s, n_kept, out);
}

__global__ void k_ls_pack(const uint32_t* __restrict__ bitmap, uint32_t w0, uint32_t w1,
                          uint32_t ms, uint64_t* send, const uint32_t* __restrict__ d_kept,
                          uint32_t cap) {
  const uint64_t total = (uint64_t)ms + cap;
  const uint32_t n_kept = *d_kept;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (i < ms) {
      const uint32_t a = w0 + 2 * (uint32_t)i, b = a + 1;
      const uint64_t lo = a <= w1 ? bitmap[a] : 0u, hi = b <= w1 ? bitmap[b] : 0u;
      send[i] = lo | (hi << 32);
    } else if (i - ms >= n_kept) {
      send[i] = ~0ull;
    }
  }
}

// The all-gathered contributions of P ranks (P blocks of ms + cap slots): the mark words are
// OR-ed over ranks into bitmap[w0, w1], the kept pairs copied to kept (P * cap, pads
// included) and n_kept = P * cap.
__global__ void k_ls_unpack(const uint64_t* __restrict__ recv, uint32_t P, uint32_t ms,
                            uint32_t cap, uint32_t* bitmap, uint32_t w0, uint32_t w1,
                            uint64_t* __restrict__ kept, uint32_t* n_kept) {
  const uint64_t stride = (uint64_t)ms + cap;
  const uint32_t nw = w1 - w0 + 1;
  const uint64_t total = (uint64_t)nw + (kept ? (uint64_t)P * cap : 0ull);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    if (i < nw) {
      uint32_t v = 0;
      for (uint32_t r = 0; r < P; ++r) {
        const uint64_t s = recv[r * stride + (i >> 1)];
        v |= (uint32_t)(i & 1 ? s >> 32 : s);
      }
      bitmap[w0 + i] = v;
    } else {
      const uint64_t j = i - nw, r = j / cap, q = j - r * cap;
      kept[j] = recv[r * stride + ms + q];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && n_kept) *n_kept = P * cap;
}

void launch_ls_pack(const uint32_t* bitmap, uint32_t w0, uint32_t w1, uint32_t ms, uint64_t* send,
                    const uint32_t* n_kept, uint32_t cap, hipStream_t s) {
  const uint64_t total = (uint64_t)ms + cap;
  if (total)
    hipLaunchKernelGGL(k_ls_pack, dim3(grid_for(total)), dim3(BLOCK), 0, s, bitmap, w0, w1, ms, send,
                       n_kept, cap);
}

void launch_ls_unpack(const uint64_t* recv, uint32_t P, uint32_t ms, uint32_t cap, uint32_t* bitmap,
                      uint32_t w0, uint32_t w1, uint64_t* kept, uint32_t* n_kept, hipStream_t s) {
  const uint64_t total = (uint64_t)(w1 - w0 + 1) + (kept ? (uint64_t)P * cap : 0ull);
  hipLaunchKernelGGL(k_ls_unpack, dim3(grid_for(total)), dim3(BLOCK), 0, s, recv, P, ms, cap, bitmap,
                     w0, w1, kept, n_kept);
}

// Items of one forest over n ranks for a union build: (parent[v] << 32 | v); a root's INVALID
// parent becomes an INVALID hi, which sorts after every rank.
// The kb loop's interleaved parent / hint words: (INVALID, 0) to start; the parents out.
__global__ void k_pj_init(uint64_t* pj, uint32_t n) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
    pj[v] = (uint64_t)INV;
}
__global__ void k_pj_parents(const uint64_t* __restrict__ pj, uint32_t n, uint32_t* parent) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
    parent[v] = (uint32_t)pj[v];
}
void launch_pj_init(uint32_t* pj, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_pj_init, dim3(grid_for(n)), dim3(BLOCK), 0, s, (uint64_t*)pj, n);
}
void launch_pj_parents(const uint32_t* pj, uint32_t n, uint32_t* parent, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_pj_parents, dim3(grid_for(n)), dim3(BLOCK), 0, s, (const uint64_t*)pj, n,
                            parent);
}

__global__ void k_forest_items(const uint32_t* __restrict__ parent, uint32_t n,
                               uint64_t* __restrict__ items) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
    items[v] = ((uint64_t)parent[v] << 32) | v;
}

void launch_forest_items(const uint32_t* parent, uint32_t n, uint64_t* items, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_forest_items, dim3(grid_for(n)), dim3(BLOCK), 0, s, parent, n, items);
}

// ---- reductions of the in-process rank group (sheep_comm.cpp LocalComm) ---------------------
template <typename T, bool MAX>
__global__ void k_reduce_ptrs(T* dst, const T* const* srcs, int P, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    T v = srcs[0][i];
    for (int q = 1; q < P; ++q) v = MAX ? (srcs[q][i] > v ? srcs[q][i] : v) : (T)(v + srcs[q][i]);
    dst[i] = v;
  }
}

void launch_sum_ptrs_u32(uint32_t* dst, const uint32_t* const* srcs, int P, size_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_reduce_ptrs<uint32_t, false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, dst, srcs, P, n);
}
void launch_sum_ptrs_u64(uint64_t* dst, const uint64_t* const* srcs, int P, size_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_reduce_ptrs<uint64_t, false>), dim3(grid_for(n)), dim3(BLOCK), 0, s, dst, srcs, P, n);
}
void launch_max_ptrs_i64(int64_t* dst, const int64_t* const* srcs, int P, size_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL((k_reduce_ptrs<int64_t, true>), dim3(grid_for(n)), dim3(BLOCK), 0, s, dst, srcs, P, n);
}

// ---- .dat ingest (LLAMA's load_direct of XS1 records, graph_wrapper.h:43-63) -----------------
__global__ void k_strip_xs1(const uint32_t* __restrict__ raw, uint64_t n, uint32_t* __restrict__ uv,
                            uint32_t* max_id) {
  uint32_t mx = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t t = raw[3 * i], h = raw[3 * i + 1];
    ((uint2*)uv)[i] = make_uint2(t, h);
    const uint32_t top = max(t, h);  // an id 0xFFFFFFFF (INVALID) saturates: the host rejects it
    mx = max(mx, top == INV ? INV : top + 1);
  }
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(max_id, mx);
}

void launch_strip_xs1(const uint32_t* raw, uint64_t n, uint32_t* uv, uint32_t* max_id, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_strip_xs1, dim3(grid_for(n)), dim3(BLOCK), 0, s, raw, n, uv, max_id);
}

__global__ void k_iota(uint32_t* p, uint32_t n) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = i;
}

void launch_iota(uint32_t* p, uint32_t n, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_iota, dim3(grid_for(n)), dim3(BLOCK), 0, s, p, n);
}

// Merge (jnode.cpp:174-201): insert every edge (v, parent_b[v]) of tree B into tree A;
// pst_weight sums (u32 wrap-around, as the reference's esize_t += ).
__global__ void k_merge(uint32_t* parent_a, uint32_t* __restrict__ pst_a,
                        const uint32_t* __restrict__ parent_b, const uint32_t* __restrict__ pst_b,
                        uint32_t n, uint32_t* jump) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    pst_a[v] += pst_b[v];
    uint32_t p = parent_b[v];
    if (p != INV) zip_insert(parent_a, jump, v, p);
  }
}

void launch_merge(uint32_t* parent_a, uint32_t* pst_a, const uint32_t* parent_b,
                  const uint32_t* pst_b, uint32_t n, uint32_t* jump, hipStream_t s) {
  if (n == 0) return;
  (void)hipMemsetAsync(jump, 0, (size_t)n * 4, s);
  hipLaunchKernelGGL(k_merge, dim3(grid_for(n)), dim3(BLOCK), 0, s, parent_a, pst_a, parent_b,
                     pst_b, n, jump);
}

// ---------------------------------------------------------------------------------------
// R-MAT generator (rmat.h).
// ---------------------------------------------------------------------------------------
__global__ void k_rmat(uint2* __restrict__ uv, int scale, uint64_t seed, uint64_t e_begin,
                       uint64_t n) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint32_t t, h;
    sheep_rmat::edge(e_begin + i, scale, seed, &t, &h);
    uv[i] = make_uint2(t, h);
  }
}

__global__ void k_powerlaw(uint2* __restrict__ uv, sheep_pl::Table t, uint64_t seed,
                           uint64_t e_begin, uint64_t n) {
  uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint32_t a, b;
    sheep_pl::edge(t, e_begin + i, seed, &a, &b);
    uv[i] = make_uint2(a, b);
  }
}

void launch_powerlaw(uint32_t* uv, uint32_t n, double gamma, double i0, uint64_t seed,
                     uint64_t e_begin, uint64_t e_end, hipStream_t s) {
  if (e_end <= e_begin) return;
  const sheep_pl::Table t = sheep_pl::powerlaw_table(n, gamma, i0);
  hipLaunchKernelGGL(k_powerlaw, dim3(grid_for(e_end - e_begin)), dim3(BLOCK), 0, s, (uint2*)uv, t,
                     seed, e_begin, e_end - e_begin);
}

void launch_rmat(uint32_t* uv, int scale, uint64_t seed, uint64_t e_begin, uint64_t e_end,
                 hipStream_t s) {
  if (e_end <= e_begin) return;
  hipLaunchKernelGGL(k_rmat, dim3(grid_for(e_end - e_begin)), dim3(BLOCK), 0, s, (uint2*)uv, scale,
                     seed, e_begin, e_end - e_begin);
}

}  // namespace sheep
