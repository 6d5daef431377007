// Certificate of an elimination tree on the GPU (sheep_verify_tree_dev) and the TREEFAQS digest
// of a tree in HBM (sheep_tree_facts_dev); DESIGN.md §4.7 has the theorem and the byte counts.
//
// In rank space, with every parent INVALID or in (v, n_seq) (heap order), the forest is the
// elimination tree of the records iff
//   (A) for every record (lo, hi), hi is an ancestor of lo, and
//   (B) every non-root v has a witness: a record (x, parent[v]) with x in the subtree of v.
// Both are interval tests once every rank has its entry and exit position in an Euler tour of
// the forest, and the tour comes from the children lists by list ranking.  No pass follows
// parent pointers or walks one vertex's children: the work is O(n log n + m log(max kids)) and
// the steps O(log n), whatever the height (a path) or the fan-out (a star).
//
//   k_vf_heap      heap order, roots                          one pass over parent
//   k_vf_items     (parent << 32 | v), roots under the virtual parent n; radix_sort_u64 by parent
//   k_vf_runs      first and last slot of every parent's run of the sorted items
//   k_vf_succ      the 2n arcs' successors as (succ << 32 | 1) cells (verify_layout.h)
//   k_vf_jump      pointer jumping, ceil(log2 2n) rounds, double-buffered
//   k_vf_times     (tin, tout) per rank, tin per children-list slot
//   k_vf_records   per record: pst recount, (A), the witness mark of the child of hi above lo
//   k_vf_final     per rank: unwitnessed non-roots, pst mismatches
//   k_vf_weights / k_vf_scan_* / k_vf_facts   depths and pst-weighted depths as prefix sums in
//                  tour order; width, roots, heights, edges, halo
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sheep_amd kernels are written for gfx950 only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sheep_internal.h"
#include "verify_layout.h"

namespace sheep {

static constexpr int VF_BLOCK = 256;
static constexpr int VF_SCAN_T = 1024;           // threads of a scan block
static constexpr int VF_SCAN_TILE = 4 * VF_SCAN_T;  // values of a scan tile

static inline unsigned vf_grid(uint64_t n) {
  uint64_t g = (n + VF_BLOCK - 1) / VF_BLOCK;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, 4096));
}

// The low word of a counter word holds a rank minimum (little endian; the high word stays 0).
__device__ __forceinline__ void vf_min_rank(unsigned long long* w, uint32_t v) {
  if (v != INV) atomicMin((uint32_t*)w, v);
}

__global__ void k_vf_init(unsigned long long* ws) {
  const int t = threadIdx.x;
  if (t < VF_WS_WORDS) ws[t] = (t == VF_MIN || t == VF_HALO) ? (unsigned long long)INV : 0ull;
}

__global__ void k_vf_heap(const uint32_t* __restrict__ parent, uint32_t n, unsigned long long* ws) {
  unsigned long long bad = 0, roots = 0;
  uint32_t first = INV;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t p = parent[v];
    if (!vf_heap_ok(v, p, n)) { ++bad; first = min(first, v); }
    roots += p == INV;
  }
  bad = vf_wave_sum(bad);
  roots = vf_wave_sum(roots);
  first = vf_wave_min(first);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&ws[VF_HEAP], bad);
    if (roots) atomicAdd(&ws[VF_ROOTS], roots);
    vf_min_rank(&ws[VF_MIN], first);
  }
}

__global__ void k_vf_items(const uint32_t* __restrict__ parent, uint32_t n,
                           uint64_t* __restrict__ items) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x)
    items[v] = vf_item(v, parent[v], n);
}

// kfirst / klast (n + 1 entries, kfirst filled with VF_NONE): the run of every parent.
__global__ void k_vf_runs(const uint64_t* __restrict__ kids, uint32_t n,
                          uint32_t* __restrict__ kfirst, uint32_t* __restrict__ klast) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t p = vf_par(kids[i]);
    if (i == 0 || vf_par(kids[i - 1]) != p) kfirst[p] = i;
    if (i + 1 == n || vf_par(kids[i + 1]) != p) klast[p] = i;
  }
}

__global__ void k_vf_succ(const uint64_t* __restrict__ kids, const uint32_t* __restrict__ kfirst,
                          uint32_t n, uint64_t* __restrict__ cells) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    uint32_t sd, su;
    vf_succ(kids, kfirst, n, i, &sd, &su);
    const uint32_t v = vf_kid(kids[i]);
    cells[vf_down(v)] = vf_cell(sd);
    cells[vf_up(n, v)] = vf_cell(su);
  }
}

__global__ void k_vf_jump(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint32_t n2) {
  for (uint64_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n2; a += gridDim.x * blockDim.x) {
    uint64_t x = src[a];
    const uint32_t s = (uint32_t)(x >> 32);
    if (s != VF_END) x = vf_jump(x, src[s]);
    dst[a] = x;
  }
}

__global__ void k_vf_times(const uint64_t* __restrict__ cells, const uint64_t* __restrict__ kids,
                           uint32_t n, uint2* __restrict__ tt, uint32_t* __restrict__ ktin) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t v = vf_kid(kids[i]);
    const uint32_t tin = vf_pos(cells[vf_down(v)], n), tout = vf_pos(cells[vf_up(n, v)], n);
    tt[v] = make_uint2(tin, tout);
    ktin[i] = tin;
  }
}

struct VfRec {
  const uint32_t* rank;
  uint32_t n_ids, n_seq;
  const uint32_t* parent;
  const uint2* tt;
  const uint32_t *kfirst, *klast, *ktin;
  const uint64_t* kids;
  uint32_t* cnt;     // nullable: the pst recount
  uint8_t* witness;  // one byte per rank, plain stores of 1
  uint32_t* err;
};

// One record: the edge pass's rule (sheep_kernels.hip "Edge pass") for what counts, then (A)
// and the witness.  Returns false for a record that violates (A); *lo_out its lower rank.
__device__ __forceinline__ bool vf_record(const VfRec& R, uint32_t x, uint32_t y, uint32_t* lo_out) {
  if (x == y) return true;
  const bool ox = x >= R.n_ids, oy = y >= R.n_ids;
  const uint32_t rx = ox ? INV : R.rank[x], ry = oy ? INV : R.rank[y];
  if ((ox && ry != INV) || (oy && rx != INV)) { atomicOr(R.err, ERR_RANGE); return true; }
  const uint32_t lo = min(rx, ry), hi = max(rx, ry);
  if (lo == INV) return true;
  // a rank map that points past the tree would index out of every table below
  if (lo >= R.n_seq || (hi != INV && hi >= R.n_seq)) { atomicOr(R.err, ERR_RANGE); return true; }
  if (R.cnt) atomicAdd(&R.cnt[lo], 1u);
  if (hi == INV || lo == hi) return true;
  const uint2 tl = R.tt[lo], th = R.tt[hi];
  if (!vf_in_subtree(tl.x, th.x, th.y)) { *lo_out = lo; return false; }
  uint32_t c = lo;
  if (R.parent[lo] != hi) {
    // the child of hi whose interval holds tin[lo]: the last slot of hi's list with tin <= it
    uint32_t a = R.kfirst[hi], b = R.klast[hi];
    if (a == VF_NONE) return true;  // (unreachable: hi has a descendant)
    while (a < b) {
      const uint32_t mid = a + (b - a + 1) / 2;
      if (R.ktin[mid] <= tl.x) a = mid; else b = mid - 1;
    }
    c = vf_kid(R.kids[a]);
  }
  R.witness[c] = 1;
  return true;
}

// Two records per 16-byte load; the record before a 16-byte boundary and an odd last one are
// thread 0's.
__global__ void __launch_bounds__(VF_BLOCK)
k_vf_records(const uint32_t* __restrict__ uv, uint64_t m, VfRec R, unsigned long long* ws) {
  unsigned long long bad = 0;
  uint32_t first = INV;
  auto one = [&](uint32_t x, uint32_t y) {
    uint32_t lo = INV;
    if (!vf_record(R, x, y, &lo)) { ++bad; first = min(first, lo); }
  };
  const uint64_t head = (((uintptr_t)uv & 15u) && m) ? 1 : 0;
  const uint64_t pairs = (m - head) / 2;
  const uint4* p4 = (const uint4*)(uv + 2 * head);
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < pairs;
       j += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 r = p4[j];
    one(r.x, r.y);
    one(r.z, r.w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) one(uv[0], uv[1]);
    const uint64_t tail = head + 2 * pairs;
    if (tail < m) one(uv[2 * tail], uv[2 * tail + 1]);
  }
  bad = vf_wave_sum(bad);
  first = vf_wave_min(first);
  if ((threadIdx.x & 63) == 0) {
    if (bad) atomicAdd(&ws[VF_A], bad);
    vf_min_rank(&ws[VF_MIN], first);
  }
}

__global__ void k_vf_final(const uint32_t* __restrict__ parent, const uint32_t* __restrict__ pst,
                           const uint32_t* __restrict__ cnt, const uint8_t* __restrict__ witness,
                           uint32_t n, unsigned long long* ws) {
  unsigned long long nb = 0, np = 0;
  uint32_t first = INV;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const bool b = parent[v] != INV && !witness[v];
    const bool p = pst && pst[v] != cnt[v];
    nb += b;
    np += p;
    if (b || p) first = min(first, v);
  }
  nb = vf_wave_sum(nb);
  np = vf_wave_sum(np);
  first = vf_wave_min(first);
  if ((threadIdx.x & 63) == 0) {
    if (nb) atomicAdd(&ws[VF_B], nb);
    if (np) atomicAdd(&ws[VF_PST], np);
    vf_min_rank(&ws[VF_MIN], first);
  }
}

// ---- facts: depths as prefix sums in tour order ---------------------------------------------
// wv[pos] = +1 / -1 and we[pos] = +pst / -pst of the arc at tour position pos.
__global__ void k_vf_weights(const uint2* __restrict__ tt, const uint32_t* __restrict__ pst,
                             uint32_t n, long long* __restrict__ wv, long long* __restrict__ we) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint2 t = tt[v];
    const long long w = pst[v];
    wv[t.x] = 1;
    wv[t.y] = -1;
    we[t.x] = w;
    we[t.y] = -w;
  }
}

// Inclusive scan of a block's VF_SCAN_T values (one per thread); *total: the block's sum.
__device__ __forceinline__ long long vf_block_scan(long long x, long long* total) {
  __shared__ long long wsum[VF_SCAN_T / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  __syncthreads();  // (a second call's writes wait for the first call's reads)
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  long long base = 0, all = 0;
  for (int k = 0; k < VF_SCAN_T / 64; ++k) {
    const long long s = wsum[k];
    if (k < w) base += s;
    all += s;
  }
  *total = all;
  return x + base;
}

// sums[b] = sum of tile b.
__global__ void __launch_bounds__(VF_SCAN_T)
k_vf_scan_sums(const long long* __restrict__ in, uint64_t n, long long* __restrict__ sums) {
  const uint64_t base = (uint64_t)blockIdx.x * VF_SCAN_TILE + 4 * (uint64_t)threadIdx.x;
  long long x = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (base + k < n) x += in[base + k];
  long long total;
  vf_block_scan(x, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// Exclusive scan of the nt tile sums in place: one block, each thread a run of them.
__global__ void __launch_bounds__(VF_SCAN_T) k_vf_scan_top(long long* sums, uint64_t nt) {
  const uint64_t per = (nt + VF_SCAN_T - 1) / VF_SCAN_T;
  const uint64_t b = per * threadIdx.x, e = b + per < nt ? b + per : nt;
  long long x = 0;
  for (uint64_t i = b; i < e; ++i) x += sums[i];
  long long total;
  long long run = vf_block_scan(x, &total) - x;
  for (uint64_t i = b; i < e; ++i) {
    const long long s = sums[i];
    sums[i] = run;
    run += s;
  }
}

// Inclusive scan in place, given the exclusive tile sums.
__global__ void __launch_bounds__(VF_SCAN_T)
k_vf_scan_apply(long long* __restrict__ io, uint64_t n, const long long* __restrict__ sums) {
  const uint64_t base = (uint64_t)blockIdx.x * VF_SCAN_TILE + 4 * (uint64_t)threadIdx.x;
  long long v[4];
  long long x = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = base + k < n ? io[base + k] : 0;
    x += v[k];
  }
  long long total;
  long long run = vf_block_scan(x, &total) - x + sums[blockIdx.x];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    run += v[k];
    if (base + k < n) io[base + k] = run;
  }
}

// sv / se: the inclusive scans of wv / we.  A rank's height in vertices is sv[tin], in pst
// weight se[tin] (JNodeTable::Facts folds the same sums from the leaves up; the maxima agree).
__global__ void k_vf_facts(const uint2* __restrict__ tt, const uint32_t* __restrict__ pst, uint32_t n,
                           const long long* __restrict__ sv, const long long* __restrict__ se,
                           unsigned long long* ws) {
  unsigned long long width = 0, edges = 0, vh = 0, eh = 0;
  uint32_t halo = INV;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const unsigned long long w = pst[v];
    width = max(width, w + 1);
    edges += w;
    if (w + 1 > 3) halo = min(halo, v);
    const uint32_t tin = tt[v].x;
    vh = max(vh, (unsigned long long)sv[tin]);
    eh = max(eh, (unsigned long long)se[tin]);
  }
  width = vf_wave_max(width);
  edges = vf_wave_sum(edges);
  vh = vf_wave_max(vh);
  eh = vf_wave_max(eh);
  halo = vf_wave_min(halo);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&ws[VF_WIDTH], width);
    if (edges) atomicAdd(&ws[VF_EDGES], edges);
    atomicMax(&ws[VF_VH], vh);
    atomicMax(&ws[VF_EH], eh);
    vf_min_rank(&ws[VF_HALO], halo);
  }
}

// ---- launchers ------------------------------------------------------------------------------

void launch_vf_heap(const uint32_t* parent, uint32_t n, unsigned long long* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_vf_init, dim3(1), dim3(64), 0, s, ws);
  if (n) hipLaunchKernelGGL(k_vf_heap, dim3(vf_grid(n)), dim3(VF_BLOCK), 0, s, parent, n, ws);
}

void launch_vf_items(const uint32_t* parent, uint32_t n, uint64_t* items, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_vf_items, dim3(vf_grid(n)), dim3(VF_BLOCK), 0, s, parent, n, items);
}

void launch_vf_tour(const VfTour& T, hipStream_t s) {
  const uint32_t n = T.n;
  if (n == 0) return;
  const dim3 g(vf_grid(n)), b(VF_BLOCK);
  launch_fill(T.kfirst, VF_NONE, (uint64_t)n + 1, s);
  hipLaunchKernelGGL(k_vf_runs, g, b, 0, s, T.kids, n, T.kfirst, T.klast);
  hipLaunchKernelGGL(k_vf_succ, g, b, 0, s, T.kids, (const uint32_t*)T.kfirst, n, T.cells_a);
  const uint64_t* src = T.cells_a;
  uint64_t* dst = T.cells_b;
  const dim3 g2(vf_grid(2ull * n));
  for (int r = vf_rounds(n); r > 0; --r) {
    hipLaunchKernelGGL(k_vf_jump, g2, b, 0, s, src, dst, 2u * n);
    uint64_t* t = (uint64_t*)src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(k_vf_times, g, b, 0, s, src, T.kids, n, T.tt, T.ktin);
}

void launch_vf_records(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_ids,
                       const uint32_t* parent, const VfTour& T, uint32_t* cnt, uint8_t* witness,
                       unsigned long long* ws, uint32_t* err, hipStream_t s) {
  if (m == 0) return;
  VfRec R;
  R.rank = rank;
  R.n_ids = n_ids;
  R.n_seq = T.n;
  R.parent = parent;
  R.tt = T.tt;
  R.kfirst = T.kfirst;
  R.klast = T.klast;
  R.ktin = T.ktin;
  R.kids = T.kids;
  R.cnt = cnt;
  R.witness = witness;
  R.err = err;
  hipLaunchKernelGGL(k_vf_records, dim3(vf_grid((m + 1) / 2)), dim3(VF_BLOCK), 0, s, uv, m, R, ws);
}

void launch_vf_final(const uint32_t* parent, const uint32_t* pst, const uint32_t* cnt,
                     const uint8_t* witness, uint32_t n, unsigned long long* ws, hipStream_t s) {
  if (n) hipLaunchKernelGGL(k_vf_final, dim3(vf_grid(n)), dim3(VF_BLOCK), 0, s, parent, pst, cnt,
                            witness, n, ws);
}

size_t vf_scan_tiles(uint32_t n) { return (size_t)((2ull * n + VF_SCAN_TILE - 1) / VF_SCAN_TILE); }

void launch_vf_scan(long long* io, uint32_t n, long long* sums, hipStream_t s) {
  if (n == 0) return;
  const uint64_t n2 = 2ull * n, nt = vf_scan_tiles(n);
  hipLaunchKernelGGL(k_vf_scan_sums, dim3((unsigned)nt), dim3(VF_SCAN_T), 0, s, (const long long*)io,
                     n2, sums);
  hipLaunchKernelGGL(k_vf_scan_top, dim3(1), dim3(VF_SCAN_T), 0, s, sums, nt);
  hipLaunchKernelGGL(k_vf_scan_apply, dim3((unsigned)nt), dim3(VF_SCAN_T), 0, s, io, n2,
                     (const long long*)sums);
}

void launch_vf_facts(const VfTour& T, const uint32_t* pst, long long* wv, long long* we,
                     long long* sums, unsigned long long* ws, hipStream_t s) {
  const uint32_t n = T.n;
  if (n == 0) return;
  hipLaunchKernelGGL(k_vf_weights, dim3(vf_grid(n)), dim3(VF_BLOCK), 0, s, (const uint2*)T.tt, pst, n,
                     wv, we);
  for (long long* w : {wv, we}) launch_vf_scan(w, n, sums, s);
  hipLaunchKernelGGL(k_vf_facts, dim3(vf_grid(n)), dim3(VF_BLOCK), 0, s, (const uint2*)T.tt, pst, n,
                     (const long long*)wv, (const long long*)we, ws);
}

}  // namespace sheep
