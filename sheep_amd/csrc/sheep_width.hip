// Exact width and fill of an elimination tree on the GPU (sheep_tree_widths_dev); DESIGN.md §4.9
// has the theorem and the byte counts.
//
// In rank space, width[j] = 1 + |jxn(j)| is the number of row subtrees that contain j: the row
// subtree of an upper end hi is the union of the tree paths from its distinct lower ends up to
// hi.  With the lower ends of one hi in tour order a_1 .. a_k, put +1 at every a_i and -1 at
// LCA(a_i, a_i+1): the sum over the subtree of j is then 1 for every j on the row subtree and
// every ancestor of hi, 0 elsewhere; -1 at parent[hi] ends it at hi.  A rank without lower end
// is its own row subtree (+1 at itself, -1 at its parent).  An id outside the sequence is never
// eliminated: it stays in every bag up to the roots, so its pairs whose LCA is the virtual root
// put no -1 and it has no parent.  The weights sit at tin positions; one inclusive scan gives
// every subtree sum.  No bag is stored, nothing follows parent pointers or walks a children
// list, and the only loop longer than O(log n) is the scan of one 64-entry block.
//
//   k_tw_cells     depths, in-block prefix / suffix minima, block minima     one wave per block
//   k_tw_level     one level of the sparse table over the block minima
//   k_tw_arcs      per tour position the tin of the rank a minimum there names (width_layout.h)
//   k_tw_keys      per record: (A), the key (hi << 32 | tin lo); radix_sort_u64 by key
//   k_tw_runs      per distinct key: +1 at tin lo, -1 at the LCA with the key before it
//   k_tw_ranks     per rank: +1 without lower end, -1 per child
//   (scan)         launch_vf_scan over the 2n weights
//   k_tw_final     width per rank; max, fill, halo
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sheep_amd kernels are written for gfx950 only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sheep_internal.h"
#include "verify_layout.h"
#include "width_layout.h"

namespace sheep {

static constexpr int TW_THREADS = 256;

static inline unsigned tw_grid(uint64_t n) {
  uint64_t g = (n + TW_THREADS - 1) / TW_THREADS;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, 4096));
}

__global__ void k_tw_init(unsigned long long* ws) {
  const int t = threadIdx.x;
  if (t < TW_WS_WORDS) ws[t] = t == TW_HALO ? (unsigned long long)INV : 0ull;
}

// One wave per block of 64 tour positions (TW_BLOCK is the wave width).
__global__ void __launch_bounds__(TW_THREADS)
k_tw_cells(const long long* __restrict__ sv, uint64_t n2, uint32_t nb, uint32_t* __restrict__ depth,
           uint64_t* __restrict__ pre, uint64_t* __restrict__ suf, uint64_t* __restrict__ tab0) {
  const int lane = threadIdx.x & 63;
  const uint32_t waves = gridDim.x * (TW_THREADS / 64);
  for (uint32_t b = blockIdx.x * (TW_THREADS / 64) + (threadIdx.x >> 6); b < nb; b += waves) {
    const uint64_t pos = (uint64_t)b * TW_BLOCK + lane;
    const bool in = pos < n2;
    const uint32_t d = in ? (uint32_t)sv[pos] : 0u;
    const uint64_t c = in ? tw_cell(d, (uint32_t)pos) : ~0ull;
    uint64_t p = c, q = c;
    for (int o = 1; o < 64; o <<= 1) {
      const uint64_t y = __shfl_up((unsigned long long)p, o);
      const uint64_t z = __shfl_down((unsigned long long)q, o);
      if (lane >= o) p = tw_min(p, y);
      if (lane + o < 64) q = tw_min(q, z);
    }
    if (in) {
      depth[pos] = d;
      pre[pos] = p;
      suf[pos] = q;
    }
    if (lane == 0) tab0[b] = q;
  }
}

// Level k of the table from level k - 1: len = tw_level_len(nb, k) entries.
__global__ void k_tw_level(const uint64_t* __restrict__ below, uint64_t* __restrict__ level,
                           uint32_t len, uint32_t half) {
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < len; b += gridDim.x * blockDim.x)
    level[b] = tw_min(below[b], below[b + half]);
}

__global__ void k_tw_arcs(const uint2* __restrict__ tt, const uint32_t* __restrict__ parent, uint32_t n,
                          uint32_t* __restrict__ lca_tin) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint2 t = tt[v];
    const uint32_t up = tw_arc_lca(true, v, parent[v]);
    lca_tin[t.x] = t.x;  // tw_arc_lca(false, v, .) = v
    lca_tin[t.y] = up == TW_NONE ? TW_NONE : tt[up].x;
  }
}

struct TwRec {
  const uint32_t* rank;
  uint32_t n_ids, n_seq;
  const uint2* tt;
  uint32_t* err;
};

// One record's key: the edge pass's rule for what counts (as vf_record, sheep_verify.hip).
// *bad: hi is no ancestor of lo, property (A) of the certificate.
__device__ __forceinline__ uint64_t tw_record(const TwRec& R, uint32_t x, uint32_t y, bool* bad) {
  if (x == y) return TW_SKIP;
  const bool ox = x >= R.n_ids, oy = y >= R.n_ids;
  const uint32_t rx = ox ? INV : R.rank[x], ry = oy ? INV : R.rank[y];
  if ((ox && ry != INV) || (oy && rx != INV)) { atomicOr(R.err, ERR_RANGE); return TW_SKIP; }
  const uint32_t lo = min(rx, ry), hi = max(rx, ry);
  if (lo == INV) return TW_SKIP;  // both ends outside the sequence
  if (lo >= R.n_seq || (hi != INV && hi >= R.n_seq)) { atomicOr(R.err, ERR_RANGE); return TW_SKIP; }
  if (lo == hi) return TW_SKIP;  // (a rank map that repeats a rank)
  const uint2 tl = R.tt[lo];
  if (hi == INV) return tw_key(tw_outside_key(R.n_seq, rx == INV ? x : y), tl.x);
  const uint2 th = R.tt[hi];
  if (!vf_in_subtree(tl.x, th.x, th.y)) { *bad = true; return TW_SKIP; }
  return tw_key(hi, tl.x);
}

// keys[i] for every record i; two records per 16-byte load as k_vf_records.
__global__ void __launch_bounds__(TW_THREADS)
k_tw_keys(const uint32_t* __restrict__ uv, uint64_t m, TwRec R, uint64_t* __restrict__ keys,
          unsigned long long* ws) {
  unsigned long long nbad = 0;
  auto one = [&](uint64_t i, uint32_t x, uint32_t y) {
    bool bad = false;
    keys[i] = tw_record(R, x, y, &bad);
    nbad += bad;
  };
  const uint64_t head = (((uintptr_t)uv & 15u) && m) ? 1 : 0;
  const uint64_t pairs = (m - head) / 2;
  const uint4* p4 = (const uint4*)(uv + 2 * head);
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < pairs;
       j += (uint64_t)gridDim.x * blockDim.x) {
    const uint4 r = p4[j];
    one(head + 2 * j, r.x, r.y);
    one(head + 2 * j + 1, r.z, r.w);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (head) one(0, uv[0], uv[1]);
    const uint64_t tail = head + 2 * pairs;
    if (tail < m) one(tail, uv[2 * tail], uv[2 * tail + 1]);
  }
  nbad = vf_wave_sum(nbad);
  if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(&ws[TW_A], nbad);
}

struct TwRmq {
  const uint32_t* depth;
  const uint64_t *pre, *suf, *tab;
  const uint32_t* lca_tin;
  uint32_t nb;
};

// Over the sorted keys.  A key equal to the one before it is a duplicate record; the key before
// a distinct key is the previous distinct one.  The -1 targets of neighbouring keys are often
// one rank (a star's centre takes one per leaf): each run of equal targets over adjacent lanes
// issues one atomic.
__global__ void __launch_bounds__(TW_THREADS)
k_tw_runs(const uint64_t* __restrict__ keys, uint64_t m, uint32_t n_seq, TwRmq Q,
          unsigned long long* __restrict__ wt, uint8_t* __restrict__ has_lower) {
  const int lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < m; base += stride) {
    const uint64_t i = base + threadIdx.x;
    uint32_t target = TW_NONE;
    if (i < m) {
      const uint64_t k = keys[i];
      const uint64_t kp = i ? keys[i - 1] : TW_SKIP;
      if (k != TW_SKIP && (i == 0 || kp != k)) {
        const uint32_t hi = tw_key_hi(k), t = tw_key_tin(k);
        atomicAdd(&wt[t], 1ull);
        if (hi < n_seq) has_lower[hi] = 1;
        if (i && tw_key_hi(kp) == hi) {
          const uint64_t c =
              tw_range_min(Q.depth, Q.pre, Q.suf, Q.tab, Q.nb, tw_key_tin(kp), t);
          if (tw_cell_depth(c) != 0) target = Q.lca_tin[tw_cell_pos(c)];
        }
      }
    }
    const uint32_t before = __shfl_up(target, 1);
    const bool first = lane == 0 || before != target;
    const uint64_t firsts = __ballot(first);
    if (first && target != TW_NONE) {
      const uint64_t above = lane == 63 ? 0ull : firsts >> (lane + 1);
      const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
      atomicAdd(&wt[target], 0ull - (unsigned long long)len);
    }
  }
}

// After k_tw_runs: a rank's own +1 when no record has it as upper end, -1 for each child.  One
// thread owns a rank's tin position.
__global__ void k_tw_ranks(const uint2* __restrict__ tt, const uint32_t* __restrict__ kfirst,
                           const uint32_t* __restrict__ klast, const uint8_t* __restrict__ has_lower,
                           uint32_t n, unsigned long long* __restrict__ wt) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t f = kfirst[v];
    const unsigned long long kids = f == VF_NONE ? 0ull : (unsigned long long)(klast[v] - f) + 1ull;
    wt[tt[v].x] += (has_lower[v] ? 0ull : 1ull) - kids;
  }
}

__global__ void k_tw_final(const uint2* __restrict__ tt, const uint32_t* __restrict__ pst, uint32_t n,
                           const long long* __restrict__ S, uint32_t* __restrict__ width_out,
                           unsigned long long* ws) {
  unsigned long long wmax = 0, fill = 0;
  uint32_t halo = INV;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint2 t = tt[v];
    const unsigned long long w = (unsigned long long)tw_subtree_sum(S, t.x, t.y);
    if (width_out) width_out[v] = (uint32_t)w;
    wmax = max(wmax, w);
    fill += w - 1ull - (unsigned long long)pst[v];  // wraps as the reference's size_t sum
    if (w > 3) halo = min(halo, v);
  }
  wmax = vf_wave_max(wmax);
  fill = vf_wave_sum(fill);
  halo = vf_wave_min(halo);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&ws[TW_WIDTH], wmax);
    if (fill) atomicAdd(&ws[TW_FILL], fill);
    if (halo != INV) atomicMin((uint32_t*)&ws[TW_HALO], halo);  // low word (little endian)
  }
}

// ---- launchers ------------------------------------------------------------------------------

void launch_tw_rmq(const VfTour& T, const uint32_t* parent, const long long* sv, const TwBufs& B,
                   unsigned long long* ws, hipStream_t s) {
  hipLaunchKernelGGL(k_tw_init, dim3(1), dim3(64), 0, s, ws);
  const uint32_t n = T.n;
  if (n == 0) return;
  const uint64_t n2 = 2ull * n;
  const uint32_t nb = tw_blocks(n2);
  hipLaunchKernelGGL(k_tw_cells, dim3(tw_grid((uint64_t)nb * 64)), dim3(TW_THREADS), 0, s, sv, n2, nb,
                     B.depth, B.pre, B.suf, B.tab);
  for (int k = 1; k < tw_levels(nb); ++k) {
    const uint32_t len = tw_level_len(nb, k);
    hipLaunchKernelGGL(k_tw_level, dim3(tw_grid(len)), dim3(TW_THREADS), 0, s,
                       (const uint64_t*)(B.tab + tw_tab_ix(nb, k - 1, 0)), B.tab + tw_tab_ix(nb, k, 0),
                       len, 1u << (k - 1));
  }
  hipLaunchKernelGGL(k_tw_arcs, dim3(tw_grid(n)), dim3(TW_THREADS), 0, s, (const uint2*)T.tt, parent, n,
                     B.lca_tin);
}

void launch_tw_keys(const uint32_t* uv, uint64_t m, const uint32_t* rank, uint32_t n_ids,
                    const VfTour& T, uint64_t* keys, unsigned long long* ws, uint32_t* err,
                    hipStream_t s) {
  if (m == 0) return;
  TwRec R;
  R.rank = rank;
  R.n_ids = n_ids;
  R.n_seq = T.n;
  R.tt = T.tt;
  R.err = err;
  hipLaunchKernelGGL(k_tw_keys, dim3(tw_grid((m + 1) / 2)), dim3(TW_THREADS), 0, s, uv, m, R, keys, ws);
}

void launch_tw_weights(const uint64_t* keys, uint64_t m, const VfTour& T, const TwBufs& B,
                       long long* wt, hipStream_t s) {
  const uint32_t n = T.n;
  if (n == 0) return;
  (void)hipMemsetAsync(wt, 0, 2ull * n * 8, s);
  (void)hipMemsetAsync(B.has_lower, 0, n, s);
  if (m) {
    TwRmq Q;
    Q.depth = B.depth;
    Q.pre = B.pre;
    Q.suf = B.suf;
    Q.tab = B.tab;
    Q.lca_tin = B.lca_tin;
    Q.nb = tw_blocks(2ull * n);
    hipLaunchKernelGGL(k_tw_runs, dim3(tw_grid(m)), dim3(TW_THREADS), 0, s, keys, m, n, Q,
                       (unsigned long long*)wt, B.has_lower);
  }
  hipLaunchKernelGGL(k_tw_ranks, dim3(tw_grid(n)), dim3(TW_THREADS), 0, s, (const uint2*)T.tt,
                     (const uint32_t*)T.kfirst, (const uint32_t*)T.klast,
                     (const uint8_t*)B.has_lower, n, (unsigned long long*)wt);
}

void launch_tw_final(const VfTour& T, const uint32_t* pst, const long long* S, uint32_t* width_out,
                     unsigned long long* ws, hipStream_t s) {
  if (T.n)
    hipLaunchKernelGGL(k_tw_final, dim3(tw_grid(T.n)), dim3(TW_THREADS), 0, s, (const uint2*)T.tt, pst,
                       T.n, S, width_out, ws);
}

}  // namespace sheep
