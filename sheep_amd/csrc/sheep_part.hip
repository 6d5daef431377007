// Forward partition of a tree in HBM (sheep_partition_dev): every pass over all ranks.  The
// sequential part, the packing of the few ranks whose subtree outweighs a part, is the host's
// (part_layout.h); DESIGN.md §4.10 has the method and the proof sketch.
//
// With the tour of sheep_verify.hip, pst at the tin positions and one inclusive scan give every
// subtree sum S0; the ranks with S0 > max_component (H) are compacted in rank order for the
// host's walk; the parts the host packed come back as +d / -d at the tin / tout of the packed
// ranks, and a second scan read at tin[v] is the part of v's nearest packed ancestor-or-self.
// No kernel follows parent pointers or walks one rank's children.
//
//   once per call
//   k_pt_reduce    total and maximum of pst, maximum of seq
//   k_pt_weights   pst at tin, 0 at tout; launch_vf_scan
//   k_pt_sums      S0 per rank from the scan
//   k_pt_slots     S0 in children-list slot order: a cut rank's kids and the roots are two plain
//                  copies of a slot range (the kids array and this one)
//   once per k
//   k_pt_flag      the H flags; launch_scan_exclusive gives every heavy rank its index in H
//   k_pt_heavy     the H records (part_layout.h PtHeavy), ascending in rank
//   k_pt_deltas    the host's deltas at tin / tout of a zeroed tour; launch_vf_scan
//   k_pt_store     parts[seq[v]] = scan at tin[v], as int16
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "sheep_amd kernels are written for gfx950 only"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sheep_internal.h"
#include "part_layout.h"
#include "verify_layout.h"
#include "width_layout.h"

namespace sheep {

static constexpr int PT_THREADS = 256;

static inline unsigned pt_grid(uint64_t n) {
  uint64_t g = (n + PT_THREADS - 1) / PT_THREADS;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(g, 4096));
}

__global__ void k_pt_init(unsigned long long* ws) {
  if (threadIdx.x < PT_WS_WORDS) ws[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(PT_THREADS)
k_pt_reduce(const uint32_t* __restrict__ pst, const uint32_t* __restrict__ seq, uint32_t n,
            unsigned long long* ws) {
  unsigned long long total = 0, wmax = 0, smax = 0;
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const unsigned long long w = pst[v];
    total += w;
    wmax = max(wmax, w);
    smax = max(smax, (unsigned long long)seq[v]);
  }
  total = vf_wave_sum(total);
  wmax = vf_wave_max(wmax);
  smax = vf_wave_max(smax);
  if ((threadIdx.x & 63) == 0) {
    if (total) atomicAdd(&ws[PT_TOTAL], total);
    atomicMax(&ws[PT_WMAX], wmax);
    atomicMax(&ws[PT_SEQMAX], smax);
  }
}

// One thread owns both tour positions of its rank.
__global__ void k_pt_weights(const uint2* __restrict__ tt, const uint32_t* __restrict__ pst, uint32_t n,
                             long long* __restrict__ wt) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint2 t = tt[v];
    wt[t.x] = pst[v];
    wt[t.y] = 0;
  }
}

__global__ void k_pt_sums(const uint2* __restrict__ tt, const long long* __restrict__ S, uint32_t n,
                          unsigned long long* __restrict__ s0) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint2 t = tt[v];
    s0[v] = (unsigned long long)tw_subtree_sum(S, t.x, t.y);
  }
}

__global__ void k_pt_slots(const uint64_t* __restrict__ kids, const unsigned long long* __restrict__ s0,
                           uint32_t n, unsigned long long* __restrict__ ks0) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    ks0[i] = s0[vf_kid(kids[i])];
}

// flag has n + 1 entries, the last one 0: its exclusive scan ends with |H|.
__global__ void k_pt_flag(const unsigned long long* __restrict__ s0, uint32_t n,
                          unsigned long long max_component, uint32_t* __restrict__ flag) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += gridDim.x * blockDim.x)
    flag[v] = v < n && s0[v] > max_component;
}

// A heavy rank's parent is heavy (S0 does not shrink upwards), so idx[parent] is its index in H.
__global__ void k_pt_heavy(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ idx,
                           const uint32_t* __restrict__ parent, const unsigned long long* __restrict__ s0,
                           const uint32_t* __restrict__ kfirst, const uint32_t* __restrict__ klast,
                           uint32_t n, uint32_t nh, PtHeavy* __restrict__ out) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    if (!flag[v]) continue;
    const uint32_t i = idx[v];
    if (i >= nh) continue;  // (unreachable: nh is the scan's total)
    const uint32_t p = parent[v];
    PtHeavy h;
    h.rank = v;
    h.pidx = p == INV ? PT_NONE : idx[p];
    h.s0 = s0[v];
    h.kfirst = kfirst[v];
    h.klast = klast[v];
    out[i] = h;
  }
}

// Each packed rank appears once, and its two tour positions are its own.
__global__ void k_pt_deltas(const PtDelta* __restrict__ deltas, uint32_t nd, const uint2* __restrict__ tt,
                            uint32_t n, long long* __restrict__ wt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nd; i += gridDim.x * blockDim.x) {
    const PtDelta d = deltas[i];
    if (d.rank >= n) continue;  // (unreachable: the host packs ranks of this tree)
    const uint2 t = tt[d.rank];
    wt[t.x] = d.d;
    wt[t.y] = -(long long)d.d;
  }
}

// row: n_vid int16, filled with -1.  The caller has checked max(seq) < n_vid; the test here keeps
// a sequence that changed under the call from storing outside the row.
__global__ void k_pt_store(const uint2* __restrict__ tt, const long long* __restrict__ S,
                           const uint32_t* __restrict__ seq, uint32_t n, uint32_t n_vid,
                           int16_t* __restrict__ row, uint32_t* err) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t id = seq[v];
    if (id >= n_vid) { atomicOr(err, ERR_RANGE); continue; }
    row[id] = (int16_t)S[tt[v].x];
  }
}

// ---- launchers ------------------------------------------------------------------------------

void launch_pt_reduce(const uint32_t* pst, const uint32_t* seq, uint32_t n, unsigned long long* ws,
                      hipStream_t s) {
  hipLaunchKernelGGL(k_pt_init, dim3(1), dim3(64), 0, s, ws);
  if (n) hipLaunchKernelGGL(k_pt_reduce, dim3(pt_grid(n)), dim3(PT_THREADS), 0, s, pst, seq, n, ws);
}

void launch_pt_sums(const VfTour& T, const uint32_t* pst, long long* wt, long long* sums,
                    unsigned long long* s0, unsigned long long* ks0, hipStream_t s) {
  const uint32_t n = T.n;
  if (n == 0) return;
  const dim3 g(pt_grid(n)), b(PT_THREADS);
  hipLaunchKernelGGL(k_pt_weights, g, b, 0, s, (const uint2*)T.tt, pst, n, wt);
  launch_vf_scan(wt, n, sums, s);
  hipLaunchKernelGGL(k_pt_sums, g, b, 0, s, (const uint2*)T.tt, (const long long*)wt, n, s0);
  hipLaunchKernelGGL(k_pt_slots, g, b, 0, s, (const uint64_t*)T.kids, (const unsigned long long*)s0, n,
                     ks0);
}

void launch_pt_flag(const unsigned long long* s0, uint32_t n, uint64_t max_component, uint32_t* flag,
                    uint32_t* idx, uint32_t* tmp, hipStream_t s) {
  hipLaunchKernelGGL(k_pt_flag, dim3(pt_grid((uint64_t)n + 1)), dim3(PT_THREADS), 0, s, s0, n,
                     (unsigned long long)max_component, flag);
  launch_scan_exclusive(flag, idx, (uint64_t)n + 1, tmp, s);
}

void launch_pt_heavy(const uint32_t* flag, const uint32_t* idx, const uint32_t* parent,
                     const unsigned long long* s0, const VfTour& T, uint32_t nh, PtHeavy* out,
                     hipStream_t s) {
  if (T.n && nh)
    hipLaunchKernelGGL(k_pt_heavy, dim3(pt_grid(T.n)), dim3(PT_THREADS), 0, s, flag, idx, parent, s0,
                       (const uint32_t*)T.kfirst, (const uint32_t*)T.klast, T.n, nh, out);
}

void launch_pt_push(const PtDelta* deltas, uint32_t nd, const VfTour& T, long long* wt, long long* sums,
                    const uint32_t* seq, uint32_t n_vid, int16_t* row, uint32_t* err, hipStream_t s) {
  const uint32_t n = T.n;
  (void)hipMemsetAsync(row, 0xFF, (size_t)n_vid * 2, s);
  if (n == 0) return;
  (void)hipMemsetAsync(wt, 0, 2ull * n * 8, s);
  if (nd)
    hipLaunchKernelGGL(k_pt_deltas, dim3(pt_grid(nd)), dim3(PT_THREADS), 0, s, deltas, nd,
                       (const uint2*)T.tt, n, wt);
  launch_vf_scan(wt, n, sums, s);
  hipLaunchKernelGGL(k_pt_store, dim3(pt_grid(n)), dim3(PT_THREADS), 0, s, (const uint2*)T.tt,
                     (const long long*)wt, seq, n, n_vid, row, err);
}

}  // namespace sheep
