// SNAP text (.net) ingest: decimal text in HBM -> the u32 token sequence that is the records
// (net_layout.h has the semantics and the arithmetic; net_pass in sheep_capi.cpp feeds chunks).
//
// Per chunk of n bytes (starts at a token boundary, ends with whitespace), three launches:
//   k_net_count  one 16-byte load per lane, its token-start mask, the tile's token count
//   k_net_scan   one block: exclusive scan of the tile counts; the pass's running token count
//                advances (NET_BASE = the chunk's first token index, NET_TOTAL += its tokens)
//   k_net_parse  the masks again, each start ranked inside its tile; the lane that owns a start
//                walks its digits (past its own word or tile, never past the chunk) and stores
//                the value at its token index, or lowers the stop pair for an irregular token
// A pass's words (NET_*) live on the device, so a chunk is enqueue-only.  The count pass is the
// same code without stores.
#include "net_layout.h"
#include "sheep_internal.h"

namespace sheep {
namespace {

static_assert(NET_LANES == 256, "k_net_count / k_net_parse: four waves per tile");

// Token starts of word w (lane-uniform control flow: every lane of the wave calls this).
__device__ __forceinline__ uint32_t net_lane_starts(const uint8_t* __restrict__ text, uint32_t n,
                                                    uint32_t w) {
  const uint32_t nwords = (n + NET_WORD - 1) / NET_WORD;
  uint32_t ws = 0xFFFFu;  // a word past the chunk: whitespace
  if (w < nwords) {
    const uint4 x = ((const uint4*)text)[w];
    ws = net_ws_mask(x.x, x.y, x.z, x.w, min(NET_WORD, n - w * NET_WORD));
  }
  // The predecessor byte's class: the neighbouring lane's last byte; a wave's first lane loads it.
  uint32_t pred = ((uint32_t)__shfl_up((int)ws, 1) >> 15) & 1u;
  if ((threadIdx.x & 63u) == 0) pred = (w == 0 || w >= nwords) ? 1u : net_is_ws(text[w * NET_WORD - 1]);
  return net_start_mask(ws, pred != 0);
}

__global__ __launch_bounds__(NET_LANES) void k_net_count(const uint8_t* __restrict__ text,
                                                         uint32_t n,
                                                         uint32_t* __restrict__ tile_count) {
  __shared__ uint32_t wsum[NET_LANES / 64];
  uint32_t c = __popc(net_lane_starts(text, n, blockIdx.x * NET_LANES + threadIdx.x));
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// Inclusive scan of v over the block's threads in thread order; *total = the block's sum.
template <int THREADS>
__device__ __forceinline__ uint32_t net_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, o);
    if (lane >= (uint32_t)o) v += u;
  }
  __syncthreads();  // wsum may still be read from the previous call
  if (lane == 63) wsum[wv] = v;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < THREADS / 64; ++i) {
    const uint32_t s = wsum[i];
    if ((uint32_t)i < wv) before += s;
    all += s;
  }
  *total = all;
  return v + before;
}

constexpr int NET_SCAN_THREADS = 1024;
// tiles[i]: the tile's token count in, the tokens of the chunk before the tile out (both fit
// u32: a chunk is at most 2^30 + 1 bytes).
__global__ __launch_bounds__(NET_SCAN_THREADS) void k_net_scan(uint32_t* __restrict__ tiles,
                                                               uint32_t ntiles,
                                                               unsigned long long* state) {
  __shared__ uint32_t wsum[NET_SCAN_THREADS / 64];
  uint32_t run = 0;
  for (uint32_t base = 0; base < ntiles; base += NET_SCAN_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < ntiles ? tiles[i] : 0u;
    uint32_t total;
    const uint32_t incl = net_block_scan<NET_SCAN_THREADS>(v, wsum, &total);
    if (i < ntiles) tiles[i] = run + incl - v;
    run += total;
  }
  if (threadIdx.x == 0) {
    const unsigned long long t = state[NET_TOTAL];
    state[NET_BASE] = t;
    state[NET_TOTAL] = t + run;
  }
}

template <bool STORE>
__global__ __launch_bounds__(NET_LANES) void k_net_parse(const uint8_t* __restrict__ text,
                                                         uint32_t n,
                                                         const uint32_t* __restrict__ tile_off,
                                                         unsigned long long* state,
                                                         uint64_t file_off, uint64_t lo2,
                                                         uint64_t hi2, uint32_t* __restrict__ uv) {
  __shared__ uint32_t wsum[NET_LANES / 64];
  const uint32_t w = blockIdx.x * NET_LANES + threadIdx.x;
  uint32_t starts = net_lane_starts(text, n, w);
  const uint32_t c = __popc(starts);
  uint32_t total;
  const uint32_t incl = net_block_scan<NET_LANES>(c, wsum, &total);
  uint64_t t = state[NET_BASE] + tile_off[blockIdx.x] + (incl - c);
  uint32_t mx = 0;
  for (; starts; starts &= starts - 1, ++t) {
    if (STORE && !net_in_window(t, lo2, hi2)) continue;
    const uint32_t pos = w * NET_WORD + (uint32_t)__ffs((int)starts) - 1u;
    uint32_t v;
    if (net_parse_token(text, pos, n, &v)) {
      if (STORE) {
        uv[t - lo2] = v;
        mx = max(mx, net_top(v));
      }
    } else if (!STORE) {
      atomicMin(&state[NET_STOP_TOK], (unsigned long long)t);
      atomicMin(&state[NET_STOP_OFF], (unsigned long long)(file_off + pos));
    }
  }
  if (STORE) {
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63u) == 0 && mx) atomicMax((uint32_t*)&state[NET_MAX], mx);
  }
}

}  // namespace

void launch_net_chunk(const uint8_t* text, uint32_t n, uint64_t file_off, uint32_t* tiles,
                      unsigned long long* state, uint32_t* uv, uint64_t lo2, uint64_t hi2,
                      hipStream_t s) {
  if (n == 0) return;
  const uint32_t nt = net_tiles(n);
  hipLaunchKernelGGL(k_net_count, dim3(nt), dim3(NET_LANES), 0, s, text, n, tiles);
  hipLaunchKernelGGL(k_net_scan, dim3(1), dim3(NET_SCAN_THREADS), 0, s, tiles, nt, state);
  if (uv)
    hipLaunchKernelGGL(k_net_parse<true>, dim3(nt), dim3(NET_LANES), 0, s, text, n, tiles, state,
                       file_off, lo2, hi2, uv);
  else
    hipLaunchKernelGGL(k_net_parse<false>, dim3(nt), dim3(NET_LANES), 0, s, text, n, tiles, state,
                       file_off, lo2, hi2, (uint32_t*)nullptr);
}

}  // namespace sheep
