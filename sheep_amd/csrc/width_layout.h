// Index arithmetic of the exact tree widths (sheep_width.hip): the sort keys of the records, the
// range-minimum structure over the Euler tour's depths, how a query splits over it and how the
// arc at a minimum names the lowest common ancestor.  Plain C++17, shared by the kernels and the
// host (tests/cpp/width_layout.cpp compiles it with g++ under the sanitizers and checks every
// query against a linear scan and every LCA against a parent walk).
//
// The tour is verify_layout.h's: 2n arcs, tin[v] = pos(down v), tout[v] = pos(up v).  E[pos] is
// the depth after the arc at pos, a root being at depth 1 and the virtual root at 0 (the
// inclusive +1 / -1 prefix sum).  A cell packs (E[pos] << 32 | pos): the plain 64-bit minimum of
// cells is a minimum of E and carries a position that attains it.
//   block b           = positions [64 b, 64 b + 64)
//   pre[pos], suf[pos]  minimum of the cells from the block's first position to pos / from pos to
//                       the block's last position
//   table level k     = minima of 2^k consecutive blocks, level 0 = the block minima; tab_levels
//                       levels of nb entries each (entries past nb - 2^k + 1 of a level unused)
// A query [l, r] inside one block scans its at most 64 depths; otherwise it is suf[l], pre[r] and,
// if blocks lie between, two overlapping table entries.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHEEP_HD __host__ __device__
#else
#define SHEEP_HD
#endif

namespace sheep {

constexpr uint32_t TW_NONE = 0xFFFFFFFFu;
constexpr uint64_t TW_SKIP = ~0ull;  // key of a record that counts nothing; sorts last
constexpr int TW_BLOCK_LOG = 6;
constexpr uint32_t TW_BLOCK = 1u << TW_BLOCK_LOG;

// Sort key of a record in rank space: its upper end, then the tour position of its lower end.
// An id outside the sequence is never eliminated: as an upper end it takes the key n_seq + id,
// above every rank (the caller keeps n_seq + n_ids within 2^32).
SHEEP_HD inline uint64_t tw_key(uint32_t hi_key, uint32_t tin_lo) {
  return ((uint64_t)hi_key << 32) | tin_lo;
}
SHEEP_HD inline uint32_t tw_key_hi(uint64_t key) { return (uint32_t)(key >> 32); }
SHEEP_HD inline uint32_t tw_key_tin(uint64_t key) { return (uint32_t)key; }
SHEEP_HD inline uint32_t tw_outside_key(uint32_t n_seq, uint32_t id) { return n_seq + id; }

SHEEP_HD inline uint64_t tw_cell(uint32_t depth, uint32_t pos) { return ((uint64_t)depth << 32) | pos; }
SHEEP_HD inline uint32_t tw_cell_depth(uint64_t c) { return (uint32_t)(c >> 32); }
SHEEP_HD inline uint32_t tw_cell_pos(uint64_t c) { return (uint32_t)c; }
SHEEP_HD inline uint64_t tw_min(uint64_t a, uint64_t b) { return a < b ? a : b; }

SHEEP_HD inline uint32_t tw_block_of(uint32_t pos) { return pos >> TW_BLOCK_LOG; }
SHEEP_HD inline uint32_t tw_blocks(uint64_t n2) { return (uint32_t)((n2 + TW_BLOCK - 1) >> TW_BLOCK_LOG); }
// floor(log2 x), x >= 1
SHEEP_HD inline int tw_log2(uint32_t x) {
  int k = 0;
  while (x >>= 1) ++k;
  return k;
}
SHEEP_HD inline int tw_levels(uint32_t nb) { return nb ? tw_log2(nb) + 1 : 0; }
SHEEP_HD inline uint64_t tw_tab_ix(uint32_t nb, int level, uint32_t b) { return (uint64_t)level * nb + b; }
// entries of level k that are defined: blocks b with b + 2^k <= nb
SHEEP_HD inline uint32_t tw_level_len(uint32_t nb, int level) { return nb - (1u << level) + 1u; }

// How a query [l, r] (l <= r) reads the structure.
struct TwQuery {
  bool in_block;     // scan the depths of [l, r]
  bool has_mid;      // blocks between: min(tab[t0], tab[t1])
  uint64_t t0, t1;   // table indices (tw_tab_ix)
};
SHEEP_HD inline TwQuery tw_query(uint32_t l, uint32_t r, uint32_t nb) {
  TwQuery q;
  q.t0 = q.t1 = 0;
  const uint32_t bl = tw_block_of(l), br = tw_block_of(r);
  q.in_block = bl == br;
  q.has_mid = !q.in_block && br - bl > 1;
  if (q.has_mid) {
    const uint32_t cnt = br - bl - 1;
    const int k = tw_log2(cnt);
    q.t0 = tw_tab_ix(nb, k, bl + 1);
    q.t1 = tw_tab_ix(nb, k, br - (1u << k));
  }
  return q;
}
// The minimum cell of [l, r]: depth (n2 entries), pre / suf (n2 each), tab (tw_levels * nb).
SHEEP_HD inline uint64_t tw_range_min(const uint32_t* depth, const uint64_t* pre, const uint64_t* suf,
                                      const uint64_t* tab, uint32_t nb, uint32_t l, uint32_t r) {
  const TwQuery q = tw_query(l, r, nb);
  if (q.in_block) {
    uint64_t best = tw_cell(depth[l], l);
    for (uint32_t p = l + 1; p <= r; ++p) best = tw_min(best, tw_cell(depth[p], p));
    return best;
  }
  uint64_t best = tw_min(suf[l], pre[r]);
  if (q.has_mid) best = tw_min(best, tw_min(tab[q.t0], tab[q.t1]));
  return best;
}

// What the arc at a tour position says about a minimum there: a down arc into v names v, an up
// arc out of v names parent[v] (TW_NONE: the virtual root).  lca_tin[pos] holds that rank's tin,
// the position its weight goes to.
SHEEP_HD inline uint32_t tw_arc_lca(bool up, uint32_t v, uint32_t parent_v) { return up ? parent_v : v; }

// width[j] from the inclusive scan S of the weights at tin positions: the sum over [tin, tout].
SHEEP_HD inline long long tw_subtree_sum(const long long* S, uint32_t tin, uint32_t tout) {
  return S[tout] - (tin ? S[tin - 1] : 0);
}

}  // namespace sheep
