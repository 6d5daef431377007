// Index arithmetic of the tree verifier (sheep_verify.hip): the children lists' sort items, the
// Euler tour's arcs and their successors, what the tour positions mean, and the report's words.
// Plain C++17, shared by the kernels and the host (tests/cpp/verify_layout.cpp compiles it with
// g++ under the sanitizers and checks it against a recursive DFS).
//
// The forest over ranks [0, n) becomes one tree under the virtual parent n.  Its children
// lists are the items (parent << 32 | v) sorted by parent, stably, so each list ascends in v:
// slot i holds the child (uint32_t)kids[i] of kids[i] >> 32, and kfirst[p] (n + 1 entries) is
// p's first slot or VF_NONE.  Every rank v has two arcs, down(v) = v and up(v) = n + v; the
// tour enters v by down(v), walks its children in list order and leaves by up(v).  The top
// level roots are the virtual parent's children: the tour starts at the smallest root's down
// arc and ends (VF_END) after the largest root's up arc.  With pos(a) the number of arcs before
// a, tin[v] = pos(down v) and tout[v] = pos(up v):
//   u is in the subtree of v (v included)  iff  tin[v] <= tin[u] < tout[v]
//   size[v] = (tout[v] - tin[v] + 1) / 2
//   depth[v] (a root's is 0) = (arcs down - arcs up) before down(v); pre[v] = arcs down before it
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SHEEP_HD __host__ __device__
#else
#define SHEEP_HD
#endif

namespace sheep {

constexpr uint32_t VF_NONE = 0xFFFFFFFFu;  // INVALID parent; no children
constexpr uint32_t VF_END = 0xFFFFFFFFu;   // successor of the tour's last arc

// Heap order: a parent is INVALID or in (v, n).  Nothing may follow parent pointers that fail it.
SHEEP_HD inline bool vf_heap_ok(uint32_t v, uint32_t p, uint32_t n) {
  return p == VF_NONE || (p > v && p < n);
}

SHEEP_HD inline uint64_t vf_item(uint32_t v, uint32_t p, uint32_t n) {
  return ((uint64_t)(p == VF_NONE ? n : p) << 32) | v;
}
SHEEP_HD inline uint32_t vf_kid(uint64_t item) { return (uint32_t)item; }
SHEEP_HD inline uint32_t vf_par(uint64_t item) { return (uint32_t)(item >> 32); }

SHEEP_HD inline uint32_t vf_down(uint32_t v) { return v; }
SHEEP_HD inline uint32_t vf_up(uint32_t n, uint32_t v) { return n + v; }

// Successors of the two arcs of the child in slot i.
SHEEP_HD inline void vf_succ(const uint64_t* kids, const uint32_t* kfirst, uint32_t n, uint32_t i,
                             uint32_t* after_down, uint32_t* after_up) {
  const uint32_t v = vf_kid(kids[i]), p = vf_par(kids[i]);
  const uint32_t f = kfirst[v];
  *after_down = f != VF_NONE ? vf_down(vf_kid(kids[f])) : vf_up(n, v);
  if (i + 1 < n && vf_par(kids[i + 1]) == p)
    *after_up = vf_down(vf_kid(kids[i + 1]));
  else
    *after_up = p == n ? VF_END : vf_up(n, p);
}

// A list cell of the ranking: (successor << 32 | arcs from here to the end of the tour).
SHEEP_HD inline uint64_t vf_cell(uint32_t succ) {
  return ((uint64_t)succ << 32) | (succ == VF_END ? 0u : 1u);
}
// One pointer-jumping step of cell x whose successor's cell is y.
SHEEP_HD inline uint64_t vf_jump(uint64_t x, uint64_t y) {
  return (y & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)x + (uint32_t)y);
}
// Rounds after which every cell of 2n arcs has reached the end.
inline int vf_rounds(uint32_t n) {
  int r = 0;
  while ((1ull << r) < 2ull * n) ++r;
  return r;
}
// Tour position of an arc from its ranked cell.
SHEEP_HD inline uint32_t vf_pos(uint64_t cell, uint32_t n) { return 2u * n - 1u - (uint32_t)cell; }

SHEEP_HD inline bool vf_in_subtree(uint32_t tin_u, uint32_t tin_v, uint32_t tout_v) {
  return tin_v <= tin_u && tin_u < tout_v;
}
SHEEP_HD inline uint32_t vf_size(uint32_t tin, uint32_t tout) { return (tout - tin + 1u) / 2u; }
// depth: the inclusive prefix sum of the arcs' +1 / -1 at tin, less one.
SHEEP_HD inline uint32_t vf_pre(uint32_t tin, uint32_t depth) { return (tin + depth) / 2u; }

// The report of sheep_verify_tree_dev (include/sheep_amd.h) from the device counters.
inline void vf_report(uint64_t report[8], uint64_t heap_bad, uint64_t a_bad, uint64_t b_bad,
                      uint64_t pst_bad, uint32_t min_rank) {
  for (int i = 0; i < 8; ++i) report[i] = 0;
  report[0] = heap_bad;
  if (heap_bad) {
    report[1] = report[2] = report[3] = ~0ull;  // not computed: a cycle is possible
  } else {
    report[1] = a_bad;
    report[2] = b_bad;
    report[3] = pst_bad;
  }
  report[4] = min_rank;
}

}  // namespace sheep
