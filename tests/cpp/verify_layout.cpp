// The tree verifier's host-side index arithmetic (sheep_amd/csrc/verify_layout.h) against a
// recursive DFS: for small forests the sort items, the children runs, the Euler tour's
// successors, a sequential walk of the list and the pointer-jumping rounds must give every
// rank's tour positions, and from them pre, size and depth equal to the DFS's; then the report
// assembly.  Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_verify_layout.py.  Prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "verify_layout.h"

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

struct Dfs {
  std::vector<std::vector<uint32_t>> kids;
  std::vector<uint32_t> pre, size, depth;
  uint32_t clock = 0;
  uint32_t visit(uint32_t v, uint32_t d) {
    pre[v] = clock++;
    depth[v] = d;
    uint32_t s = 1;
    for (uint32_t k : kids[v]) s += visit(k, d + 1);
    return size[v] = s;
  }
};

static void check_forest(const char* name, const std::vector<uint32_t>& parent) {
  const uint32_t n = (uint32_t)parent.size();
  for (uint32_t v = 0; v < n; ++v) CHECK(vf_heap_ok(v, parent[v], n), "%s: rank %u", name, v);

  // the reference: children in ascending order, roots in ascending order
  Dfs d;
  d.kids.resize(n);
  d.pre.resize(n);
  d.size.resize(n);
  d.depth.resize(n);
  for (uint32_t v = 0; v < n; ++v)
    if (parent[v] != VF_NONE) d.kids[parent[v]].push_back(v);
  for (uint32_t v = 0; v < n; ++v)
    if (parent[v] == VF_NONE) d.visit(v, 0);

  // the verifier's construction
  std::vector<uint64_t> kids(n);
  for (uint32_t v = 0; v < n; ++v) kids[v] = vf_item(v, parent[v], n);
  std::stable_sort(kids.begin(), kids.end(),
                   [](uint64_t a, uint64_t b) { return vf_par(a) < vf_par(b); });
  std::vector<uint32_t> kfirst(n + 1, VF_NONE);
  for (uint32_t i = 0; i < n; ++i)
    if (i == 0 || vf_par(kids[i - 1]) != vf_par(kids[i])) kfirst[vf_par(kids[i])] = i;
  std::vector<uint64_t> cells(2 * (size_t)n);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t sd, su;
    vf_succ(kids.data(), kfirst.data(), n, i, &sd, &su);
    const uint32_t v = vf_kid(kids[i]);
    cells[vf_down(v)] = vf_cell(sd);
    cells[vf_up(n, v)] = vf_cell(su);
  }

  // sequential walk from the first root's down arc
  std::vector<uint32_t> pos(2 * (size_t)n, VF_NONE);
  std::vector<long long> level(2 * (size_t)n, 0);  // inclusive +1 / -1 prefix sum
  uint32_t steps = 0;
  long long run = 0;
  for (uint32_t a = n ? vf_down(vf_kid(kids[kfirst[n]])) : VF_END; a != VF_END;
       a = (uint32_t)(cells[a] >> 32)) {
    CHECK(a < 2 * n && steps < 2 * n, "%s: walk leaves the list", name);
    if (a >= 2 * n || steps >= 2 * n) return;
    CHECK(pos[a] == VF_NONE, "%s: arc %u twice", name, a);
    pos[a] = steps++;
    run += a < n ? 1 : -1;
    level[pos[a]] = run;
  }
  CHECK(steps == 2 * n, "%s: %u arcs walked of %u", name, steps, 2 * n);
  CHECK(run == 0, "%s: tour does not close", name);

  // pointer jumping, double-buffered, vf_rounds(n) rounds
  std::vector<uint64_t> a = cells, b(cells.size());
  for (int r = vf_rounds(n); r > 0; --r) {
    for (size_t i = 0; i < a.size(); ++i) {
      const uint32_t s = (uint32_t)(a[i] >> 32);
      b[i] = s != VF_END ? vf_jump(a[i], a[s]) : a[i];
    }
    a.swap(b);
  }
  for (size_t i = 0; i < a.size(); ++i) {
    CHECK((uint32_t)(a[i] >> 32) == VF_END, "%s: arc %zu not at the end", name, i);
    CHECK(vf_pos(a[i], n) == pos[i], "%s: arc %zu ranked %u, walked %u", name, i, vf_pos(a[i], n),
          pos[i]);
  }

  for (uint32_t v = 0; v < n; ++v) {
    const uint32_t tin = pos[vf_down(v)], tout = pos[vf_up(n, v)];
    const uint32_t depth = (uint32_t)(level[tin] - 1);
    CHECK(depth == d.depth[v], "%s: depth[%u] = %u, DFS %u", name, v, depth, d.depth[v]);
    CHECK(vf_pre(tin, depth) == d.pre[v], "%s: pre[%u] = %u, DFS %u", name, v, vf_pre(tin, depth),
          d.pre[v]);
    CHECK(vf_size(tin, tout) == d.size[v], "%s: size[%u] = %u, DFS %u", name, v,
          vf_size(tin, tout), d.size[v]);
  }
  // the interval test against the DFS's preorder intervals
  for (uint32_t u = 0; u < n; ++u)
    for (uint32_t v = 0; v < n; ++v) {
      const bool in = d.pre[v] <= d.pre[u] && d.pre[u] < d.pre[v] + d.size[v];
      CHECK(vf_in_subtree(pos[vf_down(u)], pos[vf_down(v)], pos[vf_up(n, v)]) == in,
            "%s: %u in subtree of %u", name, u, v);
    }
}

int main() {
  const uint32_t X = VF_NONE;
  check_forest("single", {X});
  check_forest("two-roots", {X, X});
  check_forest("pair", {1, X});
  {
    std::vector<uint32_t> p(64);
    for (uint32_t v = 0; v < 64; ++v) p[v] = v + 1 < 64 ? v + 1 : X;
    check_forest("path", p);
    for (uint32_t v = 0; v < 64; ++v) p[v] = v + 1 < 64 ? 63 : X;
    check_forest("star", p);
    for (uint32_t v = 0; v < 63; ++v) p[v] = v < 62 ? 62 - (61 - v) / 2 : X;
    p.resize(63);
    check_forest("binary", p);
  }
  check_forest("two-trees", {2, 2, 5, 4, X, X});           // roots 4 and 5, the smaller one last in
  check_forest("known-answer", {3, 6, 3, 6, 5, X, X});     // tests/golden/known_answer.json
  check_forest("isolated-between", {X, 3, X, 4, X, X, 7, X});
  std::mt19937 rng(12345);
  for (int t = 0; t < 50; ++t) {
    const uint32_t n = 1 + rng() % 64;
    std::vector<uint32_t> p(n);
    for (uint32_t v = 0; v < n; ++v)
      p[v] = (v + 1 == n || rng() % 5 == 0) ? X : v + 1 + rng() % (n - v - 1);
    check_forest("random", p);
  }

  CHECK(!vf_heap_ok(3, 3, 8) && !vf_heap_ok(3, 2, 8) && !vf_heap_ok(3, 8, 8) && vf_heap_ok(3, 4, 8) &&
        vf_heap_ok(7, X, 8), "heap order");
  CHECK(vf_rounds(1) == 1 && vf_rounds(2) == 2 && vf_rounds(3) == 3 && vf_rounds(4) == 3 &&
        vf_rounds(5) == 4 && vf_rounds((1u << 20) + 2) == 22, "rounds");
  uint64_t r[8];
  vf_report(r, 0, 0, 0, 0, X);
  CHECK(r[0] == 0 && r[1] == 0 && r[2] == 0 && r[3] == 0 && r[4] == X && !r[5] && !r[6] && !r[7],
        "clean report");
  vf_report(r, 0, 2, 1, 3, 17);
  CHECK(r[0] == 0 && r[1] == 2 && r[2] == 1 && r[3] == 3 && r[4] == 17, "counts");
  vf_report(r, 1, 5, 5, 5, 9);
  CHECK(r[0] == 1 && r[1] == ~0ull && r[2] == ~0ull && r[3] == ~0ull && r[4] == 9 && !r[5],
        "heap violation hides the rest");

  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
