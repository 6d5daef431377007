// The exact tree widths' host-side index arithmetic (sheep_amd/csrc/width_layout.h) on forests
// of up to 64 ranks: the range-minimum structure over the Euler tour's depths (every [l, r]
// query against a linear scan), the arc -> LCA rule (every pair of ranks against a parent walk),
// the sort keys, and the whole weight construction of sheep_width.hip replayed on the host over
// random multigraphs with ends outside the sequence, against bags unioned up the tree.
// Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_width_layout.py.  Prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <set>
#include <vector>

#include "verify_layout.h"
#include "width_layout.h"

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

static const uint32_t X = VF_NONE;

// The tour of a heap-ordered forest (children and roots ascending, as verify_layout.h) and the
// structure sheep_width.hip builds over it.
struct Tour {
  uint32_t n = 0, nb = 0;
  std::vector<uint32_t> parent, tin, tout, depth, lca_tin, node_at, nkids;
  std::vector<uint64_t> pre, suf, tab;

  void walk(const std::vector<std::vector<uint32_t>>& kids, uint32_t v, uint32_t d, uint32_t& clock) {
    tin[v] = clock;
    depth[clock++] = d;
    for (uint32_t k : kids[v]) walk(kids, k, d + 1, clock);
    tout[v] = clock;
    depth[clock++] = d - 1;
  }
  explicit Tour(const std::vector<uint32_t>& p) : n((uint32_t)p.size()), parent(p) {
    const uint32_t n2 = 2 * n;
    tin.resize(n);
    tout.resize(n);
    depth.resize(n2);
    nkids.assign(n, 0);
    std::vector<std::vector<uint32_t>> kids(n);
    for (uint32_t v = 0; v < n; ++v)
      if (p[v] != X) { kids[p[v]].push_back(v); ++nkids[p[v]]; }
    uint32_t clock = 0;
    for (uint32_t v = 0; v < n; ++v)
      if (p[v] == X) walk(kids, v, 1, clock);
    lca_tin.resize(n2);
    node_at.resize(n2);
    for (uint32_t v = 0; v < n; ++v) {
      lca_tin[tin[v]] = tin[tw_arc_lca(false, v, p[v])];
      const uint32_t up = tw_arc_lca(true, v, p[v]);
      lca_tin[tout[v]] = up == TW_NONE ? TW_NONE : tin[up];
      node_at[tin[v]] = v;
      node_at[tout[v]] = X;
    }
    nb = tw_blocks(n2);
    pre.resize(n2);
    suf.resize(n2);
    tab.assign((size_t)tw_levels(nb) * nb, ~0ull);
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t lo = b * TW_BLOCK, hi = std::min(n2, lo + TW_BLOCK);
      uint64_t run = ~0ull;
      for (uint32_t q = lo; q < hi; ++q) pre[q] = run = tw_min(run, tw_cell(depth[q], q));
      run = ~0ull;
      for (uint32_t q = hi; q-- > lo;) suf[q] = run = tw_min(run, tw_cell(depth[q], q));
      tab[tw_tab_ix(nb, 0, b)] = run;
    }
    for (int k = 1; k < tw_levels(nb); ++k)
      for (uint32_t b = 0; b < tw_level_len(nb, k); ++b)
        tab[tw_tab_ix(nb, k, b)] = tw_min(tab[tw_tab_ix(nb, k - 1, b)],
                                          tab[tw_tab_ix(nb, k - 1, b + (1u << (k - 1)))]);
  }
  uint64_t range_min(uint32_t l, uint32_t r) const {
    return tw_range_min(depth.data(), pre.data(), suf.data(), tab.data(), nb, l, r);
  }
  uint32_t walk_lca(uint32_t a, uint32_t b) const {  // X: different trees
    while (a != b) {
      if (a == X || b == X) return X;
      if (a < b) a = parent[a]; else b = parent[b];
    }
    return a;
  }
};

static void check_rmq(const char* name, const std::vector<uint32_t>& p) {
  const Tour T(p);
  const uint32_t n2 = 2 * T.n;
  for (uint32_t l = 0; l < n2; ++l) {
    uint32_t best = T.depth[l];
    for (uint32_t r = l; r < n2; ++r) {
      best = std::min(best, T.depth[r]);
      const uint64_t c = T.range_min(l, r);
      CHECK(tw_cell_depth(c) == best, "%s: min of [%u, %u] = %u, scan %u", name, l, r,
            tw_cell_depth(c), best);
      const uint32_t at = tw_cell_pos(c);
      CHECK(at >= l && at <= r && T.depth[at] == best, "%s: argmin of [%u, %u] at %u", name, l, r, at);
    }
  }
  for (uint32_t a = 0; a < T.n; ++a)
    for (uint32_t b = 0; b < T.n; ++b) {
      if (a == b || T.tin[a] > T.tin[b]) continue;
      const uint64_t c = T.range_min(T.tin[a], T.tin[b]);
      const uint32_t want = T.walk_lca(a, b);
      if (tw_cell_depth(c) == 0) {
        CHECK(want == X, "%s: LCA(%u, %u) is the virtual root, walk %u", name, a, b, want);
      } else {
        const uint32_t t = T.lca_tin[tw_cell_pos(c)];
        CHECK(t != TW_NONE && want != X && T.node_at[t] == want, "%s: LCA(%u, %u) walk %u", name, a, b,
              want);
      }
    }
}

// Liu's elimination tree of rank-space records (lo < hi), by walks with path compression.
static std::vector<uint32_t> etree(uint32_t n, std::vector<std::pair<uint32_t, uint32_t>> e) {
  std::sort(e.begin(), e.end(), [](auto a, auto b) { return a.second < b.second; });
  std::vector<uint32_t> parent(n, X), anc(n, X);
  for (auto [lo, hi] : e) {
    uint32_t r = lo;
    while (true) {
      const uint32_t a = anc[r];
      if (a == hi) break;
      anc[r] = hi;
      if (a == X) { parent[r] = hi; break; }
      r = a;
    }
  }
  return parent;
}

// Records over ids [0, n_ids): seq holds n of them; the rest are outside.  The widths by the
// kernels' construction against bags unioned up the tree.
static void check_widths(std::mt19937& rng, uint32_t n, uint32_t n_out, uint32_t m) {
  const uint32_t n_ids = n + n_out;
  std::vector<uint32_t> ids(n_ids), rank(n_ids, X);
  for (uint32_t i = 0; i < n_ids; ++i) ids[i] = i;
  std::shuffle(ids.begin(), ids.end(), rng);
  for (uint32_t r = 0; r < n; ++r) rank[ids[r]] = r;
  std::vector<std::pair<uint32_t, uint32_t>> uv(m), inside;
  for (auto& r : uv) r = {rng() % n_ids, rng() % n_ids};
  for (auto [x, y] : uv) {
    const uint32_t a = rank[x], b = rank[y];
    if (a != X && b != X && a != b) inside.push_back({std::min(a, b), std::max(a, b)});
  }
  const std::vector<uint32_t> parent = etree(n, inside);
  const Tour T(parent);

  // brute force: bags as sets, an outside id as n + id
  std::vector<std::set<uint32_t>> bag(n);
  std::vector<uint64_t> pst(n, 0);
  for (auto [x, y] : uv) {
    if (x == y) continue;
    const uint32_t a = rank[x], b = rank[y];
    if (a == X && b == X) continue;
    const uint32_t lo = std::min(a, b);
    bag[lo].insert(std::max(a, b) == X ? tw_outside_key(n, a == X ? x : y) : std::max(a, b));
    ++pst[lo];
  }
  std::vector<uint64_t> want(n);
  for (uint32_t j = 0; j < n; ++j) {
    bag[j].erase(j);
    want[j] = 1 + bag[j].size();
    if (parent[j] != X) bag[parent[j]].insert(bag[j].begin(), bag[j].end());
  }

  // the kernels' construction
  std::vector<uint64_t> keys;
  for (auto [x, y] : uv) {
    uint64_t k = TW_SKIP;
    const uint32_t a = rank[x], b = rank[y];
    const uint32_t lo = std::min(a, b), hi = std::max(a, b);
    if (x != y && lo != X) {
      if (hi == X) {
        k = tw_key(tw_outside_key(n, a == X ? x : y), T.tin[lo]);
      } else {
        CHECK(vf_in_subtree(T.tin[lo], T.tin[hi], T.tout[hi]), "(A) holds on an elimination tree");
        k = tw_key(hi, T.tin[lo]);
      }
    }
    keys.push_back(k);
  }
  std::sort(keys.begin(), keys.end());
  std::vector<long long> wt(2 * (size_t)n, 0);
  std::vector<uint8_t> has(n, 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    const uint64_t k = keys[i];
    if (k == TW_SKIP || (i && keys[i - 1] == k)) continue;
    const uint32_t hi = tw_key_hi(k), t = tw_key_tin(k);
    CHECK(tw_key(hi, t) == k, "key round trip");
    wt[t] += 1;
    if (hi < n) has[hi] = 1;
    if (i && tw_key_hi(keys[i - 1]) == hi) {
      const uint64_t c = T.range_min(tw_key_tin(keys[i - 1]), t);
      if (tw_cell_depth(c) != 0) wt[T.lca_tin[tw_cell_pos(c)]] -= 1;
    }
  }
  for (uint32_t v = 0; v < n; ++v) wt[T.tin[v]] += (has[v] ? 0 : 1) - (long long)T.nkids[v];
  for (size_t q = 1; q < wt.size(); ++q) wt[q] += wt[q - 1];
  uint64_t fill = 0, fill_want = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t w = (uint64_t)tw_subtree_sum(wt.data(), T.tin[j], T.tout[j]);
    CHECK(w == want[j], "n %u out %u m %u: width[%u] = %llu, bags %llu", n, n_out, m, j,
          (unsigned long long)w, (unsigned long long)want[j]);
    fill += w - 1 - pst[j];
    fill_want += want[j] - 1 - pst[j];
  }
  CHECK(fill == fill_want, "fill");
}

int main() {
  check_rmq("single", {X});
  check_rmq("two-roots", {X, X});
  check_rmq("pair", {1, X});
  {
    std::vector<uint32_t> p(64);
    for (uint32_t v = 0; v < 64; ++v) p[v] = v + 1 < 64 ? v + 1 : X;
    check_rmq("path", p);  // 128 positions: two blocks, depths rising then falling
    for (uint32_t v = 0; v < 64; ++v) p[v] = v + 1 < 64 ? 63 : X;
    check_rmq("star", p);
    for (uint32_t v = 0; v < 64; ++v) p[v] = X;
    check_rmq("roots", p);
    p.resize(63);
    for (uint32_t v = 0; v < 63; ++v) p[v] = v < 62 ? 62 - (61 - v) / 2 : X;
    check_rmq("binary", p);
    p.resize(33);  // 66 positions: the second block holds two
    for (uint32_t v = 0; v < 33; ++v) p[v] = v + 1 < 33 ? v + 1 : X;
    check_rmq("path-33", p);
  }
  check_rmq("known-answer", {3, 6, 3, 6, 5, X, X});  // tests/golden/known_answer.json
  std::mt19937 rng(4321);
  for (int t = 0; t < 40; ++t) {
    const uint32_t n = 1 + rng() % 64;
    std::vector<uint32_t> p(n);
    for (uint32_t v = 0; v < n; ++v)
      p[v] = (v + 1 == n || rng() % 5 == 0) ? X : v + 1 + rng() % (n - v - 1);
    check_rmq("random", p);
  }
  // the table alone, on more blocks than 64 ranks give: every block range of a long path
  {
    std::vector<uint32_t> p(1500);
    for (uint32_t v = 0; v < 1500; ++v) p[v] = (v + 1 == 1500 || v % 97 == 96) ? X : v + 1;
    const Tour T(p);
    for (uint32_t l = 0; l < 3000; l += 37)
      for (uint32_t r = l; r < 3000; r += 29) {
        uint32_t best = T.depth[l];
        for (uint32_t q = l; q <= r; ++q) best = std::min(best, T.depth[q]);
        const uint64_t c = T.range_min(l, r);
        CHECK(tw_cell_depth(c) == best && tw_cell_pos(c) >= l && tw_cell_pos(c) <= r &&
                  T.depth[tw_cell_pos(c)] == best,
              "long: [%u, %u]", l, r);
      }
  }
  for (int t = 0; t < 60; ++t) {
    const uint32_t n = 1 + rng() % 64;
    check_widths(rng, n, t % 3 ? rng() % 8 : 0, rng() % (4 * n + 1));
  }

  CHECK(tw_blocks(0) == 0 && tw_blocks(1) == 1 && tw_blocks(64) == 1 && tw_blocks(65) == 2, "blocks");
  CHECK(tw_log2(1) == 0 && tw_log2(2) == 1 && tw_log2(3) == 1 && tw_log2(4) == 2 &&
            tw_log2(0xFFFFFFFFu) == 31, "log2");
  CHECK(tw_levels(0) == 0 && tw_levels(1) == 1 && tw_levels(2) == 2 && tw_levels(5) == 3, "levels");
  CHECK(tw_level_len(5, 0) == 5 && tw_level_len(5, 2) == 2, "level length");
  CHECK(tw_key(7, 9) < tw_key(8, 0) && tw_key(7, 9) < tw_key(7, 10) && tw_key(0xFFFFFFFEu, 5) < TW_SKIP,
        "key order");
  CHECK(tw_cell(2, 100) < tw_cell(3, 0) && tw_min(tw_cell(2, 100), tw_cell(2, 7)) == tw_cell(2, 7),
        "cell order");

  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
