// The host half of sheep_partition_dev (sheep_amd/csrc/part_layout.h) on heap-ordered forests of
// up to 64 ranks, against a direct restatement of lib/partition.h's forwardPartition on ONE kids
// table for a whole k list (so the orders an earlier k's std::sort left behind matter).  What the
// kernels do is replayed here in plain loops: subtree sums, the children lists in slot order, the
// ordered compaction of the heavy ranks, and the push-down as one prefix sum over the Euler
// tour.  Stand-alone (its own main), built with -fsanitize=address,undefined by
// tests/test_part_layout.py.  Prints "ok".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <random>
#include <vector>

#include "part_layout.h"

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

static const uint32_t X = PT_NONE;
typedef int16_t part_t;
static const part_t INVALID_PART = -1;

// lib/partition.h:56-95 with pst weights, on kids lists that live as long as the table.
struct RefTable {
  std::vector<uint32_t> parent;
  std::vector<uint64_t> w;
  std::vector<std::vector<uint32_t>> kids;  // makeKids: ascending
  RefTable(const std::vector<uint32_t>& p, const std::vector<uint64_t>& ww) : parent(p), w(ww), kids(p.size()) {
    for (uint32_t v = 0; v < p.size(); ++v)
      if (p[v] != X) kids[p[v]].push_back(v);
  }
  std::vector<part_t> partition(size_t const max_component) {
    const size_t n = parent.size();
    std::vector<part_t> parts(n, INVALID_PART);
    std::vector<size_t> part_size;
    std::vector<size_t> below(n, 0);
    for (uint32_t id = 0; id != n; ++id) {
      below.at(id) += w[id];
      if (below.at(id) > max_component) {
        std::sort(kids[id].begin(), kids[id].end(),
                  [&below](uint32_t const l, uint32_t const r) { return below.at(l) > below.at(r); });
        do {
          for (auto it = kids[id].begin(); below.at(id) > max_component && it != kids[id].end(); ++it) {
            uint32_t const kid = *it;
            if (parts.at(kid) != INVALID_PART) continue;
            for (part_t cp = 0; cp != (part_t)part_size.size(); ++cp) {
              if (part_size.at(cp) + below.at(kid) <= max_component) {
                below.at(id) -= below.at(kid);
                part_size.at(cp) += below.at(kid);
                parts.at(kid) = cp;
                break;
              }
            }
          }
          if (below.at(id) > max_component) part_size.push_back(0);
        } while (below.at(id) > max_component);
      }
      if (parent[id] != X) below.at(parent[id]) += below.at(id);
    }
    for (uint32_t id = n - 1; id != (uint32_t)-1; --id) {
      if (parts.at(id) == INVALID_PART && parent[id] != X) parts.at(id) = parts.at(parent[id]);
      while (parts.at(id) == INVALID_PART) {
        for (part_t cp = part_size.size() - 1; cp != -1; --cp) {
          if (part_size.at(cp) + below.at(id) <= max_component) {
            part_size.at(cp) += below.at(id);
            parts.at(id) = cp;
            break;
          }
        }
        if (parts.at(id) == INVALID_PART) part_size.push_back(0);
      }
    }
    return parts;
  }
};

// What the device leaves for the host, and the push-down it runs afterwards.
struct Dev {
  uint32_t n;
  std::vector<uint32_t> parent, kfirst, klast, slot_kid, tin, tout;
  std::vector<uint64_t> w, s0, slot_s0;
  std::vector<PtKid> roots;

  void walk(uint32_t v, uint32_t& clock) {
    tin[v] = clock++;
    if (kfirst[v] != X)
      for (uint32_t i = kfirst[v]; i <= klast[v]; ++i) walk(slot_kid[i], clock);
    tout[v] = clock++;
  }
  Dev(const std::vector<uint32_t>& p, const std::vector<uint64_t>& ww)
      : n((uint32_t)p.size()), parent(p), kfirst(n + 1, X), klast(n + 1, X), tin(n), tout(n), w(ww), s0(ww) {
    for (uint32_t v = 0; v < n; ++v)
      if (p[v] != X) s0[p[v]] += s0[v];  // heap order: a kid comes before its parent
    // the items (parent << 32 | v) sorted by parent, roots under the virtual parent n
    std::vector<uint64_t> items(n);
    for (uint32_t v = 0; v < n; ++v) items[v] = ((uint64_t)(p[v] == X ? n : p[v]) << 32) | v;
    std::sort(items.begin(), items.end());
    slot_kid.resize(n);
    slot_s0.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t par = (uint32_t)(items[i] >> 32);
      slot_kid[i] = (uint32_t)items[i];
      slot_s0[i] = s0[slot_kid[i]];
      if (kfirst[par] == X) kfirst[par] = i;
      klast[par] = i;
    }
    if (kfirst[n] != X)
      for (uint32_t i = kfirst[n]; i <= klast[n]; ++i) roots.push_back({slot_kid[i], slot_s0[i]});
    uint32_t clock = 0;
    for (auto const& r : roots) walk(r.kid, clock);
  }
  std::vector<PtHeavy> heavy(uint64_t maxc) const {
    std::vector<uint32_t> idx(n, X);
    std::vector<PtHeavy> H;
    for (uint32_t v = 0; v < n; ++v)
      if (s0[v] > maxc) idx[v] = (uint32_t)H.size(), H.push_back({v, X, s0[v], kfirst[v], klast[v]});
    for (auto& h : H)
      if (parent[h.rank] != X) h.pidx = idx[parent[h.rank]];
    return H;
  }
  std::vector<part_t> push_down(const std::vector<PtDelta>& deltas) const {
    std::vector<long long> wt(2 * (size_t)n, 0);
    for (auto const& d : deltas) {
      CHECK(wt[tin[d.rank]] == 0 && wt[tout[d.rank]] == 0, "rank %u has two deltas", d.rank);
      wt[tin[d.rank]] = d.d;
      wt[tout[d.rank]] = -(long long)d.d;
    }
    for (size_t i = 1; i < wt.size(); ++i) wt[i] += wt[i - 1];
    std::vector<part_t> parts(n);
    for (uint32_t v = 0; v < n; ++v) parts[v] = (part_t)wt[tin[v]];
    return parts;
  }
};

struct Stats {
  uint64_t runs = 0, cuts = 0, reused = 0;  // reused: runs whose cuts fetched nothing new
};

// One forest, one k list on one table.  A k at which a rank outweighs a part is skipped, as the
// driver refuses it.
static void run_case(const std::vector<uint32_t>& parent, const std::vector<uint64_t>& w,
                     const std::vector<int>& ks, double balance, Stats& st, const char* what) {
  RefTable ref(parent, w);
  Dev dev(parent, w);
  PtOrders orders;
  size_t total = 0, wmax = 0;
  for (uint64_t x : w) total += x, wmax = std::max<size_t>(wmax, x);
  for (int k : ks) {
    const size_t maxc = pt_max_component(total, (int16_t)k, balance);
    if (wmax > maxc) continue;  // refused before the walk, by both paths
    const std::vector<part_t> want = ref.partition(maxc);
    const std::vector<PtHeavy> H = dev.heavy(maxc);
    for (size_t i = 0; i < H.size(); ++i)
      CHECK(H[i].pidx == X || (H[i].pidx > i && H[H[i].pidx].rank == parent[H[i].rank]),
            "%s: H not closed upwards at %zu", what, i);
    uint64_t fetched_before = 0;
    for (auto const& o : orders) fetched_before += o.second.size();
    PtOut out;
    const int rc = pt_partition(H.data(), H.size(), dev.roots.data(), dev.roots.size(), maxc, orders,
                                [&](uint32_t a, uint32_t b, std::vector<PtKid>& L) {
                                  CHECK(a <= b && b < dev.n, "%s: slots %u..%u", what, a, b);
                                  for (uint32_t i = a; i <= b; ++i) L.push_back({dev.slot_kid[i], dev.slot_s0[i]});
                                },
                                out);
    CHECK(rc == 0, "%s: k %d returned %d", what, k, rc);
    if (rc) return;
    const std::vector<part_t> got = dev.push_down(out.deltas);
    part_t top = -1;
    for (part_t p : want) top = std::max(top, p);
    CHECK(got == want, "%s: parts differ at k %d (n %zu)", what, k, parent.size());
    CHECK(out.created == (uint32_t)(top + 1), "%s: created %u, want %d", what, out.created, top + 1);
    ++st.runs;
    st.cuts += out.cuts;
    uint64_t fetched_after = 0;
    for (auto const& o : orders) fetched_after += o.second.size();
    CHECK(fetched_after - fetched_before == out.kids_fetched, "%s: fetch count", what);
    if (out.cuts && out.kids_fetched == 0) ++st.reused;
  }
}

static std::vector<uint32_t> random_forest(std::mt19937_64& rng, uint32_t n, int shape) {
  std::vector<uint32_t> p(n, X);
  for (uint32_t v = 0; v + 1 < n; ++v) {
    switch (shape) {
      case 0: p[v] = v + 1 + (uint32_t)(rng() % (n - v - 1)); break;           // random tree
      case 1: p[v] = rng() % 4 == 0 ? X : v + 1 + (uint32_t)(rng() % (n - v - 1)); break;  // many roots
      case 2: p[v] = v + 1; break;                                             // path
      case 3: p[v] = n - 1; break;                                             // star
      case 4: p[v] = std::min<uint32_t>(n - 1, v + 1 + (uint32_t)(rng() % 3)); break;  // tall
      default: p[v] = rng() % 2 ? X : std::min<uint32_t>(n - 1, v + 1 + (uint32_t)(rng() % 5)); break;
    }
  }
  return p;
}

int main() {
  Stats st;
  // below == max_component must not cut: a chain 0 -> 1 -> 2 with weights 2, 2, 0.
  {
    const std::vector<uint32_t> p = {1, 2, X};
    const std::vector<uint64_t> w = {2, 2, 0};
    Dev dev(p, w);
    PtOrders orders;
    PtOut out;
    auto fetch = [&](uint32_t a, uint32_t b, std::vector<PtKid>& L) {
      for (uint32_t i = a; i <= b; ++i) L.push_back({dev.slot_kid[i], dev.slot_s0[i]});
    };
    // k = 1, balance 1.0: max_component 4 = the root's below
    std::vector<PtHeavy> H = dev.heavy(4);
    CHECK(H.empty(), "S0 == max_component is light");
    CHECK(pt_partition(H.data(), H.size(), dev.roots.data(), dev.roots.size(), 4, orders, fetch, out) == 0, "k 1");
    CHECK(out.cuts == 0 && out.created == 1, "k 1: cuts %llu created %u", (unsigned long long)out.cuts, out.created);
    CHECK(dev.push_down(out.deltas) == (std::vector<part_t>{0, 0, 0}), "k 1 parts");
    // k = 2: max_component 2.  Rank 0 (below 2) is whole, rank 1 (4) is cut once, rank 2 ends at 2.
    H = dev.heavy(2);
    CHECK(H.size() == 2 && H[0].rank == 1 && H[1].rank == 2 && H[0].pidx == 1, "heavy ranks 1, 2");
    CHECK(pt_partition(H.data(), H.size(), dev.roots.data(), dev.roots.size(), 2, orders, fetch, out) == 0, "k 2");
    CHECK(out.cuts == 1 && out.created == 2, "k 2: cuts %llu created %u", (unsigned long long)out.cuts, out.created);
    CHECK(dev.push_down(out.deltas) == (std::vector<part_t>{0, 1, 1}), "k 2 parts");
    run_case(p, w, {1, 2, 1}, 1.0, st, "chain");
  }
  // bins past int16: 40000 unit roots, max_component 1
  {
    const uint32_t n = 40000;
    std::vector<PtKid> roots(n);
    for (uint32_t v = 0; v < n; ++v) roots[v] = {v, 1};
    PtOrders orders;
    PtOut out;
    auto fetch = [&](uint32_t, uint32_t, std::vector<PtKid>&) {};
    CHECK(pt_partition(nullptr, 0, roots.data(), n, 1, orders, fetch, out) == -ERANGE, "bins past 32767");
    CHECK(pt_partition(nullptr, 0, roots.data(), 32767, 1, orders, fetch, out) == 0 && out.created == 32767,
          "32767 bins fit");
  }
  std::mt19937_64 rng(20240607);
  const std::vector<std::vector<int>> klists = {{2, 3, 7, 3}, {5, 2, 2, 9, 4}, {3}, {16, 2, 16}, {1, 4, 1}};
  for (int it = 0; it < 6000; ++it) {
    const uint32_t n = 1 + (uint32_t)(rng() % 64);
    const std::vector<uint32_t> p = random_forest(rng, n, it % 6);
    std::vector<uint64_t> w(n);
    const int wk = (it / 6) % 5;
    for (uint32_t v = 0; v < n; ++v)
      w[v] = wk == 0 ? 1 : wk == 1 ? rng() % 2 : wk == 2 ? rng() % 4 : wk == 3 ? 3 : (rng() % 8 == 0 ? rng() % 9 : 0);
    const double balance = it % 3 == 0 ? 1.0 : it % 3 == 1 ? 1.03 : 1.5;
    run_case(p, w, klists[(it / 30) % klists.size()], balance, st, "random");
  }
  // all weights zero: nothing is heavy, every root lands in bin 0
  run_case(random_forest(rng, 50, 1), std::vector<uint64_t>(50, 0), {2, 3}, 1.03, st, "zero");
  CHECK(st.runs > 8000, "only %llu partitions ran", (unsigned long long)st.runs);
  CHECK(st.cuts > 8000, "only %llu cuts", (unsigned long long)st.cuts);
  CHECK(st.reused > 100, "only %llu runs cut on kept orders alone", (unsigned long long)st.reused);
  if (fails) {
    fprintf(stderr, "%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
