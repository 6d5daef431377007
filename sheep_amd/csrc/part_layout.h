// Host half of the forward partition of a tree in HBM (sheep_partition_dev; kernels in
// sheep_part.hip; DESIGN.md §4.10 has the method and the proof sketch).  Plain C++17 without HIP:
// the records the kernels hand over, the walk over the heavy ranks, the reference's sort and
// first-fit packing of a cut rank's kids, the kids orders kept from one k to the next, the roots'
// packing and the deltas of the push-down.  tests/cpp/part_layout.cpp compiles it with g++ under
// the sanitizers and checks it against a restatement of lib/partition.h's loop on one table.
//
// In rank space, with w = pst, S0[v] the subtree sum of w and H = { v : S0[v] > max_component }:
//   * H is closed upwards (weights are not negative), so it is a forest of its own;
//   * a rank outside H is never cut, and `below` of the reference is S0[v] when it reaches v;
//   * a rank of H starts at S0[h] - sum of its heavy kids' S0 + sum of their final `below`.
// Only a cut rank (below > max_component) looks at its kids: their ranks ascending (slots
// kfirst..klast of the tour's children lists, as makeKids orders them) or in the order an earlier
// k's std::sort left them, each with S0 (light) or the final below (heavy).
#pragma once
#include <errno.h>
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

namespace sheep {

constexpr uint32_t PT_NONE = 0xFFFFFFFFu;
constexpr size_t PT_MAX_BINS = 32767;  // parts are int16 (part_t)

// One heavy rank, as the compaction kernel writes it (ascending in rank): 24 bytes.
struct PtHeavy {
  uint32_t rank;
  uint32_t pidx;    // index in H of the parent, PT_NONE for a root
  uint64_t s0;      // subtree sum of pst
  uint32_t kfirst;  // slots of its children list (PT_NONE: no kids)
  uint32_t klast;
};
static_assert(sizeof(PtHeavy) == 24, "k_pt_heavy writes six words per record");

// A kid (or a root) and its subtree sum, as two plain copies of a slot range give them.
struct PtKid {
  uint32_t kid;
  uint64_t s0;
};

// +d at tin[rank], -d at tout[rank] (k_pt_deltas): 8 bytes.
struct PtDelta {
  uint32_t rank;
  int32_t d;
};
static_assert(sizeof(PtDelta) == 8, "uploaded as one u64 per delta");

// Partition::Partition (lib/partition.h:45), the expression kept as it stands there.
inline size_t pt_max_component(size_t total_weight, int16_t num_parts, double balance_factor) {
  size_t max_component = (total_weight / num_parts) * balance_factor;
  return max_component;
}

// The kids orders that forwardPartition's in-place std::sort leaves behind, keyed by rank: only
// ranks that were cut at some k have an entry, every other list is still ascending.
typedef std::unordered_map<uint32_t, std::vector<PtKid>> PtOrders;

struct PtOut {
  std::vector<PtDelta> deltas;
  uint32_t created = 0;  // largest part + 1
  uint64_t cuts = 0, kids_fetched = 0, longest = 0;
};

namespace pt_detail {

struct Val {
  uint32_t kid;
  int32_t part;
  uint64_t s0, val;
};

// Index in H (ascending in rank) of a rank known to be there.
inline size_t h_index(const PtHeavy* H, size_t nh, uint32_t rank) {
  size_t a = 0, b = nh;
  while (a < b) {
    const size_t mid = a + (b - a) / 2;
    if (H[mid].rank < rank) a = mid + 1; else b = mid;
  }
  return a;
}

// Smallest bin load: a kid whose value does not fit on top of it fits nowhere.
inline uint64_t min_load(const std::vector<uint64_t>& bins) {
  uint64_t m = ~0ull;
  for (uint64_t b : bins) m = b < m ? b : m;
  return m;
}

}  // namespace pt_detail

// One k.  H: the nh heavy ranks for this max_component; roots: the top-level roots ascending in
// rank; fetch(kfirst, klast, out) appends the kids of slots [kfirst, klast] with their S0 to out.
// Returns 0, or -ERANGE when the bins would pass PT_MAX_BINS.  The caller has refused a rank
// whose own weight exceeds max_component (the loops below would not end).
template <class Fetch>
int pt_partition(const PtHeavy* H, size_t nh, const PtKid* roots, size_t n_roots,
                 uint64_t max_component, PtOrders& orders, Fetch&& fetch, PtOut& out) {
  using pt_detail::Val;
  out = PtOut();
  std::vector<uint64_t> below(nh), kid_s0(nh, 0), kid_below(nh, 0);
  std::vector<int32_t> hpart(nh, -1);  // the part a heavy rank was packed into, if any
  std::vector<uint64_t> part_size;
  struct Assigned { uint32_t kid; int32_t part; size_t parent; };
  std::vector<Assigned> assigned;
  std::vector<Val> V;
  int32_t top = -1;

  for (size_t i = 0; i < nh; ++i) {
    uint64_t b = H[i].s0 - kid_s0[i] + kid_below[i];
    if (b > max_component) {
      ++out.cuts;
      std::vector<PtKid>& L = orders[H[i].rank];
      if (L.empty() && H[i].kfirst != PT_NONE) {
        fetch(H[i].kfirst, H[i].klast, L);
        out.kids_fetched += L.size();
      }
      out.longest = std::max<uint64_t>(out.longest, L.size());
      V.resize(L.size());
      for (size_t j = 0; j < L.size(); ++j) {
        V[j].kid = L[j].kid;
        V[j].part = -1;
        V[j].s0 = L[j].s0;
        V[j].val = L[j].s0 > max_component ? below[pt_detail::h_index(H, i, L[j].kid)] : L[j].s0;
      }
      // partition.cpp:104: the unstable sort, on the same order with the same comparisons
      std::sort(V.begin(), V.end(), [](Val const& l, Val const& r) { return l.val > r.val; });
      for (size_t j = 0; j < L.size(); ++j) {
        L[j].kid = V[j].kid;
        L[j].s0 = V[j].s0;
      }
      // partition.cpp:105-121.  Bins only fill up while a rank is cut, so three shortcuts skip
      // comparisons that cannot succeed and change no result: a value that does not fit on a
      // lower bound of the lightest bin fits nowhere; the kids after a failed one with its value
      // fail too (nothing changed in between); and the bins that refused a value refuse it again.
      uint64_t lightest = pt_detail::min_load(part_size);  // a lower bound from here on
      uint64_t seen_val = ~0ull;  // bins [0, seen_bins) have refused this value
      size_t seen_bins = 0;
      size_t first = 0;  // every kid before it is packed
      do {
        while (first < V.size() && V[first].part >= 0) ++first;
        for (size_t j = first; b > max_component && j < V.size(); ++j) {
          Val& e = V[j];
          if (e.part >= 0) continue;
          bool fits = false;
          if (!part_size.empty() && lightest + e.val <= max_component) {
            size_t cp = e.val == seen_val ? seen_bins : 0;
            for (; cp != part_size.size(); ++cp) {
              if (part_size[cp] + e.val <= max_component) {
                b -= e.val;
                part_size[cp] += e.val;
                e.part = (int32_t)cp;
                fits = true;
                break;
              }
            }
            seen_val = e.val;
            seen_bins = cp;
            if (!fits) lightest = pt_detail::min_load(part_size);
          }
          if (!fits)
            while (j + 1 < V.size() && V[j + 1].val == e.val) ++j;
        }
        if (b > max_component) {
          if (part_size.size() >= PT_MAX_BINS) return -ERANGE;
          part_size.push_back(0);
          lightest = 0;
        }
      } while (b > max_component);
      for (Val const& e : V) {
        if (e.part < 0) continue;
        assigned.push_back({e.kid, e.part, i});
        top = std::max(top, e.part);
        if (e.s0 > max_component) hpart[pt_detail::h_index(H, i, e.kid)] = e.part;
      }
    }
    below[i] = b;
    if (H[i].pidx != PT_NONE) {
      kid_s0[H[i].pidx] += H[i].s0;
      kid_below[H[i].pidx] += b;
    }
  }

  // partition.cpp:140-156: the roots in descending rank, each into the last bin that takes it.
  for (size_t r = n_roots; r-- > 0;) {
    const bool heavy = roots[r].s0 > max_component;
    const size_t hi = heavy ? pt_detail::h_index(H, nh, roots[r].kid) : 0;
    const uint64_t val = heavy ? below[hi] : roots[r].s0;
    int32_t part = -1;
    while (part < 0) {
      for (size_t cp = part_size.size(); cp-- > 0;) {
        if (part_size[cp] + val <= max_component) {
          part_size[cp] += val;
          part = (int32_t)cp;
          break;
        }
      }
      if (part < 0) {
        if (part_size.size() >= PT_MAX_BINS) return -ERANGE;
        part_size.push_back(0);
      }
    }
    if (heavy) hpart[hi] = part;
    top = std::max(top, part);
    if (part) out.deltas.push_back({roots[r].kid, part});
  }

  // The push-down over H alone: the part of each heavy rank's nearest packed ancestor-or-self
  // (a parent comes after its kids, a heavy root is packed).
  std::vector<int32_t>& pf = hpart;
  for (size_t i = nh; i-- > 0;)
    if (pf[i] < 0) pf[i] = H[i].pidx != PT_NONE ? pf[H[i].pidx] : 0;
  for (auto const& a : assigned) {
    const int32_t d = a.part - pf[a.parent];
    if (d) out.deltas.push_back({a.kid, d});
  }
  out.created = (uint32_t)(top + 1);
  return 0;
}

}  // namespace sheep
