// JTree (reference: lib/jtree.h:39-188): vid -> jnid index plus the elimination tree of the
// graph under seq.  The tree is built on the GPU (sheep_build_tree).  Of the chordal-extension
// options, make_kids + make_pst + make_jxn (-k -e -j) give every node's exact width 1 + |jxn|
// (sheep_tree_widths: computed on the GPU, no bag is stored, so memory_limit has nothing to
// cap); a width limit, the width search and rooting (-w/-x) are out of scope and rejected.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "defs.h"
#include "graph_wrapper.h"
#include "jnode.h"
#include "sheep_call.h"

class JTree {
  std::vector<jnid_t> index;  // vid -> jnid (jtree.h:44)

 public:
  JNodeTable jnodes;

  struct Options {  // jtree.h:71-108
    bool verbose = false;
    bool make_pad = true;
    bool make_kids = false, make_pst = false, make_jxn = false;
    size_t memory_limit = 1 * GIGA, width_limit = (size_t)-1;
    bool find_max_width = false, do_rooting = false;
    size_t rooting_limit = 0;
    // the bags only with the children and pst lists they are made from (the reference's
    // Options::isValid); the lists alone have no consumer here
    bool isSupported() const {
      bool const lists = make_kids || make_pst || make_jxn;
      return make_pad && (!lists || (make_kids && make_pst && make_jxn)) &&
             width_limit == (size_t)-1 && !find_max_width && !do_rooting && rooting_limit == 0;
    }
  };

  template <typename GraphType>
  JTree(GraphType const& graph, std::vector<vid_t> const& seq, Options opts = Options()) {
    build(graph, seq, opts);
  }
  // built into a mapped .tre (jtree.h:125-137: the table is the file, jnode.cpp:52-74)
  template <typename GraphType>
  JTree(GraphType const& graph, std::vector<vid_t> const& seq, char const* filename,
        Options opts = Options())
      : jnodes(filename, (jnid_t)seq.size()) {
    build(graph, seq, opts);
  }
  // graph2tree -i -r in one collective step (ranks of a joined ProcessGroup, comm.h): the tree
  // of the union of every rank's partial graph under the shared seq, on every rank — the
  // result of JTree(partial graph) + jnodes.mpi_merge() without the partial trees.
  struct Collective {};
  template <typename GraphType>
  JTree(GraphType const& graph, std::vector<vid_t> const& seq, Collective, Options opts = Options()) {
    if (!opts.isSupported() || opts.make_jxn)  // a rank's shard cannot give the union's widths
      throw std::invalid_argument("JTree: chordal-extension options are not built on MI355X");
    make_index(seq);
    graph.to_device();
    std::vector<jnid_t> parent(seq.size());
    std::vector<esize_t> pst(seq.size());
    if (!seq.empty())
      sheep_check(sheep_build_tree_multi(graph.records_data(), graph.records(), seq.data(),
                                         (uint32_t)seq.size(), parent.data(), pst.data()),
                  "JTree (collective)");
    jnodes.assign(parent, pst);
  }

  // open constructor (jtree.h:138-143): the .tre mapped in place
  JTree(std::vector<vid_t> const& seq, char const* filename) : jnodes(filename) { make_index(seq); }

  jnid_t vid2jnid(vid_t X) const { return X < index.size() ? index[X] : INVALID_JNID; }
  size_t size() const { return jnodes.size(); }

  std::vector<vid_t> get_sequence() const {
    std::vector<vid_t> seq(size());
    for (vid_t X = 0; X != index.size(); ++X)
      if (index[X] != INVALID_JNID) seq.at(index[X]) = X;
    return seq;
  }

  void print() const {
    std::vector<vid_t> s = get_sequence();
    for (jnid_t id = 0; id != size(); ++id) {
      printf("%4zu:%-8zu", (size_t)id, (size_t)s.at(id));
      jnodes.print(id);
    }
  }

  // Validity as jtree.cpp:238-300 intends: heap order, and for every edge the higher endpoint
  // is an ancestor of the lower one (the reference's check reads index.at(X) where it meant
  // index.at(nbr); this one checks the intended property).  O(m * height): a debug option.
  template <typename GraphType>
  bool isValid(GraphType const& graph, std::vector<vid_t> const& seq, Options = Options()) const {
    for (jnid_t id = 0; id < size(); ++id)
      if (jnodes.parent(id) != INVALID_JNID && jnodes.parent(id) <= id) return false;
    for (vid_t X : seq) {
      if (!graph.isNode(X)) continue;
      jnid_t cur = vid2jnid(X);
      for (auto e = graph.getEdgeItr(X); !e.isEnd(); ++e) {
        jnid_t nb = vid2jnid(*e);
        if (nb == INVALID_JNID || nb >= cur) continue;
        while (nb != INVALID_JNID && nb < cur) nb = jnodes.parent(nb);
        if (nb != cur) return false;
      }
    }
    return true;
  }

  // Certificate on the GPU (sheep_verify_tree): true iff this table is THE elimination tree of
  // the graph's records under seq, pst_weight included.  Linear work whatever the height, so it
  // runs at full size, and unlike isValid it rejects a heap-ordered forest that merely keeps
  // every higher endpoint above the lower one.  report: the 8 words of include/sheep_amd.h.
  template <typename GraphType>
  bool certify(GraphType const& graph, std::vector<vid_t> const& seq, uint64_t report[8]) const {
    if (seq.size() != size()) throw std::invalid_argument("certify: sequence and tree sizes differ");
    graph.to_device();
    std::vector<jnid_t> parent = jnodes.parents();
    std::vector<esize_t> pst = jnodes.psts();
    sheep_check(sheep_verify_tree(graph.records_data(), graph.records(), seq.data(),
                                  (uint32_t)seq.size(), parent.data(), pst.data(), report),
                "JTree::certify");
    return report[0] == 0 && report[1] == 0 && report[2] == 0 && report[3] == 0;
  }

 private:
  void make_index(std::vector<vid_t> const& seq) {
    if (seq.empty()) return;
    index.assign(*std::max_element(seq.begin(), seq.end()) + 1, INVALID_JNID);
    for (jnid_t id = 0; id != seq.size(); ++id) index[seq[id]] = id;
  }

  template <typename GraphType>
  void build(GraphType const& graph, std::vector<vid_t> const& seq, Options opts) {
    if (!opts.isSupported())
      throw std::invalid_argument("JTree: chordal-extension options are not built on MI355X");
    make_index(seq);
    graph.to_device();
    std::vector<jnid_t> parent(seq.size());
    std::vector<esize_t> pst(seq.size());
    if (!seq.empty())
      sheep_check(sheep_build_tree(graph.records_data(), graph.records(), seq.data(),
                                   (uint32_t)seq.size(), parent.data(), pst.data()),
                  "JTree");
    jnodes.assign(parent, pst);
    if (opts.make_jxn) {  // no width limit exists, so the tree is the one just built
      std::vector<uint32_t> width(seq.size());
      uint64_t facts[9];
      sheep_check(sheep_tree_widths(graph.records_data(), graph.records(), seq.data(),
                                    (uint32_t)seq.size(), parent.data(), pst.data(), width.data(),
                                    facts),
                  "JTree (widths)");
      jnodes.makeKids();
      jnodes.setWidths(std::move(width));
    }
  }
};
