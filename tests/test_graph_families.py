"""The structured graph families (tests/graph_families.py) on the CPU: for every family at the
sizes S and L the CPU checker's tree, the closed form (where there is one) and a plain-Python
Liu union-find agree bit for bit, so that the GPU tests (tests/test_tree_families_gpu.py) can
lean on the checker for deep chains, forests of many roots and all-ties sequences.  Also: the
property the leapfrog family exists for, the merge of partial trees on chains, and the constants
of the tree loop that the families' spacings are built around."""
import os
import re

import numpy as np
import pytest

import graph_families as gf
from conftest import ROOT

SIZES = ("S", "L")
CASES = [(name, z) for z in SIZES for name in gf.NAMES]


@pytest.mark.parametrize("name,size", CASES, ids=["%s-%s" % c for c in CASES])
def test_checker_closed_form_and_liu_agree(oracle, name, size):
    f = gf.make(name, size)
    assert np.array_equal(np.sort(f.seq), np.arange(f.n_ids)), "seq is a permutation of the ids"
    p, s = oracle.build_tree(f.uv, f.seq)
    lp, ls = gf.liu_parent(f.uv, f.seq), gf.pst_plain(f.uv, f.seq)
    assert np.array_equal(p, lp), "checker parent != Liu"
    assert np.array_equal(s, ls), "checker pst != bincount"
    assert int(ls.sum()) == f.uv.shape[0]  # no self-loops: every record has one lower end
    if f.parent is not None:
        assert np.array_equal(p, f.parent), "checker parent != closed form"
        assert np.array_equal(s, f.pst), "checker pst != closed form"


@pytest.mark.parametrize("size", ["S", "L", "B"])
def test_leapfrog_giant_is_overtaken(size):
    """Among ranks < n/2 the largest component is A's (it holds rank 0); among ranks < 7n/8 it is
    B's, larger than A's by more than 4/256 of the ranks: an anchor picked from 256 samples at the
    first cut sits in A, at the second it has to move (k_kb_pick keeps the previous anchor only
    within 4 samples of the best), after giant bits were set for A."""
    f = gf.make("leapfrog", size)
    n = f.n_ids
    q = n // 4
    roots, sizes = gf.component_sizes_below(f.uv, f.seq, n // 2)
    a_root = int(roots[0])
    assert sizes[a_root] == max(sizes.values())
    assert (roots[:q] == a_root).sum() == sizes[a_root] and sizes[a_root] > 0.95 * q
    big_b = max(c for r, c in sizes.items() if r != a_root)
    assert 256 * big_b >= 3 * (n // 2)  # B's part holds samples too: the pick has a choice
    cut = 7 * n // 8
    roots, sizes = gf.component_sizes_below(f.uv, f.seq, cut)
    a_root = int(roots[0])
    b_root = max(sizes, key=sizes.get)
    assert b_root != a_root and (roots[:q] != b_root).all()
    assert sizes[b_root] - sizes[a_root] > 4 * cut / 256


@pytest.mark.parametrize("size", ["S", "L", "B"])
@pytest.mark.parametrize("bridge", ["last", "mid"])
def test_two_giants_are_comparable(bridge, size):
    """Below the bridge's hi end the two largest components are the even and the odd graph, within
    a few ranks of each other."""
    f = gf.make("two-giants-" + bridge, size)
    top = f.n_ids - 1 if bridge == "last" else f.n_ids // 2
    roots, sizes = gf.component_sizes_below(f.uv, f.seq, top)
    big = sorted(sizes.items(), key=lambda rc: -rc[1])[:2]
    assert big[1][1] > 0.9 * big[0][1]
    assert {r % 2 for r, _ in big} == {0, 1}  # a component's root is its highest rank
    roots, sizes = gf.component_sizes_below(f.uv, f.seq, top + 1)
    assert roots[big[0][0]] == roots[big[1][0]]  # the bridge joins them


@pytest.mark.parametrize("name", ["path-asc", "grid-rows"])
def test_merge_of_shards_equals_whole(oracle, name):
    """Partial trees of 3 record shards, merged pairwise, are the whole tree: on a chain of
    height n - 1 and on a grid, where the partial trees are forests of many roots."""
    f = gf.make(name, "S")
    whole = oracle.build_tree(f.uv, f.seq)
    R = f.uv.shape[0]
    trees = [oracle.build_tree(f.uv[R * i // 3: R * (i + 1) // 3], f.seq) for i in range(3)]
    assert sum(int((t[0] == gf.INVALID).sum()) for t in trees) > 3 * 1000  # many roots each
    acc = trees[0]
    for t in trees[1:]:
        acc = oracle.merge(acc[0], acc[1], t[0], t[1])
    assert np.array_equal(acc[0], whole[0]) and np.array_equal(acc[1], whole[1])


def test_degree_order_is_the_checkers_sequence(oracle):
    for name in ("grid-rows", "path-asc", "cliques-inter", "bipartite"):
        f = gf.make(name, "S")
        for mode in (oracle.LLAMA, oracle.FILE):
            assert np.array_equal(gf.degree_order(f.uv, f.n_ids), oracle.degree_sequence(f.uv, mode))
    assert np.array_equal(gf.make("grid-degree", "S").seq,
                          oracle.degree_sequence(gf.make("grid-rows", "S").uv))


def test_sizes_reach_the_paths_they_are_for():
    """S, L and B are the smallest sizes at which the loop's paths exist (see graph_families)."""
    for name in gf.NAMES:
        s, l = gf.make(name, "S"), gf.make(name, "L")
        assert 2 * gf.KM_WIN < s.n_ids < 71000 and s.n_ids / 16 > 2 * gf.SCAN_LIMIT * 32
        assert (1 << 18) < l.n_ids < 301000
        assert s.n_ids & (s.n_ids - 1) and l.n_ids & (l.n_ids - 1)
    for name in gf.GRAPHS:  # the hi-bin path: from 2^20 records
        m = gf.make(name, "B").uv.shape[0]
        assert (1 << 20) <= m < (1 << 20) + (1 << 12), (name, m)
    f = gf.make("window", "L")  # KM_CHUNK consecutive records in hi order span four windows
    assert f.uv.shape[0] > gf.KM_CHUNK
    hi = np.sort(f.uv.max(axis=1))
    assert hi[gf.KM_CHUNK - 1] - hi[0] >= 4 * gf.KM_WIN - 16
    hi = np.sort(gf.make("window", "S").uv.max(axis=1))
    assert hi[-1] - hi[0] > gf.KM_WIN  # S: one chunk, wider than its window


def test_sparse_star_spacings():
    """The leaves' gaps are the four spacings, each in a stretch of its own, and each stretch is
    wider than the widest bucket of the GPU tests' option sets (n / 8 ranks: 8 rank cuts), so it
    crosses a bucket boundary under each of them."""
    for name, head in (("sparse-star", 1), ("sparse-star-head", 4375)):
        f = gf.make(name, "S")
        lo, hi = gf.ranks_of(f.uv, f.seq)
        leaves = np.sort(hi[lo == 0])
        leaves = leaves[leaves >= head]
        gaps = np.diff(leaves)
        per = leaves.size // 4
        assert per >= 3 and leaves.size == 4 * per
        for i, d in enumerate(gf.SPINE_SPACINGS):
            assert (gaps[i * per: (i + 1) * per - 1] == d).all()
            assert (per - 1) * d > f.n_ids // 8
        # everything else: disjoint pairs outside the centre's component
        other = lo != 0
        assert np.unique(np.concatenate([lo[other], hi[other]])).size == 2 * other.sum()
        assert not np.isin(leaves, np.concatenate([lo[other], hi[other]])).any()


def test_loop_constants_match_the_source():
    """The spacings and sizes are built around three constants of sheep_kernels.hip."""
    src = open(os.path.join(ROOT, "sheep_amd", "csrc", "sheep_kernels.hip")).read()
    assert int(re.search(r"constexpr uint32_t KB_SCAN_LIMIT = (\d+);", src).group(1)) == gf.SCAN_LIMIT
    assert int(re.search(r"constexpr uint32_t KM_WIN = (\d+);", src).group(1)) == gf.KM_WIN
    assert int(re.search(r"constexpr int KM_CHUNK = (\d+);", src).group(1)) == gf.KM_CHUNK
