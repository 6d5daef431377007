"""The tree build on structured graph families (tests/graph_families.py), bit-exact.

The bucket loop's anchor pick, giant bitmap, spine and LDS window "only shape the work, never
the result"; the rest of the suite checks that on R-MAT and power-law streams, where one giant
forms once and grows.  Here: inputs without a giant, with two, with a giant that is overtaken
(the anchor moves and the bitmap is cleared after bits were set), marks at the spine's run
limit, all-ones bitmaps, chains of height n - 1 and ranks beyond the map's window — through the
explicit-sequence entry under every loop option set, the degree-ordered pipeline on its radix
and hi-bin paths, the forest merge and the lockstep loop.

Every comparison is bit-exact on seq, parent and pst against the CPU checker and, where the
family has one, the closed form: both are asserted, so that a checker regression cannot hide a
kernel one (tests/test_graph_families.py pins the checker itself on these inputs).  Cases run
S before L before B, so that a structure on which the loop goes quadratic shows as a slow small
case first."""
import numpy as np
import pytest

import graph_families as gf

pytestmark = pytest.mark.gpu

OPTION_SETS = [
    {},
    {"kb_pipe": 0},                          # one stream: rebase, map, apply in turn
    {"kb_rlink": 0},                         # every kept pair through the zipper's lane queue
    {"kb_gsum": 1},                          # the giant summary in the map's LDS
    {"kb_buckets": 64, "kb_rankb": 64},      # narrow buckets: marks and bridges on bucket edges
    {"kb_buckets": 4, "kb_rankb": 8},        # wide buckets: long in-bucket chains
]
# families whose records are spread evenly over the hi ranks: no bucket holds half of them, so
# the default loop is the pipelined one, over more than one bucket
EVEN = ("path-asc", "cliques-block", "cliques-inter", "grid-rows")


def _oid(opts):
    return ",".join("%s=%s" % kv for kv in opts.items()) or "default"


@pytest.fixture(scope="module")
def api(gpu):
    from sheep_amd import api

    return api


_REF = {}


def _ref(key, make):
    """A reference computed once per module, shared read-only."""
    if key not in _REF:
        out = make()
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def _checker_tree(oracle, name, size):
    f = gf.make(name, size)
    return _ref((name, size), lambda: oracle.build_tree(f.uv, f.seq))


def _checker_degree_tree(oracle, name, size, mode):
    f = gf.make(name, size)

    def make():
        seq = oracle.degree_sequence(f.uv, mode)
        return (seq,) + tuple(oracle.build_tree(f.uv, seq))

    return _ref((name, size, "degree", mode), make)


def _to_device(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a).view(np.int32)).cuda().view(torch.uint32)


def _u32(t, n):
    return t[:n].cpu().numpy().view(np.uint32)


def _assert_tree(f, got_parent, got_pst, p, s):
    assert np.array_equal(got_parent, p), "parent != checker"
    assert np.array_equal(got_pst, s), "pst != checker"
    if f.parent is not None:
        assert np.array_equal(got_parent, f.parent), "parent != closed form"
        assert np.array_equal(got_pst, f.pst), "pst != closed form"


# The map's window is left only by a chunk whose his span more than KM_WIN ranks, and a chunk
# lies in one bucket: at L the 8 rank cuts are 37 500 ranks apart, and these option sets add
# fewer record cuts between them than the defaults do.
WIDE = [{"kb_buckets": 4, "kb_rankb": 8}, {"kb_buckets": 4, "kb_rankb": 8, "kb_pipe": 0}]
EXPLICIT = ([(n, "S", o) for n in gf.NAMES for o in OPTION_SETS] +
            [(n, "L", {}) for n in gf.NAMES] +
            [(n, "L", o) for n in ("window", "window-giant", "window-degree") for o in WIDE])


@pytest.mark.parametrize("name,size,opts", EXPLICIT,
                         ids=["%s-%s-%s" % (n, z, _oid(o)) for n, z, o in EXPLICIT])
def test_explicit_sequence(oracle, api, options, name, size, opts):
    """api.build_tree(uv, seq): the radix-sort path, pst from the edge pass; at S under every
    loop option set, at L (groups of ranks share a sort key) under the defaults, and the window
    families at L with buckets wider than the map's window."""
    options(**opts)
    f = gf.make(name, size)
    p, s = _checker_tree(oracle, name, size)
    t = api.build_tree(f.uv, f.seq)
    _assert_tree(f, t.parent, t.pst, p, s)


DEGREE = ([(n, "S", mode, {}) for n in gf.GRAPHS for mode in (0, 1)] +
          [("window-degree", "L", mode, {}) for mode in (0, 1)] +
          [(n, "B", mode, o) for n in gf.GRAPHS for o in ({}, {"bin_direct": 0}) for mode in (0, 1)])


@pytest.mark.parametrize("name,size,mode,opts", DEGREE,
                         ids=["%s-%s-mode%d-%s" % (n, z, m, _oid(o)) for n, z, m, o in DEGREE])
def test_degree_pipeline(oracle, gpu, options, name, size, mode, opts):
    """device.graph2tree in both degree conventions: S (below 2^20 records: the radix sort with
    the degrees at hand, pst from the maps' hi counts) and B (hi bins, filled directly or through
    the scatter), and at L the window family built for the degree order (hi counts of ranks
    beyond the map's window).  seq is the library's own: path, star and cliques are all-ties inputs, so its
    counting sort must keep id order."""
    import torch
    from sheep_amd import capi, device

    options(**opts)
    f = gf.make(name, size)
    seq, p, s = _checker_degree_tree(oracle, name, size, mode)
    s_d, p_d, w_d, n = device.graph2tree(_to_device(f.uv), f.n_ids, mode)
    torch.cuda.synchronize()
    t = dict(capi.last_timings())
    assert n == seq.size
    got_seq, got_p, got_w = _u32(s_d, n), _u32(p_d, n), _u32(w_d, n)
    assert np.array_equal(got_seq, seq), "seq != checker"
    assert np.array_equal(got_seq, gf.degree_order(f.uv, f.n_ids)), "seq != stable degree order"
    assert np.array_equal(got_p, p), "parent != checker"
    assert np.array_equal(got_w, s), "pst != checker"
    if f.parent is not None and np.array_equal(seq, f.seq):  # the degree order is the family's
        assert np.array_equal(got_p, f.parent) and np.array_equal(got_w, f.pst)
    # the phases that ran: pst from the hi counts; below 2^22 records no partitioned gathers,
    # below 2^25 neither the fused front pass nor sampled capacities (so no exact degree pass)
    assert "pst" in t and "tree_insert" in t
    assert "partition" not in t and "front_fused" not in t and "degree_exact" not in t
    if name in EVEN:  # pipelined, over several buckets (one map launch each)
        assert "kb_loop_host" in t and t.get("kb_map#", 0) >= 2


@pytest.mark.parametrize("name", ["path-asc", "star-first", "grid-rows", "two-giants-last"])
def test_forest_merge(oracle, gpu, api, name):
    """The checker's partial trees of 3 record shards (chains of height ~n, not R-MAT's shallow
    forests) through the forest merge's own bucket loop: device.merge_forests of all three is
    the whole tree, and api.merge_trees pairwise equals the checker's merge at every step."""
    import torch
    from sheep_amd import device

    f = gf.make(name, "S")
    n = f.n_ids
    wp, ws = _checker_tree(oracle, name, "S")
    R = f.uv.shape[0]
    parts = _ref((name, "S", "parts"), lambda: sum(
        (oracle.build_tree(f.uv[R * r // 3: R * (r + 1) // 3], f.seq) for r in range(3)), ()))
    parents, psts = parts[0::2], parts[1::2]
    got = device.merge_forests(_to_device(np.stack(parents)), n)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(got, n), wp)
    if f.parent is not None:
        assert np.array_equal(_u32(got, n), f.parent)
    acc = (parents[0], psts[0])
    g = None
    for q, w in zip(parents[1:], psts[1:]):
        g = api.merge_trees(api.JNodeTable(acc[0], acc[1]), api.JNodeTable(q, w))
        acc = oracle.merge(acc[0], acc[1], q, w)
        assert np.array_equal(g.parent, acc[0]) and np.array_equal(g.pst, acc[1])
    assert np.array_equal(g.parent, wp) and np.array_equal(g.pst, ws)


@pytest.mark.parametrize("name", ["path-asc", "cliques-inter", "two-giants-last", "two-giants-mid",
                                  "leapfrog"])
def test_lockstep(oracle, gpu, name):
    """The lockstep loop with P = 3 shards on one device against the checker's serial tree."""
    import torch
    from sheep_amd import device
    from sheep_amd.dist import lockstep_local, shard_bounds

    device.init(0)
    f = gf.make(name, "S")
    seq, p, s = _checker_degree_tree(oracle, name, "S", 0)
    full = _to_device(f.uv)
    m = f.uv.shape[0]
    shards = [full[slice(*shard_bounds(m, r, 3))].contiguous() for r in range(3)]
    s_d, p_d, w_d, n = lockstep_local(shards, f.n_ids, 0)
    torch.cuda.synchronize()
    assert n == seq.size
    assert np.array_equal(_u32(s_d, n), seq)
    assert np.array_equal(_u32(p_d, n), p)
    assert np.array_equal(_u32(w_d, n), s)
    if f.parent is not None and np.array_equal(seq, f.seq):
        assert np.array_equal(_u32(p_d, n), f.parent) and np.array_equal(_u32(w_d, n), f.pst)
