"""The tree certificate (sheep_verify_tree_dev) and the tree facts (sheep_tree_facts_dev).

Accept: every structured family with its closed-form (or Liu's) tree, the inputs that break a
pass proportional to the height or to one vertex's children (a path of 2^20 + 2 ranks, stars of
2^20 leaves), hep-th and the known-answer graph, and the library's own trees of R-MAT and
power-law streams, of a sub-sequence and of merged halves.  The facts equal the CPU checker's
and the published ones.

Reject: on tiny inputs every mutation's report equals, word for word, a brute-force verifier
written here from the definitions (ancestor sets by walking parent pointers; no code shared
with the library): (A) the higher end of every record is an ancestor of the lower end, (B)
every non-root v has a record (x, parent[v]) with x in v's subtree, pst[r] = the non-loop
records whose lower-rank end is r.  A heap-order violation must come back at once with the
other counts "not computed": nothing may follow parent pointers that can form a cycle."""
import json
import os

import numpy as np
import pytest

import graph_families as gf
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
MAX = 0xFFFFFFFFFFFFFFFF
CLEAN = [0, 0, 0, 0, INV, 0, 0, 0]


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda().view(torch.uint32)


def _rank_map(seq, n_ids):
    rank = np.full(max(n_ids, 1), INV, np.uint32)
    rank[seq] = np.arange(seq.size, dtype=np.uint32)
    return rank


def _verify(uv, rank, n_seq, parent, pst):
    """The 8 report words from host arrays through the device entry point."""
    from sheep_amd import device

    return device.verify_tree(_dev(uv), _dev(rank), n_seq, _dev(parent),
                              None if pst is None else _dev(pst))["words"]


def _facts(parent, pst):
    from sheep_amd import device

    return device.tree_facts(_dev(parent), _dev(pst))


_TREES = {}


def _family_tree(name, size):
    """(family, parent, pst): the closed form where the family has one, else Liu's tree."""
    if (name, size) not in _TREES:
        f = gf.make(name, size)
        parent = f.parent if f.parent is not None else gf.liu_parent(f.uv, f.seq)
        pst = f.pst if f.pst is not None else gf.pst_plain(f.uv, f.seq)
        _TREES[(name, size)] = (f, parent, pst)
    return _TREES[(name, size)]


# ---- accept ----------------------------------------------------------------------------------

BIG = ("path-asc", "star-last", "star-first")
ACCEPT = [(n, "S") for n in gf.NAMES] + [(n, "B") for n in BIG]


@pytest.mark.parametrize("name,size", ACCEPT, ids=["%s-%s" % c for c in ACCEPT])
def test_families_verify_clean_and_facts(gpu, oracle, name, size):
    f, parent, pst = _family_tree(name, size)
    rank = _rank_map(f.seq, f.n_ids)
    assert _verify(f.uv, rank, f.seq.size, parent, pst) == CLEAN
    assert _facts(parent, pst) == oracle.facts(parent, pst)


def test_big_inputs_are_what_they_claim():
    """Height 2^20 + 1 and 2^20 children, in closed form."""
    p = gf.make("path-asc", "B").parent
    assert p.size == (1 << 20) + 2 and np.array_equal(p[:-1], np.arange(1, p.size))
    s = gf.make("star-last", "B").parent
    assert np.count_nonzero(s == s.size - 1) == 1 << 20


def test_unaligned_and_odd_record_ranges(gpu):
    """A record array that starts 8 bytes past a 16-byte boundary, and odd record counts."""
    from sheep_amd import device

    f, parent, pst = _family_tree("grid-rows", "S")
    rank = _dev(_rank_map(f.seq, f.n_ids))
    uv = _dev(np.concatenate([np.zeros((1, 2), np.uint32), f.uv]))  # a self-loop in front
    p, s = _dev(parent), _dev(pst)
    assert uv.data_ptr() % 16 == 0 and uv[1:].data_ptr() % 16 == 8
    for view in (uv, uv[1:], uv[2:], uv[1:-1]):
        got = device.verify_tree(view, rank, f.seq.size, p, s)["words"]
        short = view.shape[0] < f.uv.shape[0]
        assert (got[0], got[1]) == (0, 0)
        assert (got[2:4] == [0, 0]) == (not short), (view.shape, got)


def test_empty_sequence(gpu):
    from sheep_amd import device

    e = _dev(np.zeros(0, np.uint32))
    uv = _dev(np.array([[1, 2]], np.uint32))
    rank = _dev(np.full(3, INV, np.uint32))
    assert device.verify_tree(uv, rank, 0, e, e)["words"] == [0] * 8
    assert device.tree_facts(e, e) == dict(width=0, roots=0, vheight=0, eheight=0, verts=0, edges=0,
                                           halo=INV, core=INV, fill=0)


def test_hep_th(gpu, hep_edges):
    from sheep_amd import api

    pub = json.load(open(os.path.join(GOLDEN, "hep_th_published.json")))["treefaqs"]
    seq, tree = api.graph2tree(hep_edges)
    r = api.verify_tree(hep_edges, seq, tree)
    assert r["valid"] and r["words"] == CLEAN
    assert api.tree_facts(tree) == pub


def test_known_answer(gpu):
    """Self-loops and duplicate records."""
    from sheep_amd import api

    k = json.load(open(os.path.join(GOLDEN, "known_answer.json")))
    uv = np.array(k["records"], np.uint32)
    seq = np.array(k["llama_seq"], np.uint32)
    parent = np.array([INV if p < 0 else p for p in k["parent"]], np.uint32)
    tree = api.JNodeTable(parent, np.array(k["pst"], np.uint32))
    assert api.verify_tree(uv, seq, tree)["words"] == CLEAN
    assert api.tree_facts(tree) == k["treefaqs"]
    assert _verify(uv, _rank_map(seq, 7), 7, parent, None) == CLEAN  # pst not checked


STREAMS = [("rmat16", {}), ("rmat18", {}), ("powerlaw", {}),
           ("rmat16", {"kb_buckets": 64, "kb_rankb": 64}), ("rmat16", {"kb_buckets": 4, "kb_rankb": 8}),
           ("powerlaw", {"kb_buckets": 64, "kb_rankb": 64}), ("powerlaw", {"kb_buckets": 4, "kb_rankb": 8})]


@pytest.mark.parametrize("stream,opts", STREAMS,
                         ids=["%s-%s" % (s, ",".join("%s=%s" % kv for kv in o.items()) or "default")
                              for s, o in STREAMS])
def test_graph2tree_output_verifies(gpu, oracle, options, stream, opts):
    """device.graph2tree's own seq, parent and pst; its facts against the CPU checker's."""
    import torch
    from sheep_amd import device

    options(**opts)
    if stream == "powerlaw":
        n_ids = 100000
        uv = device.powerlaw(n_ids, 1000000, 2.3, 100.0, 3)
    else:
        scale = int(stream[4:])
        n_ids = 1 << scale
        uv = device.rmat(scale, 16, 1)
    seq, parent, pst, n = device.graph2tree(uv, n_ids)
    torch.cuda.synchronize()
    rank = _dev(_rank_map(seq[:n].cpu().numpy().view(np.uint32), n_ids))
    assert device.verify_tree(uv, rank, n, parent[:n], pst[:n])["words"] == CLEAN
    if not opts:
        hp, hs = (t[:n].cpu().numpy().view(np.uint32) for t in (parent, pst))
        assert device.tree_facts(parent[:n], pst[:n]) == oracle.facts(hp, hs)


def test_sub_sequence(gpu, oracle):
    """A seq without every 7th id of the degree sequence: records that leave seq count for pst at
    their end in seq, and are no edges."""
    import torch
    from sheep_amd import device

    uv = oracle.rmat(14, 16, 2)
    seq = oracle.degree_sequence(uv)
    seq = seq[np.arange(seq.size) % 7 != 6]
    rank = _dev(_rank_map(seq, 1 << 14))
    d_uv = _dev(uv)
    parent, pst = device.build_tree(d_uv, rank, seq.size)
    torch.cuda.synchronize()
    assert device.verify_tree(d_uv, rank, seq.size, parent[:seq.size], pst[:seq.size])["words"] == CLEAN


# ---- the brute-force verifier ------------------------------------------------------------------

def brute_force(uv, rank, n_seq, parent, pst):
    """The report by the definitions.  Heap order first; then ancestor sets by walking."""
    n = n_seq
    par = [int(p) for p in parent]
    heap = [v for v in range(n) if not (par[v] == INV or v < par[v] < n)]
    if heap:
        return [len(heap), MAX, MAX, MAX, min(heap), 0, 0, 0]
    anc = np.zeros((n, n), bool)  # anc[v, a]: a is a proper ancestor of v
    for v in range(n):
        a = par[v]
        while a != INV:
            anc[v, a] = True
            a = par[a]
    edges = []
    count = [0] * n
    for x, y in np.asarray(uv, np.int64).tolist():
        if x == y:
            continue
        rx = int(rank[x]) if x < len(rank) else INV
        ry = int(rank[y]) if y < len(rank) else INV
        lo, hi = min(rx, ry), max(rx, ry)
        if lo == INV:
            continue
        count[lo] += 1
        if hi != INV:
            edges.append((lo, hi))
    bad_a = [lo for lo, hi in edges if not anc[lo, hi]]
    good = [(lo, hi) for lo, hi in edges if anc[lo, hi]]
    by_hi = {}
    for lo, hi in good:
        by_hi.setdefault(hi, []).append(lo)
    bad_b = []
    for v in range(n):
        if par[v] == INV:
            continue
        los = by_hi.get(par[v], [])
        if not any(x == v or anc[x, v] for x in los):
            bad_b.append(v)
    bad_p = [] if pst is None else [v for v in range(n) if int(pst[v]) != count[v]]
    first = min(bad_a + bad_b + bad_p, default=INV)
    return [0, len(bad_a), len(bad_b), len(bad_p), first, 0, 0, 0]


TINY = {
    "two-giants": lambda: gf.two_giants(2001),
    "grid": lambda: gf.grid(31, "rows"),
    "cliques": lambda: gf.cliques(50),
    "bintree": lambda: gf.binary_tree(1023, "leaves"),
    "window": lambda: gf.window(2049),
}
_TINY = {}


def _tiny(name):
    if name not in _TINY:
        f = TINY[name]()
        parent = f.parent if f.parent is not None else gf.liu_parent(f.uv, f.seq)
        pst = f.pst if f.pst is not None else gf.pst_plain(f.uv, f.seq)
        rank = _rank_map(f.seq, f.n_ids)
        lo, hi = gf.ranks_of(f.uv, f.seq)
        _TINY[name] = (f, parent, pst, rank, lo, hi)
    return _TINY[name]


def _subtree(parent, v):
    """The ranks of T[v], by walking up from every rank."""
    out = []
    for x in range(v + 1):
        a = x
        while a != INV and a < v:
            a = int(parent[a])
        if a == v:
            out.append(x)
    return out


def _mutate(name, kind):
    """(parent, pst, expected leading words or None) of one mutation of the family's tree."""
    f, parent, pst, rank, lo, hi = _tiny(name)
    n = f.seq.size
    p, s = parent.copy(), pst.copy()
    if kind == "graft-root":
        v = int(np.nonzero(parent == INV)[0][0])
        assert v + 1 < n
        p[v] = v + 1  # any higher rank is in another tree: a root's descendants are below it
        return p, s, (0, 0, 1, 0, v)
    if kind == "graft-sibling":
        for v in range(n):
            q = int(parent[v])
            if q == INV:
                continue
            sub = set(_subtree(parent, v))
            touched = {int(h) for l, h in zip(lo.tolist(), hi.tolist()) if l in sub}
            for w in range(v + 1, q):
                a = w
                while int(parent[a]) != q and int(parent[a]) != INV and int(parent[a]) < q:
                    a = int(parent[a])
                if int(parent[a]) == q and a != v and w not in touched:
                    p[v] = w
                    return p, s, None
        raise AssertionError("no sibling graft in " + name)
    if kind == "lift":
        v = next(v for v in range(n) if parent[v] != INV and parent[int(parent[v])] != INV)
        p[v] = parent[int(parent[v])]
        return p, s, None
    if kind == "detach":
        v = next(v for v in range(n) if parent[v] != INV)
        p[v] = INV
        return p, s, None
    if kind == "pst":
        a, b = np.nonzero(pst > 0)[0][[0, -1]]
        assert a != b
        s[a] += 1
        s[b] -= 1
        return p, s, (0, 0, 0, 2, int(a))
    v = n // 2
    p[v] = {"self": v, "down": v - 1, "n-seq": n}[kind]
    return p, s, (1, MAX, MAX, MAX, v)


HEAP = ["self", "down", "n-seq"]
MUTATIONS = {
    "two-giants": ["graft-sibling", "lift", "detach", "pst"] + HEAP,
    "grid": ["lift", "detach", "pst"] + HEAP,  # row-major: one chain, no siblings to graft under
    "cliques": ["graft-root", "lift", "detach", "pst"] + HEAP,
    "bintree": ["graft-sibling", "lift", "detach", "pst"] + HEAP,
    "window": ["graft-root", "detach", "pst"] + HEAP,
}
REJECT = [(n, k) for n, ks in MUTATIONS.items() for k in ks]


@pytest.mark.parametrize("name", list(TINY))
def test_tiny_trees_are_valid_by_brute_force(gpu, name):
    f, parent, pst, rank, _, _ = _tiny(name)
    assert brute_force(f.uv, rank, f.seq.size, parent, pst) == CLEAN
    assert _verify(f.uv, rank, f.seq.size, parent, pst) == CLEAN


@pytest.mark.parametrize("name,kind", REJECT, ids=["%s-%s" % c for c in REJECT])
def test_mutations_are_rejected_with_exact_counts(gpu, name, kind):
    f, _, _, rank, _, _ = _tiny(name)
    p, s, want = _mutate(name, kind)
    ref = brute_force(f.uv, rank, f.seq.size, p, s)
    assert any(ref[:4]), "the mutation must break the tree"
    if want is not None:
        assert tuple(ref[:5]) == want
    assert _verify(f.uv, rank, f.seq.size, p, s) == ref
    if kind == "graft-sibling":
        assert ref[0] == 0 and ref[1] == 0 and ref[2] >= 1 and ref[3] == 0  # (B) alone
    if kind == "lift":
        assert ref[1] >= 1  # (A)


@pytest.mark.parametrize("scale", [10, 14])
def test_partial_tree(gpu, oracle, scale):
    """The tree of the first half of the records against all of them: rejected; at scale 10 with
    the brute force's counts.  The merge of both halves' trees verifies clean."""
    import torch
    from sheep_amd import device

    uv = oracle.rmat(scale, 16, 5)
    seq = oracle.degree_sequence(uv)
    n = seq.size
    h_rank = _rank_map(seq, 1 << scale)
    rank, d_uv = _dev(h_rank), _dev(uv)
    half = uv.shape[0] // 2
    pa, sa = device.build_tree(d_uv[:half], rank, n)
    pb, sb = device.build_tree(d_uv[half:], rank, n)
    torch.cuda.synchronize()
    got = device.verify_tree(d_uv, rank, n, pa[:n], sa[:n])["words"]
    assert got[0] == 0 and got[1] + got[2] > 0
    if scale == 10:
        hp, hs = (t[:n].cpu().numpy().view(np.uint32) for t in (pa, sa))
        assert got == brute_force(uv, h_rank, n, hp, hs)
    assert device.verify_tree(d_uv[:half], rank, n, pa[:n], sa[:n])["words"] == CLEAN
    device.merge_into(pa, sa, pb, sb, n)
    torch.cuda.synchronize()
    assert device.verify_tree(d_uv, rank, n, pa[:n], sa[:n])["words"] == CLEAN


def test_tree_facts_refuses_a_heap_violation(gpu):
    import errno

    from sheep_amd import capi

    _, parent, pst, _, _, _ = _tiny("cliques")
    p = parent.copy()
    p[7] = 7
    with pytest.raises(capi.SheepError) as e:
        _facts(p, pst)
    assert e.value.code == -errno.EINVAL
