"""The exact tree widths (sheep_tree_widths_dev / sheep_tree_widths, graph2tree -k -e -j).

Every expected value comes from tests/width_reference.py: the bags as Python sets unioned up the
tree, and JNodeTable::Facts over their sizes.  Covered: every structured family at its small
size, closed forms (clique, path, star), hep-th, the sizes at which the range-minimum structure
changes shape (one block, two, a table of one level, of several), a multigraph with self-loops
whose fill wraps, sequences that omit ids (records with one end or both ends outside), forests
of many roots with outside ids that span them, the error returns, the host-pointer call, and the
command line."""
import errno
import json
import os
import re
import subprocess

import numpy as np
import pytest

import graph_families as gf
import width_reference as wr
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
BIN = os.path.join(ROOT, "sheep_amd", "bin")
HEP = os.path.join(GOLDEN, "hep-th.dat")


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda().view(torch.uint32)


def _rank_map(seq, n_ids):
    rank = np.full(max(n_ids, 1), INV, np.uint32)
    rank[seq] = np.arange(seq.size, dtype=np.uint32)
    return rank


def _widths(uv, seq, n_ids, parent, pst, want_widths=True):
    """(numpy widths, facts) from host arrays through the device entry point."""
    from sheep_amd import device

    w, f = device.tree_widths(_dev(uv), _dev(_rank_map(seq, n_ids)), seq.size, _dev(parent),
                              _dev(pst), want_widths)
    return (w.cpu().numpy().view(np.uint32) if want_widths else None), f


def _check(uv, seq, n_ids, parent, pst):
    """Widths and all nine facts against the brute force; returns them."""
    want = wr.brute_widths(uv, seq, parent, n_ids)
    got, facts = _widths(uv, seq, n_ids, parent, pst)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "width[%d] = %d, bags %d (%d differ)" % (bad[0], got[bad[0]], want[bad[0]],
                                                                 bad.size)
    assert facts == wr.facts(parent, pst, want)
    return got, facts


def _tree_of(uv, seq, n_ids):
    """Liu's tree of the records with both ends in seq; pst by the build's rule (a record that
    leaves seq counts at its end in seq)."""
    rank = wr.rank_map(seq, n_ids)
    a, b = rank[uv[:, 0].astype(np.int64)], rank[uv[:, 1].astype(np.int64)]
    both = (a >= 0) & (b >= 0)
    parent = gf.liu_parent(uv[both], seq) if both.any() else np.full(seq.size, INV, np.uint32)
    lo = np.where(a < 0, b, np.where(b < 0, a, np.minimum(a, b)))
    count = (uv[:, 0] != uv[:, 1]) & ((a >= 0) | (b >= 0)) & (a != b)
    pst = np.bincount(lo[count], minlength=seq.size).astype(np.uint32)
    return parent, pst


def _random_graph(n, m, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, size=(m, 2)).astype(np.uint32)


# ---- families and closed forms ----------------------------------------------------------------

@pytest.mark.parametrize("name", gf.NAMES)
def test_families(gpu, name):
    f = gf.make(name, "S")
    parent = f.parent if f.parent is not None else gf.liu_parent(f.uv, f.seq)
    pst = f.pst if f.pst is not None else gf.pst_plain(f.uv, f.seq)
    _check(f.uv, f.seq, f.n_ids, parent, pst)


def test_clique_64(gpu):
    i, j = np.triu_indices(64, 1)
    uv = np.stack([j, i], axis=1).astype(np.uint32)
    r = np.arange(64)
    parent = np.where(r < 63, r + 1, INV).astype(np.uint32)
    pst = (63 - r).astype(np.uint32)
    got, facts = _check(uv, r.astype(np.uint32), 64, parent, pst)
    assert got.tolist() == list(range(64, 0, -1))
    assert facts["fill"] == 0 and facts["width"] == 64 and facts["halo"] == 0


def test_path_4097(gpu):
    f = gf.path(4097, "asc")
    got, facts = _check(f.uv, f.seq, f.n_ids, f.parent, f.pst)
    assert got.tolist() == [2] * 4096 + [1]
    assert facts["fill"] == 0 and facts["halo"] == INV and facts["vheight"] == 4097


def test_star_5000_centre_last(gpu):
    """The centre's run of lower ends is 4999 long: 4998 pairs whose LCA is the centre."""
    f = gf.star(5000, "last")
    got, facts = _check(f.uv, f.seq, f.n_ids, f.parent, f.pst)
    assert got.tolist() == [2] * 4999 + [1]
    assert facts["fill"] == 0 and facts["width"] == 2


_HEP = {}


def _hep(hep_edges):
    """hep-th: the library's sequence and tree, and the brute force's widths and facts (once)."""
    if not _HEP:
        from sheep_amd import api

        seq, tree = api.graph2tree(hep_edges)
        want = wr.brute_widths(hep_edges, seq, tree.parent)
        _HEP.update(seq=seq, tree=tree, want=want, facts=wr.facts(tree.parent, tree.pst, want))
    return _HEP


def test_hep_th(gpu, hep_edges):
    from sheep_amd import api

    h = _hep(hep_edges)
    got, facts = api.tree_widths(hep_edges, h["seq"], h["tree"])
    assert np.array_equal(got, h["want"])
    assert facts == h["facts"]
    assert facts["width"] > api.tree_facts(h["tree"])["width"]  # not 1 + max pst_weight
    assert facts["fill"] > 0


# ---- the range-minimum structure's shapes -------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049])
def test_random_graphs_at_block_and_table_boundaries(gpu, n):
    """2n tour positions: inside one 64-position block (n <= 32), two blocks, and block counts
    just below, at and above a power of two (64 blocks at n = 2048)."""
    uv = _random_graph(n, 4 * n, 100 + n)
    seq = np.random.default_rng(n).permutation(n).astype(np.uint32)
    parent, pst = _tree_of(uv, seq, n)
    _check(uv, seq, n, parent, pst)


def test_path_with_chords_spans_every_table_level(gpu):
    """A 5000-path with 200 random chords: 157 blocks, chords of every length."""
    rng = np.random.default_rng(7)
    i = np.arange(4999)
    chords = rng.integers(0, 5000, size=(200, 2))
    uv = np.concatenate([np.stack([i, i + 1], axis=1), chords]).astype(np.uint32)
    seq = np.arange(5000, dtype=np.uint32)
    parent, pst = _tree_of(uv, seq, 5000)
    spans = np.abs(chords[:, 0] - chords[:, 1])
    assert spans.max() > 4096 and (spans < 64).any()
    _check(uv, seq, 5000, parent, pst)


def test_unaligned_and_odd_record_ranges(gpu):
    """A record array that starts 8 bytes past a 16-byte boundary, and odd record counts."""
    from sheep_amd import device

    n = 700
    uv = _random_graph(n, 2801, 11)
    seq = np.arange(n, dtype=np.uint32)
    d_uv = _dev(np.concatenate([np.zeros((1, 2), np.uint32), uv]))  # a self-loop in front
    assert d_uv.data_ptr() % 16 == 0 and d_uv[1:].data_ptr() % 16 == 8
    rank = _dev(_rank_map(seq, n))
    for view, h in ((d_uv, uv), (d_uv[1:], uv), (d_uv[2:], uv[1:]), (d_uv[1:-1], uv[:-1])):
        parent, pst = _tree_of(h, seq, n)
        w, facts = device.tree_widths(view, rank, n, _dev(parent), _dev(pst))
        want = wr.brute_widths(h, seq, parent, n)
        assert np.array_equal(w.cpu().numpy().view(np.uint32), want)
        assert facts == wr.facts(parent, pst, want)


# ---- multigraphs, ends outside the sequence, forests --------------------------------------------

def test_known_answer_fill_wraps(gpu):
    """Self-loops and duplicate records: pst counts duplicates, a bag does not, so the fill is the
    reference's wrapped size_t sum."""
    from sheep_amd import api

    k = json.load(open(os.path.join(GOLDEN, "known_answer.json")))
    uv = np.array(k["records"], np.uint32)
    seq = np.array(k["llama_seq"], np.uint32)
    parent = np.array([INV if p < 0 else p for p in k["parent"]], np.uint32)
    pst = np.array(k["pst"], np.uint32)
    want = wr.brute_widths(uv, seq, parent)
    ref = wr.facts(parent, pst, want)
    assert int(np.sum(want.astype(np.int64) - 1 - pst)) < 0 and ref["fill"] >= 1 << 63
    got, facts = api.tree_widths(uv, seq, api.JNodeTable(parent, pst))
    assert np.array_equal(got, want)
    assert facts == ref


def test_sequence_that_omits_ids(gpu):
    """Every 5th id is outside the sequence: its records keep it in the bags up to the root."""
    n_ids = 3000
    uv = _random_graph(n_ids, 4 * n_ids, 21)
    ids = np.random.default_rng(22).permutation(n_ids)
    seq = ids[ids % 5 != 4].astype(np.uint32)
    out = uv % 5 == 4
    assert (out.sum(axis=1) == 1).any() and (out.sum(axis=1) == 2).any()
    parent, pst = _tree_of(uv, seq, n_ids)
    got, facts = _check(uv, seq, n_ids, parent, pst)
    assert facts["width"] > 1 + int(pst.max()) or facts["fill"] > 0


def test_forest_of_many_roots_with_outside_ids_across_them(gpu):
    """Sparse records: hundreds of trees and isolated ranks; an outside id's lower ends lie in
    several trees, so the minimum between two of them is the virtual root."""
    n_ids = 4000
    uv = _random_graph(n_ids, 1500, 31)
    hub = np.stack([np.full(300, 3999), np.random.default_rng(32).integers(0, 3990, 300)], axis=1)
    uv = np.concatenate([uv, hub.astype(np.uint32)])
    seq = np.arange(3990, dtype=np.uint32)  # ids 3990 .. 3999 are outside
    parent, pst = _tree_of(uv, seq, n_ids)
    assert np.count_nonzero(parent == INV) > 500
    _check(uv, seq, n_ids, parent, pst)


# ---- the calls ----------------------------------------------------------------------------------

def test_host_and_device_calls_agree_and_widths_are_optional(gpu):
    from sheep_amd import api, capi

    n = 2049
    uv = _random_graph(n, 4 * n, 41)
    seq = np.random.default_rng(42).permutation(n).astype(np.uint32)
    parent, pst = _tree_of(uv, seq, n)
    dw, dfacts = _widths(uv, seq, n, parent, pst)
    hw, hfacts = api.tree_widths(uv, seq, api.JNodeTable(parent, pst))
    assert np.array_equal(dw, hw) and dfacts == hfacts
    none, nfacts = _widths(uv, seq, n, parent, pst, want_widths=False)
    assert none is None and nfacts == dfacts
    names = [k for k, _ in capi.last_timings()]
    assert "tw_sort" in names and "tw_weights" in names and "vf_tour" in names


def test_empty_sequence(gpu):
    from sheep_amd import device

    e = _dev(np.zeros(0, np.uint32))
    uv = _dev(np.array([[1, 2]], np.uint32))
    rank = _dev(np.full(3, INV, np.uint32))
    w, facts = device.tree_widths(uv, rank, 0, e, e)
    assert w.numel() == 0
    assert facts == dict(width=0, roots=0, vheight=0, eheight=0, verts=0, edges=0, halo=INV,
                         core=INV, fill=0)


def _ancestor_violations(uv, seq, n_ids, parent):
    rank = wr.rank_map(seq, n_ids)
    bad = 0
    for x, y in np.asarray(uv, np.int64).tolist():
        lo, hi = sorted((int(rank[x]), int(rank[y])))
        if lo < 0 or lo == hi:
            continue
        a = lo
        while a != INV and a < hi:
            a = int(parent[a])
        bad += a != hi
    return bad


def test_a_tree_that_is_not_the_records_is_refused(gpu):
    """One parent re-pointed to its grandparent: the records below it no longer have their upper
    end as an ancestor, and the call names how many."""
    from sheep_amd import capi

    f = gf.grid(31, "rows")
    parent = gf.liu_parent(f.uv, f.seq)
    pst = gf.pst_plain(f.uv, f.seq)
    v = next(v for v in range(f.seq.size)
             if parent[v] != INV and parent[int(parent[v])] != INV)
    p = parent.copy()
    p[v] = parent[int(parent[v])]
    bad = _ancestor_violations(f.uv, f.seq, f.n_ids, p)
    assert bad >= 1 and _ancestor_violations(f.uv, f.seq, f.n_ids, parent) == 0
    with pytest.raises(capi.SheepError) as e:
        _widths(f.uv, f.seq, f.n_ids, p, pst)
    assert e.value.code == -errno.EINVAL
    assert "%d records" % bad in str(e.value)
    _check(f.uv, f.seq, f.n_ids, parent, pst)  # the library is fine afterwards


def test_heap_violation_and_id_out_of_range(gpu):
    from sheep_amd import capi

    f = gf.cliques(50)
    p = f.parent.copy()
    p[7] = 7
    with pytest.raises(capi.SheepError) as e:
        _widths(f.uv, f.seq, f.n_ids, p, f.pst)
    assert e.value.code == -errno.EINVAL
    uv = np.concatenate([f.uv, np.array([[f.n_ids + 5, 3]], np.uint32)])
    with pytest.raises(capi.SheepError) as e:
        _widths(uv, f.seq, f.n_ids, f.parent, f.pst)
    assert e.value.code == -errno.ERANGE
    _check(f.uv, f.seq, f.n_ids, f.parent, f.pst)


# ---- the command line ---------------------------------------------------------------------------

def test_graph2tree_kej_prints_the_true_treefaqs_and_widths(gpu, hep_edges):
    h = _hep(hep_edges)
    out = subprocess.run([os.path.join(BIN, "graph2tree"), HEP, "-k", "-e", "-j", "-f", "-t"],
                         capture_output=True, text=True, check=True).stdout
    faqs = {k: int(v) for k, v in re.findall(r"(width|roots|vheight|eheight|verts|edges|halo|core|fill):(\d+)",
                                             out)}
    assert faqs == h["facts"]
    rows = re.findall(r"^\s*(\d+):(\d+)\s+(\d+):w\s*\d+:pre\s*(\d+):pst", out, re.M)
    assert len(rows) == h["seq"].size
    assert [int(r[2]) for r in rows] == h["want"].tolist()
    assert [int(r[1]) for r in rows] == h["seq"].tolist()


@pytest.mark.parametrize("flags", [["-j"], ["-k", "-e"], ["-k", "-e", "-j", "-w", "5"],
                                   ["-k", "-e", "-j", "-x"]])
def test_graph2tree_still_refuses_the_rest(flags):
    out = subprocess.run([os.path.join(BIN, "graph2tree"), HEP] + flags, capture_output=True,
                         text=True)
    assert out.returncode == 1 and "ERROR" in out.stdout
