"""sheep_partition_dev (api.partition_dev): forwardPartition of a tree that stays in HBM, bit for
bit what the host's sheep_partition (api.partition) gives, the created counts included.  Every
k list runs in ONE call on each side, so the kids orders that one k's std::sort leaves behind
are the next k's start on both.

Shapes: hep-th over every k the reference published; the structured families (a height of n, one
cut rank with 70 000 equal kids, thousands of roots packed from the last bin down); R-MAT and
power-law trees where a fifth to a half of the ranks are heavy; the refusals; C2 at full size
against the checker's committed digests.

Time: the host side of the star at size B (2^20 equal kids, k = 256) is the reference's loop as
it stands, about 10 s of first-fit passes on the host; every other case takes a few seconds at
most."""
import hashlib
import json
import os

import numpy as np
import pytest

import graph_families as gf
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

INV = 0xFFFFFFFF
FAMILY_KS = [2, 3, 16, 64, 3]
FAMILIES = ("path-asc", "path-rand", "star-last", "bintree-leaves", "cliques-block", "grid-rows",
            "two-giants-last")


def _dev(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda().view(torch.uint32)


def _host(t):
    return t.cpu().numpy()


def _family_tree(oracle, name, size):
    """The family's own parent, pst and seq; the checker's tree where it has no closed form."""
    f = gf.make(name, size)
    if f.parent is not None:
        return f.parent, f.pst, f.seq
    parent, pst = oracle.build_tree(f.uv, f.seq)
    return parent, pst, f.seq


def _both(api, parent, pst, seq, ks, **kw):
    """(device parts as numpy rows, created) and the host's, each from one call."""
    got, got_created = api.partition_dev(_dev(parent), _dev(pst), _dev(seq), ks, **kw)
    want, want_created = api.partition(api.JNodeTable(parent, pst), seq, ks)
    return _host(got), got_created, want, want_created


def _assert_equal(got, got_created, want, want_created, ks):
    assert got.dtype == np.int16 and got.shape[0] == len(ks)
    for i, k in enumerate(ks):
        assert got[i].shape == want[i].shape, k
        assert np.array_equal(got[i], want[i]), (i, k)
    assert got_created == want_created


def test_hep_th_every_published_k(gpu, oracle, hep_edges):
    from sheep_amd import api

    pub = json.load(open(os.path.join(GOLDEN, "hep_th_published.json")))
    seq = oracle.degree_sequence(hep_edges)
    parent, pst = oracle.build_tree(hep_edges, seq)
    ks = list(range(2, 33))
    got, got_created, want, want_created = _both(api, parent, pst, seq, ks)
    _assert_equal(got, got_created, want, want_created, ks)
    for k, p, c in zip(ks, got, got_created):
        rec = next(r for r in pub["partitions"] if r["k"] == k)
        assert c == rec["created"], k
        assert (int((p == 0).sum()), int((p == 1).sum())) == (rec["size0"], rec["size1"]), k


@pytest.mark.parametrize("name", FAMILIES)
def test_families(gpu, oracle, name):
    from sheep_amd import api

    parent, pst, seq = _family_tree(oracle, name, "S")
    _assert_equal(*_both(api, parent, pst, seq, FAMILY_KS), FAMILY_KS)


def test_centre_heavier_than_a_part_is_refused(gpu):
    """star-first: the centre's pst is n - 1, more than total / 2 * balance.  -EINVAL, no hang."""
    import errno

    from sheep_amd import api

    f = gf.make("star-first", "S")
    with pytest.raises(api.SheepError) as e:
        api.partition_dev(_dev(f.parent), _dev(f.pst), _dev(f.seq), [2])
    assert e.value.code == -errno.EINVAL
    with pytest.raises(api.SheepError):
        api.partition(api.JNodeTable(f.parent, f.pst), f.seq, [2])


@pytest.mark.parametrize("name", ("path-asc", "star-last"))
def test_a_million_ranks_under_a_second(gpu, oracle, name):
    """Size B: a chain of 2^20 + 2 ranks (nearly all of them heavy) and a star whose one cut
    rank has 2^20 equal kids.  The device call, host packing included, stays under a second
    between two events on its stream."""
    import torch

    from sheep_amd import api

    parent, pst, seq = _family_tree(oracle, name, "B")
    ks = [16, 256]
    dp, dw, ds = _dev(parent), _dev(pst), _dev(seq)
    api.partition_dev(dp, dw, ds, ks)  # scratch and pinned staging are allocated here
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    got, got_created = api.partition_dev(dp, dw, ds, ks)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1)
    print("%s B: partition_dev ks=%s %.1f ms, phases %s" % (name, ks, ms, gpu.last_timings()))
    want, want_created = api.partition(api.JNodeTable(parent, pst), seq, ks)
    _assert_equal(_host(got), got_created, want, want_created, ks)
    assert ms < 1000.0


def _built_on_device(records, n_ids):
    import torch

    from sheep_amd import device

    seq, parent, pst, n = device.graph2tree(records, n_ids)
    torch.cuda.synchronize()
    return seq, parent, pst, n


@pytest.mark.parametrize("what", ("rmat16", "rmat18", "powerlaw18"))
def test_trees_built_on_the_device(gpu, what):
    """R-MAT and power-law trees as sheep_graph2tree_dev leaves them: a fifth to a half of the
    ranks are heavy, a few hundred are cut."""
    import torch

    from sheep_amd import api, device

    if what == "powerlaw18":
        n_ids = 1 << 18
        uv = device.powerlaw(n_ids, 1 << 22, 2.3, 100.0, 7)
    else:
        scale = int(what[4:])
        n_ids = 1 << scale
        uv = device.rmat(scale, 16, scale)
    seq, parent, pst, n = _built_on_device(uv, n_ids)
    ks = [16, 64, 256]
    got, got_created = api.partition_dev(parent, pst, seq, ks, n_seq=n)
    heavy = [v for name, v in gpu.last_timings() if name == "part_H"]
    print("%s: n_seq %d, |H| per k %s" % (what, n, heavy))
    u32 = lambda t: t[:n].view(torch.int32).cpu().numpy().view(np.uint32)  # noqa: E731
    want, want_created = api.partition(api.JNodeTable(u32(parent), u32(pst)), u32(seq), ks)
    _assert_equal(_host(got), got_created, want, want_created, ks)


def test_one_table_for_every_k(gpu, oracle):
    """ks = [4, 4] on the star: the second k starts from the kids order the first one's
    std::sort left, on the device as on the host; a fresh call may give another row."""
    from sheep_amd import api

    parent, pst, seq = _family_tree(oracle, "star-last", "S")
    got, got_created, want, want_created = _both(api, parent, pst, seq, [4, 4])
    _assert_equal(got, got_created, want, want_created, [4, 4])
    fresh, fresh_created, host_fresh, host_created = _both(api, parent, pst, seq, [4])
    _assert_equal(fresh, fresh_created, host_fresh, host_created, [4])
    assert np.array_equal(fresh[0], got[0])
    # the same bins are filled either way: only which equal kid lands where may differ
    assert np.array_equal(np.bincount(got[1] + 1), np.bincount(fresh[0] + 1))


def test_refusals_and_the_tail_of_a_wider_row(gpu):
    import errno

    from sheep_amd import api

    parent = np.array([2, 2, 4, 4, INV, INV], np.uint32)
    pst = np.array([1, 1, 1, 1, 0, 0], np.uint32)
    seq = np.array([7, 3, 5, 0, 9, 2], np.uint32)
    ks = [1, 2, 3]
    _assert_equal(*_both(api, parent, pst, seq, ks), ks)
    # n_vid above max(seq) + 1: -1 in the tail, the head unchanged
    wide, created = api.partition_dev(_dev(parent), _dev(pst), _dev(seq), ks, n_vid=37)
    want, want_created = api.partition(api.JNodeTable(parent, pst), seq, ks)
    wide = _host(wide)
    assert wide.shape == (3, 37) and created == want_created
    for i in range(3):
        assert np.array_equal(wide[i, :10], want[i])
        assert (wide[i, 10:] == -1).all()
    # a seq id >= n_vid
    with pytest.raises(api.SheepError) as e:
        api.partition_dev(_dev(parent), _dev(pst), _dev(seq), ks, n_vid=9)
    assert e.value.code == -errno.ERANGE
    # a forest not in heap order: a parent below its child, and a self-parent
    for bad in (np.array([2, 2, 1, 4, INV, INV], np.uint32), np.array([0, 2, 4, 4, INV, INV], np.uint32)):
        with pytest.raises(api.SheepError) as e:
            api.partition_dev(_dev(bad), _dev(pst), _dev(seq), ks)
        assert e.value.code == -errno.EINVAL
    # and the call after a refusal is sound
    _assert_equal(*_both(api, parent, pst, seq, ks), ks)


def test_c2_fullsize_digests(gpu):
    """C2 (RMAT-22 seed 22) as test_fullsize_gpu.py builds it, against the checker's digests."""
    from sheep_amd import api, device

    d = json.load(open(os.path.join(GOLDEN, "digests.json")))["c2_rmat22"]
    uv = device.rmat(d["scale"], d["edgefactor"], d["seed"])
    seq, parent, pst, n = _built_on_device(uv, d["n_ids"])
    assert n == d["n_seq"]
    ks = [16, 64, 256]
    parts, created = api.partition_dev(parent, pst, seq, ks, n_seq=n)
    parts = _host(parts)
    for i, k in enumerate(ks):
        want = d["partition"][str(k)]
        h = hashlib.sha256(np.ascontiguousarray(parts[i]).view(np.uint8)).hexdigest()[:16]
        assert (h, created[i]) == (want["parts"], want["created"]), k
    del uv
    gpu.call("sheep_release")
