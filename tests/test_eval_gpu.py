"""Partition evaluation (sheep_evaluate*) and edge split (sheep_partition_edges*) on the GPU
against the brute force of tests/eval_reference.py, exact: closed-form graphs, ragged record
counts through both key kernels, the part counts around the LDS-histogram switch, pass
planning, empty parts, empty inputs and every refusal include/sheep_amd.h promises.  Every
case runs through the device entry and the host entry."""
import ctypes
import functools

import numpy as np
import pytest

import eval_cases as C
from eval_reference import EVAL_KEYS, brute_evaluate, brute_partition_edges

pytestmark = pytest.mark.gpu
INV = 0xFFFFFFFF
ERANGE, EINVAL = -34, -22


@pytest.fixture(scope="module")
def api(gpu):
    from sheep_amd import api

    return api


def _cuda(a):
    """A numpy array (uint32 / int16) as a cuda tensor of the same type."""
    import torch

    a = np.array(a)  # a copy: the shared cases are read-only
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).cuda().view(torch.uint32)
    return torch.from_numpy(a).cuda()


def _rank(seq, n_ids):
    rank = np.full(n_ids, INV, np.uint32)
    rank[seq] = np.arange(seq.size, dtype=np.uint32)
    return rank


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a.size else None


def dev_evaluate(uv, parts, rank, k):
    from sheep_amd import device

    return device.evaluate(_cuda(uv), _cuda(parts), _cuda(rank), n_parts=k)


def host_evaluate(uv, parts, seq, k):
    from sheep_amd import capi

    out = np.full(11, 7, np.uint64)
    capi.call("sheep_evaluate", _ptr(uv), uv.shape[0], _ptr(parts), parts.size, _ptr(seq),
              seq.size, k, _ptr(out))
    return dict(zip(EVAL_KEYS, (int(x) for x in out)))


def dev_split(uv, parts, rank, k):
    from sheep_amd import device

    out, start = device.partition_edges(_cuda(uv), _cuda(parts), _cuda(rank), k)
    out = out.cpu().numpy().view(np.uint32)
    return [out[int(start[p]):int(start[p + 1])] for p in range(k)], start


@functools.lru_cache(maxsize=None)
def _wanted(make, *args):
    """A case and its brute-force answers, computed once and shared (read only)."""
    uv, parts, seq, k = make(*args)
    for a in (uv, parts, seq):
        a.setflags(write=False)
    return (uv, parts, seq, k), brute_evaluate(uv, parts, seq), brute_partition_edges(uv, parts, seq, k)


def check_evaluate(case, want, oracle=None):
    uv, parts, seq, k = case
    assert dev_evaluate(uv, parts, _rank(seq, parts.size), k) == want
    assert host_evaluate(uv, parts, seq, k) == want
    if oracle is not None:
        assert oracle.evaluate(uv, parts, seq) == want


def assert_split(got, want):
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want]
    assert np.array_equal(np.concatenate(got), np.concatenate(want))


def check_split(api, case, want):
    uv, parts, seq, k = case
    got, start = dev_split(uv, parts, _rank(seq, parts.size), k)
    assert start[0] == 0 and start[k] == sum(w.shape[0] for w in want)
    assert_split(got, want)
    assert_split(api.partition_edges(uv, parts, seq, k), want)


def check_five_records(api):
    """The valid call after a refusal: its numbers are known."""
    case, ev, split = _wanted(C.five_records)
    assert {k: ev[k] for k in C.FIVE} == C.FIVE
    check_evaluate(case, ev)
    check_split(api, case, split)


# ---- closed forms ---------------------------------------------------------------------------

CLOSED = [
    ("path", (C.path,), C.PATH),
    ("path reversed", (C.path, True), C.PATH),
    ("star, centre last", (C.star, False), C.STAR_CENTRE_LAST),
    ("star, centre first", (C.star, True), C.STAR_CENTRE_FIRST),
    ("clique", (C.clique,), C.CLIQUE),
    ("five records", (C.five_records,), C.FIVE),
]


@pytest.mark.parametrize("ep", [None, 10], ids=["one sort", "passes"])
@pytest.mark.parametrize("name,make,numbers", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_forms(oracle, api, options, name, make, numbers, ep):
    """Self-loops as one entry, duplicates, a vertex with self-loops only, sequence positions
    (not id order) deciding down and up: the literal numbers, the brute force and the checker.
    With 1024 entries per pass the path, the stars and the clique also go through the id-range
    passes (the stars' centre, 1000 entries, nearly fills one)."""
    if ep:
        options(eval_pass=ep)
    case, ev, split = _wanted(*make)
    assert {k: ev[k] for k in numbers} == numbers
    check_evaluate(case, ev, oracle)
    if ep is None:
        check_split(api, case, split)
        if name == "five records":
            assert [[tuple(r) for r in g.tolist()] for g in split] == C.FIVE_SPLIT


# ---- record counts ----------------------------------------------------------------------------

RAGGED = [1, 2, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193]
# eval_pass cannot go below 10, so a stream takes the id-range passes only beyond 512 records:
# these counts put a single record, a partial wave and a wave plus one lane in the last
# workgroup of k_ev_keys_range (8191 and 8193 above do so at 33 workgroups)
RAGGED_PASSES = [513, 575, 576, 577, 767, 769]


@pytest.mark.parametrize("m", RAGGED)
def test_ragged_record_counts(oracle, api, m):
    """Partial waves, partial workgroups, one record; 2m and m across the radix tile (8192)."""
    case, ev, split = _wanted(C.multigraph, m)
    check_evaluate(case, ev, oracle)
    check_split(api, case, split)


@pytest.mark.parametrize("m", RAGGED + RAGGED_PASSES)
def test_ragged_record_counts_in_id_range_passes(oracle, options, m):
    """The same streams at 1024 entries per pass: beyond 512 records every key goes through the
    wave-aggregated append of k_ev_keys_range, whose last workgroup is ragged."""
    case, ev, _ = _wanted(C.multigraph, m)
    assert C.llama_degree(case[0], 300).max() < C.PASS_CAP  # else -EINVAL, not a pass
    options(eval_pass=10)
    check_evaluate(case, ev, oracle)


def test_no_records(api):
    """m == 0: eleven zeros, part_start all zero, on both entries (with and without ids)."""
    from sheep_amd import device

    zeros = dict.fromkeys(EVAL_KEYS, 0)
    uv = np.zeros((0, 2), np.uint32)
    parts = np.array([0, 1, -1, 2], np.int16)
    seq = np.array([3, 1, 0], np.uint32)
    assert dev_evaluate(uv, parts, _rank(seq, 4), 3) == zeros
    assert host_evaluate(uv, parts, seq, 3) == zeros
    assert host_evaluate(uv, parts[:0], seq[:0], 3) == zeros
    out, start = device.partition_edges(_cuda(uv), _cuda(parts), _cuda(_rank(seq, 4)), 3)
    assert start.tolist() == [0, 0, 0, 0]
    assert [g.shape[0] for g in api.partition_edges(uv, parts, seq, 3)] == [0, 0, 0]
    assert [g.shape[0] for g in api.partition_edges(uv, parts[:0], seq[:0], 3)] == [0, 0, 0]


# ---- part counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2047, 2048, 2049])
def test_part_counts_around_the_lds_histograms(oracle, api, k):
    """k <= 2048 keeps the balances in LDS, k = 2049 in global memory; k = 1 cuts nothing."""
    case, ev, split = _wanted(C.multigraph, 4096, 2000, k, 12)
    if k == 1:
        assert ev["edges_cut"] == ev["vcom_vol"] == ev["ecv_down"] == 0
    check_evaluate(case, ev, oracle)
    check_split(api, case, split)


def test_largest_part_count_mostly_empty(oracle, api):
    """n_parts = 32768, the documented maximum, with four parts in use: the split fills
    part_start across two gaps of thousands of empty parts."""
    case, ev, split = _wanted(C.sparse_parts)
    assert sum(1 for s in split if s.shape[0]) == 4
    check_evaluate(case, ev, oracle)
    check_split(api, case, split)


def test_split_trailing_empty_parts(api):
    """No record in parts 20001..32767: part_start stays at the total to its end."""
    case, _, split = _wanted(C.trailing_gap)
    assert split[20000].shape[0] and not any(s.shape[0] for s in split[20001:])
    check_split(api, case, split)
    _, start = dev_split(case[0], case[1], _rank(case[2], case[1].size), case[3])
    assert (start[20001:] == start[32768]).all()


def test_all_self_loops(oracle, api):
    """Every vertex is a node, nothing is cut, every part of the split is empty."""
    case, ev, split = _wanted(C.all_self_loops)
    assert ev["edges"] == 500 and ev["nodes"] == np.unique(case[0]).size and ev["edges_cut"] == 0
    check_evaluate(case, ev, oracle)
    check_split(api, case, split)
    _, start = dev_split(case[0], case[1], _rank(case[2], case[1].size), case[3])
    assert not start.any()


# ---- pass planning ----------------------------------------------------------------------------

def test_pass_filled_exactly_and_hub_alone_in_its_pass(oracle, options):
    """run + deg == cap at id 7, then a hub of cap entries whose leaves fall in later passes:
    the passes give what one sort gives."""
    case, ev, _ = _wanted(C.pass_boundary)
    check_evaluate(case, ev, oracle)
    one_sort = dev_evaluate(case[0], case[1], _rank(case[2], case[1].size), case[3])
    options(eval_pass=10)
    check_evaluate(case, ev, oracle)
    assert dev_evaluate(case[0], case[1], _rank(case[2], case[1].size), case[3]) == one_sort


def test_vertex_larger_than_a_pass_is_einval_and_leaves_nothing_behind(options):
    from sheep_amd import capi

    uv, parts, seq, k = C.oversized_hub()
    options(eval_pass=10)
    with pytest.raises(capi.SheepError) as e:
        dev_evaluate(uv, parts, _rank(seq, parts.size), k)
    assert e.value.code == EINVAL
    with pytest.raises(capi.SheepError) as e:
        host_evaluate(uv, parts, seq, k)
    assert e.value.code == EINVAL
    case, ev, _ = _wanted(C.path)
    assert {key: ev[key] for key in C.PATH} == C.PATH
    check_evaluate(case, ev)  # still 1024 entries per pass: two passes


# ---- refusals ---------------------------------------------------------------------------------

def _refused(code, f, *args):
    from sheep_amd import capi

    with pytest.raises(capi.SheepError) as e:
        f(*args)
    assert e.value.code == code


def _triangle():
    """0-1, 1-2, 2-0 and the isolated id 3 (no record)."""
    uv = np.array([[0, 1], [1, 2], [2, 0]], np.uint32)
    return uv, np.array([0, 1, 1, 0], np.int16), np.array([2, 0, 1], np.uint32)


def test_evaluate_refuses_parts_out_of_range(api):
    uv, parts, seq = _triangle()
    want = brute_evaluate(uv, parts, seq)
    for bad in (2, -1, -32768):  # n_parts itself, INVALID_PART, the sign bit alone
        p = parts.copy()
        p[1] = bad
        _refused(ERANGE, dev_evaluate, uv, p, _rank(seq, 4), 2)
        _refused(ERANGE, host_evaluate, uv, p, seq, 2)
        check_five_records(api)
    p = parts.copy()
    p[3] = -1  # no record at id 3: its part is never looked at
    assert dev_evaluate(uv, p, _rank(seq, 4), 2) == want
    assert host_evaluate(uv, p, seq, 2) == want
    assert host_evaluate(uv, p[:3], seq, 2) == want  # nor is a part missing past the array's end


def test_evaluate_refuses_a_vertex_outside_the_sequence(api):
    uv, parts, seq = _triangle()
    _refused(ERANGE, dev_evaluate, uv, parts, _rank(seq[:2], 4), 2)
    _refused(ERANGE, host_evaluate, uv, parts, seq[:2], 2)
    check_five_records(api)


@pytest.mark.parametrize("ep", [None, 10], ids=["one sort", "passes"])
@pytest.mark.parametrize("bad", ["n_ids", "far"])
def test_evaluate_refuses_an_id_out_of_range(api, options, bad, ep):
    """One record of 1000 names an id >= n_ids (the device entry; the host entry sizes n_ids
    itself).  The key kernels run before anyone reads the error word: they must not look the
    id up."""
    if ep:
        options(eval_pass=ep)
    uv, parts, seq, k = C.multigraph(1000)
    uv = uv.copy()
    uv[617, 1] = parts.size if bad == "n_ids" else 0xFFFFFFF0
    _refused(ERANGE, dev_evaluate, uv, parts, _rank(seq, parts.size), k)
    check_five_records(api)


SPLIT_REFUSALS = {
    # parts of ids 0, 1, 2; ids in seq order: the record is (0, 1), id 0 first in seq
    "chosen endpoint without a part": ([-1, 1, 0], [0, 1, 2]),
    "other endpoint without a part": ([0, -1, 0], [0, 1, 2]),
    "chosen endpoint's part >= n_parts": ([2, 1, 0], [0, 1, 2]),
    "other endpoint's part >= n_parts": ([0, 2, 0], [0, 1, 2]),
    "chosen endpoint outside the sequence": ([0, 1, 0], [1, 2]),
    "other endpoint outside the sequence": ([0, 1, 0], [0, 2]),
}


@pytest.mark.parametrize("why", SPLIT_REFUSALS)
def test_split_refuses_what_the_writer_asserts(api, why):
    """Both endpoints of a record need a position and a part, whichever end owns the record."""
    parts, seq = SPLIT_REFUSALS[why]
    parts, seq = np.array(parts, np.int16), np.array(seq, np.uint32)
    uv = np.array([[2, 2], [1, 0], [2, 2]], np.uint32)
    _refused(ERANGE, dev_split, uv, parts, _rank(seq, 3), 2)
    _refused(ERANGE, api.partition_edges, uv, parts, seq, 2)
    check_five_records(api)


def test_split_skips_a_self_loop_on_a_vertex_without_part_or_position(api):
    uv = np.array([[2, 2], [1, 0], [2, 2]], np.uint32)
    parts, seq = np.array([0, 1, -1], np.int16), np.array([1, 0], np.uint32)
    got, start = dev_split(uv, parts, _rank(seq, 3), 2)
    assert start.tolist() == [0, 0, 1] and got[1].tolist() == [[0, 1]]
    got = api.partition_edges(uv, parts, seq, 2)
    assert [g.tolist() for g in got] == [[], [[0, 1]]]


@pytest.mark.parametrize("bad", [(5, 300), (300, 301), (0xFFFFFFF0, 7)],
                         ids=["one end", "both ends, the lower n_ids", "far"])
def test_split_refuses_an_id_out_of_range_after_a_larger_call(api, bad):
    """The earlier, larger call leaves its keys in the scratch that this call sorts in: the
    refused record must still get a key of its own (after every part), not a stale one."""
    case, _, split = _wanted(C.multigraph, 8193)
    check_split(api, case, split)
    uv, parts, seq, k = C.multigraph(257)
    uv = uv.copy()
    uv[100] = bad
    _refused(ERANGE, dev_split, uv, parts, _rank(seq, parts.size), k)
    check_five_records(api)
