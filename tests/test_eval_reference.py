"""The brute-force evaluation and edge split (tests/eval_reference.py) against the CPU checker
and against numbers known in closed form.  No GPU: this pins the reference that
tests/test_eval_gpu.py holds the kernels to."""
import numpy as np
import pytest

import eval_cases as C
from eval_reference import EVAL_KEYS, brute_evaluate, brute_partition_edges


def test_keys_are_the_checkers(oracle):
    assert EVAL_KEYS == oracle.EVAL_KEYS


@pytest.mark.parametrize("k", [2, 16])
def test_brute_equals_checker_on_hep_th(oracle, hep_edges, k):
    seq = oracle.degree_sequence(hep_edges)
    p, s = oracle.build_tree(hep_edges, seq)
    parts = oracle.PartTree(p, s).partition(seq, k)
    assert brute_evaluate(hep_edges, parts, seq) == oracle.evaluate(hep_edges, parts, seq)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_brute_equals_checker_on_rmat_random_parts(oracle, seed):
    uv = oracle.rmat(10, 16, seed)
    rng = np.random.default_rng(seed)
    parts = rng.integers(0, 11, 1 << 10).astype(np.int16)
    seq = rng.permutation(np.unique(uv)).astype(np.uint32)
    assert brute_evaluate(uv, parts, seq) == oracle.evaluate(uv, parts, seq)


@pytest.mark.parametrize("m", [1, 65, 8193])
def test_brute_equals_checker_on_multigraphs(oracle, m):
    uv, parts, seq, _ = C.multigraph(m)
    assert brute_evaluate(uv, parts, seq) == oracle.evaluate(uv, parts, seq)


CLOSED = [
    ("path", lambda: C.path(), C.PATH),
    ("path reversed", lambda: C.path(reverse=True), C.PATH),
    ("star, centre last", lambda: C.star(False), C.STAR_CENTRE_LAST),
    ("star, centre first", lambda: C.star(True), C.STAR_CENTRE_FIRST),
    ("clique", C.clique, C.CLIQUE),
    ("five records", C.five_records, C.FIVE),
]


@pytest.mark.parametrize("name,make,numbers", CLOSED, ids=[c[0] for c in CLOSED])
def test_closed_forms(oracle, name, make, numbers):
    uv, parts, seq, _ = make()
    got = brute_evaluate(uv, parts, seq)
    assert {k: got[k] for k in numbers} == numbers
    assert oracle.evaluate(uv, parts, seq) == got


def test_five_records_split():
    uv, parts, seq, k = C.five_records()
    got = brute_partition_edges(uv, parts, seq, k)
    assert [[tuple(r) for r in g.tolist()] for g in got] == C.FIVE_SPLIT
    assert len(brute_partition_edges(uv, parts, seq)) == 2  # largest part + 1


def test_brute_split_equals_the_sorted_restatement():
    """The node-by-node walk against an independent statement of the writer's order: by part,
    then X, then record."""
    uv, parts, seq, k = C.multigraph(8193)
    pos = np.full(parts.size, -1, np.int64)
    pos[seq] = np.arange(seq.size)
    x, y = uv.min(axis=1).astype(np.int64), uv.max(axis=1).astype(np.int64)
    idx = np.nonzero(x != y)[0]
    owner = np.where(pos[x[idx]] < pos[y[idx]], parts[x[idx]], parts[y[idx]])
    order = np.lexsort((idx, x[idx], owner))
    want = np.stack([x[idx][order], y[idx][order]], 1)
    got = brute_partition_edges(uv, parts, seq, k)
    assert [g.shape[0] for g in got] == np.bincount(owner, minlength=k).tolist()
    assert np.array_equal(np.concatenate(got), want)


def test_generated_inputs_are_what_the_gpu_tests_assume():
    """The pass-planning graphs: 128 entries on each of ids 0..7, 1024 on the hub, one more on
    the oversized hub; every ragged multigraph's largest degree is below a pass."""
    uv, parts, seq, _ = C.pass_boundary()
    deg = C.llama_degree(uv, parts.size)
    assert deg[:8].tolist() == [128] * 8 and deg[8] == C.PASS_CAP and (deg[9:] == 1).all()
    uv, parts, seq, _ = C.oversized_hub()
    assert C.llama_degree(uv, parts.size)[0] == C.PASS_CAP + 1
    for m in (513, 8193):
        uv, parts, seq, _ = C.multigraph(m)
        assert C.llama_degree(uv, 300).max() < C.PASS_CAP
