"""Inputs of the partition-evaluation and edge-split tests: graphs whose numbers are known in
closed form, and seeded random multigraphs.  A case is (uv, parts, seq, n_parts): (m, 2)
uint32 records, int16 part per vertex id, uint32 ids in sequence order, the part count."""
import numpy as np


def _case(uv, parts, seq, k):
    return (np.ascontiguousarray(np.asarray(uv, np.uint32).reshape(-1, 2)),
            np.ascontiguousarray(parts, np.int16), np.ascontiguousarray(seq, np.uint32), int(k))


def path(reverse=False):
    """0-1-...-999 in blocks of 64 ids: 15 cut edges, every boundary vertex sees one other part."""
    v = np.arange(1000)
    seq = v[::-1] if reverse else v
    return _case(np.stack([v[:-1], v[1:]], 1), v // 64, seq, 16)


PATH = dict(edges_cut=15, vcom_vol=30, vertex_bal=64, ecv_hash=15, ecv_down=15, down_bal=64,
            ecv_up=15, up_bal=64, edges=999, nodes=1000)


def star(centre_first):
    """Leaves 0..999 in part leaf % 7, centre 1000 in part 0."""
    leaf = np.arange(1000)
    uv = np.stack([leaf, np.full(1000, 1000)], 1)
    parts = np.append(leaf % 7, 0)
    seq = np.append(1000, leaf) if centre_first else np.append(leaf, 1000)
    return _case(uv, parts, seq, 7)


STAR = dict(edges_cut=857, vcom_vol=863, vertex_bal=144, ecv_hash=6, edges=1000, nodes=1001)
STAR_CENTRE_LAST = dict(STAR, ecv_down=6, ecv_up=0, down_bal=143, up_bal=1000)
STAR_CENTRE_FIRST = dict(STAR, ecv_down=0, ecv_up=6, down_bal=1000, up_bal=143)


def clique():
    """K40, part v % 5, identity sequence."""
    i, j = np.triu_indices(40, 1)
    return _case(np.stack([i, j], 1), np.arange(40) % 5, np.arange(40), 5)


CLIQUE = dict(edges_cut=640, vcom_vol=160, ecv_down=150, ecv_up=150, vertex_bal=8)


def five_records():
    """Self-loops (one a vertex's only record), a duplicate in both orientations."""
    return _case([[0, 0], [0, 1], [1, 0], [2, 2], [1, 1]], [0, 1, 1], [2, 0, 1], 2)


FIVE = dict(edges_cut=2, vcom_vol=2, vertex_bal=2, ecv_hash=1, hash_bal=2, ecv_down=1, down_bal=2,
            ecv_up=1, up_bal=2, edges=3, nodes=3)
FIVE_SPLIT = [[(0, 1), (0, 1)], []]


def multigraph(m, n_ids=300, k=5, seed=11):
    """m random records over n_ids ids, about 10 % of them self-loops and 10 % copies of another
    record; random parts in [0, k); seq a random permutation of the ids that occur."""
    rng = np.random.default_rng([seed, m, n_ids, k])
    uv = rng.integers(0, n_ids, (m, 2))
    loops = rng.random(m) < 0.1
    uv[loops, 1] = uv[loops, 0]
    dup = np.nonzero(rng.random(m) < 0.1)[0]
    uv[dup] = uv[rng.integers(0, m, dup.size)]
    parts = rng.integers(0, k, n_ids)
    seq = rng.permutation(np.unique(uv))
    return _case(uv, parts, seq, k)


def sparse_parts():
    """n_parts = 32768 of which only 0, 1, 20000 and 32767 occur: 32764 empty parts, in two
    long gaps, none after the last."""
    uv, _, seq, _ = multigraph(4096, n_ids=2000, k=4, seed=13)
    rng = np.random.default_rng(14)
    parts = np.array([0, 1, 20000, 32767])[rng.integers(0, 4, 2000)]
    return _case(uv, parts, seq, 32768)


def trailing_gap():
    """As sparse_parts without part 32767: the empty run reaches the end of part_start."""
    uv, parts, seq, k = sparse_parts()
    return _case(uv, np.where(parts == 32767, 20000, parts), seq, k)


def all_self_loops():
    rng = np.random.default_rng(15)
    v = rng.integers(0, 300, 1000)
    return _case(np.stack([v, v], 1), rng.integers(0, 5, 300), rng.permutation(np.unique(v)), 5)


PASS_CAP = 1024  # adjacency entries per id-range pass at eval_pass = 10


def pass_boundary():
    """Ids 0..7 with exactly 128 adjacency entries each (100 copies of (2i, 2i+1) and 28
    self-loops on either end): the first pass is full at id 7 (run + deg == cap).  Id 8 is the
    centre of a star with 1024 leaves 9..1032: a pass of its own, its neighbours in the next."""
    rec = []
    for a in range(0, 8, 2):
        rec += [(a, a + 1)] * 100 + [(a, a)] * 28 + [(a + 1, a + 1)] * 28
    rec += [(8, leaf) if leaf % 2 else (leaf, 8) for leaf in range(9, 9 + PASS_CAP)]
    rng = np.random.default_rng(16)
    n = 9 + PASS_CAP
    return _case(rng.permutation(np.array(rec)), rng.integers(0, 5, n), rng.permutation(n), 5)


def oversized_hub():
    """A star with one leaf more than a pass holds."""
    leaf = np.arange(1, PASS_CAP + 2)
    n = PASS_CAP + 2
    return _case(np.stack([np.zeros_like(leaf), leaf], 1), np.arange(n) % 5, np.arange(n), 5)


def llama_degree(uv, n_ids):
    """Adjacency entries per id."""
    deg = np.bincount(uv[:, 0], minlength=n_ids)
    other = uv[uv[:, 0] != uv[:, 1], 1]
    return deg + np.bincount(other, minlength=n_ids)
