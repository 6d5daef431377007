"""Structured graph families for the tree build, with their elimination trees in closed form.

The tree loop's anchor pick, giant bitmap, spine and LDS window are tuned on R-MAT and power-law
streams, where one giant forms once and only grows.  These families are the inputs with another
shape: no giant, two giants, a giant that is overtaken, chains of height n - 1, marks at the
spine's run limit, ranks beyond the map's window (DESIGN.md section 4.6 has the table of family
-> rule).

Every generator returns a Family: the records ``uv`` (u32, m x 2, shuffled, endpoints in random
order), an explicit sequence ``seq``, and where a closed form exists the expected ``parent`` and
``pst`` in rank space (rank = position in ``seq``).  ``pst[r]`` counts the non-loop records
whose lower-rank endpoint is r (duplicates count).  ``liu_parent`` and ``pst_plain`` are
references that share no code with the library or the CPU checker.  Plain numpy; no fixture.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

INVALID = 0xFFFFFFFF

# The constants of the tree loop that the sizes and spacings below are built around
# (sheep_kernels.hip; tests/test_graph_families.py reads them back from the source).
SCAN_LIMIT = 64    # launch_kb_apply: bitmap words a spine search looks ahead
KM_WIN = 32768     # k_kb_map: ranks of a chunk's LDS window
KM_CHUNK = 8192    # k_kb_map: records of a chunk
SPINE_SPACINGS = (SCAN_LIMIT * 32 - 32, SCAN_LIMIT * 32, SCAN_LIMIT * 32 + 32, 2 * SCAN_LIMIT * 32)
CLIQUE = 8


class Family(NamedTuple):
    name: str
    uv: np.ndarray                 # (m, 2) u32 ids
    seq: np.ndarray                # (n,) u32 ids, rank = position
    parent: Optional[np.ndarray]   # (n,) u32 ranks, INVALID for roots; None: no closed form
    pst: Optional[np.ndarray]      # (n,) u32
    n_ids: int


def _u32(x):
    a = np.ascontiguousarray(x, dtype=np.uint32)
    a.setflags(write=False)
    return a


def _records(lo, hi, seed):
    """Records (lo[i], hi[i]) in shuffled order with the two endpoints swapped at random."""
    rng = np.random.default_rng(seed)
    uv = np.stack([np.asarray(lo, np.int64), np.asarray(hi, np.int64)], axis=1)
    swap = rng.random(uv.shape[0]) < 0.5
    uv[swap] = uv[swap][:, ::-1]
    return _u32(uv[rng.permutation(uv.shape[0])])


def _family(name, lo, hi, seq, parent, pst, seed):
    seq = _u32(seq)
    return Family(name, _records(lo, hi, seed), seq, None if parent is None else _u32(parent),
                  None if pst is None else _u32(pst), int(seq.size))


# ---- references ---------------------------------------------------------------------------

def ranks_of(uv, seq):
    """The records in rank space as (lo, hi) int64 arrays, self-loops dropped."""
    rank = np.full(int(max(int(seq.max()), int(uv.max()))) + 1, -1, np.int64)
    rank[seq] = np.arange(seq.size)
    a, b = rank[uv[:, 0]], rank[uv[:, 1]]
    assert (a >= 0).all() and (b >= 0).all(), "every endpoint needs a rank"
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    keep = lo != hi
    return lo[keep], hi[keep]


def liu_parent(uv, seq):
    """Liu's elimination tree: the records sorted by higher rank, then for each one the walk up
    the ancestor pointers from its lower end, compressing onto the higher end."""
    lo, hi = ranks_of(uv, seq)
    order = np.argsort(hi, kind="stable")
    los, his = lo[order].tolist(), hi[order].tolist()
    n = int(seq.size)
    parent = [-1] * n
    anc = [-1] * n
    for i, j in zip(los, his):
        r = i
        while True:
            a = anc[r]
            if a == j:
                break
            anc[r] = j
            if a == -1:
                parent[r] = j
                break
            r = a
    out = np.array(parent, np.int64)
    out[out < 0] = INVALID
    return out.astype(np.uint32)


def pst_plain(uv, seq):
    lo, _ = ranks_of(uv, seq)
    return np.bincount(lo, minlength=seq.size).astype(np.uint32)


def degree_order(uv, n_ids):
    """The ids of degree > 0 by degree, ties in id order (none of the families has a self-loop,
    so both degree conventions give this sequence)."""
    deg = np.bincount(uv.reshape(-1).astype(np.int64), minlength=n_ids)
    ids = np.argsort(deg, kind="stable")
    return _u32(ids[deg[ids] > 0])


def component_sizes_below(uv, seq, cut):
    """{root rank: size} of the graph on the records whose higher rank is below ``cut``: a
    plain union-find (path halving, link to the higher rank) in Python lists."""
    lo, hi = ranks_of(uv, seq)
    keep = hi < cut
    uf = list(range(cut))
    for a, b in zip(lo[keep].tolist(), hi[keep].tolist()):
        while uf[a] != a:
            uf[a] = uf[uf[a]]
            a = uf[a]
        while uf[b] != b:
            uf[b] = uf[uf[b]]
            b = uf[b]
        if a != b:
            uf[min(a, b)] = max(a, b)
    roots = np.empty(cut, np.int64)
    for v in range(cut - 1, -1, -1):  # links go upwards: a parent is resolved before its child
        roots[v] = v if uf[v] == v else roots[uf[v]]
    r, c = np.unique(roots, return_counts=True)
    return roots, dict(zip(r.tolist(), c.tolist()))


# ---- families -----------------------------------------------------------------------------

def path(n, order="asc", seed=1):
    """Records (i, i + 1).  asc / desc: one chain of height n - 1, parent[r] = r + 1."""
    i = np.arange(n - 1)
    if order == "asc":
        seq = np.arange(n)
    elif order == "desc":
        seq = np.arange(n)[::-1]
    else:
        seq = np.random.default_rng(seed + 1000).permutation(n)
    closed = order in ("asc", "desc")
    parent = np.append(np.arange(1, n), INVALID) if closed else None
    pst = np.append(np.ones(n - 1, np.int64), 0) if closed else None
    return _family("path-" + order, i, i + 1, seq, parent, pst, seed)


def star(n, centre="last", seed=2):
    """centre last: one hi run of n - 1 records, parent[r] = n - 1.  centre first: every rank of
    every later bucket is a mark of the centre's component, parent[r] = r + 1."""
    leaves = np.arange(n - 1)
    if centre == "last":
        lo, hi = leaves, np.full(n - 1, n - 1)
        parent = np.append(np.full(n - 1, n - 1), INVALID)
        pst = np.append(np.ones(n - 1, np.int64), 0)
    else:
        lo, hi = np.zeros(n - 1, np.int64), leaves + 1
        parent = np.append(np.arange(1, n), INVALID)
        pst = np.zeros(n, np.int64)
        pst[0] = n - 1
    return _family("star-" + centre, lo, hi, np.arange(n), parent, pst, seed)


def sparse_star(n, head=0, seed=3):
    """Centre rank 0; its leaves in four stretches, d ranks apart for d in SPINE_SPACINGS (one
    word inside the spine's look-ahead, exactly at it, one word past it, twice it); every other
    rank joined to its neighbour only.  Each stretch is wider than n / 8 ranks, the widest
    bucket under the suite's option sets, so it crosses bucket boundaries.  The etree: the centre
    and its leaves in rank order are one chain; each pair is an edge.

    head > 0: ranks [1, head) are leaves too.  The centre's component then holds enough of the
    pick's 256 samples to be the anchor, so its leaves are marks and the spine's run cut decides
    which of them are chained and which are queued; with head = 0 the pick falls back to the
    host's anchor, and the leaves are ordinary kept pairs."""
    start = max(head, 1) + 7
    per = (n - start - 1) // sum(SPINE_SPACINGS)
    assert per >= 3, "n too small for four stretches"
    leaves = []
    at = start
    for d in SPINE_SPACINGS:
        for _ in range(per):
            leaves.append(at)
            at += d
    leaves = np.array(leaves)
    assert leaves[-1] < n
    star_hi = np.concatenate([np.arange(1, head), leaves]) if head > 1 else leaves
    is_star = np.zeros(n, bool)
    is_star[0] = True
    is_star[star_hi] = True
    rest = np.nonzero(~is_star)[0]
    rest = rest[: rest.size // 2 * 2].reshape(-1, 2)
    lo = np.concatenate([np.zeros(star_hi.size, np.int64), rest[:, 0]])
    hi = np.concatenate([star_hi, rest[:, 1]])
    parent = np.full(n, INVALID, np.int64)
    chain = np.concatenate([[0], star_hi])
    parent[chain[:-1]] = chain[1:]
    parent[rest[:, 0]] = rest[:, 1]
    pst = np.zeros(n, np.int64)
    pst[0] = star_hi.size
    pst[rest[:, 0]] = 1
    name = "sparse-star" if head <= 1 else "sparse-star-head"
    return _family(name, lo, hi, np.arange(n), parent, pst, seed)


def cliques(k, layout="block", seed=4):
    """k disjoint cliques of CLIQUE vertices: no giant at any bucket."""
    c = CLIQUE
    n = k * c
    i, j = np.triu_indices(c, 1)
    q = np.repeat(np.arange(k), i.size)
    if layout == "block":      # rank r in clique r // c
        lo, hi = q * c + np.tile(i, k), q * c + np.tile(j, k)
        r = np.arange(n)
        parent = np.where(r % c == c - 1, INVALID, r + 1)
        pst = c - 1 - r % c
    else:                      # rank r in clique r % k
        lo, hi = np.tile(i, k) * k + q, np.tile(j, k) * k + q
        r = np.arange(n)
        parent = np.where(r + k < n, r + k, INVALID)
        pst = c - 1 - r // k
    return _family("cliques-" + layout, lo, hi, np.arange(n), parent, pst, seed)


def bipartite(a, b, seed=5):
    """K(a, b), side A first: every B rank has a records whose lo ends fold to one root."""
    n = a + b
    lo = np.repeat(np.arange(a), b)
    hi = a + np.tile(np.arange(b), a)
    r = np.arange(n)
    parent = np.where(r < a, a, r + 1)
    parent[-1] = INVALID
    pst = np.where(r < a, b, 0)
    return _family("bipartite", lo, hi, np.arange(n), parent, pst, seed)


def binary_tree(n, order="leaves", seed=6):
    """Heap numbering: id i > 0 is joined to (i - 1) // 2.  Leaves first (rank = n - 1 - id): the
    etree is the tree itself, height log2 n.  Root first: height n - 1, no closed form here."""
    i = np.arange(1, n)
    if order == "leaves":
        seq = np.arange(n)[::-1]
        r = np.arange(n)
        parent = n - 1 - ((n - 2 - r) // 2)
        parent[-1] = INVALID
        pst = np.append(np.ones(n - 1, np.int64), 0)
    else:
        seq, parent, pst = np.arange(n), None, None
    return _family("bintree-" + order, i, (i - 1) // 2, seq, parent, pst, seed)


def grid(w, order="rows", seed=7):
    """w x w, 4-neighbour, in row-major order or in the degree sequence."""
    ids = np.arange(w * w).reshape(w, w)
    lo = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
    hi = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    f = _family("grid-" + order, lo, hi, np.arange(w * w), None, None, seed)
    return f if order == "rows" else f._replace(seq=degree_order(f.uv, w * w))


def _random_records(rng, ranks, m):
    """m records between random ranks of ``ranks`` (duplicates stay, self-loops are redrawn)."""
    e = ranks[rng.integers(0, ranks.size, size=(m + m // 32 + 64, 2))]
    e = e[e[:, 0] != e[:, 1]][:m]
    assert e.shape[0] == m
    return e[:, 0], e[:, 1]


def two_giants(n, bridge="last", degree=8, seed=8):
    """Two random graphs of the given mean degree on the even and on the odd ranks (the pick's
    samples split evenly between them), joined by one record whose hi end is the last rank or
    rank n // 2."""
    rng = np.random.default_rng(seed + 2000)
    r = np.arange(n)
    parts = [_random_records(rng, r[p::2], (n // 2) * degree // 2) for p in (0, 1)]
    top = n - 1 if bridge == "last" else n // 2
    other = top - 1  # the other parity
    lo = np.concatenate([parts[0][0], parts[1][0], [other]])
    hi = np.concatenate([parts[0][1], parts[1][1], [top]])
    return _family("two-giants-" + bridge, lo, hi, np.arange(n), None, None, seed)


def leapfrog(n, degree=8, seed=9):
    """A random graph A on ranks [0, n/4), another, B, on [n/4, n), and the record (0, n - 1).
    Below rank n/2 the largest component is A's; below 7n/8 it is B's, by far more than the
    pick's hysteresis: the anchor has to move, and the giant bitmap to be cleared, after bits
    were set for A (tests/test_graph_families.py asserts this from a plain union-find)."""
    rng = np.random.default_rng(seed + 3000)
    r = np.arange(n)
    q = n // 4
    a = _random_records(rng, r[:q], q * degree // 2)
    b = _random_records(rng, r[q:], (n - q) * degree // 2)
    lo = np.concatenate([a[0], b[0], [0]])
    hi = np.concatenate([a[1], b[1], [n - 1]])
    return _family("leapfrog", lo, hi, np.arange(n), None, None, seed)


def window(n, seed=10):
    """Records (i, n/2 + 16 i) for i < n/32, the sequence padded with every other id: KM_CHUNK
    consecutive records in hi order span 16 x KM_CHUNK ranks, four windows of the map."""
    i = np.arange(n // 32)
    hi = n // 2 + 16 * i
    parent = np.full(n, INVALID, np.int64)
    parent[i] = hi
    pst = np.zeros(n, np.int64)
    pst[i] = 1
    return _family("window", i, hi, np.arange(n), parent, pst, seed)


def window_giant(n, seed=11):
    """The window family with its lo ends in one component: rank 0 is also joined to every rank
    below n/32.  That component is the anchor's, so the far ends, 16 ranks apart with nothing
    between them, are marks, most of them beyond the window of their chunk (global atomics on
    the bucket's bitmap).  The etree is one chain: the star's, then the far ends in order."""
    h = n // 32
    i = np.arange(h)
    far = n // 2 + 16 * i
    parent = np.full(n, INVALID, np.int64)
    parent[: h - 1] = np.arange(1, h)
    parent[h - 1] = far[0]
    parent[far[:-1]] = far[1:]
    pst = np.zeros(n, np.int64)
    pst[:h] = 1
    pst[0] = h
    return _family("window-giant", np.concatenate([np.zeros(h - 1, np.int64), i]),
                   np.concatenate([np.arange(1, h), far]), np.arange(n), parent, pst, seed)


def window_degree(n, seed=12):
    """The window family for the entry points that order by degree, where every rank has a
    record and the map counts each hi's records for pst: ids below n/32 are joined to the far
    ids n/2 + 16 i, and every other id to one hub, the last id.  All degrees but the hub's are 1,
    so the degree order is the id order, and the 15 ranks between two far ends are lo ends only:
    the far records' his are 16 ranks apart with nothing between them."""
    h = n // 32
    i = np.arange(h)
    far = n // 2 + 16 * i
    pad = np.ones(n, bool)
    pad[i] = pad[far] = pad[n - 1] = False
    pad = np.nonzero(pad)[0]
    parent = np.full(n, INVALID, np.int64)
    parent[i] = far
    parent[pad] = n - 1
    pst = np.zeros(n, np.int64)
    pst[i] = pst[pad] = 1
    return _family("window-degree", np.concatenate([i, pad]),
                   np.concatenate([far, np.full(pad.size, n - 1)]), np.arange(n), parent, pst, seed)


# ---- the cases of the suite ---------------------------------------------------------------
# S: n ~ 70 001 (more than 2 KM_WIN; >= 4000 ranks per bucket at the 16 default buckets, above the
# spine's 2048-rank look-ahead; off every power of two).  L: n ~ 300 001 (n > 2^18: groups of
# ranks share a sort key).  B: m just above 2^20 records, where the degree-ordered pipeline
# groups the records by hi bins.
_CASES = {
    "path-asc": lambda z: path({"S": 70001, "L": 300001, "B": (1 << 20) + 2}[z], "asc"),
    "path-desc": lambda z: path({"S": 70001, "L": 300001, "B": (1 << 20) + 2}[z], "desc"),
    "path-rand": lambda z: path({"S": 70001, "L": 300001, "B": (1 << 20) + 2}[z], "rand"),
    "star-last": lambda z: star({"S": 70001, "L": 300001, "B": (1 << 20) + 1}[z], "last"),
    "star-first": lambda z: star({"S": 70001, "L": 300001, "B": (1 << 20) + 1}[z], "first"),
    "sparse-star": lambda z: sparse_star({"S": 70001, "L": 300001, "B": 2097153}[z]),
    "sparse-star-head": lambda z: sparse_star(*{"S": (70001, 4375), "L": (300001, 18750),
                                                "B": (1973801, 123362)}[z]),
    "cliques-block": lambda z: cliques({"S": 8750, "L": 37501, "B": 37450}[z], "block"),
    "cliques-inter": lambda z: cliques({"S": 8750, "L": 37501, "B": 37450}[z], "inter"),
    "bipartite": lambda z: bipartite(*{"S": (8, 69993), "L": (3, 299998), "B": (300, 3500)}[z]),
    "bintree-leaves": lambda z: binary_tree({"S": 70001, "L": 300001, "B": (1 << 20) + 2}[z],
                                            "leaves"),
    "bintree-root": lambda z: binary_tree({"S": 70001, "L": 300001, "B": (1 << 20) + 2}[z], "root"),
    "grid-rows": lambda z: grid({"S": 265, "L": 548, "B": 725}[z], "rows"),
    "grid-degree": lambda z: grid({"S": 265, "L": 548, "B": 725}[z], "degree"),
    "two-giants-last": lambda z: two_giants(*{"S": (70001, "last", 8), "L": (300001, "last", 8),
                                              "B": (131073, "last", 16)}[z]),
    "two-giants-mid": lambda z: two_giants(*{"S": (70001, "mid", 8), "L": (300001, "mid", 8),
                                             "B": (131073, "mid", 16)}[z]),
    "leapfrog": lambda z: leapfrog(*{"S": (70001, 8), "L": (300001, 8), "B": (131073, 16)}[z]),
    "window": lambda z: window({"S": 70001, "L": 300001}[z]),
    "window-giant": lambda z: window_giant({"S": 70001, "L": 300001}[z]),
    "window-degree": lambda z: window_degree({"S": 70001, "L": 300001}[z]),
}
NAMES = tuple(_CASES)
# one entry per distinct set of records (a family's sequence variants share theirs), for the
# entry points that compute their own sequence; the window families need ranks without records
GRAPHS = ("path-asc", "star-last", "star-first", "sparse-star", "sparse-star-head",
          "cliques-block", "cliques-inter", "bipartite", "bintree-leaves", "grid-rows",
          "two-giants-last", "two-giants-mid", "leapfrog")


@functools.lru_cache(maxsize=None)
def make(name, size):
    """The family ``name`` at size class S, L or B (arrays are read-only and shared)."""
    return _CASES[name](size)
