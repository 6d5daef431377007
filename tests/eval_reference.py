"""Brute-force partition evaluation and edge split, the reference for sheep_evaluate* and
sheep_partition_edges*.

Partition::evaluate(graph) and evaluate(graph, seq) (partition.cpp:428-521) and
writePartitionedGraph (partition.cpp:588-630), restated vertex by vertex over adjacency lists
built in record order: a record x != y is the two entries x -> y and y -> x, a record x == x is
the one entry x -> x, duplicates stay.  Python sets and lists, no sorting, no distinct counts,
no histogram tricks.  Plain Python and numpy, no code shared with the library or the checker.
"""
import numpy as np

EVAL_KEYS = ("edges_cut", "vcom_vol", "vertex_bal", "ecv_hash", "hash_bal", "ecv_down",
             "down_bal", "ecv_up", "up_bal", "edges", "nodes")
CORMEN_S = 2654435769  # floor((sqrt(5) - 1) / 2 * 2^32), partition.cpp:420-424
NO_POS = 0xFFFFFFFF  # an id that seq does not list


def _hash(v):
    return (v * CORMEN_S) & 0xFFFFFFFF


def adjacency(uv):
    """{X: [Y, ...]} in record order."""
    adj = {}
    for x, y in np.asarray(uv, np.int64).reshape(-1, 2).tolist():
        adj.setdefault(x, []).append(y)
        if x != y:
            adj.setdefault(y, []).append(x)
    return adj


def positions(seq):
    return {int(v): i for i, v in enumerate(np.asarray(seq, np.int64).tolist())}


def brute_evaluate(uv, parts, seq):
    """The 11 numbers of EVAL_KEYS.  ``parts``: part per vertex id (an id without a record may
    have any value); ``seq``: the ids in sequence order."""
    adj = adjacency(uv)
    pos = positions(seq)
    parts = np.asarray(parts, np.int64).tolist()
    vbal, hbal, dbal, ubal = {}, {}, {}, {}
    cut = vcom = ecvh = ecvd = ecvu = entries = 0

    def bump(d, p):
        d[p] = d.get(p, 0) + 1

    for X in sorted(adj):
        xp = parts[X]
        xpos = pos.get(X, NO_POS)
        bump(vbal, xp)
        vs, hs, ds, us = {xp}, set(), set(), set()
        for Y in adj[X]:
            entries += 1
            yp = parts[Y]
            ypos = pos.get(Y, NO_POS)
            if X < Y and xp != yp:
                cut += 1
            vs.add(yp)
            hp = xp if _hash(X) < _hash(Y) else yp
            hs.add(hp)
            if X < Y:
                bump(hbal, hp)
            ds.add(xp if xpos < ypos else yp)  # a tie is a self-loop: yp (== xp)
            us.add(xp if xpos > ypos else yp)
            if xpos < ypos:
                bump(dbal, xp)
            if xpos > ypos:
                bump(ubal, xp)
        vcom += len(vs) - 1
        ecvh += len(hs) - 1
        ecvd += len(ds) - 1
        ecvu += len(us) - 1
    top = lambda d: max(d.values()) if d else 0  # noqa: E731
    return dict(zip(EVAL_KEYS, (cut, vcom, top(vbal), ecvh, top(hbal), ecvd, top(dbal), ecvu,
                                top(ubal), entries // 2, len(adj))))


def brute_partition_edges(uv, parts, seq, n_parts=None):
    """Per part, the (X, Y) pairs the node-by-node writer emits, as (n, 2) uint32 arrays
    (``n_parts`` lists; by default as many as the largest part needs)."""
    adj = adjacency(uv)
    pos = positions(seq)
    parts = np.asarray(parts, np.int64).tolist()
    if n_parts is None:
        n_parts = max(parts) + 1
    out = [[] for _ in range(n_parts)]
    for X in sorted(adj):
        for Y in adj[X]:
            if Y > X:
                out[parts[X] if pos[X] < pos[Y] else parts[Y]].append((X, Y))
    return [np.array(o, np.uint32).reshape(-1, 2) for o in out]
