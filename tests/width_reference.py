"""Brute-force bags of a tree decomposition, the reference for the exact tree widths.

The bag of node j, jxn(j), is built as the reference builds it (jnode.h:230-255 newUnion): the
union of the children's bags and of j's own post-order neighbours, without j itself.  The bags
are Python sets unioned up the tree, the smaller into the larger; a set is handed to the parent
once its size has been recorded.  An id outside the sequence is never eliminated and so never
leaves a bag; it is kept as the element ``n + id``.  Plain Python and numpy, no code shared
with the library.
"""
import numpy as np

INVALID = 0xFFFFFFFF
FACT_KEYS = ("width", "roots", "vheight", "eheight", "verts", "edges", "halo", "core", "fill")


def rank_map(seq, n_ids):
    rank = np.full(n_ids, -1, np.int64)
    rank[np.asarray(seq, np.int64)] = np.arange(len(seq))
    return rank


def brute_widths(uv, seq, parent, n_ids=None):
    """width[j] = 1 + |jxn(j)| for every rank j, as a uint64 array."""
    uv = np.asarray(uv, np.int64).reshape(-1, 2)
    n = len(seq)
    if n_ids is None:
        n_ids = int(max(int(np.max(seq)) if n else 0, int(uv.max()) if uv.size else 0)) + 1
    rank = rank_map(seq, n_ids)
    ru, rv = rank[uv[:, 0]], rank[uv[:, 1]]
    pst = [[] for _ in range(n)]  # post-order neighbours: the upper ends of each lower end
    for x, y, a, b in zip(uv[:, 0].tolist(), uv[:, 1].tolist(), ru.tolist(), rv.tolist()):
        if x == y or (a < 0 and b < 0):
            continue
        if a < 0:
            pst[b].append(n + x)
        elif b < 0:
            pst[a].append(n + y)
        elif a < b:
            pst[a].append(b)
        elif b < a:
            pst[b].append(a)
    bags = [None] * n
    width = np.zeros(n, np.uint64)
    par = [int(p) for p in parent]
    for j in range(n):  # heap order: every child comes before its parent
        bag = bags[j]
        own = pst[j]
        if bag is None:
            bag = set(own)
        else:
            bag.update(own)
        bag.discard(j)
        width[j] = 1 + len(bag)
        bags[j] = None
        p = par[j]
        if p != INVALID:
            assert p > j, "forest not in heap order"
            q = bags[p]
            if q is None:
                bags[p] = bag
            elif len(q) < len(bag):
                bag.update(q)
                bags[p] = bag
            else:
                q.update(bag)
    return width


def facts(parent, pst, width):
    """JNodeTable::Facts (jnode.cpp:256-290) over the given widths, as a dict (FACT_KEYS); the
    fill is the reference's size_t sum, modulo 2^64."""
    n = len(parent)
    vh = [0] * n
    eh = [0] * n
    f = dict.fromkeys(FACT_KEYS, 0)
    f["halo"] = f["core"] = INVALID
    fill = 0
    for j in range(n):
        w, s, p = int(width[j]), int(pst[j]), int(parent[j])
        f["verts"] += 1
        f["edges"] += s
        f["width"] = max(f["width"], w)
        fill += w - s - 1
        vh[j] += 1
        eh[j] += s
        if p != INVALID:
            vh[p] = max(vh[p], vh[j])
            eh[p] = max(eh[p], eh[j])
        else:
            f["vheight"] = max(f["vheight"], vh[j])
            f["eheight"] = max(f["eheight"], eh[j])
            f["roots"] += 1
        if f["halo"] == INVALID and w > 3:
            f["halo"] = j
        if f["core"] == INVALID and w >= f["width"]:
            f["core"] = j
    f["fill"] = fill % (1 << 64)
    return f
