#!/usr/bin/env python3
"""Time the exact tree widths (sheep_tree_widths_dev) next to the tree build, in one process.

For each R-MAT scale (edge factor 16, seed 1): the records are generated in HBM, graph2tree builds
the tree (timed from the second call on, like the widths: the first call of either allocates its
scratch), then sheep_tree_widths_dev runs ``--runs`` times.  One JSON line per scale: the wall
times, the phase times of the last run from sheep_last_timings, the scratch the call holds (from
its sizes) and the TREEFAQS it returned.

    python scripts/tree_widths_bench.py --scales 22 26 --runs 3
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scratch_bytes(n, m):
    """Bytes of device scratch of one call over n ranks and m records."""
    n2 = 2 * n
    nb = (n2 + 63) // 64
    levels = int(math.log2(nb)) + 1 if nb else 0
    return {
        "keys": 2 * 8 * m,
        "tour": 8 * n * 2 + 4 * (n + 1) * 2 + 16 * n * 2 + 8 * n + 4 * n,  # VfTour (sheep_internal.h)
        "depth_pre_suf_lca": n2 * (4 + 16 + 4),
        "table": nb * 8 * levels,
        "has_lower": n,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[22, 26])
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import torch

    from sheep_amd import capi, device

    device.init(0)
    for scale in args.scales:
        n_ids = 1 << scale
        m = 16 << scale
        need = 8 * m * 3 + 64 * n_ids * 4
        free, _ = torch.cuda.mem_get_info()
        if need > 0.8 * free:
            print(json.dumps({"scale": scale, "skipped": "needs %d bytes, %d free" % (need, free)}))
            continue
        uv = device.rmat(scale, 16, 1)
        build_ms = []
        for _ in range(args.runs + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            seq, parent, pst, n = device.graph2tree(uv, n_ids)
            torch.cuda.synchronize()
            build_ms.append((time.perf_counter() - t) * 1e3)
        rank = torch.full((n_ids,), -1, dtype=torch.int32, device="cuda")
        rank[seq.view(torch.int32)[:n].to(torch.int64)] = torch.arange(n, dtype=torch.int32,
                                                                       device="cuda")
        rank = rank.view(torch.uint32)
        width_ms = []
        for _ in range(args.runs + 1):
            torch.cuda.synchronize()
            t = time.perf_counter()
            width, facts = device.tree_widths(uv, rank, n, parent[:n], pst[:n])
            width_ms.append((time.perf_counter() - t) * 1e3)  # the call synchronises
        phases = {k: round(v, 3) for k, v in capi.last_timings()}
        sb = scratch_bytes(n, uv.shape[0])
        print(json.dumps({
            "scale": scale, "n_seq": n, "records": uv.shape[0],
            "graph2tree_ms": [round(x, 2) for x in build_ms[1:]],
            "tree_widths_ms": [round(x, 2) for x in width_ms[1:]],
            "tree_widths_first_call_ms": round(width_ms[0], 2),
            "phases_ms": phases, "scratch_bytes": sb, "scratch_total": sum(sb.values()),
            "facts": facts,
        }), flush=True)
        del uv, seq, parent, pst, rank, width
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
