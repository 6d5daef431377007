#!/usr/bin/env python3
"""Time the forward partition of a tree in HBM (sheep_partition_dev) next to the path it replaces,
in one process.

For each R-MAT scale (edge factor 16, seed = scale: C2 is scale 22, C4 scale 26), graph2tree builds
the tree in HBM; then, for ks = 16 64 256 in one call and after one warm-up call each, device
events on the stream time ``--runs`` calls of

  dev    sheep_partition_dev on the tree where it lies;
  host   what a caller did before: download parent / pst / seq, sheep_partition on the host (the
         loop of lib/partition.h as it stands), upload the parts.

Both must give the same parts, bit for bit; the script stops if they do not.  One JSON line per
scale: the runs, the phase split of the last dev run from sheep_last_timings (the part_heavy /
part_host / part_push entries and the |H|, cuts and kids-fetched counts in k order) and the split
of the host path (download, partition, upload) by wall clock.

    python scripts/partition_bench.py --scales 22 26 --runs 3
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = [16, 64, 256]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", type=int, nargs="+", default=[22, 26])
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()

    import numpy as np
    import torch

    from sheep_amd import api, capi, device

    device.init(0)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return out, t0.elapsed_time(t1)

    for scale in args.scales:
        n_ids = 1 << scale
        m = 16 << scale
        need = 8 * m * 3 + 64 * n_ids * 4
        free, _ = torch.cuda.mem_get_info()
        if need > 0.8 * free:
            print(json.dumps({"scale": scale, "skipped": "needs %d bytes, %d free" % (need, free)}))
            continue
        uv = device.rmat(scale, 16, scale)
        seq, parent, pst, n = device.graph2tree(uv, n_ids)
        torch.cuda.synchronize()
        t = time.perf_counter()
        seq, parent, pst, n = device.graph2tree(uv, n_ids)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t) * 1e3
        del uv
        torch.cuda.empty_cache()
        n_vid = int((seq[:n].view(torch.int32).to(torch.int64) & 0xFFFFFFFF).max().item()) + 1

        def dev():
            return api.partition_dev(parent, pst, seq, KS, n_seq=n, n_vid=n_vid)

        split = {}

        def host():
            t = time.perf_counter()
            u32 = lambda x: x[:n].view(torch.int32).cpu().numpy().view(np.uint32)  # noqa: E731
            hp, hw, hs = u32(parent), u32(pst), u32(seq)
            t1 = time.perf_counter()
            parts, created = api.partition(api.JNodeTable(hp, hw), hs, KS)
            t2 = time.perf_counter()
            up = torch.from_numpy(np.stack(parts)).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            split.update(download_ms=(t1 - t) * 1e3, partition_ms=(t2 - t1) * 1e3,
                         upload_ms=(t3 - t2) * 1e3)
            return up, created

        dev_ms, host_ms = [], []
        for i in range(args.runs + 1):
            (dparts, dcreated), ms = timed(dev)
            if i:
                dev_ms.append(ms)
        timings = capi.last_timings()
        for i in range(args.runs + 1):
            (hparts, hcreated), ms = timed(host)
            if i:
                host_ms.append(ms)
        same = bool(torch.equal(dparts, hparts)) and dcreated == hcreated
        phases = {}
        for name, v in timings:
            phases.setdefault(name, []).append(round(v, 3))
        print(json.dumps({
            "scale": scale, "seed": scale, "n_seq": n, "n_vid": n_vid, "ks": KS,
            "graph2tree_ms": round(build_ms, 2), "identical": same, "created": dcreated,
            "dev_ms": [round(x, 2) for x in dev_ms], "host_path_ms": [round(x, 2) for x in host_ms],
            "dev_phases": phases, "host_path_split_ms": {k: round(v, 2) for k, v in split.items()},
        }), flush=True)
        if not same:
            sys.exit("partition_bench: the device's parts differ from the host's at scale %d" % scale)
        del seq, parent, pst, dparts, hparts
        torch.cuda.empty_cache()
        capi.call("sheep_release")


if __name__ == "__main__":
    main()
