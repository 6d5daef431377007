#!/usr/bin/env python3
"""Time the .net ingest on one GPU against the host reader it replaces.

An R-MAT graph (default scale 22: 67 M records, about 1 GB of text) is written once as SNAP text
and as XS1 records and stays in the page cache; then, alternating, RUNS runs each of
  a  SNAPReader into a vector + sheep_records_register  (what EdgeGraph(..., true) did before)
  b  sheep_records_load_net                             (count pass + storing pass on the GPU)
  q  the size query, then b                             (what EdgeGraph(..., true) does now)
  c  sheep_records_load_dat on the same records
  d  the staging loop alone, no kernel launches         (the I/O floor of one pass)
(scripts/net_ingest_bench.cpp).  Gate: b beats a by more than a's own max - min.  How far b sits
above 2 x d (two passes) is reported, not gated.  Prints the runs and one JSON summary line.

  python scripts/net_ingest_bench.py [--scale 22] [--runs 3] [--dir DIR] [--build-only]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "net_ingest_bench")
SRC = os.path.join(ROOT, "scripts", "net_ingest_bench.cpp")


def build():
    lib = os.path.join(ROOT, "sheep_amd", "libsheep_amd.so")
    deps = [SRC, lib, os.path.join(ROOT, "sheep_amd", "csrc", "net_layout.h")]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O2", "-std=c++17",
                    "--offload-arch=gfx950", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "sheep_amd", "lib"),
                    "-I", os.path.join(ROOT, "sheep_amd", "csrc"), "-o", EXE, SRC,
                    "-L", os.path.join(ROOT, "sheep_amd"), "-lsheep_amd",
                    "-Wl,-rpath,$ORIGIN/../sheep_amd"], check=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the two files go (default: a temp dir)")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        p = subprocess.run([EXE, d, str(a.scale), str(a.runs)], capture_output=True, text=True)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr)
    if p.returncode:
        return p.returncode
    rows = [json.loads(line) for line in p.stdout.splitlines()]
    arms = {k: [r["s"] for r in rows if r.get("arm") == k] for k in "abqcd"}
    med = {k: statistics.median(v) for k, v in arms.items()}
    spread_a = max(arms["a"]) - min(arms["a"])
    out = {"scale": a.scale, "runs": a.runs, "median_s": med, "a_max_minus_min_s": spread_a,
           "b_over_2d": med["b"] / (2 * med["d"]), "speedup_b_over_a": med["a"] / med["b"],
           "gate_b_beats_a": med["a"] - med["b"] > spread_a}
    print(json.dumps(out))
    return 0 if out["gate_b_beats_a"] else 1


if __name__ == "__main__":
    sys.exit(main())
