"""bench.py's run modes: a plain run times the GPU steps only, --full adds the CPU baselines,
--dump-outputs DIR writes the last timed step's (seq, parent, pst, n_seq) as float64 .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_options_default_to_a_plain_run():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def _fake_out(n_ids, n_seq):
    g = torch.Generator().manual_seed(7)
    mk = lambda: torch.randint(-2**31, 2**31 - 1, (n_ids,), generator=g,
                               dtype=torch.int32).view(torch.uint32)
    return mk(), mk(), mk(), n_seq


def _u32(t, n):
    return t[:n].view(torch.int32).numpy().view(np.uint32)


def test_dump_outputs_whole(tmp_path):
    """Few valid entries: all of them, exact as float64, and nothing past n_seq."""
    out = _fake_out(1000, 777)
    bench.dump_outputs(str(tmp_path / "d"), out)
    assert sorted(os.listdir(tmp_path / "d")) == ["n_seq.npy", "parent.npy", "pst.npy", "seq.npy"]
    for name, t in zip(("seq", "parent", "pst"), out):
        a = np.load(tmp_path / "d" / (name + ".npy"))
        assert a.dtype == np.float64 and a.shape == (777,)
        assert np.array_equal(a.astype(np.uint32), _u32(t, 777))
    assert np.load(tmp_path / "d" / "n_seq.npy").tolist() == [777.0]


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """Many valid entries: the same seeded positions of every array, identical run to run."""
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    out = _fake_out(5000, 4000)
    bench.dump_outputs(str(tmp_path / "a"), out)
    bench.dump_outputs(str(tmp_path / "b"), out)
    pos = np.load(tmp_path / "a" / "sample_index.npy")
    assert pos.shape == (64,) and pos.min() >= 0 and pos.max() < 4000
    assert np.all(np.diff(pos) >= 0)
    for name, t in zip(("seq", "parent", "pst"), out):
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float64
        assert np.array_equal(a.astype(np.uint32), _u32(t, 4000)[pos.astype(np.int64)])
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def _bench(*argv):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scale",
                        "12", "--seed", "1", "--cpu-scale", "10"] + list(argv),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_tree(gpu, oracle, tmp_path):
    """A plain run: the result line without the CPU baselines, and the dumped arrays are the
    checker's tree of the same seeded records."""
    d = tmp_path / "out"
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
    assert rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["unit"] == "edges/s" and rec["higher_is_better"] is True and rec["dtype"] == "u32"
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx((16 << 12) / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert "cpu_baseline" not in rec and "cpu_baseline_ir" not in rec
    uv = oracle.rmat(12, 16, 1)
    seq = oracle.degree_sequence(uv)
    parent, pst = oracle.build_tree(uv, seq)
    assert np.load(d / "n_seq.npy").tolist() == [float(len(seq))]
    for name, want in (("seq", seq), ("parent", parent), ("pst", pst)):
        got = np.load(d / (name + ".npy"))
        assert got.dtype == np.float64
        assert np.array_equal(got, want.astype(np.float64))


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baselines(gpu):
    rec = _bench("--steps", "2", "--warmup", "1", "--full")
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["cores"] == 1
    assert rec["cpu_baseline_ir"]["value"] > 0 and rec["cpu_baseline_ir"]["exact"]
