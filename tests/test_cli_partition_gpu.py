"""partition_tree -P: the forward partition on the GPU (Partition::on_device ->
sheep_partition_dev) prints what the host partition prints, apart from the timings."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sheep_amd", "bin")
HEP = os.path.join(GOLDEN, "hep-th.dat")
TIMING = re.compile(r"^(Loaded tree in|Partitioning took|Finished in): [0-9.]+ seconds$")


def run(*args):
    return subprocess.run([os.path.join(BIN, args[0])] + list(args[1:]), capture_output=True,
                          text=True)


def lines(out):
    return [x for x in out.splitlines() if not TIMING.match(x)]


def test_partition_tree_P_prints_the_host_lines(gpu, tmp_path):
    tre = str(tmp_path / "hep.tre")
    assert run("graph2tree", HEP, "-o", tre).returncode == 0
    ks = [str(k) for k in range(2, 33)]
    host = run("partition_tree", "-G", "-g", HEP, "-", tre, *ks)
    dev = run("partition_tree", "-P", "-G", "-g", HEP, "-", tre, *ks)
    assert host.returncode == 0, host.stderr
    assert dev.returncode == 0, dev.stderr
    assert len(host.stdout.splitlines()) == len(dev.stdout.splitlines())
    got, want = lines(dev.stdout), lines(host.stdout)
    assert len(want) == 31 * 11  # 2 lines of print(), 9 of evaluate, per k
    assert got == want


def test_partition_tree_P_refuses_other_weights(gpu, tmp_path):
    for flag in ("-x", "-u"):
        r = run("partition_tree", "-P", flag, "-g", HEP, "-", str(tmp_path / "none.tre"), "2")
        assert r.returncode == 1
        assert "-P" in r.stdout and "-x or -u" in r.stdout
