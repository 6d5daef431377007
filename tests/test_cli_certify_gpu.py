"""graph2tree -c certifies its tree on the GPU (JTree::certify -> sheep_verify_tree), and the same
entry point rejects the hep-th tree with one parent corrupted."""
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sheep_amd", "bin")
HEP = os.path.join(GOLDEN, "hep-th.dat")


def test_graph2tree_c_prints_valid(gpu):
    out = subprocess.run([os.path.join(BIN, "graph2tree"), HEP, "-c"], capture_output=True,
                         text=True, check=True)
    assert "Tree is valid." in out.stdout
    assert "ERROR" not in out.stdout and "certificate failed" not in out.stderr


def test_graph2tree_c_on_a_partial_load(gpu, tmp_path):
    """-l 1/2 -s SEQ: the tree of a shard is the elimination tree of that shard's records."""
    from sheep_amd import api

    sq = str(tmp_path / "hep.seq")
    api.write_sequence(api.degree_sequence(api.read_dat(HEP)), sq)
    out = subprocess.run([os.path.join(BIN, "graph2tree"), HEP, "-l", "1/2", "-s", sq, "-c"],
                         capture_output=True, text=True, check=True)
    assert "Tree is valid." in out.stdout


def test_corrupted_hep_th_tree_is_rejected(gpu, hep_edges):
    from sheep_amd import api

    seq, tree = api.graph2tree(hep_edges)
    assert api.verify_tree(hep_edges, seq, tree)["valid"]
    v = int(np.nonzero(tree.parent != api.INVALID)[0][0])
    bad = api.JNodeTable(tree.parent.copy(), tree.pst)
    bad.parent[v] = api.INVALID  # detach a non-root: its witness record now violates (A)
    r = api.verify_tree(hep_edges, seq, bad)
    assert not r["valid"] and r["heap"] == 0 and r["ancestor"] >= 1 and r["first"] <= v
    bad.parent[v] = v  # a self-parent: refused before anything follows parent pointers
    r = api.verify_tree(hep_edges, seq, bad)
    assert r["words"][:5] == [1, api.capi.NOT_COMPUTED, api.capi.NOT_COMPUTED, api.capi.NOT_COMPUTED, v]
