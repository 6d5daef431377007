"""SNAP text (.net) parsed on the GPU (sheep_read_net_dev / sheep_records_load_net,
sheep_amd/csrc/sheep_ingest.hip): the record stream equals SNAPReader's on the table of irregular
tokens, across chunk boundaries that fall inside tokens and inside separator runs, past a token
longer than a chunk (the host tail), for -l parts, at the default chunk, through the registered
device copy, and through graph2tree."""
import ctypes
import errno
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sheep_amd", "bin")
HEP = os.path.join(GOLDEN, "hep-th.dat")
WS = b" \t\n\v\f\r"
M = 4294967295

# text -> the records libstdc++'s `>> unsigned` pairs loop yields (tests/cpp/net_layout.cpp derives
# the same from SNAPReader itself)
CASES = [
    (b"1 2\n3 4\n", [(1, 2), (3, 4)]),
    (b"1 2 3", [(1, 2)]),
    (b"1 2\n# c\n3 4\n", [(1, 2)]),
    (b"# h\n1 2\n", []),
    (b"+5 6 7 8", [(5, 6), (7, 8)]),
    (b"1 -0 3 4", [(1, 0), (3, 4)]),
    (b"007 0008 1 2", [(7, 8), (1, 2)]),
    (b"12abc 3 4 5", []),
    (b"1 12abc 3 4", [(1, 12)]),
    (b"4294967295 1 2 3", [(M, 1), (2, 3)]),
    (b"4294967296 1 2 3", []),
    (b"1 99999999999999999999999 2 3", []),
    (b"1\r\n2\r\n\v3\f4", [(1, 2), (3, 4)]),
    (b"1 2 0x10 3", [(1, 2)]),
    (b"1 2 3 4.", [(1, 2), (3, 4)]),
    (b"1 2 - 3 4 5", [(1, 2)]),
    (b"1 2 3 " + b"0" * 31 + b"4 5 6", [(1, 2), (3, 4), (5, 6)]),
    (b"1 2 3 4+5 6", [(1, 2), (3, 4), (5, 6)]),
    (b"1 2 3 4-5 6 7", [(1, 2), (3, 4), (4294967291, 6)]),
    (b"-1 2 3 4", [(M, 2), (3, 4)]),
    (b"1 2 3\0 4 5 6", [(1, 2)]),
]


@pytest.fixture(scope="module")
def api(gpu):
    from sheep_amd import api

    return api


@pytest.fixture(scope="module")
def device(gpu):
    from sheep_amd import device

    return device


def records(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1, 2)


def test_case_table(gpu, device, tmp_path):
    for i, (text, want) in enumerate(CASES):
        path = tmp_path / ("c%d.net" % i)
        path.write_bytes(text)
        if any(M in r for r in want):  # 0xFFFFFFFF is no vertex id: refused, as ingest_dat does
            with pytest.raises(gpu.SheepError) as e:
                device.read_net(path)
            assert e.value.code == -errno.ERANGE, text
            continue
        uv, mx = device.read_net(path)
        want = np.array(want, np.uint32).reshape(-1, 2)
        assert np.array_equal(records(uv), want), text
        assert mx == (int(want.max()) + 1 if want.size else 0), text


def seeded_text(seed, n_records, long_token):
    """(bytes, (n, 2) uint32 records): tokens of 1 to 10 digits, separators of 1 to 3 bytes drawn
    from the six whitespace bytes; long_token: the middle token is zero-padded to 5000 bytes."""
    rng = np.random.default_rng(seed)
    n = 2 * n_records
    digits = rng.integers(1, 11, n)
    lo = np.where(digits == 1, 0, 10 ** (digits - 1))
    hi = np.minimum(10 ** digits, 0xFFFFFFFE)
    vals = (lo + (rng.random(n) * (hi - lo)).astype(np.int64)).astype(np.int64)
    runs = rng.integers(1, 4, n)
    seps = rng.integers(0, 6, (n, 3))
    parts = []
    for t in range(n):
        tok = b"%d" % vals[t]
        if long_token and t == n // 2:
            tok = tok.rjust(5000, b"0")
        parts.append(tok)
        parts.append(bytes(WS[j] for j in seps[t, :runs[t]]))
    return b"".join(parts), vals.astype(np.uint32).reshape(-1, 2)


def raw_boundaries(text, chunk):
    """The byte offsets at which buffers of `chunk` bytes end while the host cuts each after its
    last whitespace byte (net_feed, sheep_amd/csrc/net_layout.h), up to a token that does not
    end within one buffer."""
    out, pos = [], 0
    while pos + chunk < len(text):
        end = pos + chunk
        cut = end
        while cut > pos and text[cut - 1] not in WS:
            cut -= 1
        if cut == pos:
            break
        out.append(end)
        pos = cut
    return out


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    d = tmp_path_factory.mktemp("net")
    text, uv = seeded_text(7, 20000, True)
    (d / "long.net").write_bytes(text)
    plain, uv2 = seeded_text(7, 20000, False)
    assert np.array_equal(uv, uv2)
    (d / "plain.net").write_bytes(plain)
    return d, text, uv


def test_chunk_boundaries_and_the_host_tail(gpu, device, seeded):
    d, text, uv = seeded
    assert 240_000 < len(text) < 400_000
    ends = raw_boundaries(text, 4096)
    assert len(ends) > 20  # the chunks before the 5000-byte token; the host takes the rest
    assert any(text[e - 1] not in WS and text[e] not in WS for e in ends), "none inside a token"
    assert any(text[e - 1] in WS and text[e] in WS for e in ends), "none inside a separator run"
    default = gpu.set_option("net_chunk", 4096)
    try:
        for chunk in (4096, default, 65536):
            gpu.set_option("net_chunk", chunk)
            got, mx = device.read_net(d / "long.net")
            assert np.array_equal(records(got), uv), chunk
            assert mx == int(uv.max()) + 1
    finally:
        gpu.set_option("net_chunk", default)


def test_parts_and_size_query(gpu, device, options, seeded):
    d, _, uv = seeded
    path = d / "plain.net"
    assert len(raw_boundaries(path.read_bytes(), 4096)) > 60
    options(net_chunk=4096)
    m = uv.shape[0]
    whole, mx = device.read_net(path)
    assert np.array_equal(records(whole), uv) and mx == int(uv.max()) + 1
    for part in (1, 2, 3):
        lo, hi = m * (part - 1) // 3, m * part // 3
        n = ctypes.c_uint64(0)
        gpu.call("sheep_read_net_dev", str(path).encode(), part, 3, None, 0, ctypes.byref(n),
                 None, None)
        assert n.value == hi - lo
        got, mx = device.read_net(path, part, 3)
        assert np.array_equal(records(got), uv[lo:hi]), part
        assert mx == int(uv[lo:hi].max()) + 1


@pytest.fixture(scope="module")
def rmat18(oracle, tmp_path_factory):
    uv = oracle.rmat(18, 16, 5)  # 4.2 M records, about 55 MB of text: one default-chunk boundary
    path = tmp_path_factory.mktemp("rmat") / "r18.net"
    path.write_text("\n".join("%d %d" % (a, b) for a, b in uv.tolist()))
    assert 32 << 20 < os.path.getsize(path) < 64 << 20
    return str(path), uv


def test_default_chunk(gpu, device, rmat18):
    path, uv = rmat18
    old = gpu.set_option("net_chunk", 32 << 20)
    try:
        got, mx = device.read_net(path)
    finally:
        gpu.set_option("net_chunk", old)
    assert np.array_equal(records(got), uv) and mx == int(uv.max()) + 1


def test_registered_copy(gpu, oracle, api, rmat18):
    import torch

    path, uv = rmat18
    m = uv.shape[0]
    host = np.zeros((m, 2), np.uint32)
    n = ctypes.c_uint64(0)
    mx = ctypes.c_uint32(0)
    gpu.call("sheep_records_load_net", path.encode(), 0, 0, None, 0, ctypes.byref(n), None)
    assert n.value == m
    gpu.call("sheep_records_load_net", path.encode(), 0, 0, ctypes.c_void_p(host.ctypes.data), m,
             ctypes.byref(n), ctypes.byref(mx))
    try:
        assert n.value == m and mx.value == int(uv.max()) + 1
        assert np.array_equal(host, uv)
        with pytest.raises(gpu.SheepError) as e:  # already registered
            gpu.call("sheep_records_load_net", path.encode(), 0, 0,
                     ctypes.c_void_p(host.ctypes.data), m, ctypes.byref(n), None)
        assert e.value.code == -errno.EBUSY
        seq = api.degree_sequence(host)  # through the registered device copy
        assert np.array_equal(seq, oracle.degree_sequence(uv))
        t = api.build_tree(host, seq)
        p, w = oracle.build_tree(uv, seq)
        assert np.array_equal(t.parent, p) and np.array_equal(t.pst, w)
    finally:
        gpu.call("sheep_records_release", ctypes.c_void_p(host.ctypes.data))
    torch.cuda.synchronize()


def test_cap_too_small_is_erange(gpu, device, seeded):
    import torch

    d, _, uv = seeded
    buf = torch.empty((16, 2), dtype=torch.uint32, device="cuda")
    n = ctypes.c_uint64(0)
    with pytest.raises(gpu.SheepError) as e:
        gpu.call("sheep_read_net_dev", str(d / "plain.net").encode(), 0, 0,
                 ctypes.c_void_p(buf.data_ptr()), 16, ctypes.byref(n), None, None)
    assert e.value.code == -errno.ERANGE and n.value == uv.shape[0]


def test_graph2tree_on_net_equals_dat(gpu, oracle, api, hep_edges, tmp_path):
    """graph2tree on hep-th rewritten as text: the .tre is byte-identical to the .dat's, whole and
    for -l 2/3."""
    net = str(tmp_path / "hep-th.net")
    open(net, "w").write("".join("%d %d\n" % (a, b) for a, b in hep_edges.tolist()))
    sq = str(tmp_path / "hep.seq")
    open(sq, "w").write("".join("%d\n" % x for x in oracle.degree_sequence(hep_edges)))

    def tre(graph, name, *flags):
        out = str(tmp_path / name)
        subprocess.run([os.path.join(BIN, "graph2tree"), graph] + list(flags) + ["-o", out],
                       capture_output=True, text=True, check=True)
        return open(out, "rb").read()

    a = tre(HEP, "dat.tre")
    assert len(a) == 60884 and tre(net, "net.tre") == a
    b = tre(HEP, "dat2.tre", "-l", "2/3", "-s", sq)
    assert tre(net, "net2.tre", "-l", "2/3", "-s", sq) == b
    assert a != b
