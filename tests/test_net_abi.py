"""The .net ingest's entry points in the C-ABI (no GPU needed): declared, exported, bound; ABI
1.2; their argument errors answer before any device is touched; the option net_chunk."""
import ctypes
import errno
import os
import subprocess

from sheep_amd import capi, device

NEW = ("sheep_read_net_dev", "sheep_records_load_net")


def test_header_declares_and_library_exports_them():
    syms = capi.header_symbols()
    L = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in NEW:
        assert s in syms, s
        assert s in exported, s
        assert getattr(L, s).argtypes is not None, s
    assert callable(device.read_net)


def test_abi_is_1_2_or_later():
    v = capi.lib().sheep_abi_version()
    assert v >> 16 == 1
    assert v & 0xFFFF >= 2


def test_argument_errors_without_a_device(tmp_path):
    L = capi.lib()
    m = ctypes.c_uint64(7)
    path = tmp_path / "g.net"
    path.write_text("1 2\n3 4\n")
    p = str(path).encode()
    missing = str(tmp_path / "none.net").encode()
    for f, extra in ((L.sheep_read_net_dev, (None,)), (L.sheep_records_load_net, ())):
        assert f(None, 0, 0, None, 0, ctypes.byref(m), None, *extra) == -errno.EINVAL
        assert b"null path" in L.sheep_last_error()
        assert f(p, 0, 3, None, 0, ctypes.byref(m), None, *extra) == -errno.EINVAL
        assert b"part" in L.sheep_last_error()
        assert f(p, 4, 3, None, 0, ctypes.byref(m), None, *extra) == -errno.EINVAL
        assert f(missing, 0, 0, None, 0, ctypes.byref(m), None, *extra) == -errno.ENOENT
        assert b"none.net" in L.sheep_last_error()
        # the argument errors come first, whatever else is wrong
        assert f(missing, 9, 3, None, 0, ctypes.byref(m), None, *extra) == -errno.EINVAL
    assert m.value == 7


def test_net_chunk_option_is_kept_in_range():
    old = capi.set_option("net_chunk", 1)
    try:
        if "SHEEP_NET_CHUNK" not in os.environ:
            assert old == 32 << 20  # the default
        assert capi.set_option("net_chunk", 65536 + 7) == 4096
        assert capi.set_option("net_chunk", 1 << 40) == 65536
        assert capi.set_option("net_chunk", -1) == 1 << 30
        assert capi.set_option("net_chunk", old) == 4096
    finally:
        capi.set_option("net_chunk", old)
