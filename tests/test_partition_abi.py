"""sheep_partition_dev in the C-ABI (no GPU needed): declared, exported, bound, and the refusals
that are answered before any device is touched."""
import ctypes
import errno
import subprocess

import numpy as np

from sheep_amd import api, capi


def test_header_declares_and_library_exports_it():
    L = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "sheep_partition_dev" in capi.header_symbols()
    assert "sheep_partition_dev" in exported
    assert len(L.sheep_partition_dev.argtypes) == 11
    # the host entry it mirrors takes the same arguments but the stream
    assert len(L.sheep_partition.argtypes) == 10
    assert callable(api.partition_dev)


def test_abi_minor_is_at_least_4_major_kept():
    v = capi.lib().sheep_abi_version()
    assert v >> 16 == 1
    assert v & 0xFFFF >= 4


def _args(n_seq=1, ks=(2,), parent=True, pst=True, seq=True, parts=True, with_ks=True):
    """Arguments whose pointers are host memory: a call that went on to the device with them
    would fail otherwise than with the refusal under test."""
    one = (ctypes.c_uint32 * 4)()
    p = ctypes.cast(one, ctypes.c_void_p)
    k = np.asarray(ks, np.int32)
    created = (ctypes.c_uint32 * max(len(ks), 1))()
    return ([p if parent else None, p if pst else None, n_seq, p if seq else None,
             ctypes.c_void_p(k.ctypes.data) if with_ks else None, len(ks), 1.03,
             p if parts else None, 4, created, None], (one, k, created))


def test_null_arguments_and_empty_tree_are_einval_without_a_device():
    L = capi.lib()
    E = -errno.EINVAL
    for missing in ("parent", "pst", "seq", "parts"):
        a, keep = _args(**{missing: False})
        assert L.sheep_partition_dev(*a) == E, missing
        assert b"null" in L.sheep_last_error()
    a, keep = _args(with_ks=False)
    assert L.sheep_partition_dev(*a) == E
    a, keep = _args(n_seq=0)
    assert L.sheep_partition_dev(*a) == E
    assert b"empty" in L.sheep_last_error()
    # created_out is optional: its absence is not what is refused
    a, keep = _args(n_seq=0)
    a[9] = None
    assert L.sheep_partition_dev(*a) == E


def test_k_outside_the_part_range_is_einval_without_a_device():
    L = capi.lib()
    for ks in ((0,), (-1,), (32768,), (2, 3, 0), (2, 1 << 20)):
        a, keep = _args(ks=ks)
        assert L.sheep_partition_dev(*a) == -errno.EINVAL, ks
        assert b"k outside" in L.sheep_last_error()


def test_an_empty_k_list_is_nothing_to_do():
    a, keep = _args(ks=())
    assert capi.lib().sheep_partition_dev(*a) == 0
