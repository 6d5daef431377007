"""The exact tree widths' entry points in the C-ABI (no GPU needed): declared, exported, bound,
and their argument checks answer before any device is touched."""
import ctypes
import errno
import subprocess

from sheep_amd import capi

NEW = ("sheep_tree_widths_dev", "sheep_tree_widths")


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
    assert len(L.sheep_tree_widths_dev.argtypes) == 10
    assert len(L.sheep_tree_widths.argtypes) == 8


def test_abi_minor_is_at_least_3_major_kept():
    v = capi.lib().sheep_abi_version()
    assert v >> 16 == 1
    assert v & 0xFFFF >= 3


def test_null_arguments_are_einval_without_a_device():
    L = capi.lib()
    out = (ctypes.c_uint64 * 9)()
    one = (ctypes.c_uint32 * 2)()
    p = ctypes.cast(one, ctypes.c_void_p)
    E = -errno.EINVAL
    # no output words
    assert L.sheep_tree_widths_dev(p, 1, p, 1, 1, p, p, p, None, None) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_tree_widths(p, 1, p, 1, p, p, p, None) == E
    # records, rank map / sequence, parents, pst missing
    assert L.sheep_tree_widths_dev(None, 1, p, 1, 1, p, p, p, out, None) == E
    assert L.sheep_tree_widths_dev(p, 1, None, 1, 1, p, p, p, out, None) == E
    assert L.sheep_tree_widths_dev(p, 1, p, 1, 1, None, p, p, out, None) == E
    assert L.sheep_tree_widths_dev(p, 1, p, 1, 1, p, None, p, out, None) == E
    assert L.sheep_tree_widths(None, 1, p, 1, p, p, p, out) == E
    assert L.sheep_tree_widths(p, 1, None, 1, p, p, p, out) == E
    assert L.sheep_tree_widths(p, 1, p, 1, None, p, p, out) == E
    assert L.sheep_tree_widths(p, 1, p, 1, p, None, p, out) == E
    # more records than u32 offsets reach
    assert L.sheep_tree_widths_dev(p, 1 << 32, p, 1, 1, p, p, p, out, None) == E
    assert L.sheep_tree_widths(p, 1 << 32, p, 1, p, p, p, out) == E


def test_empty_sequence_on_the_host_entry_needs_no_device():
    """n_seq == 0 is valid: zeros, halo and core INVALID (the host-pointer call returns before it
    uploads)."""
    L = capi.lib()
    out = (ctypes.c_uint64 * 9)(*([7] * 9))
    assert L.sheep_tree_widths(None, 0, None, 0, None, None, None, out) == 0
    assert dict(zip(capi.FACT_KEYS, out)) == dict(width=0, roots=0, vheight=0, eheight=0, verts=0,
                                                  edges=0, halo=capi.INVALID, core=capi.INVALID,
                                                  fill=0)
