"""The tree certificate's entry points in the C-ABI (no GPU needed): declared, exported, bound,
and their argument checks answer before any device is touched."""
import ctypes
import errno
import subprocess

from sheep_amd import capi

NEW = ("sheep_verify_tree_dev", "sheep_verify_tree", "sheep_tree_facts_dev")


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


def test_abi_minor_bumped_major_kept():
    v = capi.lib().sheep_abi_version()
    assert v >> 16 == 1
    assert v & 0xFFFF >= 1


def test_null_arguments_are_einval_without_a_device():
    L = capi.lib()
    report = (ctypes.c_uint64 * 8)()
    out = (ctypes.c_uint64 * 9)()
    one = (ctypes.c_uint32 * 2)()
    p = ctypes.cast(one, ctypes.c_void_p)
    E = -errno.EINVAL
    # no report / no output
    assert L.sheep_verify_tree_dev(p, 1, p, 1, 1, p, p, None, None) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_verify_tree(p, 1, p, 1, p, p, None) == E
    assert L.sheep_tree_facts_dev(p, p, 1, None, None) == E
    # records, rank map, sequence, parents missing
    assert L.sheep_verify_tree_dev(None, 1, p, 1, 1, p, p, report, None) == E
    assert L.sheep_verify_tree_dev(p, 1, None, 1, 1, p, p, report, None) == E
    assert L.sheep_verify_tree_dev(p, 1, p, 1, 1, None, p, report, None) == E
    assert L.sheep_verify_tree(None, 1, p, 1, p, p, report) == E
    assert L.sheep_verify_tree(p, 1, None, 1, p, p, report) == E
    assert L.sheep_verify_tree(p, 1, p, 1, None, p, report) == E
    assert L.sheep_tree_facts_dev(None, p, 1, out, None) == E
    assert L.sheep_tree_facts_dev(p, None, 1, out, None) == E
    # more records than u32 offsets reach
    assert L.sheep_verify_tree_dev(p, 1 << 32, p, 1, 1, p, p, report, None) == E
    assert L.sheep_verify_tree(p, 1 << 32, p, 1, p, p, report) == E


def test_empty_sequence_on_the_host_entry_needs_no_device():
    """n_seq == 0 is valid: an all-zero report (the host-pointer call returns before it uploads)."""
    L = capi.lib()
    report = (ctypes.c_uint64 * 8)(*([7] * 8))
    assert L.sheep_verify_tree(None, 0, None, 0, None, None, report) == 0
    assert list(report) == [0] * 8


def test_report_dict():
    d = capi.report_dict([0, 0, 0, 0, capi.INVALID, 0, 0, 0])
    assert d["valid"] and d["first"] == capi.INVALID
    d = capi.report_dict([1] + [capi.NOT_COMPUTED] * 3 + [5, 0, 0, 0])
    assert not d["valid"] and d["heap"] == 1 and d["witness"] == capi.NOT_COMPUTED and d["first"] == 5
