"""The partition evaluation's and the edge split's entry points in the C-ABI (no GPU needed):
declared, exported, bound, and their argument checks answer before any device is touched."""
import ctypes
import errno
import subprocess

from sheep_amd import capi

ENTRIES = {"sheep_evaluate_dev": 8, "sheep_evaluate": 8, "sheep_partition_edges_dev": 9,
           "sheep_partition_edges": 9}
E = -errno.EINVAL


def _args():
    buf = (ctypes.c_uint64 * 16)()
    return ctypes.cast(buf, ctypes.c_void_p), buf


def test_header_declares_and_library_exports_them():
    syms = capi.header_symbols()
    L = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", capi.lib_path], capture_output=True,
                         text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s, n_args in ENTRIES.items():
        assert s in syms, s
        assert s in exported, s
        assert len(getattr(L, s).argtypes) == n_args, s


def test_evaluate_null_arguments_are_einval_without_a_device():
    L = capi.lib()
    p, _ = _args()
    # device entry (d_uv, m, d_parts, d_rank, n_ids, n_parts, out, stream)
    assert L.sheep_evaluate_dev(None, 1, p, p, 2, 1, p, None) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_evaluate_dev(p, 1, None, p, 2, 1, p, None) == E
    assert L.sheep_evaluate_dev(p, 1, p, None, 2, 1, p, None) == E
    assert L.sheep_evaluate_dev(p, 1, p, p, 2, 1, None, None) == E
    assert L.sheep_evaluate_dev(None, 0, None, None, 0, 1, None, None) == E  # out, even at m = 0
    # host entry (edges_uv, m, parts, n_parts_vid, seq, n_seq, n_parts, out)
    assert L.sheep_evaluate(None, 1, p, 2, p, 2, 1, p) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_evaluate(p, 1, None, 2, p, 2, 1, p) == E
    assert L.sheep_evaluate(p, 1, p, 2, None, 2, 1, p) == E
    assert L.sheep_evaluate(p, 1, p, 2, p, 2, 1, None) == E


def test_partition_edges_null_arguments_are_einval_without_a_device():
    L = capi.lib()
    p, _ = _args()
    # device entry (d_uv, m, d_parts, d_rank, n_ids, n_parts, d_out, part_start, stream)
    assert L.sheep_partition_edges_dev(None, 1, p, p, 2, 1, p, p, None) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_partition_edges_dev(p, 1, None, p, 2, 1, p, p, None) == E
    assert L.sheep_partition_edges_dev(p, 1, p, None, 2, 1, p, p, None) == E
    assert L.sheep_partition_edges_dev(p, 1, p, p, 2, 1, None, p, None) == E
    assert L.sheep_partition_edges_dev(p, 1, p, p, 2, 1, p, None, None) == E
    assert L.sheep_partition_edges_dev(None, 0, None, None, 0, 1, None, None, None) == E
    # host entry (edges_uv, m, parts, n_parts_vid, seq, n_seq, n_parts, out_uv, part_start)
    assert L.sheep_partition_edges(None, 1, p, 2, p, 2, 1, p, p) == E
    assert b"null" in L.sheep_last_error()
    assert L.sheep_partition_edges(p, 1, None, 2, p, 2, 1, p, p) == E
    assert L.sheep_partition_edges(p, 1, p, 2, None, 2, 1, p, p) == E
    assert L.sheep_partition_edges(p, 1, p, 2, p, 2, 1, None, p) == E
    assert L.sheep_partition_edges(p, 1, p, 2, p, 2, 1, p, None) == E
    assert L.sheep_partition_edges(None, 0, None, 0, None, 0, 1, None, None) == E


def test_part_counts_outside_the_int16_range_are_einval_without_a_device():
    L = capi.lib()
    p, _ = _args()
    for k in (0, 32769):
        assert L.sheep_evaluate_dev(p, 1, p, p, 2, k, p, None) == E
        assert b"n_parts" in L.sheep_last_error()
        assert L.sheep_evaluate(p, 1, p, 2, p, 2, k, p) == E
        assert L.sheep_partition_edges_dev(p, 1, p, p, 2, k, p, p, None) == E
        assert L.sheep_partition_edges(p, 1, p, 2, p, 2, k, p, p) == E
        assert b"n_parts" in L.sheep_last_error()


def test_record_counts_beyond_the_offsets_are_einval_without_a_device():
    """The evaluation sorts one key per adjacency entry, 2m of them (u32 offsets): 2m >= 2^32 is
    refused; the edge split sorts one key per record.  Neither entry reads a record first."""
    L = capi.lib()
    p, _ = _args()
    assert L.sheep_evaluate_dev(p, 1 << 31, p, p, 2, 1, p, None) == E
    assert b"2^31" in L.sheep_last_error()
    assert L.sheep_evaluate(p, 1 << 31, p, 2, p, 2, 1, p) == E
    assert b"2^31" in L.sheep_last_error()
    assert L.sheep_partition_edges_dev(p, 1 << 32, p, p, 2, 1, p, p, None) == E
    assert b"2^32" in L.sheep_last_error()
    assert L.sheep_partition_edges(p, 1 << 32, p, 2, p, 2, 1, p, p) == E
    assert b"2^32" in L.sheep_last_error()


def test_nothing_to_evaluate_on_the_host_entries_needs_no_device():
    """m == 0 and n_seq == 0: the host-pointer calls return zeros before they upload."""
    L = capi.lib()
    out = (ctypes.c_uint64 * 11)(*([7] * 11))
    assert L.sheep_evaluate(None, 0, None, 0, None, 0, 3, out) == 0
    assert list(out) == [0] * 11
    start = (ctypes.c_uint64 * 5)(*([7] * 5))
    assert L.sheep_partition_edges(None, 0, None, 0, None, 0, 3, None, start) == 0
    assert list(start) == [0, 0, 0, 0, 7]  # n_parts + 1 words, no more
