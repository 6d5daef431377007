"""Inputs that the front half's 1/256 sample misjudges (2^25 records over 2^20 ids: the smallest
size at which the fused and sampled passes are taken), shared by test_gpu_parity.py (the one-GPU
driver) and test_multi_gpu.py (the multi-rank driver), and their CPU-checker references, each
computed once per session."""
import numpy as np

M, N_IDS = 1 << 25, 1 << 20


def xy_overflow_records():
    """Every 256th record (the sampled ones) joins ids 0 and 1, the others spread over 2^20 ids,
    so every other degree bucket and y digit outgrows its capacity."""
    rng = np.random.default_rng(3)
    uv = rng.integers(0, N_IDS, size=(M, 2), dtype=np.uint32)
    uv[::256] = (0, 1)
    return uv


def y_overflow_records():
    """Only the y regions overflow: every 256th record (the sampled ones) has a uniform head, the
    others a head in one y digit's 1024 ids, while the tails stay uniform (the x buckets fit)."""
    rng = np.random.default_rng(21)
    uv = rng.integers(0, N_IDS, size=(M, 2), dtype=np.uint32)
    keep = np.zeros(M, bool)
    keep[::256] = True
    uv[~keep, 1] = rng.integers(5 << 10, 6 << 10, size=int((~keep).sum()), dtype=np.uint32)
    return uv


def uniform_records(seed):
    """2^25 uniform records over the same id space: nothing overflows."""
    return np.random.default_rng(seed).integers(0, N_IDS, size=(M, 2), dtype=np.uint32)


def to_device(uv):
    import torch

    return torch.from_numpy(uv.view(np.int32)).cuda().view(torch.uint32)


class SharedReference:
    """The CPU checker for one named input (the same records every time): its sequence and tree
    are computed by the first test that asks and kept, unchanged, for the others."""

    _memo = {}

    def __init__(self, oracle, name):
        self.oracle, self.name = oracle, name

    def _once(self, key, make):
        key = (self.name,) + key
        if key not in self._memo:
            out = make()
            for a in (out if isinstance(out, tuple) else (out,)):
                a.setflags(write=False)
            self._memo[key] = out
        return self._memo[key]

    def degree_sequence(self, uv, mode=0):
        return self._once(("seq", mode), lambda: self.oracle.degree_sequence(uv, mode))

    def build_tree(self, uv, seq):
        return self._once(("tree",), lambda: tuple(self.oracle.build_tree(uv, seq)))
