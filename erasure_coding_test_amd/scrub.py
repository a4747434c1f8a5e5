"""Stripe scrub (ecgpu_scrub_* in include/ecgpu.h): is every stripe still a
codeword, and if not, which shard is wrong?

A :class:`ScrubPlan` holds the m x k GF(2^8) coding matrix on the GPU and a
table of device pointers for many stripes; ``launch`` enqueues one fused
verify pass (the k + m shards read once, nothing written for a clean stripe)
plus the blame of the bad stripes, asynchronously on a HIP stream and
graph-capturable like :class:`~.plan.StripePlan`.  ``results`` reads the
per-stripe verdicts; ``repair`` hands the stripes with exactly one suspect to
one :class:`~.rebuild.RebuildPlan` and scrubs again.  w = 8 and device memory
only.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Sequence

import torch

from . import _native as N
from ._buffers import addr
from .rebuild import RebuildPlan

SCRUB_MAX_M = 8
_NO_POSITION = 2**64 - 1


class _Result(ctypes.Structure):  # ecgpu_scrub_result
    _fields_ = [("bad_bytes", ctypes.c_uint64 * SCRUB_MAX_M), ("bad_cols", ctypes.c_uint64),
                ("first_bad", ctypes.c_uint64), ("blame", ctypes.c_uint64)]


class ScrubResult(NamedTuple):
    bad_bytes: tuple           # per coding row: positions whose syndrome byte is non-zero
    bad_cols: int              # bad positions
    first_bad: Optional[int]   # lowest bad position, None when clean
    suspects: list             # shard ids (0..k+m-1) that alone explain every bad position

    @property
    def clean(self) -> bool:
        return self.bad_cols == 0


def blame_matrix(k: int, m: int, matrix: Sequence[int]):
    """(pivots[k], ratios[m*k]) of the blame test (ecgpu_scrub_blame_matrix; host only)."""
    pivots, ratios = (N.c_int * k)(), (N.c_int * (m * k))()
    N.check(N.lib.ecgpu_scrub_blame_matrix(k, m, N.int_array(matrix), pivots, ratios), "ecgpu_scrub_blame_matrix")
    return list(pivots), list(ratios)


class ScrubPlan:
    def __init__(self, k: int, m: int, matrix: Sequence[int], device: int = -1):
        matrix = [int(c) for c in matrix]
        if k >= 1 and m >= 1 and len(matrix) != k * m:
            raise ValueError("matrix must hold m * k entries")
        self.k, self.m, self.matrix = k, m, matrix
        self.device = torch.cuda.current_device() if device < 0 else device
        self._p = N.lib.ecgpu_scrub_create(k, m, 8, N.int_array(matrix), self.device)
        if not self._p:
            raise N.EcgpuError(f"ecgpu_scrub_create failed: {N.last_error()}")
        self.stripes, self.size = 0, 0

    def bind_stripes(self, shards: Sequence[Sequence], size: int) -> "ScrubPlan":
        """shards[s] = the k+m shard buffers of stripe s (ids 0..k+m-1): CUDA
        tensors or raw device addresses."""
        k, n = self.k, self.k + self.m
        flat = [[addr(b) for b in st] for st in shards]
        if any(len(st) != n for st in flat):
            raise ValueError("every stripe needs k + m shards")
        N.check(N.lib.ecgpu_scrub_bind(self._p, len(flat), N.ptr_array([a for st in flat for a in st[:k]]),
                                       N.ptr_array([a for st in flat for a in st[k:]]), size), "ecgpu_scrub_bind")
        self.stripes, self.size = len(flat), size
        return self

    def _stream(self, stream):
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        return stream or None

    def launch(self, stream: Optional[int] = None) -> None:
        N.check(N.lib.ecgpu_scrub_launch(self._p, self._stream(stream)), "ecgpu_scrub_launch")

    def results(self, stream: Optional[int] = None) -> list:
        """Waits for `stream` (torch's current stream by default) and returns
        one :class:`ScrubResult` per bound stripe."""
        buf = (_Result * max(1, self.stripes))()
        n = N.check(N.lib.ecgpu_scrub_read(self._p, self._stream(stream), buf, self.stripes), "ecgpu_scrub_read")
        out = []
        for r in buf[:max(0, n)]:
            out.append(ScrubResult(tuple(int(v) for v in r.bad_bytes[:self.m]), int(r.bad_cols),
                                   None if r.first_bad == _NO_POSITION else int(r.first_bad),
                                   [i for i in range(self.k + self.m) if (r.blame >> i) & 1]))
        return out

    @property
    def engine(self) -> int:
        """0: the specialised 16-B-column kernel runs for the current binding, 1: the byte kernel only."""
        return N.check(N.lib.ecgpu_scrub_engine(self._p), "ecgpu_scrub_engine")

    @property
    def device_results(self) -> int:
        """Device address of the raw ecgpu_scrub_result array (blame meaningful only where bad_cols > 0)."""
        return int(N.lib.ecgpu_scrub_device_results(self._p) or 0)

    def repair(self, shards: Sequence[Sequence], size: int):
        """Scrub, rebuild every stripe that has exactly one suspect shard (one
        RebuildPlan: a single launch whichever shard each stripe lost), scrub
        again.

        Returns ``(repaired, unrepaired, results_after)``: repaired = [(stripe,
        shard)] whose stripe is clean afterwards, unrepaired = the stripes
        still bad (no single suspect -- left untouched -- or a rebuild the
        second scrub did not confirm)."""
        self.bind_stripes(shards, size)
        self.launch()
        tried = {s: r.suspects[0] for s, r in enumerate(self.results()) if not r.clean and len(r.suspects) == 1}
        rebuild = RebuildPlan(self.k, self.m, self.matrix, device=self.device)
        if tried:
            rebuild.bind_stripes(shards, [[tried[s]] if s in tried else [] for s in range(len(shards))], size).launch()
        self.launch()
        after = self.results()  # waits for the stream: the rebuild is done
        rebuild.close()
        repaired = [(s, tried[s]) for s in sorted(tried) if after[s].clean]
        unrepaired = [s for s, r in enumerate(after) if not r.clean]
        return repaired, unrepaired, after

    def close(self) -> None:
        if getattr(self, "_p", None):
            N.lib.ecgpu_scrub_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
