"""Rebuilds whose stripes lost different shards (ecgpu_multiplan_* in
include/ecgpu.h).

A :class:`~.plan.DecodePlan` applies one erasure pattern's fused map to every
stripe of a launch.  Under rotated placement a failed device held shard
``s mod (k + m)`` of stripe ``s``, and a scrub reports a different suspect per
stripe: many patterns, a handful of stripes each.  A :class:`MultiMapPlan`
holds several coefficient matrices of one shape on the GPU and picks one per
stripe in a single launch; :func:`rebuild_groups` turns per-stripe erasure
lists into such groups on the host, and :class:`RebuildPlan` binds and
launches them.  w = 8 and device memory only.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import torch

from . import _native as N
from ._buffers import addr
from .jerasure import decode_plan as _decode_map
from .plan import DecodePlan

MAX_ROWS = 4  # rows of one multiplan launch (gf_device.hpp kMaxRows)


class MultiMapPlan:
    """``nmaps`` coefficient matrices of one rows x nsrc shape;
    ``dst[s][r] = XOR_j maps[map_of[s]][r][j] * src[s][j]`` in one launch."""

    def __init__(self, rows: int, nsrc: int, maps: Sequence[Sequence[int]], device: int = -1):
        maps = [[int(c) for c in mp] for mp in maps]
        if rows >= 1 and nsrc >= 1 and any(len(mp) != rows * nsrc for mp in maps):
            raise ValueError("every map must hold rows * nsrc entries")
        self.rows, self.nsrc, self.maps = rows, nsrc, maps
        self.device = torch.cuda.current_device() if device < 0 else device
        self._p = N.lib.ecgpu_multiplan_create(rows, nsrc, len(maps), N.int_array([c for mp in maps for c in mp]),
                                               self.device)
        if not self._p:
            raise N.EcgpuError(f"ecgpu_multiplan_create failed: {N.last_error()}")
        self.stripes, self.size = 0, 0

    def bind(self, map_of: Sequence[int], srcs: Sequence[Sequence], dsts: Sequence[Sequence],
             size: int) -> "MultiMapPlan":
        """map_of[s]: the map of stripe s; srcs[s][j] / dsts[s][r]: device
        buffers (CUDA tensors or raw device addresses)."""
        if not len(map_of) == len(srcs) == len(dsts):
            raise ValueError("map_of, srcs and dsts must list the same number of stripes")
        flat_s = [addr(b) for row in srcs for b in row]
        flat_d = [addr(b) for row in dsts for b in row]
        if len(flat_s) != len(srcs) * self.nsrc or len(flat_d) != len(dsts) * self.rows:
            raise ValueError("every stripe needs nsrc sources and rows destinations")
        N.check(N.lib.ecgpu_multiplan_bind(self._p, len(srcs), N.int_array(map_of), N.ptr_array(flat_s),
                                           N.ptr_array(flat_d), size), "ecgpu_multiplan_bind")
        self.stripes, self.size = len(srcs), size
        return self

    def launch(self, stream: Optional[int] = None) -> None:
        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        N.check(N.lib.ecgpu_multiplan_launch(self._p, stream or None), "ecgpu_multiplan_launch")

    @property
    def engine(self) -> int:
        """0: the specialised 16-B-column kernel runs for the current binding, 1: the byte kernel only."""
        return N.check(N.lib.ecgpu_multiplan_engine(self._p), "ecgpu_multiplan_engine")

    def close(self) -> None:
        if getattr(self, "_p", None):
            N.lib.ecgpu_multiplan_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RebuildGroup(NamedTuple):
    n_out: int       # rows of every map of the group
    n_src: int       # sources of every map
    patterns: list   # per map: the erasure pattern (sorted tuple of shard ids)
    maps: list       # per map: coefs[n_out][n_src], the fused map of jerasure_matrix_decode
    out_ids: list    # per map: the shard ids it writes
    src_ids: list    # per map: the shard ids it reads
    stripes: list    # stripe indices of the group, ascending
    map_of: list     # per stripe of `stripes`: index into maps


def rebuild_groups(k: int, m: int, matrix, erasures_per_stripe: Sequence[Sequence[int]], row_k_ones: int = 0) -> list:
    """Host only: per-stripe erasure lists to the groups one launch each can
    rebuild.  A list is normalised to the sorted tuple of its distinct ids;
    stripes with an empty list are left out.  Each pattern's fused map is the
    one :class:`~.plan.DecodePlan` would apply; patterns are deduplicated and
    grouped by ``(n_out, n_src)``.  Groups come in ascending ``(n_out, n_src)``
    order, a group's maps in order of first use.  ValueError, naming the
    stripe, for a pattern the reference cannot decode -- before any group is
    returned."""
    fused = {}   # pattern -> (out_ids, src_ids, rows)
    order = []   # (stripe, pattern)
    for s, erasures in enumerate(erasures_per_stripe):
        pattern = tuple(sorted({int(e) for e in erasures}))
        if not pattern:
            continue
        if pattern not in fused:
            try:
                got = _decode_map(k, m, matrix, list(pattern), row_k_ones)
            except N.EcgpuError as ex:
                raise ValueError(f"stripe {s}: erasure pattern {list(pattern)} is invalid: {ex}") from None
            if got is None:
                raise ValueError(f"stripe {s}: unrecoverable erasure pattern {list(pattern)} "
                                 "(the reference decode returns -1)")
            fused[pattern] = got
        order.append((s, pattern))
    groups = {}  # (n_out, n_src) -> RebuildGroup under construction
    index = {}   # pattern -> index in its group's maps
    for s, pattern in order:
        out_ids, src_ids, rows = fused[pattern]
        if not out_ids:
            continue  # nothing of this stripe to write
        g = groups.setdefault((len(out_ids), len(src_ids)),
                              RebuildGroup(len(out_ids), len(src_ids), [], [], [], [], [], []))
        if pattern not in index:
            index[pattern] = len(g.maps)
            g.patterns.append(pattern)
            g.maps.append([list(r) for r in rows])
            g.out_ids.append(list(out_ids))
            g.src_ids.append(list(src_ids))
        g.stripes.append(s)
        g.map_of.append(index[pattern])
    return [groups[key] for key in sorted(groups)]


class RebuildPlan:
    """Rebuilds stripes that each lost their own set of shards.

    One :class:`MultiMapPlan` per group of :func:`rebuild_groups` -- at most m
    groups in practice, one for a single-device failure -- so a launch is one
    kernel launch per group whatever the number of patterns.  A group whose
    maps write more than 4 shards (m > 4) is outside the multiplan's launch
    shape and falls back to one :class:`~.plan.DecodePlan` per pattern.
    """

    def __init__(self, k: int, m: int, matrix: Sequence[int], device: int = -1, row_k_ones: int = 0):
        self.k, self.m, self.matrix = k, m, [int(c) for c in matrix]
        self.row_k_ones = row_k_ones
        self.device = torch.cuda.current_device() if device < 0 else device
        self.groups, self._plans = [], []
        self.stripes, self.size = 0, 0

    def bind_stripes(self, shards: Sequence[Sequence], erasures_per_stripe: Sequence[Sequence[int]],
                     size: int) -> "RebuildPlan":
        """shards[s] = the k+m shard buffers of stripe s (ids 0..k+m-1), as in
        DecodePlan.bind_stripes; erasures_per_stripe[s] = the shard ids stripe
        s lost (empty: the stripe is left alone)."""
        if len(shards) != len(erasures_per_stripe):
            raise ValueError("shards and erasures_per_stripe must list the same number of stripes")
        groups = rebuild_groups(self.k, self.m, self.matrix, erasures_per_stripe, self.row_k_ones)
        self.close()
        for g in groups:
            if g.n_out <= MAX_ROWS:
                plan = MultiMapPlan(g.n_out, g.n_src, [[c for r in mp for c in r] for mp in g.maps], self.device)
                self._plans.append(plan)
                plan.bind(g.map_of, [[shards[s][i] for i in g.src_ids[mi]] for s, mi in zip(g.stripes, g.map_of)],
                          [[shards[s][i] for i in g.out_ids[mi]] for s, mi in zip(g.stripes, g.map_of)], size)
            else:
                for mi, pattern in enumerate(g.patterns):
                    plan = DecodePlan(self.k, self.m, self.matrix, list(pattern), self.row_k_ones, self.device)
                    self._plans.append(plan)
                    plan.bind_stripes([shards[s] for s, i in zip(g.stripes, g.map_of) if i == mi], size)
        self.groups = groups
        self.stripes, self.size = len(shards), size
        return self

    @property
    def plans(self) -> list:
        """The bound plans, one launch each: a MultiMapPlan per group (DecodePlans for a group of more than 4 outputs)."""
        return list(self._plans)

    def launch(self, stream: Optional[int] = None) -> None:
        for plan in self._plans:
            plan.launch(stream)

    def close(self) -> None:
        for plan in getattr(self, "_plans", []):
            plan.close()
        self._plans = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
