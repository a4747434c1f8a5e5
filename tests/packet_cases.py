"""Cases and reference for the GF(2) packet path (csrc/packets.hip,
csrc/gf_kernels_packets.hpp), shared by tests/test_packet_cases.py (no GPU)
and tests/test_packet_kernels_gpu.py.

The reference is `replay`: the schedule's {src dev, src packet, dst dev, dst
packet, xor?} rows run strictly in order, per super-packet, on copies of the
buffers -- what the reference's jerasure_do_scheduled_operations does
(jerasure.cpp:1153-1192).  A bit-matrix call is lowered to such rows the way
jerasure_bitmatrix_dotprod works (jerasure.cpp:301-345): per output packet the
first set bit copies, later set bits XOR, an all-zero row writes nothing.
Nothing here models the library's tracker, planner or masks.

Which kernel a case must launch is written out in the tables below as
(kind, launches) for ecgpu_packet_launches -- 0 byte kernel, 1 8-byte lanes,
2 unpipelined 16-byte, 3 pipelined 16-byte, 4 unit form, 5 zero fill -- and
is never computed from the map.

Run as a program it executes every case on host arrays through whatever
executor the environment selects and prints one JSON line
(tests/test_packet_cases.py starts it with ECGPU_GPU=0: the CPU executor).
"""
import itertools
from collections import namedtuple

import numpy as np

FILL = 0xCC
GUARD = 16
KINDS = 6

# One call.  api: "schedule_encode" (k data + m coding devices of w packet
# rows, `ops`), "bitmatrix_encode" (`bm`; `ops` is its lowering),
# "do_scheduled" (one super-packet, `ops`), "dotprod" (`bm` = the w x k*w row
# block, `extra` = (src_ids, dest_id)), "decode" (`extra` = (row_k_ones, erasures)).
Case = namedtuple("Case", "name api k m w ops bm extra")


def case(name, api, k, m, w, ops, bm=None, extra=None):
    return Case(name, api, k, m, w, [tuple(int(v) for v in op) for op in ops], bm, extra)


# ------------------------------------------------------------- reference ----
def replay(ops, slots, nsp, spstride, ps):
    """The buffers after the schedule: copies of `slots` (1-D uint8 arrays, None
    where a device is unused) with every op applied in order to super-packet
    0, then to super-packet 1, ...  Packet row r of slot s in super-packet sp
    is slots[s][sp * spstride + r * ps:][:ps]."""
    out = [None if s is None else np.array(s, dtype=np.uint8) for s in slots]
    rows = 1 + max([max(o[1], o[3]) for o in ops], default=0)
    if nsp > 1 and spstride >= rows * ps:
        # the super-packets are disjoint byte ranges, so running an op on all of
        # them at once gives what one super-packet after the other gives
        # (test_packet_cases.py compares the two)
        def view(s, r):
            return np.lib.stride_tricks.as_strided(out[s][r * ps:], shape=(nsp, ps), strides=(spstride, 1))
        for sd, sr, dd, dr, x in ops:
            src, dst = view(sd, sr), view(dd, dr)
            if x:
                np.bitwise_xor(dst, src, out=dst)
            else:
                dst[...] = src
        return out
    return replay_literal(ops, slots, nsp, spstride, ps)


def replay_literal(ops, slots, nsp, spstride, ps):
    out = [None if s is None else np.array(s, dtype=np.uint8) for s in slots]
    for sp in range(nsp):
        for sd, sr, dd, dr, x in ops:
            src = out[sd][sp * spstride + sr * ps:sp * spstride + (sr + 1) * ps]
            dst = out[dd][sp * spstride + dr * ps:sp * spstride + (dr + 1) * ps]
            if x:
                dst ^= src
            else:
                dst[:] = src
    return out


def lower_rows(k, w, bits, src_ids, dest_id):
    """Schedule rows of one jerasure_bitmatrix_dotprod: bits is [w, k * w]."""
    ops = []
    for j in range(w):
        started = 0
        for x in range(k):
            dev = x if src_ids is None else src_ids[x]
            for y in range(w):
                if bits[j][x * w + y]:
                    ops.append((dev, y, dest_id, j, started))
                    started = 1
    return ops


def lower_bitmatrix(k, m, w, bm):
    """Schedule rows of jerasure_bitmatrix_encode: bm is [m * w, k * w]."""
    ops = []
    for i in range(m):
        ops += lower_rows(k, w, bm[i * w:(i + 1) * w], None, k + i)
    return ops


def direct_bitmatrix(k, m, w, bm, slots, nsp, ps):
    """Direct evaluation of a bit-matrix encode, no schedule: every coding
    packet is the XOR of the data packets its row names; a packet whose row is
    all zero keeps its bytes."""
    out = [np.array(s, dtype=np.uint8) for s in slots]
    img = [o.reshape(nsp, w, ps) for o in out]
    for r in range(m * w):
        cols = np.flatnonzero(bm[r])
        if len(cols):
            img[k + r // w][:, r % w, :] = np.bitwise_xor.reduce([slots[c // w].reshape(nsp, w, ps)[:, c % w, :]
                                                                  for c in cols], axis=0)
    return out


# -------------------------------------------------------------- builders ----
def exact_map(nsrc, R, rng, spread=False):
    """R outputs, each a non-empty random subset of nsrc sources, every source
    used: the launch has exactly this nsrc and R.  Sources are packet rows
    0..nsrc-1 of device 0 and outputs rows 0..R-1 of device 1 (k = m = 1,
    w = max(nsrc, R)); spread=True gives every source and output a device of
    its own (k = nsrc, m = R, w = 1) so each can be placed on its own."""
    M = rng.integers(0, 2, (R, nsrc), dtype=np.uint8)
    for r in range(R):
        if not M[r].any():
            M[r, rng.integers(nsrc)] = 1
    for j in range(nsrc):
        if not M[:, j].any():
            M[rng.integers(R), j] = 1
    ops = []
    for r in range(R):
        for n, j in enumerate(np.flatnonzero(M[r])):
            ops.append((j, 0, nsrc + r, 0, n > 0) if spread else (0, j, 1, r, n > 0))
    if spread:
        return case(f"exact_map({nsrc},{R},spread)", "schedule_encode", nsrc, R, 1, ops, bm=M)
    return case(f"exact_map({nsrc},{R})", "schedule_encode", 1, 1, max(nsrc, R), ops, bm=M)


def unit_bits(k, m, rng):
    """[m * 8, k * 8] bits: identity blocks in coding device 0 (and every
    fourth one: each 32-row group's first) and from data device 0 into every
    coding device; every other bit uniformly random."""
    bm = rng.integers(0, 2, (m * 8, k * 8), dtype=np.uint8)
    eye = np.eye(8, dtype=np.uint8)
    for i in range(m):
        bm[i * 8:i * 8 + 8, 0:8] = eye
        if i % 4 == 0:
            for x in range(k):
                bm[i * 8:i * 8 + 8, x * 8:x * 8 + 8] = eye
    return bm


def bitmatrix_case(name, k, m, bm):
    return case(name, "bitmatrix_encode", k, m, 8, lower_bitmatrix(k, m, 8, bm), bm=bm)


def unit_shaped(k, rng):
    return bitmatrix_case(f"unit_shaped({k})", k, 4, unit_bits(k, 4, rng))


# (variant, kind, launches): what each near miss must run on
NEAR_MISSES = [("a", 3, 1), ("b", 3, 1), ("c", 3, 1), ("d", 3, 1), ("e", 3, 1), ("f", 1, 1)]
NEAR_MISS_OFFSET = {"f": 8}  # base offset of every view; the others 0


def near_misses(k, rng):
    """{variant: (case, conforming bit-matrix it was made from, changed (row, column) list)}.
    k >= 2.  (a) an extra low-8 bit on a source of a device >= 1; (b) a
    device-0 source without its identity bit in coding device 2; (c) a
    device-0 source with one more bit in coding device 3; (d) one bit column
    of the last data device unused; (e) m = 3; (f) conforming, for 8-aligned
    bases."""
    assert k >= 2
    out = {}
    base = unit_bits(k, 4, rng)

    def variant(v, cells):
        bm = base.copy()
        for r, c in cells:
            bm[r, c] ^= 1
        out[v] = (bitmatrix_case(f"near_miss({k},{v})", k, 4, bm), base, cells)

    variant("a", [(5, 8 + 2)])             # source 10 = device 1 bit 2: low mask bits 2 and 5
    variant("b", [(2 * 8 + 6, 6)])         # source 6 = device 0 bit 6: no bit in row 22
    variant("c", [(3 * 8 + 1, 4)])         # source 4 = device 0 bit 4: also row 25
    col = (k - 1) * 8 + 3
    variant("d", [(r, col) for r in range(32) if base[r, col]])
    out["e"] = (bitmatrix_case(f"near_miss({k},e)", k, 3, base[:24].copy()), base, "rows 24..31 removed")
    out["f"] = (bitmatrix_case(f"near_miss({k},f)", k, 4, base.copy()), base, [])
    return out


def two_unit_groups(k, rng):
    return bitmatrix_case(f"two_unit_groups({k})", k, 8, unit_bits(k, 8, rng))


def accumulate(rows, rng=None):
    """b[p] ^= a[p] for every packet row, then the rotation b[p + 1] ^= b[p]:
    every destination's old content is a source."""
    ops = [(0, p, 1, p, 1) for p in range(rows)] + [(1, p, 1, (p + 1) % rows, 1) for p in range(rows)]
    return case(f"accumulate({rows})", "schedule_encode", 1, 1, rows, ops)


def all_zero(rows, spare=2):
    """Copy X to D, then XOR X into D: every output folds to zero.  D has
    `spare` more packet rows, which no op names."""
    ops = [(0, p, 1, p, x) for p in range(rows) for x in (0, 1)]
    return case(f"all_zero({rows})", "schedule_encode", 1, 1, rows + spare, ops)


def some_zero(rows):
    """Every third output folds to zero; the others are X[p] ^ X[p + 1]."""
    ops = []
    for p in range(rows):
        ops += [(0, p, 1, p, 0), (0, p if p % 3 == 0 else (p + 1) % rows, 1, p, 1)]
    return case(f"some_zero({rows})", "schedule_encode", 1, 1, rows, ops)


def some_zero_beside_unit(k, rng):
    """No map with a zero output has the unit form (its rows 0..7 are each fed
    by their own bit of every device), so this is the nearest call: m = 8,
    the first 32-row group conforming, the second with outputs 33 and 40
    folded to zero and the rest random."""
    bm = unit_bits(k, 8, rng)
    bm[32:, :] = rng.integers(0, 2, (32, k * 8), dtype=np.uint8)
    bm[32:, 0] = 1  # no all-zero row: every op below is deliberate
    ops = lower_bitmatrix(k, 8, 8, bm)
    for r in (33, 40):
        dev, row = k + r // 8, r % 8
        ops = [o for o in ops if (o[2], o[3]) != (dev, row)] + [(0, 1, dev, row, 0), (0, 1, dev, row, 1)]
    return case(f"some_zero_beside_unit({k})", "schedule_encode", k, 8, 8, ops)


def staging_bits(rng):
    """k = 3, m = 2, w = 5 random bit-matrix, rows 2 and 7 all zero."""
    bm = rng.integers(0, 2, (10, 15), dtype=np.uint8)
    bm[:, 0] = 1
    bm[[2, 7], :] = 0
    return case("staging(3,2,5)", "bitmatrix_encode", 3, 2, 5, lower_bitmatrix(3, 2, 5, bm), bm=bm)


def dotprod_case(k, m, w, src_ids, dest_id, rng):
    bits = rng.integers(0, 2, (w, k * w), dtype=np.uint8)
    bits[:, 0] = 1
    return case(f"dotprod({src_ids}->{dest_id})", "dotprod", k, m, w, lower_rows(k, w, bits, src_ids, dest_id),
                bm=bits, extra=(list(src_ids), dest_id))


# --------------------------------------------------------- case tables ----
SEED = 20260
NSRCS = list(range(1, 14)) + [16, 17]   # nc = nsrc >> 2 of 0..4, every tail length, both parities
RS = [1, 8, 9, 16, 17, 32]              # both sides of every RT boundary

# lanes of the chunk x RT sweep: (label, ECGPU_PACKET, ps, nsp, kind); one launch each
SWEEP_LANES = [
    ("knob0", 0, 16, 257, 3),
    ("knob1", 1, 16, 257, 1),
    ("knob2", 2, 16, 257, 2),
    ("knob3", 3, 16, 257, 3),
    ("bytes", 0, 5, 52, 0),
]

# unit form: (k, ECGPU_PACKET, kind, launches), at ps = 48, nsp = 86
UNIT_KS = [1, 2, 3, 7, 12]
UNIT_EXPECT = {0: (4, 1), 3: (3, 1)}
TWO_GROUPS_EXPECT = (4, 2)

# alignment routing: (ps, nsp, offset, who, kind); exact_map(9, 9, spread), one launch
ALIGN_CASES = [
    (16, 257, 0, "all", 3), (16, 257, 8, "all", 1), (16, 257, 8, "source", 1), (16, 257, 8, "destination", 1),
    (16, 257, 1, "all", 0), (16, 257, 1, "source", 0), (16, 257, 1, "destination", 0),
    (24, 86, 0, "all", 1), (24, 86, 8, "all", 1), (24, 86, 8, "source", 1), (24, 86, 8, "destination", 1),
    (24, 86, 1, "all", 0), (24, 86, 1, "source", 0), (24, 86, 1, "destination", 0),
    (8, 257, 0, "all", 1), (8, 257, 8, "all", 1), (8, 257, 8, "source", 1), (8, 257, 8, "destination", 1),
    (8, 257, 1, "all", 0), (8, 257, 1, "source", 0), (8, 257, 1, "destination", 0),
    (5, 52, 0, "all", 0), (5, 52, 8, "all", 0), (5, 52, 8, "source", 0), (5, 52, 8, "destination", 0),
    (5, 52, 1, "all", 0), (5, 52, 1, "source", 0), (5, 52, 1, "destination", 0),
]

# temporaries: rows -> launches, ps -> kind; nsp = 5
ACCUMULATE_LAUNCHES = {32: 1, 40: 2, 65: 3}
ACCUMULATE_KIND = {16: 3, 8: 1, 5: 0}

# zero outputs: rows -> kind-5 count (one per 32-row group)
ALL_ZERO_GROUPS = {3: 1, 40: 2}
# some_zero(9): (label, ECGPU_PACKET, ps, nsp, {kind: launches})
SOME_ZERO_LANES = [
    ("bytes", 0, 5, 52, {0: 1}),
    ("8-byte", 0, 8, 257, {1: 1}),
    ("16-byte unpipelined", 2, 16, 257, {2: 1}),
    ("16-byte pipelined", 0, 16, 257, {3: 1}),
]
SOME_ZERO_BESIDE_UNIT = {4: 1, 3: 1}  # ps = 16, ECGPU_PACKET = 0

STAGING_EXPECT = (3, 1)  # ps = 16: staged slots start 256-aligned
DOTPRODS = [([4, 0, 2], 1), ([1, 3, 0], 4)]  # (src_ids, dest_id), k = 3, m = 2: a data and a coding destination
DOTPROD_EXPECT = (3, 1)  # ps = 16

# decode: k = 3, m = 2, w = 3 (P = d0 + d1 + d2, Q = d0 + 2 d1 + 4 d2 over GF(8)), ps = 8
DECODE_MATRIX = [1, 1, 1, 1, 2, 4]
DECODE_SETS = [list(c) for n in (0, 1, 2) for c in itertools.combinations(range(5), n)]
DECODE_EXPECT = (1, 1)  # any erasure; none: no launch at all


def grow(*pairs):
    """Expected counter growth [kind 0..5] from (kind, launches) pairs."""
    g = [0] * KINDS
    for kind, n in pairs:
        g[kind] += n
    return g


def rng_for(*key):
    return np.random.default_rng([SEED] + [int(v) for v in key])


def sweep_case(nsrc, R):
    return exact_map(nsrc, R, rng_for(1, nsrc, R))


# ------------------------------------------------------------- buffers ----
def stride_for(size, offset=0):
    return (GUARD + offset + size + GUARD + 15) // 16 * 16


def host_image(nslots, size, offsets, rng, fill_slots=()):
    """[nslots, stride] of FILL with slot s's view -- `size` bytes at GUARD +
    offsets[s] -- random (FILL too for fill_slots)."""
    img = np.full((nslots, stride_for(size, max(offsets))), FILL, dtype=np.uint8)
    for s in range(nslots):
        if s not in fill_slots:
            img[s, GUARD + offsets[s]:GUARD + offsets[s] + size] = rng.integers(0, 256, size, dtype=np.uint8)
    return img


def views_of(img, size, offsets):
    return [img[s, GUARD + offsets[s]:GUARD + offsets[s] + size] for s in range(len(offsets))]


def expected_image(c, img, size, offsets, nsp, ps):
    """The slab after the call: `replay` on the views, everything else as it was."""
    want = img.copy()
    spstride = 0 if c.api == "do_scheduled" else c.w * ps
    for s, v in enumerate(replay(c.ops, views_of(img, size, offsets), nsp, spstride, ps)):
        want[s, GUARD + offsets[s]:GUARD + offsets[s] + size] = v
    return want


def run_case(J, c, views, nsp, ps):
    """The library call of case c on its k + m buffers."""
    size = nsp * c.w * ps
    data, coding = views[:c.k], views[c.k:]
    if c.api == "schedule_encode":
        J.jerasure_schedule_encode(c.k, c.m, c.w, c.ops, data, coding, size, ps)
    elif c.api == "bitmatrix_encode":
        J.jerasure_bitmatrix_encode(c.k, c.m, c.w, np.asarray(c.bm).ravel(), data, coding, size, ps)
    elif c.api == "do_scheduled":
        assert nsp == 1
        J.jerasure_do_scheduled_operations(views, c.ops, ps)
    elif c.api == "dotprod":
        J.jerasure_bitmatrix_dotprod(c.k, c.w, np.asarray(c.bm).ravel(), c.extra[0], c.extra[1], data, coding, size, ps)
    else:
        raise ValueError(c.api)


def decode_codeword(J, nsp, ps, rng):
    """(bit-matrix, [5, size] clean codeword) of the decode cases: random data,
    coding packets by direct evaluation."""
    k, m, w = 3, 2, 3
    bm = np.array(J.jerasure_matrix_to_bitmatrix(k, m, w, DECODE_MATRIX), dtype=np.uint8).reshape(m * w, k * w)
    assert bm[:w].tolist() == np.tile(np.eye(w, dtype=np.uint8), k).tolist()  # first coding row is ones
    size = nsp * w * ps
    slots = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(k)] + [np.zeros(size, np.uint8)] * m
    return bm, np.stack(direct_bitmatrix(k, m, w, bm, slots, nsp, ps))


def host_cases():
    """(case, nsp, ps) of every case the GPU file runs, at sizes for a CPU."""
    for nsrc in NSRCS:
        for R in RS:
            yield sweep_case(nsrc, R), 3, 8
    for k in UNIT_KS:
        yield unit_shaped(k, rng_for(2, k)), 2, 16
    for c, _, _ in near_misses(3, rng_for(3, 3)).values():
        yield c, 2, 16
    yield two_unit_groups(3, rng_for(4, 3)), 2, 16
    yield exact_map(9, 9, rng_for(5), spread=True), 7, 5
    for rows in ACCUMULATE_LAUNCHES:
        yield accumulate(rows), 5, 8
        yield accumulate(rows), 5, 5
        yield accumulate(rows)._replace(api="do_scheduled"), 1, 16
    for rows in ALL_ZERO_GROUPS:
        yield all_zero(rows), 5, 16
    yield some_zero(9), 4, 5
    yield some_zero_beside_unit(2, rng_for(6)), 2, 16
    yield staging_bits(rng_for(7)), 3, 16
    for ids, dest in DOTPRODS:
        yield dotprod_case(3, 2, 3, ids, dest, rng_for(8, dest)), 3, 16


def main():
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from erasure_coding_test_amd import _native as N, jerasure as J
    checked, bad = 0, []
    for i, (c, nsp, ps) in enumerate(host_cases()):
        size = nsp * c.w * ps
        offsets = [0] * (c.k + c.m)
        img = host_image(c.k + c.m, size, offsets, rng_for(9, i))
        got = img.copy()
        run_case(J, c, views_of(got, size, offsets), nsp, ps)
        if not np.array_equal(got, expected_image(c, img, size, offsets, nsp, ps)):
            bad.append(f"{c.name} nsp={nsp} ps={ps}")
        checked += 1
    nsp, ps = 3, 8
    bm, clean = decode_codeword(J, nsp, ps, rng_for(10))
    for rko in (0, 1):
        for er in DECODE_SETS + [[0, 2, 4]]:
            got = clean.copy()
            got[er] = 0x33
            want = got.copy() if len(er) == 3 else clean
            rc = J.jerasure_bitmatrix_decode(3, 2, 3, bm.ravel(), rko, er, list(got[:3]), list(got[3:]), clean.shape[1], ps)
            if rc != (-1 if len(er) == 3 else 0) or not np.array_equal(got, want):
                bad.append(f"decode {er} row_k_ones={rko}: rc {rc}")
            checked += 1
    print(json.dumps({"checked": checked, "mismatches": bad, "cpu_calls": N.cpu_call_count(),
                      "fallbacks": N.fallback_count(),
                      "launches": [int(N.lib.ecgpu_packet_launches(kd)) for kd in range(KINDS)]}))
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
