"""Every GF(2) packet kernel and launch shape against a schedule replay.

csrc/gf_kernels_packets.hpp has five kernels (bytes, 8-byte lanes, 16-byte
unpipelined, 16-byte pipelined, the unit form), the first four in RT = 8, 16
and 32 output rows; packets_on_ctx (csrc/packets.hip) picks one per 32-row
group from the alignment of every base and stride, ECGPU_PACKET, R and
unit_packet_map(), writes through temporaries when an output is also a source
and there is more than one group, and zero-fills a group none of whose
outputs has a source left.  The cases and the reference (numpy replay of the
schedule rows, in order) are in tests/packet_cases.py; tests/test_packet_cases.py
proves them without a GPU.

Rules of every test here: each buffer is a view into a slab pre-filled with
0xCC, at least 16 guard bytes before and after it; the whole slab is compared
bit for bit -- guards, sources and packet rows the call does not write
included; and ecgpu_packet_launches must grow by the stated count for the
stated kind and by 0 for every other kind.

Sizes are the smallest that split the work over two blocks -- one full
256-lane block and one to four live lanes in a second:

    lanes     ps   super-packets  columns  columns per packet
    16-byte   16   257            257      1
    8-byte     8   257            257      1
    8-byte    24    86            258      3
    16-byte   48    86            258      3
    byte       5    52            260      5

(ECGPU_PACKET = 1 on ps = 16 gives 514 8-byte columns, 2 per packet.)  The
rows with 3 and 5 columns per packet put a divisor that is no power of two
through packet_coords.  Its 64-bit division branch needs more than 2^32
columns, which a call whose size is an int cannot ask for: it is not reached
here and cannot be reached through the API.
"""
import functools

import numpy as np
import pytest

import packet_cases as pc
from packet_cases import FILL, GUARD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ec(gpu):
    import erasure_coding_test_amd as E
    return E


def counters(ec):
    return [int(ec._native.lib.ecgpu_packet_launches(kind)) for kind in range(pc.KINDS)]


def first_difference(got, want):
    row, pos = np.argwhere(got != want)[0]
    lo = max(0, pos - 4)
    return (f"slot {row} slab byte {pos} (views start at {GUARD} + offset): expected "
            f"{want[row, lo:pos + 12].tobytes().hex()} got {got[row, lo:pos + 12].tobytes().hex()} (from byte {lo})")


class Slab:
    """The image's rows as buffers: row s lives in device memory, pageable
    numpy memory or pinned memory as where[s] says ("device", "numpy",
    "pinned"); one backing array per kind of memory, every row of it compared."""

    def __init__(self, gpu, img, size, offsets, where="device"):
        import torch
        n = img.shape[0]
        self.img, self.size, self.offsets = img, size, offsets
        self.where = [where] * n if isinstance(where, str) else list(where)
        self.back = {}
        for wh in set(self.where):
            if wh == "device":
                self.back[wh] = torch.from_numpy(img.copy()).to(gpu)
            elif wh == "pinned":
                self.back[wh] = torch.from_numpy(img.copy()).pin_memory()
                assert self.back[wh].is_pinned()
            else:
                self.back[wh] = img.copy()
        for s, v in enumerate(self.views()):
            if self.where[s] == "device":
                assert v.data_ptr() % 16 == offsets[s] % 16

    def views(self):
        return [self.back[self.where[s]][s, GUARD + o:GUARD + o + self.size] for s, o in enumerate(self.offsets)]

    def load(self, img):
        """A new image into the same buffers."""
        import torch
        self.img = img
        for wh, b in self.back.items():
            if wh == "numpy":
                b[...] = img
            else:
                b.copy_(torch.from_numpy(img.copy()))

    def check(self, want, label):
        for wh, b in self.back.items():
            got = b if wh == "numpy" else b.cpu().numpy()
            image = np.stack([want[s] if self.where[s] == wh else self.img[s] for s in range(len(self.where))])
            if not np.array_equal(got, image):
                raise AssertionError(f"{label} ({wh} memory): {first_difference(got, image)}")


def launch(ec, c, slab, nsp, ps, growth, label):
    """The case's call on the slab's views; the counters must grow by `growth`."""
    import torch
    before = counters(ec)
    pc.run_case(ec.jerasure, c, slab.views(), nsp, ps)
    torch.cuda.synchronize()
    grew = [a - b for a, b in zip(counters(ec), before)]
    assert grew == growth, f"{label}: ecgpu_packet_launches grew by {grew}, expected {growth} (kinds 0..5)"


def run(ec, gpu, c, nsp, ps, growth, label, offsets=None, where="device", fill_slots=(), rng=None, prepared=None):
    size = nsp * c.w * ps
    offsets = offsets or [0] * (c.k + c.m)
    if prepared is None:
        img = pc.host_image(c.k + c.m, size, offsets, rng, fill_slots)
        want = pc.expected_image(c, img, size, offsets, nsp, ps)
    else:
        img, want = prepared
    slab = Slab(gpu, img, size, offsets, where)
    launch(ec, c, slab, nsp, ps, growth, label)
    slab.check(want, label)
    return want


# ------------------------------------------------------ chunk x RT sweep ----
@functools.lru_cache(maxsize=None)
def sweep_reference(nsrc, R, ps, nsp):
    """(case, image, expected image), computed once for the lanes that share a packet size."""
    c = pc.sweep_case(nsrc, R)
    size = nsp * c.w * ps
    img = pc.host_image(2, size, [0, 0], pc.rng_for(20, nsrc, R, ps))
    want = pc.expected_image(c, img, size, [0, 0], nsp, ps)
    img.setflags(write=False)
    want.setflags(write=False)
    return c, img, want


@pytest.mark.parametrize("R", pc.RS)
@pytest.mark.parametrize("lane", pc.SWEEP_LANES, ids=[ln[0] for ln in pc.SWEEP_LANES])
def test_chunk_and_rt_sweep(ec, gpu, knobs, lane, R):
    """exact_map(nsrc, R) through jerasure_schedule_encode (k = m = 1, w =
    max(nsrc, R)): nsrc 1..13, 16, 17 gives the pipelined kernel 0..4 chunks of
    four with every tail length after an even and an odd chunk count (one
    chunk: the loop leaves after its first apply, having re-read that chunk);
    R = 1, 8, 9, 16, 17, 32 sits on both sides of each RT instantiation, with
    the packet rows R..w-1 of the output device and the guards watching for a
    store to a row >= R."""
    label, knob, ps, nsp, kind = lane
    knobs.set("ECGPU_PACKET", knob)
    ran = 0
    for nsrc in pc.NSRCS:
        c, img, want = sweep_reference(nsrc, R, ps, nsp)
        run(ec, gpu, c, nsp, ps, pc.grow((kind, 1)), f"sweep {label} nsrc={nsrc} R={R} ps={ps}", prepared=(img, want))
        ran += 1
    assert ran == 15
    print(f"ran {ran} maps on {label}, R={R}")


# -------------------------------------------------------------- unit form ----
@pytest.mark.parametrize("k", pc.UNIT_KS)
def test_unit_form_random_free_bits(ec, gpu, knobs, k):
    """unit_shaped(k): the unit kernel's contract with every free mask bit
    random, on the unit kernel (ECGPU_PACKET = 0) and on the general pipelined
    one (3); ps = 48: three 16-byte columns per packet."""
    c = pc.unit_shaped(k, pc.rng_for(2, k))
    want = None
    for knob, (kind, n) in sorted(pc.UNIT_EXPECT.items()):
        knobs.set("ECGPU_PACKET", knob)
        got = run(ec, gpu, c, 86, 48, pc.grow((kind, n)), f"unit_shaped k={k} ECGPU_PACKET={knob}", rng=pc.rng_for(21, k))
        assert want is None or np.array_equal(got, want)
        want = got
    print(f"ran 2 launches of unit_shaped({k})")


def test_near_misses_take_the_general_kernels(ec, gpu):
    """Maps one bit away from the unit form, m = 3, and the unit form on
    8-aligned bases must not reach the unit kernel."""
    k = 3
    nm = pc.near_misses(k, pc.rng_for(3, k))
    ran = 0
    for v, kind, n in pc.NEAR_MISSES:
        c = nm[v][0]
        offsets = [pc.NEAR_MISS_OFFSET.get(v, 0)] * (c.k + c.m)
        run(ec, gpu, c, 257, 16, pc.grow((kind, n)), f"near miss ({v})", offsets=offsets, rng=pc.rng_for(22, ran))
        ran += 1
    assert ran == 6
    print(f"ran {ran} near misses")


def test_two_unit_groups(ec, gpu, knobs):
    """m = 8: the second group's dst and mask tables start 32 rows / nsrc words in."""
    c = pc.two_unit_groups(3, pc.rng_for(4, 3))
    run(ec, gpu, c, 257, 16, pc.grow(pc.TWO_GROUPS_EXPECT), "two unit groups", rng=pc.rng_for(23))
    knobs.set("ECGPU_PACKET", 3)
    run(ec, gpu, c, 257, 16, pc.grow((3, 2)), "two unit groups, ECGPU_PACKET=3", rng=pc.rng_for(23))


def test_consecutive_unit_calls_on_the_same_buffers(ec, gpu):
    """Two unit-form calls of one shape with different masks and data: the
    second must not see the first one's pointer or mask table in the reused
    staging slab."""
    k, nsp, ps = 7, 86, 48
    size, offsets = nsp * 8 * ps, [0] * (k + 4)
    slab = None
    for call in (0, 1):
        c = pc.unit_shaped(k, pc.rng_for(24, call))
        img = pc.host_image(k + 4, size, offsets, pc.rng_for(25, call))
        if slab is None:
            slab = Slab(gpu, img, size, offsets)
        else:
            slab.load(img)
        launch(ec, c, slab, nsp, ps, pc.grow((4, 1)), f"unit call {call}")
        slab.check(pc.expected_image(c, img, size, offsets, nsp, ps), f"unit call {call}")


# ------------------------------------------------------ alignment routing ----
@pytest.mark.parametrize("ps", [16, 24, 8, 5])
def test_alignment_routing(ec, gpu, ps):
    """exact_map(9, 9) with a device per source and per output (w = 1): every
    view, one source alone or one output alone 0, 8 or 1 bytes past a 16-byte
    boundary.  16-byte lanes need everything 16-aligned, 8-byte lanes
    8-aligned, anything else is the byte kernel's."""
    c = pc.exact_map(9, 9, pc.rng_for(5), spread=True)
    ran = 0
    for cps, nsp, offset, who, kind in pc.ALIGN_CASES:
        if cps != ps:
            continue
        offsets = [offset] * 18 if who == "all" else [0] * 18
        offsets[{"all": 0, "source": 4, "destination": 9 + 5}[who]] = offset
        run(ec, gpu, c, nsp, ps, pc.grow((kind, 1)), f"alignment ps={ps} offset={offset} on {who}", offsets=offsets,
            rng=pc.rng_for(26, ps, offset))
        ran += 1
    assert ran == 7 and len(pc.ALIGN_CASES) == 28
    print(f"ran {ran} placements at ps={ps}")


# ------------------------------------- temporaries, several super-packets ----
@pytest.mark.parametrize("where", ["device", "numpy", "pinned"])
@pytest.mark.parametrize("rows", sorted(pc.ACCUMULATE_LAUNCHES))
def test_accumulate_several_super_packets(ec, gpu, rows, where):
    """Outputs that are their own sources: 32 rows in place in one launch, 40
    and 65 through temporaries (one packet row of every super-packet per
    temporary, copied back with the super-packet pitch), the last group of 65
    with R = 1; five super-packets."""
    c = pc.accumulate(rows)
    for ps in (16, 8, 5):
        growth = pc.grow((pc.ACCUMULATE_KIND[ps], pc.ACCUMULATE_LAUNCHES[rows]))
        run(ec, gpu, c, 5, ps, growth, f"accumulate rows={rows} ps={ps} {where}", where=where,
            rng=pc.rng_for(27, rows, ps))
    print(f"ran 3 packet sizes of accumulate({rows}) in {where} memory")


def test_accumulate_do_scheduled_operations_device(ec, gpu):
    c = pc.accumulate(40)._replace(api="do_scheduled")
    run(ec, gpu, c, 1, 16, pc.grow((3, 2)), "accumulate(40) jerasure_do_scheduled_operations, device", rng=pc.rng_for(28))


# ----------------------------------------------------------- zero outputs ----
@pytest.mark.parametrize("nsp", [1, 5])
@pytest.mark.parametrize("rows", sorted(pc.ALL_ZERO_GROUPS))
def test_all_outputs_zero(ec, gpu, rows, nsp):
    """Every output folds to zero: no kernel, one zero fill per group.  The
    output device starts as 0xCC: its two packet rows no op names, so the gap
    between one super-packet's outputs and the next one's, stay 0xCC."""
    c = pc.all_zero(rows)
    for ps in (16, 5):
        want = run(ec, gpu, c, nsp, ps, pc.grow((5, pc.ALL_ZERO_GROUPS[rows])), f"all_zero rows={rows} nsp={nsp} ps={ps}",
                   fill_slots=(1,), rng=pc.rng_for(29, rows, ps))
        out = want[1, GUARD:GUARD + nsp * c.w * ps].reshape(nsp, c.w, ps)
        assert not out[:, :rows].any() and (out[:, rows:] == FILL).all()


def test_some_outputs_zero_on_every_kernel(ec, gpu, knobs):
    ran = 0
    for label, knob, ps, nsp, kinds in pc.SOME_ZERO_LANES:
        knobs.set("ECGPU_PACKET", knob)
        run(ec, gpu, pc.some_zero(9), nsp, ps, pc.grow(*kinds.items()), f"some_zero {label}", rng=pc.rng_for(30, ran))
        ran += 1
    knobs.set("ECGPU_PACKET", 0)
    run(ec, gpu, pc.some_zero_beside_unit(2, pc.rng_for(6)), 257, 16, pc.grow(*pc.SOME_ZERO_BESIDE_UNIT.items()),
        "zero outputs in the group after a unit-form group", rng=pc.rng_for(30, ran))
    assert ran + 1 == 5
    print(f"ran {ran + 1} zero-row maps")


# ------------------------------------------------------------ host staging ----
@pytest.mark.parametrize("placement", ["pageable", "pinned", "device-to-host", "host-to-device"])
def test_host_staging_placements(ec, gpu, placement):
    """A bit-matrix encode (k = 3, m = 2, w = 5, two all-zero rows) with host
    slots staged whole, outputs included, and copied back: the packets of the
    zero rows, the other slots and the guards come back as they were."""
    c = pc.staging_bits(pc.rng_for(7))
    where = {"pageable": ["numpy"] * 5, "pinned": ["pinned"] * 5, "device-to-host": ["device"] * 3 + ["numpy"] * 2,
             "host-to-device": ["numpy"] * 3 + ["device"] * 2}[placement]
    want = run(ec, gpu, c, 3, 16, pc.grow(pc.STAGING_EXPECT), f"staging {placement}", where=where, rng=pc.rng_for(31))
    img = pc.host_image(5, 3 * 5 * 16, [0] * 5, pc.rng_for(31))
    kept = want[3:, GUARD:GUARD + 240].reshape(2, 3, 5, 16)[:, :, 2]
    assert np.array_equal(kept, img[3:, GUARD:GUARD + 240].reshape(2, 3, 5, 16)[:, :, 2])


# ------------------------------------------------------ dotprod and decode ----
def test_bitmatrix_dotprod_with_src_ids(ec, gpu):
    for ids, dest in pc.DOTPRODS:
        c = pc.dotprod_case(3, 2, 3, ids, dest, pc.rng_for(8, dest))
        run(ec, gpu, c, 257, 16, pc.grow(pc.DOTPROD_EXPECT), f"dotprod src_ids={ids} dest_id={dest}", rng=pc.rng_for(32, dest))


@pytest.mark.parametrize("row_k_ones", [0, 1])
def test_bitmatrix_decode_every_erasure_set(ec, gpu, row_k_ones):
    """k = 3, m = 2, w = 3, ps = 8: every set of up to two erased devices comes
    back as the codeword it was, nothing else changes; three erasures return
    -1 and write nothing."""
    import torch
    J = ec.jerasure
    nsp, ps = 257, 8
    bm, clean = pc.decode_codeword(J, nsp, ps, pc.rng_for(10))
    size, offsets = clean.shape[1], [0] * 5
    good = np.full((5, pc.stride_for(size)), FILL, dtype=np.uint8)
    good[:, GUARD:GUARD + size] = clean
    slab, ran = None, 0
    for er in pc.DECODE_SETS + [[0, 2, 4]]:
        img = good.copy()
        img[er, GUARD:GUARD + size] = 0x33
        if slab is None:
            slab = Slab(gpu, img, size, offsets)
        else:
            slab.load(img)
        v = slab.views()
        before = counters(ec)
        rc = J.jerasure_bitmatrix_decode(3, 2, 3, bm.ravel(), row_k_ones, er, v[:3], v[3:], size, ps)
        torch.cuda.synchronize()
        grew = [a - b for a, b in zip(counters(ec), before)]
        label = f"decode erasures={er} row_k_ones={row_k_ones}"
        if len(er) == 3:
            assert rc == -1 and grew == pc.grow(), label
            slab.check(img, label)
        else:
            assert rc == 0 and grew == (pc.grow(pc.DECODE_EXPECT) if er else pc.grow()), (label, rc, grew)
            slab.check(good, label)
        ran += 1
    assert ran == 17
    print(f"ran {ran} erasure sets, row_k_ones={row_k_ones}")
