"""The transforms (the record layout among them), the selectors and the estimates on an input of 4.3 GB: byte offsets past 2^32 and more work than every
strided launch has workgroups (grid_bytes 8,192; grid_frames and k_const_select 2^20; k_mixed_choose 4,096; the estimates, the
CRC, the histograms and k_segment_copy a small multiple of the CU count), so that a workgroup goes on to a second frame, unit
or block with its carry, its totals and its LDS tile as the first one left them.

The input and the rule of the expectations are those of tests/test_past_4gib_cpu.py: eight distinct segments of 512 KiB tiled
on the device 8,195 times in an order whose only period is 140 positions, and a tail of 4,101 bytes; what a per-granule
operation gives for the buffer is the same tiling of its numpy restatement on the segments, plus the tail's.  Three buffers of
4.3 GB live for the module and are freed at its end, and every reference is computed once, in the module's fixtures.  Every
destination is poisoned before a kernel writes it and lies between guard bands; results are compared on the device, in slabs,
and a failure names the first wrong granule, the distinct segment it lies in and the byte."""
import ctypes as C
import zlib

import numpy as np
import pytest

import test_past_4gib_cpu as T
from test_context_static_cpu import pair_counts
from test_estimate_gpu import TOL
from test_lag_auto_cpu import sampled_columns
from test_lag_cpu import lag_planes_ref
from test_lag_order_gpu import FRONT, bands_intact, on_device_poisoned
from test_layout_auto_cpu import block_counts, transform_ref
from test_plane_static_cpu import plane_counts
from test_planes_gpu import FILL
from test_segment_static_cpu import segment_counts

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
SEG, NSEG, N = T.SEG, T.NSEG, T.N
ORDER = T.order(NSEG)
GUARD = 8  # doubles (or count rows) on either side of a result


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared references are read-only)


class Buffers:
    """three device buffers of N bytes (of T.LARGEST: the record layout's segments of 32 frames tile a few megabytes more)
    between poison (on_device_poisoned), and what each one holds: the tiled input, the tiled base, or nothing that a later
    test may count on.  L: the segment length of the tiling, the shared SEG unless a record size needs its own."""

    def __init__(self, torch):
        self.torch = torch
        self.idx = dev(ORDER)
        self.raw = [on_device_poisoned(torch, T.LARGEST + 16)[0] for _ in range(3)]
        self.holds = [None] * 3
        self.parts = {"x": dev(T.segments()), "base": dev(T.base_segments())}
        self.tail = dev(T.tail_bytes())
        self.orders = {SEG: (self.parts["x"], self.idx)}

    def view(self, i, offset=0, n=N):
        return self.raw[i][FRONT + offset: FRONT + offset + n]

    def intact(self, i, offset=0, n=N):
        return bands_intact(self.raw[i], FRONT + offset, n)

    def poisoned(self, i, offset=0, n=N):
        """buffer i filled with FILL -> its view of n bytes, `offset` bytes off the 256-byte boundary"""
        self.holds[i] = None
        self.raw[i].fill_(FILL)
        return self.view(i, offset, n)

    def order(self, L=SEG):
        """(the distinct segments of length L, which of them lies at each position) on the device"""
        if L not in self.orders:
            self.orders[L] = (dev(T.segments(L)), dev(T.order(T.segment_count(L))))
        return self.orders[L]

    def tiled(self, i, what="x", offset=0, L=SEG):
        """buffer i holding the tiled input ("x": T.total_bytes(L) bytes) or the base ("base": base_length bytes, no tail) -> its view"""
        n = T.total_bytes(L) if what == "x" else T.base_length(8192, SEG)
        if self.holds[i] != (what, offset, L):
            v = self.poisoned(i, offset, n)
            (parts, idx), whole = (self.order(L) if what == "x" else (self.parts[what], self.idx)), n // L
            body = v[: whole * L].view(whole, L)
            step = (512 << 20) // L  # (slabs: a gather of the whole buffer would be a fourth one)
            for f0 in range(0, whole, step):
                body[f0: f0 + step].copy_(parts[idx[f0: min(f0 + step, whole)]])
            rest = self.tail if what == "x" else parts[idx[whole]][: n - whole * L]
            v[whole * L:].copy_(rest)
            self.holds[i] = (what, offset, L)
        return self.view(i, offset, n)


@pytest.fixture(scope="module")
def bufs():
    import torch
    b = Buffers(torch)
    assert len(set(np.diff(np.nonzero((b.idx[:4096] == 0).cpu().numpy())[0]).tolist())) > 4  # (no short period)
    assert N > 1 << 32
    yield b
    del b.raw, b.parts, b.orders, b
    torch.cuda.synchronize()
    torch.cuda.empty_cache()  # (three buffers of 4.3 GB)


def mismatch(bufs, got, parts, granule, what, lo=0, hi=None, tail=None, L=SEG, idx=None):
    """got (device bytes of the whole buffer) against parts[idx[f]] for the positions lo <= f < hi (segments of L bytes) and, if
    given, `tail` behind the last position, on the device in slabs -> None, or what names the first wrong granule"""
    torch, idx = bufs.torch, bufs.idx if idx is None else idx
    nseg = T.segment_count(L)
    hi = nseg if hi is None else hi
    step = (256 << 20) // L
    for f0 in range(lo, hi, step):
        f1 = min(f0 + step, hi)
        g = got[f0 * L: f1 * L].view(-1, L)
        if not torch.equal(g, parts[idx[f0:f1]]):
            f = f0 + int((g != parts[idx[f0:f1]]).any(1).nonzero()[0])
            at = f * L + int((got[f * L: (f + 1) * L] != parts[idx[f]]).nonzero()[0])
            return f"{what} {at // granule} (position {f}, distinct segment {int(idx[f])}) differs at byte {at}"
    if tail is not None and not torch.equal(got[nseg * L:], tail):
        at = nseg * L + int((got[nseg * L:] != tail).nonzero()[0])
        return f"{what} {at // granule} (the tail) differs at byte {at}"
    return None


# ---- the references: the numpy restatements of the eight segments and the tail, once for the module ---------------------------
def per_segment(fn):
    """fn of every distinct segment, stacked, and of the tail -> two device tensors"""
    return dev(np.stack([fn(s) for s in T.segments()])), dev(fn(T.tail_bytes()))


def tiled_rows(bufs, per, tail):
    """per [8 segments, rows, columns a segment], tail [rows, its columns] on the device -> [rows, columns of the buffer]"""
    return bufs.torch.cat([per[bufs.idx].permute(1, 0, 2).reshape(per.shape[1], -1), tail], dim=1)


@pytest.fixture(scope="module")
def transform_refs():
    """{(name, E, B, inverse): (uint8[8, SEG], the tail's)}"""
    return {(name, E, B, inverse): per_segment(lambda x: T.RESTATEMENTS[name](x, E, B, inverse=inverse))
            for name, E, B in T.TRANSFORMS if name in T.LAYOUT_NAMES for inverse in (False, True)}


@pytest.fixture(scope="module")
def record_refs():
    """{(name, R, B, inverse): (uint8[8, L], the tail's)} for the record layout, L the segment length of the entry"""
    def per(fn, L):
        return dev(np.stack([fn(s) for s in T.segments(L)])), dev(fn(T.tail_bytes()))
    return {(name, R, B, inverse): per(lambda x: T.RESTATEMENTS[name](x, R, B, inverse=inverse), T.segment_length(R * B))
            for name, R, B in T.RECORD_TRANSFORMS for inverse in (False, True)}


@pytest.fixture(scope="module")
def base_refs():
    """{(name, inverse): (under the whole base, under its last quarter of a segment and 7 bytes -- position 8193's segment alone
    --, past the base, the tail)} of the restatement at E = 4, B = 4096"""
    E, B = T.BASE_E, T.BASE_B
    x, y = T.segments(), T.base_segments()
    s, cover = int(ORDER[8193]), T.base_cover(8193, 8192, SEG)
    assert 0 < cover < SEG and cover % (E * B) == 7 and T.base_cover(8192, 8192, SEG) == SEG and T.base_cover(8194, 8192, SEG) == 0
    out = {}
    for name, ref in T.BASE_RESTATEMENTS.items():
        for inverse in (False, True):
            out[name, inverse] = (dev(np.stack([ref(x[i], y[i], E, B, inverse=inverse) for i in range(8)])),
                                  dev(ref(x[s], y[s][:cover], E, B, inverse=inverse)),
                                  *per_segment(lambda v: ref(v, b"", E, B, inverse=inverse)))
    return out


@pytest.fixture(scope="module")
def mixed_refs():
    """{(B, inverse): (uint8[8 layouts, 8 segments, SEG], the eight transforms of the tail)}"""
    return {(B, inverse): (dev(np.stack([np.stack([T.layout_ref(s, k, B, inverse) for s in T.segments()]) for k in range(8)])),
                           [dev(T.layout_ref(T.tail_bytes(), k, B, inverse)) for k in range(8)])
            for B in (4096, 65536) for inverse in (False, True)}


@pytest.fixture(scope="module")
def cost_refs(rx, bufs):
    """the host rule at B = 4096 on the restatements, tiled on the device: block_cost f64[1, nblocks], layout_cost f64[8, nblocks],
    lag_cost (E = 2) f64[4, nblocks]"""
    B = 4096

    def rows(fn):
        cost = lambda x: np.stack([rx.adaptive_cost_from_counts(block_counts(y, B), P) for y in fn(x)])  # noqa: E731
        return tiled_rows(bufs, *per_segment(cost))
    return {"block": rows(lambda x: [x]), "layout": rows(lambda x: [transform_ref(x, k, B) for k in range(8)]),
            "lag": rows(lambda x: [lag_planes_ref(x, 2, B, S) for S in T.LAGS])}


@pytest.fixture(scope="module")
def count_refs():
    """the histograms at B = 4096 on the host: plane (E = 4) and context totals -- the per-segment counts times how often each
    segment occurs, plus the tail's --, and the segment-static rows (E = 2, ranges of a segment), tiled"""
    times = np.bincount(ORDER, minlength=8).astype(np.uint64)

    def summed(fn):
        return (np.stack([fn(s) for s in T.segments()]) * times[:, None, None]).sum(0) + fn(T.tail_bytes())
    per = np.stack([segment_counts(s, 2, 4096, T.SEGMENT_BLOCKS) for s in T.segments()])
    return {"plane": summed(lambda x: plane_counts(x, 4, 4096)), "context": summed(lambda x: pair_counts(x, 4096)),
            "segment": np.concatenate([per[ORDER].reshape(-1, 256), segment_counts(T.tail_bytes(), 2, 4096, T.SEGMENT_BLOCKS)])}


# ---- 1. planes, delta_planes, zigzag_planes -------------------------------------------------------------------------------
# (name, E, B, offset of the source from a 16-byte boundary)
TRANSFORM_CASES = [(name, E, B, 0) for name, E, B in T.TRANSFORMS if name in T.LAYOUT_NAMES and ((E, B) != (2, 4096) or name == "planes")] + \
                  [(name, 2, 4096, 1) for name in T.LAYOUT_NAMES] + [("delta", 1, 4096, 1), ("zigzag", 1, 4096, 1)]


@pytest.mark.parametrize("name,E,B,off", TRANSFORM_CASES)
def test_layout_transforms(rx, bufs, transform_refs, name, E, B, off):
    """Aligned, B = 4096 at the smallest E the call takes: 2^20 + 384 frames at E = 1, where a workgroup of k_delta_unplanes
    takes a second frame, and those frames lie past 2^32; the forward kernels and k_planes have a workgroup per 256 groups, the
    last of them past 2^32.  E = 8, B = 65536: a frame is a whole segment, 16 rows of the inverse.  One byte off: the byte
    kernels, forward a thread per byte striding from 8,192 workgroups, inverse a workgroup per frame, every offset past 2^32.
    At E = 2 those are 2^19 + 192 frames of 8 KiB, fewer than the 2^20 workgroups of grid_frames; the filters run at E = 1 too,
    where 384 workgroups of k_delta_unplanes_bytes go on to a second frame.  Forward and inverse against the tiled restatement,
    and the inverse's result through the forward kernel against the source."""
    call = getattr(rx, name if name == "planes" else name + "_planes")
    frame = E * B
    src = bufs.tiled(0, "x", off)
    for inverse in (False, True):
        dst = bufs.poisoned(1)
        call(src, E, B, inverse=inverse, out=dst)
        assert bufs.intact(1) and bufs.intact(0, off), (name, E, B, off, inverse)
        want, want_tail = transform_refs[name, E, B, inverse]
        bad = mismatch(bufs, dst, want, frame, "inverse=%s: frame" % inverse, tail=want_tail)
        assert bad is None, bad
    back = bufs.poisoned(2)
    call(dst, E, B, inverse=False, out=back)  # (dst: the inverse's result)
    assert bufs.intact(2) and bufs.intact(1)
    bad = mismatch(bufs, back, bufs.parts["x"], frame, "forward of the inverse: frame", tail=bufs.tail)
    assert bad is None, bad


# ---- 1b. record_planes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,R,B", T.RECORD_TRANSFORMS)
def test_record_layout(rx, bufs, record_refs, name, R, B):
    """The record layout (T.RECORD_TRANSFORMS says what each entry is there for): fbase = f * R * B, p * B and frame_pos past
    2^32; 8 * CUs workgroups of the fast kernels striding over 2^16 frames and more; at B = 4100 and 2036 the byte kernels from
    byte 0, forward a thread per byte and the delta inverse a thread per (frame, column) striding from 8,192 workgroups.
    Record sizes whose frames divide no power of two are tiled from segments of 32 frames.  Forward and inverse against the
    tiled restatement, and the inverse's result through the forward kernel against the source."""
    from redux_amd import api
    delta = name == "record_delta"
    L = T.segment_length(R * B)
    n = T.total_bytes(L)
    parts, idx = bufs.order(L)
    tail = bufs.tail
    src = bufs.tiled(0, "x", 0, L)
    assert src.numel() == n > 1 << 32
    for inverse in (False, True):
        fast = api.record_plan(n, B, R, delta, inverse).grid_fast
        kernel = "k_record_unplanes" if inverse else "k_record_planes"
        assert api.record_kernel_name(n, B, R, inverse, d_src=src, d_dst=bufs.view(1, 0, n)) == \
            (kernel + " + " + kernel + "_bytes" if fast else kernel + "_bytes")
        assert bool(fast) == (B % 16 == 0)
        dst = bufs.poisoned(1, 0, n)
        api.record_planes(src, R, B, delta=delta, inverse=inverse, out=dst)
        assert bufs.intact(1, 0, n) and bufs.intact(0, 0, n), (name, R, B, inverse)
        want, want_tail = record_refs[name, R, B, inverse]
        bad = mismatch(bufs, dst, want, R * B, "R=%d B=%d %s inverse=%s: frame" % (R, B, name, inverse), tail=want_tail, L=L, idx=idx)
        assert bad is None, bad
    back = bufs.poisoned(2, 0, n)
    api.record_planes(dst, R, B, delta=delta, inverse=False, out=back)  # (dst: the inverse's result)
    assert bufs.intact(2, 0, n) and bufs.intact(1, 0, n)
    bad = mismatch(bufs, back, parts, R * B, "R=%d B=%d %s forward of the inverse: frame" % (R, B, name), tail=tail, L=L, idx=idx)
    assert bad is None, bad


# ---- 2. base_planes, base_sub_planes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "base_sub"])
@pytest.mark.parametrize("off", [0, 1])
def test_base_filters(rx, bufs, base_refs, name, off):
    """E = 4, B = 4096; the base ends 1.25 segments and 7 bytes past 2^32, inside a frame and an element, and short of the
    input's end.  All three pointers aligned: the fused kernels up to the last full frame of the base (their last workgroups past
    2^32), the byte kernels for the frame the base ends in, k_planes<4> from a.end > 2^32 on.  The base one byte off: the byte
    kernels from byte 0 to a.end, striding from 8,192 workgroups.  Both directions."""
    call = getattr(rx, name + "_planes")
    E, B = T.BASE_E, T.BASE_B
    src = bufs.tiled(0, "x")
    base = bufs.tiled(1, "base", off)
    assert base.numel() == T.base_length(8192, SEG) > 1 << 32 and base.numel() < N - SEG
    for inverse in (False, True):
        dst = bufs.poisoned(2)
        call(src, base, E, B, inverse=inverse, out=dst)
        assert bufs.intact(2) and bufs.intact(0) and bufs.intact(1, off, base.numel()), (name, off, inverse)
        under, partial, past, tail = base_refs[name, inverse]
        what = "inverse=%s: frame" % inverse
        bad = mismatch(bufs, dst, under, E * B, what, 0, 8193)
        assert bad is None, bad
        f = 8193
        if not bufs.torch.equal(dst[f * SEG: (f + 1) * SEG], partial):
            at = f * SEG + int((dst[f * SEG: (f + 1) * SEG] != partial).nonzero()[0])
            raise AssertionError(f"{what} {at // (E * B)} (position {f}, where the base ends at byte {base.numel()}) differs at byte {at}")
        bad = mismatch(bufs, dst, past, E * B, what + " past the base", 8194, NSEG, tail=tail)
        assert bad is None, bad


# ---- 3. mixed_layout and choose_unit_layouts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,off", [(65536, 0), (4096, 0), (4096, 1)])
def test_mixed_layout(rx, bufs, mixed_refs, B, off):
    """B = 4096: one workgroup per unit, 2^17 + 48 units; B = 65536: 16 per unit, rotated by the unit index; the unit bases past
    2^32.  One byte off: k_mixed_bytes, forward a thread per byte from 8,192 workgroups, inverse a workgroup per unit from
    `first`.  The table is random bytes; the reference the splice of the per-segment restatements of the eight layouts."""
    torch = bufs.torch
    U = 8 * B
    ups, nunits = SEG // U, rx.mixed_units(N, B)
    assert nunits == NSEG * ups + 1
    table = T.unit_table(nunits)
    d_table = dev(table)
    k_of = (d_table & 7).long()
    src = bufs.tiled(0, "x", off)
    dst = bufs.view(1)
    u = torch.arange(NSEG * ups, device="cuda:0")
    flat = (k_of[: NSEG * ups] * 8 + bufs.idx[u // ups]) * ups + u % ups  # the unit of refs[k, s] that unit u must equal
    for inverse in (False, True):
        i = int(inverse)
        fast, general = "k_mixed_planes<%d>" % i, "k_mixed_bytes<%d>" % i
        assert rx.api.mixed_kernel_name(src, dst, B, inverse=inverse) == (general if off else fast + " + " + general)
        dst = bufs.poisoned(1)
        rx.mixed_layout(src, d_table, B, inverse=inverse, out=dst)
        assert bufs.intact(1) and bufs.intact(0, off), (B, off, inverse)
        refs, tails = mixed_refs[B, inverse]
        refs, got = refs.view(-1, U), dst[: NSEG * SEG].view(-1, U)
        step = (256 << 20) // U
        for u0 in range(0, NSEG * ups, step):
            want = refs[flat[u0: u0 + step]]
            if not torch.equal(got[u0: u0 + step], want):
                un = u0 + int((got[u0: u0 + step] != want).any(1).nonzero()[0])
                at = un * U + int((got[un] != refs[flat[un]]).nonzero()[0])
                raise AssertionError(f"inverse={inverse}: unit {un} (layout {int(k_of[un])}, position {un // ups}, distinct segment "
                                     f"{int(bufs.idx[un // ups])}) differs at byte {at}")
        assert torch.equal(dst[NSEG * SEG:], tails[int(table[-1]) & 7]), "inverse=%s: the tail's unit" % inverse


@pytest.mark.parametrize("mask", [0xFF, 0xA6])
def test_choose_unit_layouts_past_the_grid_cap(rx, mask):
    """8 (2^20 + 5) + 3 blocks of synthetic bits: 2^20 + 6 units, the last of 3 blocks, where k_mixed_choose has 4,096 workgroups
    of 256 threads -- six units are a thread's second.  Ties are planted (the lower layout wins); all layouts and a mask with
    holes; the sum of the chosen units exactly, as the integer of 2^-16 bit the kernel adds up.  The reference is choose_vec,
    choose_ref's additions on the device (tests/test_past_4gib_cpu.py holds the two equal)."""
    import torch
    nb = 8 * ((1 << 20) + 5) + 3
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(20)
    bits = torch.rand((8, nb), dtype=torch.float64, device="cuda:0", generator=gen) * 499900.0 + 100.0
    bits[5] = bits[1]                                   # exact ties -> the lower k
    bits[2, : nb // 2] = bits[6, : nb // 2]
    bits[1, ::3] *= 0.5                                 # (so that the tied rows win some units)
    bits[5, ::3] = bits[1, ::3]
    bits[3, -11:] = 50.0                                # the last full unit and the short one: layout 3, or 7 under the mask
    bits[7, -11:] = 50.0
    table, total = rx.choose_unit_layouts(bits, mask)
    want, units = T.choose_vec(torch, bits, mask)
    want = want.cpu().numpy()
    assert table.dtype == np.uint8 and table.shape == want.shape == ((1 << 20) + 6,)
    if not np.array_equal(table, want):
        un = int(np.nonzero(table != want)[0][0])
        raise AssertionError(f"mask {mask:#x}: unit {un} chose layout {table[un]}, the restatement {want[un]}")
    assert total == float(units) / 65536.0, (mask, total, units)
    assert table[-1] == table[-2] == (3 if mask == 0xFF else 7)
    assert set(want.tolist()) == ({0, 1, 2, 3, 4, 6, 7} if mask == 0xFF else {1, 2, 7})  # (5 ties with 1 everywhere: never)


# ---- 4. constant_blocks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1024, 4096])
def test_constant_blocks(rx, bufs, B):
    """B = 1024: 2^22 + 1,541 blocks, more than k_const_select's 2^20 workgroups of four waves take in one pass, so a wave goes on
    to a second block; B = 4096: 2^20 + 386 blocks, the block offsets past 2^32."""
    torch = bufs.torch
    src = bufs.tiled(0, "x")
    flags = rx.constant_blocks(src, B)
    per, tail = per_segment(lambda x: T.const_ref(x, B))
    want = torch.cat([per[bufs.idx].reshape(-1), tail])
    assert bufs.intact(0) and flags.dtype == torch.uint8 and flags.shape == want.shape == (-(-N // B),)
    assert 0 < int(want.sum()) < want.numel()
    if not torch.equal(flags, want):
        b = int((flags != want).nonzero()[0])
        raise AssertionError(f"block {b} (position {b * B // SEG}, distinct segment {int(ORDER[min(b * B // SEG, NSEG - 1)])}, "
                             f"byte {b * B}): flag {int(flags[b])}, the restatement {int(want[b])}")


# ---- 5. crc32_blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4096, SEG])
def test_crc32_blocks(rx, bufs, B):
    """the device tensor where it lies: 2^20 + 386 blocks of 4096 bytes at four lanes a block, 8,196 of 512 KiB in segments of
    the kernel's own; b * block_size past 2^32, and more items than the launch has workgroups"""
    src = bufs.tiled(0, "x")
    got = rx.crc32_blocks(src, B)
    per = np.stack([T.block_crcs(s, B) for s in T.segments()])
    want = np.concatenate([per[ORDER].reshape(-1), T.block_crcs(T.tail_bytes(), B)])
    assert want[-1] == zlib.crc32(T.tail_bytes()[-(T.TAIL % B):].tobytes())
    assert got.dtype == np.uint32 and got.shape == want.shape
    if not np.array_equal(got, want):
        b = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"block {b} (position {b * B // SEG}, byte {b * B}): CRC {got[b]:#010x}, zlib {want[b]:#010x}")


# ---- 6. block_cost, layout_cost, lag_cost -------------------------------------------------------------------------------------
def guarded_rows(torch, rows, nb):
    """a NaN-filled result of rows * nb doubles between NaN guards -> (whole tensor, pointer to the result)"""
    out = torch.full((rows * nb + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    return out, C.c_void_p(out.data_ptr() + 8 * GUARD)


def assert_rows(torch, out, want, B, what, only=None):
    """the guarded result against want f64[rows, nb] on the device, within TOL bits; only: the rows that were asked for (the
    others must still be NaN)"""
    rows, nb = want.shape
    assert bool(torch.isnan(out[:GUARD]).all()) and bool(torch.isnan(out[GUARD + rows * nb:]).all()), "guard words around d_bits were written"
    got = out[GUARD: GUARD + rows * nb].view(rows, nb)
    for r in range(rows):
        if only is not None and r not in only:
            assert bool(torch.isnan(got[r]).all()), "row %d was written without being asked for" % r
            continue
        err = (got[r] - want[r]).abs()
        ok = err <= TOL  # (a block that was not written is NaN: not ok)
        if not bool(ok.all()):
            b = int((~ok).nonzero()[0])
            raise AssertionError(f"{what}: row {r}, block {b} (byte {b * B}, distinct segment {int(ORDER[min(b * B // SEG, NSEG - 1)])}): "
                                 f"{float(got[r, b])!r} bits, the host rule {float(want[r, b])!r}")
        print("%s, row %d: max |device - host rule| = %.3g bits over %d blocks" % (what, r, float(err.max()), nb))


@pytest.mark.parametrize("off", [0, 1])
def test_block_cost(lib, bufs, cost_refs, off):
    """k_block_cost, B = 4096: 2^20 + 386 blocks where the launch has a few workgroups per CU, the input past 2^32"""
    torch, L, B = bufs.torch, lib.lib(), 4096
    src = bufs.tiled(0, "x", off)
    nb = L.redux_block_count(N, B)
    out, ptr = guarded_rows(torch, 1, nb)
    cp = lib.Params(*P)
    assert L.redux_block_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), N, B, ptr, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == lib.OK
    assert_rows(torch, out, cost_refs["block"], B, "block_cost, +%d" % off)
    assert bufs.intact(0, off)


@pytest.mark.parametrize("off,mask", [(0, 0xFF)] + [(1, 1 << k) for k in range(8)])
def test_layout_cost(lib, bufs, cost_refs, off, mask):
    """B = 4096, the rows at k * nblocks, the input past 2^32.  Aligned, all eight rows in one call: k_layout_cost<E, 2> on a grid
    of two workgroups a CU, k_layout_cost_bytes for the tail's frame.  One byte off, k_layout_cost_bytes for everything: the eight
    rows one call each."""
    torch, L, B = bufs.torch, lib.lib(), 4096
    src = bufs.tiled(0, "x", off)
    for k in range(8):
        E = 1 << (k & 3)
        fast, general = b"k_layout_cost<%d>" % E, b"k_layout_cost_bytes<%d>" % E
        assert L.redux_layout_cost_kernel_name_at(C.c_void_p(src.data_ptr()), N, B, k) == (general if off else fast + b" + " + general)
    nb = L.redux_block_count(N, B)
    out, ptr = guarded_rows(torch, 8, nb)
    cp = lib.Params(*P)
    assert L.redux_layout_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), N, B, mask, ptr,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)) == lib.OK
    assert_rows(torch, out, cost_refs["layout"], B, "layout_cost, +%d" % off, only=[k for k in range(8) if mask >> k & 1])
    assert bufs.intact(0, off)


@pytest.mark.parametrize("off,step", [(0, 1), (0, T.LAG_STEP), (1, T.LAG_STEP), (1, 1)])
def test_lag_cost(lib, bufs, cost_refs, off, step):
    """E = 2, B = 4096, lags 1, 3, 256 and 3 again: k_lag_cost on one workgroup a CU, k_lag_cost_bytes for the tail's frame or,
    one byte off, for everything.  Every frame, and every 40th: frames on both sides of 2^32 and the tail's.  (One byte off at
    every frame is the slowest case of the module: one launch of k_lag_cost_bytes, a quarter of a second.)"""
    torch, L, E, B = bufs.torch, lib.lib(), 2, 4096
    src = bufs.tiled(0, "x", off)
    fast, general = b"k_lag_cost<2>", b"k_lag_cost_bytes<2>"
    assert L.redux_lag_cost_kernel_name_at(C.c_void_p(src.data_ptr()), N, B, E) == (general if off else fast + b" + " + general)
    nblocks = L.redux_block_count(N, B)
    nb = L.redux_lag_cost_block_count(N, B, E, step)
    want = cost_refs["lag"]
    if step == 1:
        assert nb == nblocks == want.shape[1]
    else:
        cols = sampled_columns(nblocks, E, step)
        assert nb == len(cols) and cols[-2:] == [nblocks - 2, nblocks - 1]  # (the tail's frame)
        assert min(c for c in cols if c * B >= 1 << 32) == (1 << 20) + 64 and max(c for c in cols if c * B < 1 << 32) == (1 << 20) - 15
        want = want[:, torch.tensor(cols, device="cuda:0")]
    out, ptr = guarded_rows(torch, len(T.LAGS), nb)
    cp = lib.Params(*P)
    h_lags = np.asarray(T.LAGS, dtype=np.uint32)
    assert L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), N, B, E, h_lags.ctypes.data, len(T.LAGS), step, ptr,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)) == lib.OK
    assert_rows(torch, out, want, B, "lag_cost, +%d, every %d frames" % (off, step))
    got = out[GUARD: GUARD + len(T.LAGS) * nb].view(len(T.LAGS), nb)
    assert torch.equal(got[1], got[3]) and bufs.intact(0, off)  # (the repeated lag: equal, independent rows)


# ---- 7. the histograms ------------------------------------------------------------------------------------------------------
def counted(bufs, lib, nrows, call):
    """nrows count rows of 256, zeroed, between GUARD rows that must stay zero, as api.py hands them to a `_dev` histogram"""
    torch = bufs.torch
    counts = torch.zeros((nrows + 2 * GUARD) * 256, dtype=torch.int64, device="cuda:0")
    src = bufs.tiled(0, "x")
    st = call(C.c_void_p(src.data_ptr()), C.c_void_p(counts.data_ptr() + GUARD * 256 * 8), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.OK
    h = counts.cpu().numpy().reshape(-1, 256)
    assert not h[:GUARD].any() and not h[GUARD + nrows:].any() and bufs.intact(0)
    return h[GUARD: GUARD + nrows].astype(np.uint64)


def test_plane_histogram(lib, bufs, count_refs):
    """k_plane_hist, E = 4, B = 4096: block b's bytes to table b mod 4, the blocks past 2^32"""
    L, E, B = lib.lib(), 4, 4096
    got = counted(bufs, lib, E, lambda x, c, s: L.redux_plane_histogram_dev(x, N, B, E, c, None, 0, s))
    want = count_refs["plane"]
    assert int(want.sum()) == N and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


def test_segment_histogram(lib, bufs, count_refs):
    """k_segment_hist, E = 2, B = 4096, ranges of 128 blocks: a range is a segment, so the 16,392 count rows are the tiling of the
    segments' own two rows, and the tail's"""
    L, E, B, G = lib.lib(), 2, 4096, T.SEGMENT_BLOCKS
    ntables = L.redux_segment_static_table_count(L.redux_block_count(N, B), E, G)
    assert ntables == (NSEG + 1) * E
    got = counted(bufs, lib, ntables, lambda x, c, s: L.redux_segment_histogram_dev(x, N, B, E, G, c, s))
    want = count_refs["segment"]
    if not np.array_equal(got, want):
        t = int(np.nonzero((got != want).any(1))[0][0])
        raise AssertionError(f"table {t} (range {t // E}, distinct segment {int(ORDER[min(t // E, NSEG - 1)])}, plane {t % E}): "
                             f"{int(got[t].sum())} bytes counted, {int(want[t].sum())} lie there")


def test_context_histogram(lib, bufs, count_refs):
    """k_context_hist, B = 4096: the pair counts, a block's first byte under context 0"""
    L, B = lib.lib(), 4096
    got = counted(bufs, lib, 256, lambda x, c, s: L.redux_context_histogram_dev(x, N, B, c, s))
    want = count_refs["context"]
    assert int(want.sum()) == N and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()


# ---- 8. segment_copy --------------------------------------------------------------------------------------------------------
def test_segment_copy(rx, bufs):
    """Source and destination longer than 2^32 bytes; 64 segments of 1 byte to 8 MiB, one across 2^32 in the source and one in
    the destination, all 16 relative phases of source and destination beyond 2^32 (the 1.5 MiB there hold the small ones), more
    tiles than the 8 workgroups a CU the launch has.  The source holds the byte values 0 .. 254 and the destination 255: what is
    not 255 afterwards was copied."""
    torch = bufs.torch
    src = bufs.tiled(1, "x")
    bufs.holds[1] = None
    src.clamp_(max=254)
    dst = bufs.poisoned(2)
    dst.fill_(255)
    edge = 1 << 32
    segs = [(edge - 70001, 5 << 20, 1 << 20), (3 << 20, edge - 12345, 200001)]
    far = [1, 15, 16, 17, 4097, 65535, 65536, 65537, 33, 100003, 250007, 31, 64, 129, 200001, 3]
    s, d = edge + 16, edge + (192 << 10)
    for phase, n in enumerate(far):  # source phase - destination phase = 0 .. 15, both past 2^32
        segs.append((s + phase, d, n))
        s, d = s + (n + 31) // 16 * 16, d + (n + 15) // 16 * 16
    sizes = [1, 17, 65537, (3 << 20) + 1, (5 << 20) - 7, (6 << 20) + 65, (7 << 20) + 5, (8 << 20) + 3]
    i, s, d = 0, 64 << 20, 128 << 20  # the rest below 2^32, the destination at any phase
    while len(segs) < 64:
        n = sizes[i % len(sizes)]
        segs.append((s, d + i % 16, n))
        s, d, i = s + n + 7, d + n + 16 + 5, i + 1
    assert all(a + n <= N and b + n <= N for a, b, n in segs)
    assert {(a - b) % 16 for a, b, n in segs if a >= edge and b >= edge} == set(range(16))
    spans = sorted((b, b + n) for _, b, n in segs)
    assert all(spans[j][1] <= spans[j + 1][0] for j in range(len(spans) - 1))
    assert len(rx.segment_tiles(segs)) > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    rx.segment_copy(src, dst, segs)
    torch.cuda.synchronize()
    assert bufs.intact(2) and bufs.intact(1)
    for a, b, n in segs:
        if not torch.equal(dst[b: b + n], src[a: a + n]):
            at = int((dst[b: b + n] != src[a: a + n]).nonzero()[0])
            raise AssertionError(f"segment ({a}, {b}, {n}) differs at its byte {at}: destination byte {b + at}")
    copied = torch.zeros((), dtype=torch.int64, device="cuda:0")
    for o in range(0, N, 256 << 20):
        copied += (dst[o: o + (256 << 20)] != 255).sum()
    assert int(copied) == sum(n for _, _, n in segs)
