"""The input of tests/test_past_4gib_gpu.py and the rule its expectations rest on, without a GPU.

One buffer is tiled from eight distinct segments in an aperiodic order, with a short tail of its own bytes behind them.  A
segment is a whole number of every granule the device tests use (a frame, a unit of 8 blocks, a block, a segment-static range),
and granules start afresh, so the result of a per-granule operation on the buffer is the same tiling of its results on the
segments, plus the tail's.  That rule is what lets a 4.3 GB expectation be eight restatements of 512 KiB; here it is checked
for every operation of the GPU file, byte for byte and count for count, on a tiling of three segments of two granules each:
a wrong expectation must neither pass as a kernel bug nor hide one."""
import functools
import zlib

import numpy as np
import pytest

from test_base_cpu import base_planes_ref
from test_base_sub_cpu import base_sub_planes_ref
from test_const_cpu import const_ref
from test_context_static_cpu import pair_counts
from test_delta_cpu import delta_planes_ref
from test_delta_gpu import series
from test_lag_auto_cpu import sampled_columns
from test_lag_cpu import lag_planes_ref
from test_layout_auto_cpu import block_counts, transform_ref
from test_mixed_cpu import choose_ref, mixed_ref
from test_mixed_gpu import typed
from test_plane_static_cpu import plane_counts
from test_planes_cpu import planes_ref
from test_record_cpu import record_ref
from test_segment_static_cpu import segment_counts
from test_zigzag_cpu import zigzag_planes_ref

SEG = 512 << 10           # a segment of the big buffer: every granule below divides it
NSEG = 8192 + 3           # 2^32 bytes of segments and three more
TAIL = 4096 + 5           # the tail: a full block of 4096 and a short one
N = NSEG * SEG + TAIL
UNIT = 8
LAGS = [1, 3, 256, 3]     # of the lag estimates (a repeated lag at the end)
LAG_STEP = 40             # frames 0, 40, 80, ... of 8 KiB: 320 frames are 5 segments, so every offset in a segment that is a
#                           multiple of 8 frames is selected somewhere; frame 524,320 is the first one past 2^32, and the tail's
#                           frame, 524,480, is selected too
SEGMENT_BLOCKS = 128      # segment-static ranges at E = 2: 64 * E blocks of 4096 bytes, 512 KiB

# (name, restatement, E, B): the transforms of the GPU file.  The smallest E each call takes at B = 4096; E = 8 at B = 65536,
# where a frame is a whole segment; E = 2 at B = 4096 for the byte path
RESTATEMENTS = {"planes": planes_ref, "delta": delta_planes_ref, "zigzag": zigzag_planes_ref}
TRANSFORMS = [("planes", 2, 4096), ("planes", 8, 65536),
              ("delta", 1, 4096), ("delta", 8, 65536), ("delta", 2, 4096),
              ("zigzag", 1, 4096), ("zigzag", 8, 65536), ("zigzag", 2, 4096)]
# ... and the record layout, (name, R, B): the fast path with frames of 64 KiB; a frame that is a whole segment, far more
# frames than 8 * CUs workgroups; B no multiple of 16, so the byte kernels take everything: forward more bytes than grid_bytes
# has threads; at B = 2036 the delta inverse has more (frame, column) pairs than that too (at B = 4100 it has half as many);
# R = 3 and 23, whose frames divide no power of two
LAYOUT_NAMES = tuple(RESTATEMENTS)
RESTATEMENTS["record"] = lambda x, R, B, inverse=False: record_ref(x, R, B, False, inverse)
RESTATEMENTS["record_delta"] = lambda x, R, B, inverse=False: record_ref(x, R, B, True, inverse)
RECORD_TRANSFORMS = [("record_delta", 16, 4096), ("record", 256, 2048), ("record_delta", 256, 2048),
                     ("record", 4, 4100), ("record_delta", 4, 4100), ("record_delta", 4, 2036), ("record_delta", 3, 4096),
                     ("record_delta", 23, 4096)]
TRANSFORMS += RECORD_TRANSFORMS
BASE_RESTATEMENTS = {"base": base_planes_ref, "base_sub": base_sub_planes_ref}


def segment_length(granule):
    """the segment a granule is tiled with: the shared one where the granule divides it, 32 granules where it does not"""
    return SEG if SEG % granule == 0 else 32 * granule


def segment_count(L=SEG):
    """2^32 bytes of segments, rounded up, and three more"""
    return -(-(1 << 32) // L) + 3


def total_bytes(L=SEG):
    return segment_count(L) * L + TAIL


LARGEST = max(total_bytes(segment_length(R * B)) for _, R, B in RECORD_TRANSFORMS)   # what a buffer of the GPU file has to hold
BASE_E, BASE_B = 4, 4096


def order(nseg):
    """which distinct segment lies at position f: the order of the lag tests (its only period is 140 positions)"""
    f = np.arange(nseg, dtype=np.int64)
    return (f * f // 7 + f // 5 + f) % 8


def constant_segment(L):
    """L bytes in groups of four blocks of 1024 bytes: a group of one value (constant at B = 4096 too), a group of noise, a
    group of four different constant blocks, a group of the NEXT group's value (equal neighbours); group 4 is constant but for
    its last byte and group 8 but for byte 17.  (An L that is no multiple of 1024, as the record layout's segments at B = 4100
    are: the first L bytes of the next multiple.)"""
    if L % 1024:
        return constant_segment(-(-L // 1024) * 1024)[:L].copy()
    rng = np.random.default_rng(1024)
    x = np.empty(L, dtype=np.uint8)
    value = lambda q: (q * 37 + 11) & 0xFF  # noqa: E731
    for j in range(L // 1024):
        q, blk = j // 4, x[j * 1024: (j + 1) * 1024]
        if q % 4 == 0:
            blk[:] = value(q)
        elif q % 4 == 1:
            blk[:] = rng.integers(0, 256, 1024, dtype=np.uint8)
        elif q % 4 == 2:
            blk[:] = (value(q) + j) & 0xFF
        else:
            blk[:] = value(q + 1)
    if L >= 5 * 4096:
        x[5 * 4096 - 1] ^= 0x01
    if L >= 9 * 4096:
        x[8 * 4096 + 17] ^= 0x80
    return x


@functools.lru_cache(maxsize=None)
def segments(L=SEG):
    """uint8[8, L], read-only: three of iid bytes, three typed series (the delta carries are not noise), one with constant
    blocks in it, one of a single byte value"""
    rng = np.random.default_rng(L)
    out = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(3)]
    out += [series(L, seed=3), typed(L, seed=5), series(L, seed=11)]
    out += [constant_segment(L), np.full(L, 0x5A, dtype=np.uint8)]
    x = np.stack(out)
    assert x.shape == (8, L) and len({s.tobytes() for s in x}) == 8
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def base_segments(L=SEG):
    """uint8[8, L], read-only: segments(L) with one byte in eight moved by 1 .. 3 -- a related buffer for the base filters"""
    rng = np.random.default_rng(L + 1)
    y = segments(L).copy()
    y += (rng.random(y.shape) < 0.125) * rng.integers(1, 4, y.shape, dtype=np.uint8)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def tail_bytes(n=TAIL):
    t = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
    t.setflags(write=False)
    return t


def base_length(nwhole, L):
    """the base ends 1.25 segments and 7 bytes past segment nwhole's start: inside a frame (E = 4, B = 4096), inside an element"""
    return nwhole * L + L * 5 // 4 + 7


def base_cover(f, nwhole, L):
    """the bytes of the base under the segment at position f"""
    return int(min(max(base_length(nwhole, L) - f * L, 0), L))


def tile(parts, idx, tail):
    """the buffer: parts[idx[0]], parts[idx[1]], ..., tail"""
    return np.concatenate([parts[i] for i in idx] + [tail])


def tiled(fn, parts, idx, tail, axis=0):
    """the rule: the result of the per-granule operation fn on tile(parts, idx, tail), from fn of each distinct part and of the
    tail (joined along `axis`: bytes, flags and count rows along 0, the blocks of cost rows along 1)"""
    per = [fn(p) for p in parts]
    return np.concatenate([per[i] for i in idx] + [fn(tail)], axis=axis)


def layout_ref(x, k, B, inverse=False):
    """transform_ref, and its inverse: layout k = 4 F + log2 E"""
    if not inverse:
        return transform_ref(x, k, B)
    return (delta_planes_ref if k >= 4 else planes_ref)(x, 1 << (k & 3), B, inverse=True)


def unit_table(nunits, seed=7):
    """random bytes, high bits set in most: the kernels take an entry & 7"""
    t = np.random.default_rng(seed).integers(0, 256, nunits, dtype=np.uint8)
    assert (t > 7).any()
    return t


def mixed_splice(refs, tail_refs, idx, table, L, B):
    """the mixed transform of tile(parts, idx, tail) from refs[k][s] = layout k of distinct segment s and tail_refs[k]: unit u
    under table[u] & 7"""
    U = UNIT * B
    ups = L // U
    out = [refs[int(table[f * ups + j]) & 7][s][j * U: (j + 1) * U] for f, s in enumerate(idx) for j in range(ups)]
    return np.concatenate(out + [tail_refs[int(table[len(idx) * ups]) & 7]])


def block_crcs(x, B):
    return np.array([zlib.crc32(x[o: o + B].tobytes()) for o in range(0, len(x), B)], dtype=np.uint32)


def choose_sum_units(S, table):
    """what k_mixed_choose adds up: every chosen sum in 2^-16 bit, rounded half up, as an exact integer.  The scaling is a
    power of two and so exact; the one rounding is that of + 0.5, the same in any IEEE arithmetic, fused or not."""
    chosen = S[table, np.arange(len(table))]
    return int(np.floor(chosen * 65536.0 + 0.5).astype(np.uint64).sum(dtype=np.uint64))


def choose_vec(torch, bits, mask=0xFF):
    """choose_ref and choose_sum_units on a torch tensor f64[8, nblocks], where it lies: the same additions in the same order
    (a short last unit is padded with + 0.0, which changes no sum), the first smallest selected layout
    -> (uint8[nunits], the chosen sums in 2^-16 bit as one exact int)"""
    nb = bits.shape[1]
    nunits = -(-nb // UNIT)
    b = torch.zeros((8, nunits * UNIT), dtype=torch.float64, device=bits.device)
    b[:, :nb] = bits
    b = b.view(8, nunits, UNIT)
    best = torch.full((nunits,), float("inf"), dtype=torch.float64, device=bits.device)
    pick = torch.full((nunits,), 8, dtype=torch.uint8, device=bits.device)
    for k in range(8):
        if mask >> k & 1:
            s = torch.zeros(nunits, dtype=torch.float64, device=bits.device)
            for j in range(UNIT):
                s = s + b[k, :, j]
            better = (s < best) | (pick == 8)
            best, pick = torch.where(better, s, best), torch.where(better, torch.full_like(pick, k), pick)
    return pick, int(torch.floor(best * 65536.0 + 0.5).to(torch.int64).sum())


# ---- the small tiling: three positions, two granules a segment, and the tail -------------------------------------------
SMALL = (4, 6, 1)  # a typed series, the constant blocks, iid bytes


def small(L, parts=segments):
    return parts(L)[list(SMALL)], np.arange(3), tail_bytes()


def test_the_order_has_no_short_period():
    idx = order(NSEG)
    assert len(set(np.diff(np.nonzero(idx[:4096] == 0)[0]).tolist())) > 4
    assert set(idx.tolist()) == set(range(8)) and np.bincount(idx).min() > 500
    for period in range(1, 140):  # (140 = 4 * 5 * 7 is the shortest: no divisor of a grid cap, a die count or a wave count)
        assert not np.array_equal(idx[period:2048 + period], idx[:2048]), period
    assert np.array_equal(idx[140:], idx[:-140]) and (1 << 20) % 140 and 8192 % 140 and 4096 % 140
    assert len({int(idx[w]) for w in range(4)} | {int(idx[8192 + w]) for w in range(3)}) > 2
    assert N > 1 << 32 and 8192 * SEG == 1 << 32


def test_every_granule_divides_a_segment():
    for E, B in [(1, 4096), (2, 4096), (4, 4096), (8, 4096), (8, 65536)]:
        assert SEG % (E * B) == 0
    assert SEG % (UNIT * 4096) == 0 and SEG % (UNIT * 65536) == 0 and SEG % 1024 == 0
    assert SEG == SEGMENT_BLOCKS * 4096 and SEGMENT_BLOCKS % (64 * 2) == 0
    assert (NSEG * SEG // (2 * 4096)) % LAG_STEP == 0 and ((1 << 32) // 8192 + 32) % LAG_STEP == 0  # the tail; past 2^32


def test_the_segments_are_what_the_cases_need():
    x = segments()
    f4, f1 = const_ref(x[6], 4096), const_ref(x[6], 1024)
    assert 0 < f4.sum() < len(f4) and 0 < f1.sum() < len(f1) and f1.sum() > 4 * f4.sum()
    assert f4[4] == 0 and f1[16:20].tolist() == [1, 1, 1, 0]      # constant but for its last byte
    assert f4[8] == 0 and f1[32:36].tolist() == [0, 1, 1, 1]      # constant but for byte 17
    assert f4[0] == 1 and f4[12] == 1 and x[6][3 * 4096] == x[6][4 * 4096]  # (equal neighbours)
    assert const_ref(x[7], 1024).all() and not const_ref(x[0], 1024).any()
    y = base_segments()
    assert 0.05 < (x != y).mean() < 0.2
    assert base_length(8192, SEG) > 1 << 32 and base_length(8192, SEG) < N - SEG
    assert base_length(8192, SEG) % (BASE_E * BASE_B) == 7 and base_cover(8193, 8192, SEG) == SEG // 4 + 7


def test_the_record_entries_and_their_segments():
    """The record layout's entries against a list written out here (one removed fails this), and what each is there for: the
    segment is whole frames, the frames lie past 2^32, the work outnumbers what the strided launches have, and every buffer
    fits what the GPU file allocates."""
    from redux_amd import api
    assert TRANSFORMS[-8:] == [("record_delta", 16, 4096), ("record", 256, 2048), ("record_delta", 256, 2048), ("record", 4, 4100),
                               ("record_delta", 4, 4100), ("record_delta", 4, 2036), ("record_delta", 3, 4096),
                               ("record_delta", 23, 4096)] == RECORD_TRANSFORMS
    assert len(TRANSFORMS) == 8 + 8 and LAYOUT_NAMES == ("planes", "delta", "zigzag")
    assert [segment_length(R * B) for _, R, B in RECORD_TRANSFORMS] == [SEG, SEG, SEG, 524800, 524800, 260608, 32 * 3 * 4096, 32 * 23 * 4096]
    assert segment_count() == NSEG and total_bytes() == N and LARGEST == total_bytes(32 * 23 * 4096) > N
    cus = 256
    for name, R, B in RECORD_TRANSFORMS:
        L = segment_length(R * B)
        n, delta = total_bytes(L), name == "record_delta"
        assert L % (R * B) == 0 and (segment_count(L) - 3) * L >= 1 << 32 > (segment_count(L) - 4) * L and n <= LARGEST
        assert 0 < TAIL // R < B and (TAIL % R > 0) == (R != 3)    # the tail: a short frame of whole records and, but for R = 3, trailing bytes
        assert len(set(order(segment_count(L))[-3:].tolist()) | set(order(segment_count(L))[:4].tolist())) > 2
        fwd, inv = api.record_plan(n, B, R, delta, False, cus), api.record_plan(n, B, R, delta, True, cus)
        nframes = n // (R * B)
        if B % 16:  # the byte kernels alone: 8,192 workgroups of 256 threads stride over the bytes, or the (frame, column) pairs
            pairs = (nframes + 1) * R
            assert (fwd.grid_fast, inv.grid_fast, fwd.grid_bytes) == (0, 0, 8192) and n > 8192 * 256
            assert inv.grid_bytes == min(-(-(pairs if delta else n) // 256), 8192)
            assert (pairs > 8192 * 256) == (B == 2036) and inv.grid_bytes == (8192 if B == 2036 or not delta else -(-pairs // 256))
        else:       # the fast kernels, every workgroup on to further frames or tiles, and the byte kernels for the tail
            assert fwd.grid_fast == inv.grid_fast == 8 * cus < nframes and fwd.grid_bytes and inv.grid_bytes and inv.PC == R
    assert SEG // (256 * 2048) == 1 and N // SEG > 8 * 1024      # R = 256: a frame is a whole segment, more frames than 8 * CUs


@pytest.mark.parametrize("name,E,B", TRANSFORMS)
def test_transforms_tile(name, E, B):
    ref = RESTATEMENTS[name]
    parts, idx, tail = small(2 * E * B)
    x = tile(parts, idx, tail)
    for inverse in (False, True):
        want = tiled(lambda p: ref(p, E, B, inverse=inverse), parts, idx, tail)
        assert np.array_equal(ref(x, E, B, inverse=inverse), want), (name, E, B, inverse)
        assert not np.array_equal(want, x)


@pytest.mark.parametrize("name", ["base", "base_sub"])
def test_base_filters_tile(name):
    """the base covers position 0, a quarter of position 1 and seven bytes, and nothing of position 2 or the tail"""
    ref, E, B = BASE_RESTATEMENTS[name], BASE_E, BASE_B
    L = 2 * E * B
    parts, idx, tail = small(L)
    bases, _, _ = small(L, base_segments)
    x = tile(parts, idx, tail)
    y = tile(bases, idx, tail[:0])[: base_length(0, L)]
    assert [base_cover(f, 0, L) for f in range(4)] == [L, L // 4 + 7, 0, 0]
    for inverse in (False, True):
        want = np.concatenate([ref(parts[f], bases[f][: base_cover(f, 0, L)], E, B, inverse=inverse) for f in range(3)]
                              + [ref(tail, b"", E, B, inverse=inverse)])
        assert np.array_equal(ref(x, y, E, B, inverse=inverse), want), (name, inverse)
        assert np.array_equal(want[2 * L:], planes_ref(x, E, B, inverse=inverse)[2 * L:])  # past the base: the layout alone


@pytest.mark.parametrize("B", [4096, 65536])
def test_mixed_layout_tiles(B):
    L = 2 * UNIT * B
    parts, idx, tail = small(L)
    x = tile(parts, idx, tail)
    table = unit_table(3 * 2 + 1)
    for inverse in (False, True):
        refs = [[layout_ref(p, k, B, inverse) for p in parts] for k in range(8)]
        tails = [layout_ref(tail, k, B, inverse) for k in range(8)]
        assert np.array_equal(mixed_ref(x, table, B, inverse=inverse), mixed_splice(refs, tails, idx, table, L, B)), (B, inverse)


def test_the_choice_sum_is_exact():
    rng = np.random.default_rng(3)
    bits = rng.uniform(100.0, 500000.0, (8, 8 * 37 + 3))
    bits[5] = bits[1]
    table, S = choose_ref(bits, 0xA6)
    assert set(table.tolist()) <= {1, 2, 5, 7} and 5 not in table
    total = choose_sum_units(S, table)
    assert total == sum(int(S[k, u] * 65536.0 + 0.5) for u, k in enumerate(table))
    import torch
    bits[2, :100] = bits[7, :100]
    for mask in (0xFF, 0xA6, 0x84, 0x20):
        table, S = choose_ref(bits, mask)
        pick, units = choose_vec(torch, torch.from_numpy(bits), mask)
        assert pick.numpy().tolist() == table.tolist() and units == choose_sum_units(S, table), mask


@pytest.mark.parametrize("B", [1024, 4096])
def test_constant_flags_tile(B):
    parts, idx, tail = small(2 * B)
    want = tiled(lambda p: const_ref(p, B), parts, idx, tail)
    assert np.array_equal(const_ref(tile(parts, idx, tail), B), want) and want.any() and not want.all()


@pytest.mark.parametrize("B", [4096, SEG])
def test_block_crcs_tile(B):
    parts, idx, tail = small(2 * B)
    assert np.array_equal(block_crcs(tile(parts, idx, tail), B), tiled(lambda p: block_crcs(p, B), parts, idx, tail))


def test_cost_counts_tile():
    """block_cost, every row of layout_cost, and lag_cost with and without a frame step: the counts under the host rule"""
    B = 4096
    parts, idx, tail = small(2 * B)
    assert np.array_equal(block_counts(tile(parts, idx, tail), B), tiled(lambda p: block_counts(p, B), parts, idx, tail))
    for k in range(8):
        E = 1 << (k & 3)
        parts, idx, tail = small(2 * E * B)
        fn = lambda p: block_counts(transform_ref(p, k, B), B)  # noqa: E731
        assert np.array_equal(fn(tile(parts, idx, tail)), tiled(fn, parts, idx, tail)), k
    E = 2
    parts, idx, tail = small(2 * E * B)
    x = tile(parts, idx, tail)
    for S in LAGS:
        fn = lambda p: block_counts(lag_planes_ref(p, E, B, S), B)  # noqa: E731
        whole, want = fn(x), tiled(fn, parts, idx, tail)
        assert np.array_equal(whole, want), S
        cols = sampled_columns(len(whole), E, 3)  # frames 0, 3 and 6: the tail's
        assert cols == [0, 1, 6, 7, 12, 13] and np.array_equal(whole[cols], want[cols])


def test_histograms_tile():
    B = 4096
    parts, idx, tail = small(2 * 4 * B)
    x = tile(parts, idx, tail)
    per = np.stack([plane_counts(p, 4, B) for p in parts])
    assert np.array_equal(plane_counts(x, 4, B), (per * np.bincount(idx)[:, None, None]).sum(0) + plane_counts(tail, 4, B))
    per = np.stack([pair_counts(p, B) for p in parts])
    assert np.array_equal(pair_counts(x, B), (per * np.bincount(idx)[:, None, None]).sum(0) + pair_counts(tail, B))
    G, E = SEGMENT_BLOCKS, 2
    parts, idx, tail = small(2 * G * B)  # two ranges a segment
    fn = lambda p: segment_counts(p, E, B, G)  # noqa: E731
    assert np.array_equal(fn(tile(parts, idx, tail)), tiled(fn, parts, idx, tail))
    assert len(fn(tail)) == E and len(fn(parts[0])) == 2 * E
