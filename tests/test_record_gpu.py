"""The record layout on the device: the fast and the byte kernels against the numpy restatement for record sizes at powers of
two, odd sizes, either side of a 16-byte chunk and the maximum, the byte-plane kernels at R = 2, 4, 8, more frames than
workgroups, a frame whose tiles all need carries, wrapping extremes, the streams of every layer against the CPU oracle on the
transformed bytes, the host pipeline over chunks that are whole frames but not whole waves, a damaged stream, and the device
coder objects with their range reads, the container and the CLI end to end, and the C++ mirror.  Then the shapes of the
launch plan (SWEEP of test_record_cpu.py, each asserted by redux_record_plan before it runs): group counts that are no power
of two, ragged last tiles behind full ones, column ranges of every width with last ranges of 1 to 128 columns, the thresholds
of the cut, a very large block; more frames than workgroups with several tiles a frame; buffers aligned to 16 bytes and no
more; R = 2, 4, 8 with the delta."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_lag_order_gpu import FRONT, first_difference, poison_intact, poisoned
from test_planes_gpu import FILL, guarded, guards_intact, split
from test_record_cpu import SWEEP, claims_hold, generated_tables, plan_of, record_ref, resolve, tail_bytes

pytestmark = pytest.mark.gpu

PARAMS = (8, 30, 32)
# powers of two and odd sizes for the LDS layout, either side of a 16-byte chunk, and the maximum
SIZES = [2, 3, 4, 5, 8, 12, 13, 15, 16, 17, 23, 64, 255, 256]
FAST = {False: "k_record_planes", True: "k_record_unplanes"}
BYTES = {False: "k_record_planes_bytes", True: "k_record_unplanes_bytes"}


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def table_bytes(name, n):
    """n bytes of a generated table of packed structs (test_record_cpu.generated_tables), repeated as often as needed"""
    t = generated_tables(4000)[name][0]
    return np.tile(t, -(-n // len(t)))[:n].copy()


def run_dev(torch, x, R, B, delta, inverse, so=0, do=0):
    """redux_record_planes_dev of x between a poisoned source and a guarded destination at the given byte offsets
    -> (result, guards intact, the kernels the launch ran)"""
    from redux_amd import api
    assert FRONT >= 256
    L = len(x)
    ts, src = poisoned(torch, x, so)
    td, dst = guarded(torch, L, do)
    api.record_planes(src, R, B, delta=delta, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    name = api.record_kernel_name(L, B, R, inverse, d_src=src, d_dst=dst)
    return dst.cpu().numpy(), guards_intact(td, L, do) and poison_intact(ts, L, so), name


# ---- the kernels ----------------------------------------------------------------------------------------------------
# B = 64: a frame of four groups; 4096 and 4112: a tile edge and one group past it; 100 and 4099: the byte kernels, the
# buffers also one byte off.  Two full frames, a short one of B // 3 + 1 records and R - 1 trailing bytes each.
@pytest.mark.parametrize("B", [64, 4096, 4112, 100, 4099])
@pytest.mark.parametrize("R", SIZES)
def test_record_planes_dev_matches_restatement(rx, R, B):
    import torch
    rng = np.random.default_rng(R * 7 + B)
    L = 2 * R * B + (B // 3 + 1) * R + (R - 1)
    x = rng.integers(0, 256, L, dtype=np.uint8)
    fast = B % 16 == 0
    offsets = ((0, 0),) if fast else ((0, 0), (1, 0), (0, 1))
    for delta in (False, True):
        for inverse in (False, True):
            want = record_ref(x, R, B, delta, inverse)
            for so, do in offsets:
                got, intact, name = run_dev(torch, x, R, B, delta, inverse, so, do)
                assert name == (FAST[inverse] + " + " + BYTES[inverse] if fast else BYTES[inverse]), (R, B, name)
                assert np.array_equal(got, want), (R, B, delta, inverse, so, do, first_difference(got, want, R, B))
                assert intact, (R, B, delta, inverse, so, do)


def test_fast_kernels_take_unaligned_buffers_to_the_byte_path(rx):
    import torch
    R, B = 5, 64
    x = np.random.default_rng(1).integers(0, 256, 3 * R * B, dtype=np.uint8)
    for so, do in ((1, 0), (0, 3)):
        for inverse in (False, True):
            got, intact, name = run_dev(torch, x, R, B, True, inverse, so, do)
            assert name == BYTES[inverse] and intact and np.array_equal(got, record_ref(x, R, B, True, inverse))


@pytest.mark.parametrize("E", [2, 4, 8])
def test_record_layout_equals_byte_plane_kernels(rx, E):
    """kernel against kernel: R = 2, 4, 8 without the filter is api.planes at that element size, byte for byte"""
    import torch
    from redux_amd import api
    for B in (64, 4112, 100):
        x = np.random.default_rng(E + B).integers(0, 256, 3 * E * B + E * 7 + E - 1, dtype=np.uint8)
        d = torch.from_numpy(x).cuda()
        for inverse in (False, True):
            a = api.record_planes(d, E, B, inverse=inverse)
            b = api.planes(d, E, B, inverse=inverse)
            torch.cuda.synchronize()
            assert torch.equal(a, b), (E, B, inverse)


@pytest.mark.parametrize("R", [3, 16])
def test_more_frames_than_workgroups(rx, R):
    """B = 64, 20,000 frames: every workgroup walks on to further frames with whatever the one before left in LDS"""
    import torch
    B, nframes = 64, 20000
    x = np.random.default_rng(R).integers(0, 256, nframes * R * B, dtype=np.uint8)
    for delta in (False, True):
        want = record_ref(x, R, B, delta)
        got, intact, name = run_dev(torch, x, R, B, delta, False)
        assert name == FAST[False] and intact and np.array_equal(got, want), (R, delta, first_difference(got, want, R, B))
        back, intact, name = run_dev(torch, want, R, B, delta, True)
        assert name == FAST[True] and intact and np.array_equal(back, x), (R, delta, first_difference(back, x, R, B))


def test_one_frame_with_carries_between_all_tiles(rx):
    """R = 5, B = 12304: three tiles of 4096 records and one of 16, every column's sum carried across each edge"""
    import torch
    R, B = 5, 12304
    x = np.random.default_rng(5).integers(0, 256, R * B, dtype=np.uint8)
    for delta in (False, True):
        want = record_ref(x, R, B, delta)
        got, intact, _ = run_dev(torch, x, R, B, delta, False)
        assert intact and np.array_equal(got, want), (delta, first_difference(got, want, R, B))
        back, intact, _ = run_dev(torch, want, R, B, delta, True)
        assert intact and np.array_equal(back, x), (delta, first_difference(back, x, R, B))


def test_few_large_frames_split_their_columns(rx):
    """R = 255 and 256 at B = 4096: three frames of a megabyte, fewer than the CUs, so the inverse cuts the columns into
    ranges (rows leave in 16-byte pieces, the last range of R = 255 ends on a 15-byte one)"""
    import torch
    B = 4096
    for R in (255, 256, 80):
        x = np.random.default_rng(R).integers(0, 256, 3 * R * B, dtype=np.uint8)
        for delta in (False, True):
            want = record_ref(x, R, B, delta)
            back, intact, name = run_dev(torch, want, R, B, delta, True)
            assert name == FAST[True] and intact and np.array_equal(back, x), (R, delta, first_difference(back, x, R, B))


@pytest.mark.parametrize("R", [3, 16, 23])
def test_record_kernels_on_extremes(rx, R):
    """all 0xFF, and records alternating 0x00 / 0xFF: every difference and every sum wraps"""
    import torch
    for B in (4112, 100):
        n = 2 * B + 17
        cases = {"all max": np.full(n * R, 0xFF, dtype=np.uint8),
                 "0 / max": np.repeat(np.array([0, 0xFF], dtype=np.uint8)[np.arange(n) % 2], R)}
        for name, v in cases.items():
            x = np.concatenate([v, np.arange(R - 1, dtype=np.uint8)])
            y, intact, _ = run_dev(torch, x, R, B, True, False)
            assert intact and np.array_equal(y, record_ref(x, R, B, True)), (R, B, name)
            back, intact, _ = run_dev(torch, y, R, B, True, True)
            assert intact and np.array_equal(back, x), (R, B, name)


# ---- the shapes of the launch plan --------------------------------------------------------------------------------------
def where_wrong(got, want, R, B, inverse):
    """the first wrong byte as (frame, column, record): the inverse writes records, the forward call byte columns"""
    at = int(np.nonzero(got != want)[0][0])
    f, o = divmod(at, R * B)
    N = min(len(got) - f * R * B, R * B) // R
    if o >= N * R:
        return f"first wrong byte {at}: frame {f}, trailing byte {o - N * R}"
    p, i = (o % R, o // R) if inverse else (o // N, o % N)
    return f"first wrong byte {at}: frame {f}, column {p}, record {i} of {N}"


def cu_count(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_both_ways(torch, x, R, B, names, so=0, do=0):
    """forward and inverse, with and without the delta, of x against the restatement, between poison and guards"""
    for delta in (False, True):
        want = record_ref(x, R, B, delta)
        for inverse, a, b in ((False, x, want), (True, want, x)):
            got, intact, name = run_dev(torch, a, R, B, delta, inverse, so, do)
            assert name == names[inverse], (R, B, inverse, name)
            assert np.array_equal(got, b), (R, B, "inverse" if inverse else "forward", "delta" if delta else "plain", so, do,
                                            where_wrong(got, b, R, B, inverse))
            assert intact, (R, B, inverse, delta, so, do)


@pytest.mark.parametrize("key", sorted(SWEEP))
def test_the_sweep_of_the_launch_plan(rx, key):
    """SWEEP of test_record_cpu.py on the device: group counts that are no power of two, ragged last tiles behind full ones,
    every width of a column range with last ranges of 1 to 128 columns, both sides of R > 64 and of nfull < 2 * CUs, a very
    large block.  Each row first asserts, by redux_record_plan for this device, that it reaches what it is there for."""
    import torch
    cus = cu_count(torch)
    c = resolve(key, cus)
    if c is None:
        pytest.skip("no frame count gives the inverse PC = %d on a device of %d CUs (pinned for 256 CUs on the CPU)" % (SWEEP[key][2][1], cus))
    fwd, inv = claims_hold(c, 0)
    tail = tail_bytes(c)
    assert (fwd, inv) == (plan_of(c.nfull, c.R, c.B, False, cus, tail=tail), plan_of(c.nfull, c.R, c.B, True, cus, tail=tail))
    x = np.random.default_rng(len(key) + c.R * 7 + c.B).integers(0, 256, c.nfull * c.R * c.B + tail, dtype=np.uint8)
    check_both_ways(torch, x, c.R, c.B, {i: FAST[i] + (" + " + BYTES[i] if tail else "") for i in (False, True)})


def run_dev_tensor(torch, d_x, R, B, delta, inverse):
    """run_dev for an input that is on the device already -> (result on the device, guards intact)"""
    from redux_amd import api
    from test_planes_gpu import GUARD
    L = d_x.numel()
    ts = torch.full((FRONT + L + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    src = ts[FRONT: FRONT + L]
    src.copy_(d_x)
    td, dst = guarded(torch, L)
    api.record_planes(src, R, B, delta=delta, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    assert api.record_kernel_name(L, B, R, inverse, d_src=src, d_dst=dst) == FAST[inverse]
    intact = all(bool((t == FILL).all()) for t in (ts[:FRONT], ts[FRONT + L:], td[:GUARD], td[GUARD + L:])) and torch.equal(src, d_x)
    return dst, intact


@pytest.mark.parametrize("R, add", [(23, 48), (255, 16)])
def test_more_frames_than_workgroups_with_several_tiles_a_frame(rx, R, add):
    """8 * CUs + 37 frames of B = 2 * T + 48 (R = 23: three tiles, the last of 3 groups) and 2 * T + 16 (R = 255) records: some
    workgroups of the inverse walk on to a second frame of several tiles with the carries, their parity and the LDS tile the
    first left, others do not; the forward kernel's tile stride wraps.  The frames are drawn on the device from four
    distinct ones, so the restatement is of four frames."""
    import torch
    from redux_amd import api
    cus = cu_count(torch)
    nfull = 8 * cus + 37
    T = 1 << plan_of(nfull, R, 1 << 16, True, cus).lgT
    B = 2 * T + add
    fwd, inv = api.record_plan(nfull * R * B, B, R, True, False), api.record_plan(nfull * R * B, B, R, True, True)
    assert inv == (T.bit_length() - 1, R, 8 * cus, 0) and inv.grid_fast < nfull < 2 * inv.grid_fast
    assert fwd.grid_fast == 8 * cus and fwd.grid_bytes == 0 and -(-B // (1 << fwd.lgT)) >= 3 and B % (1 << fwd.lgT) == add
    assert B % T == add and nfull * R * B < 256 << 20
    rng = np.random.default_rng(R)
    x4 = rng.integers(0, 256, (4, R * B), dtype=np.uint8)
    pick = torch.from_numpy(rng.integers(0, 4, nfull)).cuda()
    assert len(set(pick[:37].tolist()) | set(pick[8 * cus:].tolist())) > 1
    d_x = torch.from_numpy(x4).cuda()[pick].reshape(-1)
    for delta in (False, True):
        want4 = record_ref(x4.reshape(-1), R, B, delta).reshape(4, R * B)
        assert not np.array_equal(want4, x4)
        d_want = torch.from_numpy(want4).cuda()[pick].reshape(-1)
        for inverse, a, b in ((False, d_x, d_want), (True, d_want, d_x)):
            got, intact = run_dev_tensor(torch, a, R, B, delta, inverse)
            if not torch.equal(got, b):
                raise AssertionError((R, B, "inverse" if inverse else "forward", "delta" if delta else "plain",
                                      where_wrong(got.cpu().numpy(), b.cpu().numpy(), R, B, inverse)))
            assert intact, (R, B, inverse, delta)


@pytest.mark.parametrize("R", [5, 16])
def test_buffers_that_are_16_byte_aligned_and_no_more(rx, R):
    """source and destination 16 and 48 bytes off a 256-byte boundary, in every combination: the fast kernels, whose 16-byte
    accesses are then aligned to 16 bytes and nothing more; 8 bytes off: the byte kernels"""
    import torch
    B = 4112
    x = np.random.default_rng(R).integers(0, 256, 2 * R * B + (B // 3 + 1) * R + R - 1, dtype=np.uint8)
    p = plan_of(2, R, B, True, 0, tail=(B // 3 + 1) * R + R - 1)
    assert p.grid_fast == 2 and p.grid_bytes and B > 1 << p.lgT
    for so in (16, 48):
        for do in (16, 48):
            check_both_ways(torch, x, R, B, {i: FAST[i] + " + " + BYTES[i] for i in (False, True)}, so, do)
    for so, do in ((8, 0), (0, 8), (8, 8), (16, 8)):
        check_both_ways(torch, x, R, B, BYTES, so, do)


@pytest.mark.parametrize("R", [2, 4, 8])
def test_small_power_of_two_records_with_the_delta(rx, R):
    """R = 2, 4, 8 at 3 and 63 groups a frame against the restatement, the delta included (test_record_layout_equals_byte_plane_kernels
    compares them with the byte-plane kernels, which have no delta)"""
    import torch
    for B in (48, 1008):
        x = np.random.default_rng(R + B).integers(0, 256, 2 * R * B + (B // 3 + 1) * R + R - 1, dtype=np.uint8)
        assert plan_of(2, R, B, True, 0).PC == R
        check_both_ways(torch, x, R, B, {i: FAST[i] + " + " + BYTES[i] for i in (False, True)})


def test_record_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    from redux_amd import api
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for R in (0, 1, 257, 1 << 20):
        for delta in (0, 1):
            for inverse in (0, 1):
                assert L.redux_record_planes_dev(pa, pb, 4096, 64, R, delta, inverse, s) == lib.INVALID_INPUT
    assert L.redux_record_planes_dev(pa, pb, 4096, 0, 3, 0, 0, s) == lib.INVALID_INPUT
    assert L.redux_record_planes_dev(pa, pb, 4096, 64, 3, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_record_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 3, 1, 0, s) == lib.INVALID_INPUT  # overlap
    torch.cuda.synchronize()
    assert bool((b == FILL).all())  # nothing was written
    assert L.redux_record_planes_dev(pa, pb, 4096, 64, 256, 1, 0, s) == lib.OK
    torch.cuda.synchronize()
    for R in (0, 1, 257):
        with pytest.raises(rx.InvalidInput):
            api.record_planes(a, R, 64, out=b)


# ---- the coder layers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("R", [3, 23])
def test_streams_equal_oracle_on_transformed_bytes(rx, R, delta):
    import torch
    B = 4096
    x = table_bytes("imu23", 2 * R * B + 1000 * R + 2)  # two full frames, a short one, trailing bytes
    f = {"record_size": R, "filter": "delta" if delta else None}
    nb = -(-len(x) // B)
    want, wst = ox.compress_blocks(record_ref(x, R, B, delta), B, PARAMS)
    assert not wst.any() and len(want) == nb
    out, offs, st = rx.compress_blocks(x, B, PARAMS, **f)                       # redux_encode_blocks_record
    assert not st.any() and split(out, offs) == want, (R, delta)
    enc = rx.DeviceEncoder(PARAMS, B, len(x), **f)                              # redux_encode_record_dev
    assert enc.front.infix == "record"
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (R, delta)
    dec = rx.DeviceDecoder(PARAMS, B, nb, **f)                                  # redux_decode_record_dev
    back, sizes, dst, dsum = dec.decode(d_out[: int(offs[-1])], d_offs, length=len(x))
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and np.array_equal(back.cpu().numpy(), x)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, PARAMS, length=len(x), **f)
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)
    other = rx.compress_blocks(x, B, PARAMS, record_size=R, filter=None if delta else "delta")  # (the flag reaches the kernel)
    assert not np.array_equal(other[0], out)


def test_host_pipeline_over_several_chunks(rx):
    """R = 23, B = 4096: chunks of a multiple of 23 blocks, whose last wave is partly filled"""
    B, R = 4096, 23
    x = table_bytes("imu23", 3 * 23 * 4 * B + 12345)
    f = {"record_size": R, "filter": "delta"}
    want = rx.compress_blocks(x, B, **f)  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B, record_size=R)[1] == 1
    ref, _ = ox.compress_blocks(record_ref(x, R, B, True)[: 2 * R * B], B, PARAMS)
    assert split(want[0], want[1])[: 2 * R] == ref
    crc = np.zeros(nb, dtype=np.uint32)
    try:
        rx.host_set_chunk_bytes(1 << 18, 1 << 18)  # 64 blocks a chunk, rounded up to 69 = 3 frames
        cb, nc = rx.host_chunk_plan(nb, B, record_size=R)
        assert cb == 69 and nc >= 3
        got = rx.compress_blocks(x, B, block_crc=crc, **f)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        crc2 = np.zeros(nb, dtype=np.uint32)
        back, sizes, st = rx.decompress_blocks(got[0], got[1], B, length=len(x), block_crc=crc2, **f)
        assert not st.any() and np.array_equal(back, x) and np.array_equal(crc, crc2)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    for b in (0, 1, 68, 69, nb - 1):  # block_crc is over the original bytes
        assert int(crc[b]) == zlib.crc32(x[b * B: (b + 1) * B].tobytes()), b


# ---- a damaged stream -------------------------------------------------------------------------------------------------
def test_damaged_stream_stays_in_bounds_and_spares_other_frames(rx, lib):
    import torch
    B, R = 4096, 3
    nfull = 4
    F = R * B
    n = nfull * F + 1000  # 12 full blocks in 4 frames, then a short frame of one block of 1000 bytes
    x = table_bytes("ticks20", n)
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, record_size=R, filter="delta")
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 13
    bad = list(streams)
    flipped = bytearray(streams[7])
    for k in range(3, len(flipped), 7):
        flipped[k] ^= 0xFF
    bad[7] = bytes(flipped[: len(flipped) // 2])  # flipped bytes, and an early end
    clean = [f for f in range(nfull) if f != 7 // R]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*PARAMS)
    wsb = L.redux_decode_record_workspace_bytes(C.byref(cp), n, B, R)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    tg, d_out = guarded(torch, n, 5)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = L.redux_decode_record_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, R, 1,
                                   C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()),
                                   C.c_void_p(summary.data_ptr()), C.c_void_p(ws_ptr), wsb,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.OK
    torch.cuda.synchronize()
    s = status.cpu().numpy()
    assert [b for b in range(nb) if s[b] != lib.OK] == [7]
    assert summary.cpu().tolist() == [int(s[7]), 1]
    assert guards_intact(tg, n, 5)
    got = d_out.cpu().numpy()
    for f in clean:  # the frames whose blocks are all OK hold the original bytes
        assert np.array_equal(got[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f
    assert np.array_equal(got[nfull * F:], x[nfull * F:])
    # the host-pointer call: the same status, and the same frames spared
    back, _, hst = rx.decompress_blocks(data, boffs.astype(np.uint64), B, PARAMS, check=False, length=n, record_size=R,
                                        filter="delta")
    assert [b for b in range(nb) if hst[b] != lib.OK] == [7]
    for f in clean:
        assert np.array_equal(back[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


# ---- the device coder objects -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [False, True])
def test_device_encoder_decoder_roundtrip_and_ranges(rx, delta):
    import torch
    B, R = 4096, 23
    n = 3 * R * B + 3 * B + 5
    x = table_bytes("imu23", n)
    f = {"record_size": R, "filter": "delta" if delta else None}
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, n, **f)
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, **f)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder(PARAMS, B, nb, **f)
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required
    F = R * B
    ranges = [(F + 100, 40), (2 * F - 7, 20)]  # one range inside a frame, one across two frames
    runs, _, virt_len = rx.range_plan(n, B, R, ranges)
    assert virt_len == 2 * F  # frames 1 and 2 only: the granule is R blocks
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, ranges)
    torch.cuda.synchronize()
    h = got.cpu().numpy()
    for (s0, m), o in zip(ranges, where):
        assert np.array_equal(h[o: o + m], x[s0: s0 + m]), (delta, s0, m)


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_end_to_end(rx, tmp_path):
    from redux_amd import cli, container
    B, R = 4096, 23
    x = table_bytes("imu23", 2 * R * B + 700 * R + 11).tobytes()  # two full frames, a short one, trailing bytes
    src = tmp_path / "imu.bin"
    src.write_bytes(x)
    names = {k: tmp_path / ("%s.rdxb" % k) for k in ("plain", "record", "delta", "crc")}
    back, part = tmp_path / "back.bin", tmp_path / "part.bin"
    head = ["-c", "-i", str(src), "--block-size", str(B)]
    assert cli.main(head + ["-o", str(names["plain"])]) == 0
    assert cli.main(head + ["-o", str(names["record"]), "--record-size", str(R)]) == 0
    assert cli.main(head + ["-o", str(names["delta"]), "--record-size", str(R), "--filter", "delta"]) == 0
    assert cli.main(head + ["-o", str(names["crc"]), "--record-size", str(R), "--filter", "delta", "--checksum"]) == 0
    blobs = {k: p.read_bytes() for k, p in names.items()}
    assert blobs["plain"][4] == 1 and blobs["plain"] == container.compress_bytes(x, B)
    for k, delta in (("record", False), ("delta", True), ("crc", True)):
        p = blobs[k]
        assert p[4] == (0x1F if k == "crc" else 15) and container.record(p) == (R, delta) and container.element_size(p) == 1
        assert p == container.compress_bytes(x, B, record_size=R, filter="delta" if delta else None, checksum=k == "crc")
        assert container.decompress_bytes(p) == x
        assert cli.main(["-d", "-i", str(names[k]), "-o", str(back)]) == 0 and back.read_bytes() == x
    print("imu23, %d bytes: plain %d, record layout %d, with the delta %d" % (len(x), len(blobs["plain"]), len(blobs["record"]),
                                                                             len(blobs["delta"])))
    assert len(blobs["delta"]) < len(blobs["record"]) < len(blobs["plain"])
    assert len(container.block_crcs(blobs["crc"])) == -(-len(x) // B)
    F = R * B
    for k in ("delta", "crc"):
        assert cli.main(["-d", "-i", str(names[k]), "-o", str(part), "--range", "%d:%d" % (F + 100, 40)]) == 0  # inside the second frame
        assert part.read_bytes() == x[F + 100: F + 140]
        assert cli.main(["-d", "-i", str(names[k]), "-o", str(part), "--range", "%d:%d" % (F - 5, 11)]) == 0   # across two frames
        assert part.read_bytes() == x[F - 5: F + 6]
    r = container.Reader(blobs["record"])
    assert r.granule_blocks == R and r.read(2 * F + 3, len(x) - 2 * F - 3) == x[2 * F + 3:]  # the short frame and its trailing bytes
    assert r.bytes_read < len(blobs["record"]) // 2
    assert container.decompress_range(blobs["delta"], F - 3, F + 6) == x[F - 3: 2 * F + 3]
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, record_size=R, filter="delta")) == b""
    est = container.estimate_bytes(x, B, record_size=R, filter="delta")  # estimated on the transformed bytes, nothing coded
    nb = -(-len(x) // B)  # (the bound of test_estimate_gpu: the ideal code length is within two bytes a block of the stream)
    assert set(est) == {"adaptive"} and abs(est["adaptive"] - len(blobs["delta"])) <= 2 * nb + 1, (est, len(blobs["delta"]))
    damaged = bytearray(blobs["crc"])
    damaged[-100] ^= 0x55
    with pytest.raises(rx.Error):
        container.decompress_bytes(bytes(damaged))


def test_cpp_record_mirror(rx, tmp_path):
    import subprocess
    from test_record_cpu import build_record_mirror_test
    out = subprocess.run([build_record_mirror_test(tmp_path), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "record mirror ok" in out.stdout, out.stdout + out.stderr
