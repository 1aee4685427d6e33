"""Folded difference against a base on the device: the fused and the byte kernels against the numpy restatement, patterns
that put a borrow at every element boundary of the packed forms, the streams of every layer against the CPU oracle on the
transformed bytes, the host pipeline over chunks and contexts, the device coder objects and their range reads, a damaged
stream, checksums, the container, `base_op="auto"` and the CLI end to end, the C++ mirror, and that the calls with a base
and without `base_op`, or with `base_op="xor"`, give what they gave before any "sub" call of the process."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_base_cpu import base_planes_ref
from test_base_sub_cpu import PARAMS, base_sub_planes_ref, build_base_sub_mirror_test, pairs
from test_planes_gpu import FILL, guarded, guards_intact, split

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def snapshots(n, seed):
    """n bytes of an fp32 pair: N(0, 0.02) weights after a relative update of 1e-3, and the weights before it"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n // 4 + 1) * 0.02).astype(np.float32)
    w2 = (w * (1 + np.float32(1e-3) * rng.standard_normal(len(w)).astype(np.float32))).astype(np.float32)
    return w2.view(np.uint8)[:n].copy(), w.view(np.uint8)[:n].copy()


def xor_calls(rx, x, y, B):
    """the streams and offsets of the base calls that existed before the operation, on (x, y): E = 1 and 4, no base_op"""
    return [rx.compress_blocks(x, B, element_size=E, base=y)[:2] for E in (1, 4)]


@pytest.fixture(scope="module", autouse=True)
def before(rx):
    """taken when the module starts: no test of this module has run, and no other module makes a "sub" call"""
    x, y = snapshots(9 * 4096 + 321, seed=21)
    y = y[: 6 * 4096 + 7]
    return x, y, xor_calls(rx, x, y, 4096)


def run_dev(rx, torch, x, y, E, B, inverse, so=0, yo=0, do=0):
    """redux_base_sub_planes_dev of x with base y between guarded buffers at the given byte offsets -> (result, guards intact)"""
    L = len(x)
    ts, src = guarded(torch, L, so)
    if L:
        src.copy_(torch.from_numpy(x).cuda())
    ty, base = guarded(torch, len(y), yo)
    if len(y):
        base.copy_(torch.from_numpy(y).cuda())
    td, dst = guarded(torch, L, do)
    rx.base_sub_planes(src, base, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    intact = guards_intact(td, L, do) and guards_intact(ts, L, so) and guards_intact(ty, len(y), yo)
    return dst.cpu().numpy(), intact and np.array_equal(src.cpu().numpy(), x) and np.array_equal(base.cpu().numpy(), y)


def check(rx, torch, x, y, E, B, so=0, yo=0, do=0):
    for inverse in (False, True):
        got, intact = run_dev(rx, torch, x, y, E, B, inverse, so, yo, do)
        want = base_sub_planes_ref(x, y, E, B, inverse=inverse)
        assert intact, (E, B, len(x), len(y), (so, yo, do), inverse)
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"E={E} B={B} len={len(x)} base_len={len(y)} offsets={(so, yo, do)} inverse={inverse}: first "
                                 f"difference at byte {at} (frame {at // (E * B)}, offset {at % (E * B)})")


# ---- the transform, byte for byte against the restatement ------------------------------------------------------------------
# (16: one group a frame; 48 and 100: the byte path; 4688: 293 groups a frame, a row of 256 and a ragged wave)
@pytest.mark.parametrize("B", [16, 48, 100, 4096, 4688])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_base_sub_planes_dev_matches_restatement(rx, E, B):
    import torch
    rng = np.random.default_rng(E * 100003 + B)
    F, W = E * B, 1024 * E  # a frame; what one wave of the fused kernels covers
    last = 3 * F + 3 * E + 1  # three frames, and a short one of three elements and a trailing byte
    for L in sorted({W - 1, W, W + 16 * E, F - 1, F, F + 1, last}):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        # no base; one byte; mid-element; mid-frame on an element boundary; a frame end; the input's length; longer
        for yl in sorted({0, 1, min(L, E + E // 2 + 1), min(L, F // 2 // E * E), min(L, F), min(L, 2 * F), L, L + 5}):
            y = rng.integers(0, 256, yl, dtype=np.uint8)
            check(rx, torch, x, y, E, B)                 # all three on 16-byte boundaries: the fused kernels where B allows
            if L == last:                                # each buffer alone, and all together, 1 and 8 bytes off
                for off in (1, 8):
                    for so, yo, do in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off)):
                        check(rx, torch, x, y, E, B, so, yo, do)
        got, intact = run_dev(rx, torch, x, x.copy(), E, B, False)
        assert intact and not got.any()                  # x == y: all-zero coder input, trailing bytes included


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_patterns_at_the_element_boundaries(rx, E):
    """x == y, y = x -+ 1, x - y = 2^(8E-1), alternating 0 / max against max / 0 (a borrow at every element boundary of a
    dword), a wrapping ramp; and the same buffers taken as FOLDED input of the inverse"""
    import torch
    dt = np.dtype("<u%d" % E)
    top, half = (1 << 8 * E) - 1, 1 << (8 * E - 1)
    rng = np.random.default_rng(E)
    for B in (4688, 100):  # the fused kernels and the byte path
        n = 3 * B + 17  # elements: three full frames and a short one
        alternating = lambda a, b: np.array([a, b], dtype=dt)[np.arange(n) % 2]
        ramp = (np.arange(n, dtype=np.uint64) * np.uint64(top // 97 + 1)).astype(dt)
        noise = rng.integers(0, 256, n * E, dtype=np.uint8).view(dt)
        one = dt.type(1)
        cases = {"x == y": (noise, noise), "y = x - 1": (noise, noise - one), "y = x + 1": (noise, noise + one),
                 "x - y = half": (noise, noise - dt.type(half)), "0 / max against max / 0": (alternating(0, top), alternating(top, 0)),
                 "max / 0 against 0 / max": (alternating(top, 0), alternating(0, top)), "a ramp against noise": (ramp, noise),
                 "noise against a ramp": (noise, ramp), "all max against all 0": (np.full(n, top, dtype=dt), np.zeros(n, dtype=dt))}
        for name, (vx, vy) in cases.items():
            x = np.concatenate([vx.view(np.uint8), np.arange(E - 1, dtype=np.uint8)])  # + trailing bytes
            y = np.concatenate([vy.view(np.uint8), np.arange(E - 1, dtype=np.uint8)[::-1]])
            for off in (0, 1):
                z, intact = run_dev(rx, torch, x, y, E, B, False, off, off, off)
                assert intact and np.array_equal(z, base_sub_planes_ref(x, y, E, B)), (E, B, name, off)
                back, intact = run_dev(rx, torch, z, y, E, B, True, off, off, off)
                assert intact and np.array_equal(back, x), (E, B, name, off)
                s, intact = run_dev(rx, torch, x, y, E, B, True, off, off, off)
                assert intact and np.array_equal(s, base_sub_planes_ref(x, y, E, B, inverse=True)), (E, B, name, off)


def test_base_sub_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    c = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert L.redux_base_sub_planes_dev(v(a), v(b), 4096, v(c), 4096, 64, 3, 0, s) == lib.INVALID_INPUT
    assert L.redux_base_sub_planes_dev(v(a), v(b), 4096, v(c), 4096, 0, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_base_sub_planes_dev(v(a), v(b), 4096, v(a, 16), 1024, 64, 2, 0, s) == lib.INVALID_INPUT   # overlaps the source
    assert L.redux_base_sub_planes_dev(v(a), v(b), 4096, v(b, 16), 1024, 64, 2, 0, s) == lib.INVALID_INPUT   # overlaps the base
    assert L.redux_base_sub_planes_dev(v(a), v(b), 4096, v(c), 4096, 64, 1, 0, s) == lib.OK
    torch.cuda.synchronize()
    with pytest.raises(rx.InvalidInput):
        rx.base_sub_planes(a, b, 3, 64)
    with pytest.raises(rx.InvalidInput):
        rx.base_sub_planes(a, b, 2, 0)


# ---- streams: the plain coder on the transformed bytes, against the oracle ------------------------------------------------
@pytest.mark.parametrize("params", [(8, 30, 32), (8, 14, 16)])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_streams_equal_oracle_on_transformed_bytes(rx, params, E):
    import torch
    B = 4096
    n = 2 * E * B + 3 * B + 77
    x, y = snapshots(n, seed=E)
    y = y[: E * B + 5 * E + 1]  # the base ends inside an element of the second frame
    # (slot: a model of 14 frequency bits freezes inside a block and can cost 15 bits per symbol afterwards)
    want, wst = ox.compress_blocks(base_sub_planes_ref(x, y, E, B), B, params, slot=2 * B + 1024)
    assert not wst.any()
    out, offs, st = rx.compress_blocks(x, B, params, element_size=E, base=y, base_op="sub")   # the host-pointer call
    assert not st.any() and split(out, offs) == want, (params, E)
    d_y = torch.from_numpy(y).cuda()
    enc = rx.DeviceEncoder(params, B, n, element_size=E, base=d_y, base_op="sub")               # the device call
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (params, E)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, params, element_size=E, length=n, base=y, base_op="sub")
    assert not st2.any() and len(back) == n and np.array_equal(back, x)
    # a longer base is used up to the input's length
    long_y = np.concatenate([y, np.zeros(n, np.uint8)])
    got = rx.compress_blocks(x, B, params, element_size=E, base=long_y, base_op="sub")
    back2, _, _ = rx.decompress_blocks(got[0], got[1], B, params, element_size=E, length=n, base=long_y, base_op="sub")
    assert np.array_equal(back2, x)


# ---- the host pipeline: chunks and contexts ---------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 8])
def test_host_pipeline_chunks_and_two_contexts(rx, E):
    """1 MiB chunks of 256 blocks; the base ends mid-element inside the second chunk, so the later chunks have no share of it"""
    B = 4096
    n = 3 * 256 * B + 12345
    x, y = snapshots(n, seed=E)
    y = y[: 300 * B + E + E // 2 + 1]
    want = rx.compress_blocks(x, B, element_size=E, base=y, base_op="sub")  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B)[1] == 1
    ref, _ = ox.compress_blocks(base_sub_planes_ref(x, y, E, B)[: 40 * B], B, PARAMS)
    assert split(want[0], want[1])[:40] == ref
    try:
        rx.host_set_chunk_bytes(1 << 20, 1 << 20)
        assert rx.host_chunk_plan(nb, B)[1] >= 2
        for devices in ([], [0, 0]):
            rx.host_set_devices(devices)
            got = rx.compress_blocks(x, B, element_size=E, base=y, base_op="sub")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), devices
            back, sizes, st = rx.decompress_blocks(got[0], got[1], B, element_size=E, length=n, base=y, base_op="sub")
            assert not st.any() and np.array_equal(back, x), devices
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_device_encoder_decoder_roundtrip_and_ranges(rx, E):
    import torch
    B = 4096
    F = E * B
    n = 4 * F + 3 * B + 5
    x, y = snapshots(n, seed=E)
    y = y[: 2 * F + 9 * E + 1]  # the base ends inside an element of the third frame
    d_in, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E, base=d_y, base_op="sub")
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, element_size=E, base=y, base_op="sub")
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, base=d_y, base_op="sub")
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required, for E = 1 too
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_in)  # (the phases are the plain coder's)
    # inside a frame, across a frame boundary, across the end of the base, the end of the short frame
    ranges = [(3, 10), (2 * F - 7, 20), (len(y) - 6, 30), (n - 9, 9)]
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, ranges)
    torch.cuda.synchronize()
    h = got.cpu().numpy()
    for (s0, m), o in zip(ranges, where):
        assert np.array_equal(h[o: o + m], x[s0: s0 + m]), (E, s0, m)
    # the last frames alone: past the base, which the decoder then gathers nothing of
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, [(3 * F + 1, 50)])
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), x[3 * F + 1: 3 * F + 51])


# ---- a damaged stream -------------------------------------------------------------------------------------------------
def test_damaged_stream_stays_in_bounds_and_spares_other_frames(rx, lib):
    import torch
    B, E = 4096, 2
    nfull = 6
    n = nfull * E * B + 1000  # 12 full blocks in 6 frames, then a short frame of one block of 1000 bytes
    F = E * B
    x, y = snapshots(n, seed=11)
    y = y[: n - 500]
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, base=y, base_op="sub")
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 13
    bad = list(streams)
    bad[8] = streams[8][: len(streams[8]) // 3]  # truncated
    clean = [f for f in range(nfull) if f != 8 // E]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*PARAMS)
    wsb = L.redux_decode_base_sub_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    d_y = torch.from_numpy(y).cuda()
    tg, d_out = guarded(torch, n, 5)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = L.redux_decode_base_sub_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                     C.c_void_p(d_y.data_ptr()), len(y), n, B, E, C.c_void_p(d_out.data_ptr()),
                                     C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()),
                                     C.c_void_p(ws_ptr), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.OK
    torch.cuda.synchronize()
    s = status.cpu().numpy()
    assert [b for b in range(nb) if s[b] != lib.OK] == [8]
    assert summary.cpu().tolist() == [int(s[8]), 1]
    assert guards_intact(tg, n, 5)
    got = d_out.cpu().numpy()
    for f in clean:  # the frames whose blocks are all OK hold the original bytes
        assert np.array_equal(got[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f
    assert np.array_equal(got[nfull * F:], x[nfull * F:])
    # the host-pointer call: the same status, only out[0 .. n) written
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs = np.zeros(nb, dtype=np.uint32)
    hst = np.zeros(nb, dtype=np.int32)
    hoffs = boffs.astype(np.uint64)
    rc = L.redux_decode_blocks_base_sub(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, y.ctypes.data, len(y), n, B, E,
                                        hout.ctypes.data, hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [8]
    assert (hout[n:] == FILL).all()
    for f in clean:
        assert np.array_equal(hout[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


# ---- checksums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 4])
def test_block_crcs_are_of_the_original_bytes(rx, E):
    B = 4096
    n = 70 * B + 333
    x, y = snapshots(n, seed=E)
    nb = 71
    want = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)], dtype=np.uint32)
    crc = np.zeros(nb, dtype=np.uint32)
    out, offs, st = rx.compress_blocks(x, B, element_size=E, block_crc=crc, base=y, base_op="sub")
    assert np.array_equal(crc, want)
    plain = rx.compress_blocks(x, B, element_size=E, base=y, base_op="sub")
    assert np.array_equal(out, plain[0]) and np.array_equal(offs, plain[1])  # the streams do not depend on block_crc
    got = np.zeros(nb, dtype=np.uint32)
    back, _, st2 = rx.decompress_blocks(out, offs, B, element_size=E, length=n, block_crc=got, base=y, base_op="sub")
    assert not st2.any() and np.array_equal(back, x) and np.array_equal(got, want)


# ---- container, base_op="auto" and the CLI -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table_pairs():
    """the pairs of the value claim (test_base_sub_cpu): 3 * 4096 + 100 elements"""
    return {(name, dtype): (E, y, x) for name, dtype, E, y, x in pairs(3 * 4096 + 100)}


def test_container_with_the_operation_pays_and_round_trips(rx, table_pairs):
    """bf16 at a relative update of 1e-2, B = 4096: the oracle's streams are 5,762 bytes against 6,817 (0.845) and both
    containers carry the same 44 + 4 * 7 bytes besides: 0.853 expected, at most 0.88 asked for.  Synthetic pairs only."""
    from redux_amd import container
    B = 4096
    E, y, x = table_pairs[("relative update 0.01", "bf16")]
    v8 = container.compress_bytes(x, B, element_size=E, base=y)
    v12 = container.compress_bytes(x, B, element_size=E, base=y, base_op="sub")
    print("bf16 pair, relative update 1e-2: version 8 %d bytes, version 12 %d bytes, %.4f" % (len(v8), len(v12), len(v12) / len(v8)))
    assert v8[4] == 8 and v12[4] == 12 and container.base_op(v8) == "xor" and container.base_op(v12) == "sub"
    assert container.base(v12) == container.base(v8) == (len(y), zlib.crc32(y.tobytes())) and container.element_size(v12) == E
    assert v8 == container.compress_bytes(x, B, element_size=E, base=y, base_op="xor")
    assert len(v12) <= 0.88 * len(v8), (len(v8), len(v12))
    assert container.decompress_bytes(v12, base=y) == x.tobytes() and container.decompress_bytes(v8, base=y) == x.tobytes()
    assert container.decompress_bytes(v12, base=y.tobytes() + b"more") == x.tobytes()   # a longer base is fine
    other = y.copy()
    other[1000] ^= 1
    for bad in (None, other, y[:-1], b""):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(v12, base=bad)
    # the payloads are the oracle's streams of the restated transform
    c = container._parse(v12)
    want, _ = ox.compress_blocks(base_sub_planes_ref(x, y, E, B), B, PARAMS)
    assert split(c.payload, c.offsets) == want
    # range reads: inside a frame, across a frame boundary
    F = E * B
    assert container.decompress_range(v12, F - 3, 2 * F, base=y) == x.tobytes()[F - 3: 3 * F - 3]
    assert container.decompress_range(v12, 5, 11, base=y) == x.tobytes()[5:16]
    # every element size, a base shorter than the data, checksums, and the empty input
    data = x.tobytes()[: 5 * B + 13]
    for E2 in (1, 2, 4, 8):
        for checksum in (False, True):
            blob = container.compress_bytes(data, B, element_size=E2, base=y[: 3 * B + 5], checksum=checksum, base_op="sub")
            assert blob[4] == (0x1C if checksum else 12) and container.base(blob)[0] == 3 * B + 5
            assert container.decompress_bytes(blob, base=y) == data
            assert container.decompress_range(blob, 3 * B - 2, 20, base=y) == data[3 * B - 2: 3 * B + 18]   # across the base's end
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, base=y, base_op="sub"), base=y) == b""
    assert container.decompress_bytes(container.compress_bytes(data, 65536, element_size=2, base=b"", base_op="sub"), base=b"") == data


def test_base_op_auto_writes_the_smaller_operations_own_container(rx, table_pairs):
    from redux_amd import container
    B = 4096
    for key, ver in ((("relative update 0.01", "bf16"), 12), (("unrelated pair", "bf16"), 8), (("unrelated pair", "fp32"), 8),
                     (("identical pair", "fp32"), 8)):   # (a tie goes to XOR)
        E, y, x = table_pairs[key]
        est = rx.estimate_base_ops(x, y, B, PARAMS, E)
        auto = container.compress_bytes(x, B, element_size=E, base=y, base_op="auto")
        print(key, est, "->", auto[4])
        assert auto[4] == ver, (key, est)
        assert auto == container.compress_bytes(x, B, element_size=E, base=y, base_op="sub" if ver == 12 else "xor")
        assert container.choose_base_op(est) == ("sub" if ver == 12 else "xor")
        assert container.decompress_bytes(auto, base=y) == x.tobytes()
    assert container.choose_base_op({"xor": 5, "sub": 5}) == "xor" and container.choose_base_op({"sub": 4, "xor": 5}) == "sub"


def test_cli_with_the_operation(rx, table_pairs, tmp_path):
    from redux_amd import cli, container
    E, y, x = table_pairs[("relative update 0.01", "bf16")]
    prev, cur, wrong = tmp_path / "step0.bf16", tmp_path / "step1.bf16", tmp_path / "wrong.bf16"
    prev.write_bytes(y.tobytes())
    cur.write_bytes(x.tobytes())
    wrong.write_bytes(x.tobytes())
    xor, sub, auto, back, part = (tmp_path / n for n in ("xor.rdxb", "sub.rdxb", "auto.rdxb", "back.bf16", "part.bf16"))
    common = ["-c", "-i", str(cur), "--block-size", "4096", "--element-size", "2", "--base", str(prev)]
    assert cli.main(common + ["-o", str(xor)]) == 0
    assert cli.main(common + ["-o", str(sub), "--base-op", "sub", "--checksum"]) == 0
    assert cli.main(common + ["-o", str(auto), "--base-op", "auto"]) == 0
    p8, p12, pa = xor.read_bytes(), sub.read_bytes(), auto.read_bytes()
    assert p8[4] == 8 and p12[4] == 0x1C and pa[4] == 12 and container.base_op(p12) == "sub"
    assert p8 == container.compress_bytes(x, 4096, element_size=2, base=y)
    assert pa == container.compress_bytes(x, 4096, element_size=2, base=y, base_op="sub")
    assert cli.main(common + ["-o", str(tmp_path / "x8"), "--base-op", "xor"]) == 0 and (tmp_path / "x8").read_bytes() == p8
    assert cli.main(["-d", "-i", str(sub), "-o", str(back), "--base", str(prev)]) == 0
    assert back.read_bytes() == x.tobytes()
    F = 2 * 4096
    assert cli.main(["-d", "-i", str(sub), "-o", str(part), "--base", str(prev), "--range", "%d:%d" % (2 * F - 11, 40)]) == 0
    assert part.read_bytes() == x.tobytes()[2 * F - 11: 2 * F + 29]
    assert cli.main(["-d", "-i", str(sub), "-o", str(back), "--base", str(wrong)]) == 3    # another file as base
    assert cli.main(["-d", "-i", str(sub), "-o", str(back)]) == 3                          # no base
    assert cli.main(["-d", "-i", str(sub), "-o", str(part), "--base", str(wrong), "--range", "0:8"]) == 3
    assert cli.main(["-c", "-i", str(cur), "-o", str(tmp_path / "x"), "--base", str(prev), "--base-op", "sub"]) == 1   # no block size


def test_cpp_base_sub_mirror(rx, tmp_path):
    import os
    import subprocess
    exe = build_base_sub_mirror_test(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([exe, os.path.join(root, "tests", "golden", "corpora", "canterbury", "lcet10.txt")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "base sub mirror ok" in out.stdout, out.stdout + out.stderr


# ---- without the operation (the last test of the module: after every "sub" call above) ------------------------------------
def test_without_the_operation_nothing_changes(rx, before):
    import torch
    B = 4096
    x, y, first = before
    torch.cuda.synchronize()
    rx.base_sub_planes(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 4, B)  # (a "sub" call, should this test run alone)
    again = xor_calls(rx, x, y, B)
    named = [rx.compress_blocks(x, B, element_size=E, base=y, base_op="xor")[:2] for E in (1, 4)]
    for (o0, f0), (o1, f1), (o2, f2) in zip(first, again, named):
        assert np.array_equal(o0, o1) and np.array_equal(f0, f1) and np.array_equal(o0, o2) and np.array_equal(f0, f2)
    for k, E in enumerate((1, 4)):  # and they are what the oracle gives for the transform that existed before
        want, _ = ox.compress_blocks(base_planes_ref(x, y, E, B), B, PARAMS)
        assert split(*first[k]) == want, E
