"""Zigzag-folded delta filter for signed series on the device: the fused and the general kernels against the numpy
restatement, extreme inputs next to the element boundaries of the packed forms, the streams of every layer against the CPU
oracle on the transformed bytes, the host pipeline over chunks and contexts, the device coder objects and their range
reads, a damaged stream, checksums, the container / CLI end to end, and that the calls without the filter and with the
delta filter give what they gave before any zigzag call of the process."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_delta_cpu import delta_planes_ref
from test_planes_cpu import lengths, planes_ref
from test_planes_gpu import FILL, guarded, guards_intact, split
from test_zigzag_cpu import build_zigzag_mirror_test, walk_and_stamps, zigzag_planes_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def series(n, seed=3):
    """n bytes of signed series: an int64, an int32 and an int16 random walk, int64 timestamps, and plain noise at the end"""
    rng = np.random.default_rng(seed)
    walk = lambda m: np.cumsum(np.round(rng.normal(0, 50, m))).astype(np.int64)
    a = walk(n // 40 + 1).astype("<i8").tobytes()[: n // 5]
    b = walk(n // 20 + 1).astype("<i4").tobytes()[: n // 5]
    c = walk(n // 10 + 1).astype("<i2").tobytes()[: n // 5]
    d = (1_700_000_000_000_000 + np.cumsum(rng.integers(900, 1100, n // 40 + 1))).astype("<u8").tobytes()[: n // 5]
    e = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer((a + b + c + d + e)[:n], dtype=np.uint8).copy()


def plain_and_delta(rx, x, B):
    """the streams and offsets of the calls that existed before the filter, on x: no filter and the delta filter, E = 1, 4"""
    return [rx.compress_blocks(x, B, element_size=E, filter=f)[:2] for E in (1, 4) for f in (None, "delta")]


@pytest.fixture(scope="module", autouse=True)
def before(rx):
    """taken when the module starts: no test of this module has run, and no other module makes a zigzag call"""
    x = series(9 * 4096 + 321, seed=21)
    return x, plain_and_delta(rx, x, 4096)


def run_dev(rx, torch, x, E, B, inverse, so=0, do=0):
    """redux_zigzag_planes_dev of x between guarded buffers at the given byte offsets -> (result, guards intact)"""
    L = len(x)
    ts, src = guarded(torch, L, so)
    if L:
        src.copy_(torch.from_numpy(x).cuda())
    td, dst = guarded(torch, L, do)
    rx.zigzag_planes(src, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), guards_intact(td, L, do) and guards_intact(ts, L, so)


# ---- the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [4096, 65536, 100, 48, 4688])   # (4688: 293 groups a frame: two iterations of the inverse,
def test_zigzag_planes_dev_matches_restatement(rx, E, B):     # the second a ragged wave; 100 and 48: the byte path)
    import torch
    rng = np.random.default_rng(E * 7 + B)
    F, W = E * B, 1024 * E  # a frame; what one wave of the fused kernels covers
    # (the last: three full frames and a short one of more than a wave, an element and a trailing byte)
    lens = lengths(E, B) + [W - 1, W, W + 16 * E, F + W, 3 * F + W + E + 1]
    for L in sorted(set(lens)):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        want = {inverse: zigzag_planes_ref(x, E, B, inverse=inverse) for inverse in (False, True)}
        for so, do in ((0, 0), (1, 0), (0, 1), (8, 8)):  # aligned; source, destination off by a byte; both by 8
            for inverse in (False, True):
                got, intact = run_dev(rx, torch, x, E, B, inverse, so, do)
                assert np.array_equal(got, want[inverse]), (E, B, L, so, do, inverse)
                assert intact, (E, B, L, so, do, inverse)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_extreme_inputs(rx, E):
    """every sign bit and carry next to an element boundary of the packed E = 1 and E = 2 forms"""
    import torch
    dt = np.dtype("<u%d" % E)
    top, half = (1 << 8 * E) - 1, 1 << (8 * E - 1)
    for B in (4688, 100):  # the fused kernels (two iterations of the inverse) and the byte path
        n = 3 * B + 17  # elements: three full frames and a short one
        alternating = lambda a, b: np.array([a, b], dtype=dt)[np.arange(n) % 2]
        cases = {"all 0": np.zeros(n, dtype=dt), "all max": np.full(n, top, dtype=dt),
                 "alternating 0 / max": alternating(0, top), "alternating max / 0": alternating(top, 0),
                 "alternating half / half - 1": alternating(half, half - 1),
                 "a ramp that wraps": (np.arange(n, dtype=np.uint64) * np.uint64(top // 97 + 1)).astype(dt)}
        for name, v in cases.items():
            x = np.concatenate([v.view(np.uint8), np.arange(E - 1, dtype=np.uint8)])  # + trailing bytes
            for off in (0, 1):
                y, intact = run_dev(rx, torch, x, E, B, False, off, off)
                assert intact and np.array_equal(y, zigzag_planes_ref(x, E, B)), (E, B, name, off)
                back, intact = run_dev(rx, torch, y, E, B, True, off, off)
                assert intact and np.array_equal(back, x), (E, B, name, off)
                # the same bytes taken as FOLDED differences: the running sum of a frame wraps many times
                s, intact = run_dev(rx, torch, x, E, B, True, off, off)
                assert intact and np.array_equal(s, zigzag_planes_ref(x, E, B, inverse=True)), (E, B, name, off)


def test_zigzag_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    assert L.redux_zigzag_planes_dev(pa, pb, 4096, 64, 3, 0, s) == lib.INVALID_INPUT
    assert L.redux_zigzag_planes_dev(pa, pb, 4096, 0, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_zigzag_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 0, s) == lib.INVALID_INPUT  # overlap
    assert L.redux_zigzag_planes_dev(pa, pb, 4096, 64, 1, 0, s) == lib.OK
    torch.cuda.synchronize()
    with pytest.raises(rx.InvalidInput):
        rx.zigzag_planes(a, 3, 64, out=b)


# ---- streams: the plain coder on the transformed bytes, against the oracle ------------------------------------------------
@pytest.mark.parametrize("params", [(8, 30, 32), (8, 14, 16)])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_streams_equal_oracle_on_transformed_bytes(rx, params, E):
    import torch
    B = 4096
    x = series(2 * E * B + 3 * B + 77, seed=E)
    # (slot: a model of 14 frequency bits freezes inside a block and can cost 15 bits per symbol afterwards)
    want, wst = ox.compress_blocks(zigzag_planes_ref(x, E, B), B, params, slot=2 * B + 1024)
    assert not wst.any()
    out, offs, st = rx.compress_blocks(x, B, params, element_size=E, filter="zigzag")   # the host-pointer call
    assert not st.any() and split(out, offs) == want, (params, E)
    enc = rx.DeviceEncoder(params, B, len(x), element_size=E, filter="zigzag")           # the device call
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (params, E)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, params, element_size=E, length=len(x), filter="zigzag")
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)


# ---- the host pipeline: chunks and contexts ---------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 8])
def test_host_pipeline_chunks_and_two_contexts(rx, E):
    B = 4096
    x = series(10 * 64 * B + 12345, seed=E)
    want = rx.compress_blocks(x, B, element_size=E, filter="zigzag")  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B)[1] == 1
    ref, _ = ox.compress_blocks(zigzag_planes_ref(x, E, B)[: 70 * B], B, (8, 30, 32))
    assert split(want[0], want[1])[:70] == ref
    try:
        rx.host_set_chunk_bytes(1 << 20, 1 << 20)  # 256 blocks a chunk
        assert rx.host_chunk_plan(nb, B)[1] >= 2
        for devices in ([], [0, 0]):
            rx.host_set_devices(devices)
            got = rx.compress_blocks(x, B, element_size=E, filter="zigzag")
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), devices
            back, sizes, st = rx.decompress_blocks(got[0], got[1], B, element_size=E, length=len(x), filter="zigzag")
            assert not st.any() and np.array_equal(back, x), devices
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_device_encoder_decoder_roundtrip_and_ranges(rx, E):
    import torch
    B = 4096
    n = 4 * E * B + 3 * B + 5
    x = series(n, seed=E)
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder((8, 30, 32), B, n, element_size=E, filter="zigzag")
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, element_size=E, filter="zigzag")
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder((8, 30, 32), B, nb, element_size=E, filter="zigzag")
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required, for E = 1 too
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_in)  # (the phases are the plain coder's)
    F = E * B
    ranges = [(3, 10), (2 * F - 7, 20), (n - 9, 9)]  # inside a frame, across a frame boundary, the end of the short frame
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, ranges)
    torch.cuda.synchronize()
    h = got.cpu().numpy()
    for (s0, m), o in zip(ranges, where):
        assert np.array_equal(h[o: o + m], x[s0: s0 + m]), (E, s0, m)


# ---- a damaged stream -------------------------------------------------------------------------------------------------
def test_damaged_stream_stays_in_bounds_and_spares_other_frames(rx, lib):
    import torch
    B, E, params = 4096, 2, (8, 30, 32)
    nfull = 6
    n = nfull * E * B + 1000  # 12 full blocks in 6 frames, then a short frame of one block of 1000 bytes
    F = E * B
    x = series(n, seed=11)
    out, offs, _ = rx.compress_blocks(x, B, params, element_size=E, filter="zigzag")
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
    cp = lib.Params(*params)
    wsb = L.redux_decode_zigzag_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    tg, d_out = guarded(torch, n, 5)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = L.redux_decode_zigzag_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E,
                                   C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()),
                                   C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(ws_ptr), wsb,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
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
    rc = L.redux_decode_blocks_zigzag(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, hout.ctypes.data,
                                      hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [8]
    assert (hout[n:] == FILL).all()
    for f in clean:
        assert np.array_equal(hout[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


# ---- checksums ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 4])
def test_block_crcs_are_of_the_original_bytes(rx, E):
    B = 4096
    x = series(70 * B + 333, seed=E)
    nb = 71
    want = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)], dtype=np.uint32)
    crc = np.zeros(nb, dtype=np.uint32)
    out, offs, st = rx.compress_blocks(x, B, element_size=E, block_crc=crc, filter="zigzag")
    assert np.array_equal(crc, want)
    plain = rx.compress_blocks(x, B, element_size=E, filter="zigzag")
    assert np.array_equal(out, plain[0]) and np.array_equal(offs, plain[1])  # the streams do not depend on block_crc
    got = np.zeros(nb, dtype=np.uint32)
    back, _, st2 = rx.decompress_blocks(out, offs, B, element_size=E, length=len(x), block_crc=got, filter="zigzag")
    assert not st2.any() and np.array_equal(back, x) and np.array_equal(got, want)


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_with_the_filter(rx, tmp_path):
    from redux_amd import cli, container
    B = 4096
    x = walk_and_stamps(8)[0].tobytes()  # the int64 random walk of the value claim: three frames and 100 elements
    src = tmp_path / "walk.i64"
    src.write_bytes(x)
    delta, zz, back, part = tmp_path / "delta.rdxb", tmp_path / "zigzag.rdxb", tmp_path / "back.i64", tmp_path / "part.i64"
    common = ["-c", "-i", str(src), "--block-size", str(B), "--element-size", "8"]
    assert cli.main(common + ["-o", str(delta), "--filter", "delta"]) == 0
    assert cli.main(common + ["-o", str(zz), "--filter", "zigzag"]) == 0
    p6, p11 = delta.read_bytes(), zz.read_bytes()
    assert p6[4] == 6 and p11[4] == 11 and container.filter(p11) == "zigzag" and container.element_size(p11) == 8
    print("int64 random walk: --filter delta %d bytes, --filter zigzag %d bytes, %.3f x" % (len(p6), len(p11), len(p11) / len(p6)))
    assert len(p11) <= 0.65 * len(p6), (len(p6), len(p11))
    assert p11 == container.compress_bytes(x, B, element_size=8, filter="zigzag")
    assert cli.main(["-d", "-i", str(zz), "-o", str(back)]) == 0
    assert back.read_bytes() == x
    F = 8 * B
    assert cli.main(["-d", "-i", str(zz), "-o", str(part), "--range", "%d:%d" % (2 * F - 11, 40)]) == 0  # over a frame boundary
    assert part.read_bytes() == x[2 * F - 11: 2 * F + 29]
    assert container.decompress_range(p11, F - 3, 2 * F) == x[F - 3: 3 * F - 3]
    for E in (1, 2, 4, 8):
        y = x[: 5 * B + 13]
        for checksum in (False, True):
            blob = container.compress_bytes(y, B, element_size=E, filter="zigzag", checksum=checksum)
            assert blob[4] == (0x1B if checksum else 11) and container.decompress_bytes(blob) == y
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, filter="zigzag")) == b""
    assert cli.main(["-c", "-i", str(src), "-o", str(tmp_path / "x"), "--filter", "zigzag"]) == 1


def test_cpp_zigzag_mirror(rx, tmp_path):
    import subprocess
    out = subprocess.run([build_zigzag_mirror_test(tmp_path), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "zigzag mirror ok" in out.stdout, out.stdout + out.stderr


# ---- without the filter (the last test of the module: after every zigzag call above) -------------------------------------
def test_without_the_filter_nothing_changes(rx, before):
    import torch
    B = 4096
    x, first = before
    torch.cuda.synchronize()
    rx.zigzag_planes(torch.from_numpy(x).cuda(), 4, B)  # (a zigzag call, should this test run alone)
    again = plain_and_delta(rx, x, B)
    for (o0, f0), (o1, f1) in zip(first, again):
        assert np.array_equal(o0, o1) and np.array_equal(f0, f1)
    k = 0
    for E in (1, 4):  # and they are what the oracle gives for the transforms that existed before
        for ref in (planes_ref(x, E, B), delta_planes_ref(x, E, B)):
            want, _ = ox.compress_blocks(ref, B, (8, 30, 32))
            assert split(*first[k]) == want, (E, k)
            k += 1
