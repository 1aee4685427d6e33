"""Lagged delta filter for interleaved channels on the device: the fused and the byte kernels against the numpy restatement
for lags around every power of two the inverse's scan steps through, the zigzag kernels at lag 1, the streams of every layer
against the CPU oracle on the transformed bytes, the host pipeline over chunks, a damaged stream, the device coder objects and
their range reads, and the container / CLI end to end."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox
from test_lag_cpu import build_lag_mirror_test, channels, lag_planes_ref
from test_planes_gpu import FILL, guarded, guards_intact, split

pytestmark = pytest.mark.gpu

PARAMS = (8, 30, 32)
LAGS = [1, 2, 3, 5, 15, 16, 17, 63, 64, 65, 255, 256]


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def interleaved(n, C_, E, seed=3):
    """n bytes of C_ interleaved random walks of E-byte integers, noise behind them"""
    rng = np.random.default_rng(seed)
    m = n // (2 * E * C_) + 1
    w = np.stack([np.cumsum(np.round(rng.normal(0, 50, m))) + 5000 * c * (-1) ** c for c in range(C_)], 1)
    a = w.reshape(-1).astype(np.int64).astype("<i%d" % E).tobytes()[: n // 2]
    return np.frombuffer((a + rng.integers(0, 256, n, dtype=np.uint8).tobytes())[:n], dtype=np.uint8).copy()


def run_dev(rx, torch, x, E, B, S, inverse, so=0, do=0, zigzag=False):
    """redux_lag_planes_dev of x between guarded buffers at the given byte offsets -> (result, guards intact)"""
    L = len(x)
    ts, src = guarded(torch, L, so)
    if L:
        src.copy_(torch.from_numpy(x).cuda())
    td, dst = guarded(torch, L, do)
    if zigzag:
        rx.zigzag_planes(src, E, B, inverse=inverse, out=dst)
    else:
        from redux_amd import api
        api.lag_planes(src, E, B, S, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), guards_intact(td, L, do) and guards_intact(ts, L, so)


# ---- the kernels ----------------------------------------------------------------------------------------------------
# B = 64: 4 groups a frame, most lags beyond a frame's 64 elements; 4096: exactly one row of the inverse; 4112: 257 groups, a
# second row of one group: the carry and, for lags that do not divide 4096, the moving chain phase; 12304: three rows and a
# group; 8192: two full rows; 100 and 4099: the byte kernels.  Three full frames, a short one and trailing bytes each; at
# 4099 also a short frame of E * B - 1 bytes, one byte less than a full one.
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [64, 4096, 4112, 8192, 12304, 100, 4099])
def test_lag_planes_dev_matches_restatement(rx, E, B):
    import torch
    rng = np.random.default_rng(E * 7 + B)
    L = 3 * E * B + (B // 3 + 1) * E + (E - 1)
    x = rng.integers(0, 256, L, dtype=np.uint8)
    for S in LAGS:
        if B == 4099 and S in (1, 3, 255, 256):
            xs = x[: 3 * E * B - 1]
            for inverse in (False, True):
                got, intact = run_dev(rx, torch, xs, E, B, S, inverse, 1, 0)
                assert intact and np.array_equal(got, lag_planes_ref(xs, E, B, S, inverse=inverse)), (E, B, S, inverse)
        want = {inverse: lag_planes_ref(x, E, B, S, inverse=inverse) for inverse in (False, True)}
        for so, do in ((0, 0), (1, 0), (0, 1)):  # aligned; source, destination off by a byte: everything on the byte path
            for inverse in (False, True):
                got, intact = run_dev(rx, torch, x, E, B, S, inverse, so, do)
                assert np.array_equal(got, want[inverse]), (E, B, S, so, do, inverse)
                assert intact, (E, B, S, so, do, inverse)
    for inverse in (False, True):  # lag 1 is the zigzag filter, kernel against kernel on the same bytes
        z, _ = run_dev(rx, torch, x, E, B, 1, inverse, zigzag=True)
        g, _ = run_dev(rx, torch, x, E, B, 1, inverse)
        assert np.array_equal(z, g), (E, B, inverse)


@pytest.mark.parametrize("E", [2, 8])
def test_lag_kernels_on_series_and_extremes(rx, E):
    """interleaved walks (small differences of both signs) and the extremes of the element range, through both paths"""
    import torch
    dt = np.dtype("<u%d" % E)
    top, half = (1 << 8 * E) - 1, 1 << (8 * E - 1)
    for B in (4112, 100):
        n = 3 * B + 17
        cases = {"walks": interleaved(n * E, 3, E).view(dt), "all max": np.full(n, top, dtype=dt),
                 "0 / max / half": np.array([0, top, half], dtype=dt)[np.arange(n) % 3],
                 "a ramp that wraps": (np.arange(n, dtype=np.uint64) * np.uint64(top // 97 + 1)).astype(dt)}
        for name, v in cases.items():
            x = np.concatenate([v.view(np.uint8), np.arange(E - 1, dtype=np.uint8)])
            for S in (2, 3, 17):
                y, intact = run_dev(rx, torch, x, E, B, S, False)
                assert intact and np.array_equal(y, lag_planes_ref(x, E, B, S)), (E, B, name, S)
                back, intact = run_dev(rx, torch, y, E, B, S, True)
                assert intact and np.array_equal(back, x), (E, B, name, S)


def test_lag_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    from redux_amd import api
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for S in (0, 257, 1 << 20):
        for inverse in (0, 1):
            assert L.redux_lag_planes_dev(pa, pb, 4096, 64, 2, S, inverse, s) == lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(pa, pb, 4096, 64, 3, 1, 0, s) == lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(pa, pb, 4096, 0, 2, 1, 0, s) == lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 1, 0, s) == lib.INVALID_INPUT  # overlap
    torch.cuda.synchronize()
    assert bool((b == FILL).all())  # nothing was written
    assert L.redux_lag_planes_dev(pa, pb, 4096, 64, 1, 256, 0, s) == lib.OK
    torch.cuda.synchronize()
    with pytest.raises(rx.InvalidInput):
        api.lag_planes(a, 3, 64, 2, out=b)


# ---- streams: the plain coder on the transformed bytes, against the oracle ------------------------------------------------
@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("S", [2, 3])
def test_streams_equal_oracle_on_transformed_bytes(rx, E, S):
    import torch
    B = 4096
    x = interleaved(12 * B + 1000, S, E, seed=E + S)  # 13 blocks, the last one short
    want, wst = ox.compress_blocks(lag_planes_ref(x, E, B, S), B, PARAMS)
    assert not wst.any() and len(want) == 13
    out, offs, st = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S)   # the host-pointer call
    assert not st.any() and split(out, offs) == want, (E, S)
    enc = rx.DeviceEncoder(PARAMS, B, len(x), element_size=E, filter="lag", lag=S)           # redux_encode_lag_dev
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (E, S)
    dec = rx.DeviceDecoder(PARAMS, B, 13, element_size=E, filter="lag", lag=S)               # redux_decode_lag_dev
    back, sizes, dst, dsum = dec.decode(d_out[: int(offs[-1])], d_offs, length=len(x))
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and np.array_equal(back.cpu().numpy(), x)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=len(x), filter="lag", lag=S)
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)
    other = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S + 1)  # (the lag reaches the kernel)
    assert not np.array_equal(other[0], out)


def test_host_pipeline_over_several_chunks(rx):
    B, E, S = 4096, 4, 3
    x = interleaved(10 * 64 * B + 12345, S, E, seed=9)
    want = rx.compress_blocks(x, B, element_size=E, filter="lag", lag=S)  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B)[1] == 1
    ref, _ = ox.compress_blocks(lag_planes_ref(x, E, B, S)[: 70 * B], B, PARAMS)
    assert split(want[0], want[1])[:70] == ref
    try:
        rx.host_set_chunk_bytes(1 << 20, 1 << 20)  # 256 blocks a chunk, cut at frame boundaries
        assert rx.host_chunk_plan(nb, B)[1] >= 2
        got = rx.compress_blocks(x, B, element_size=E, filter="lag", lag=S)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        back, sizes, st = rx.decompress_blocks(got[0], got[1], B, element_size=E, length=len(x), filter="lag", lag=S)
        assert not st.any() and np.array_equal(back, x)
    finally:
        rx.host_set_chunk_bytes(0, 0)


# ---- a damaged stream -------------------------------------------------------------------------------------------------
def test_damaged_stream_stays_in_bounds_and_spares_other_frames(rx, lib):
    import torch
    B, E, S = 4096, 2, 3
    nfull = 6
    n = nfull * E * B + 1000  # 12 full blocks in 6 frames, then a short frame of one block of 1000 bytes
    F = E * B
    x = interleaved(n, S, E, seed=11)
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S)
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 13
    bad = list(streams)
    flipped = bytearray(streams[8])
    for k in range(3, len(flipped), 7):
        flipped[k] ^= 0xFF
    bad[8] = bytes(flipped[: len(flipped) // 2])  # flipped bytes, and an early end
    clean = [f for f in range(nfull) if f != 8 // E]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*PARAMS)
    wsb = L.redux_decode_lag_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    tg, d_out = guarded(torch, n, 5)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = L.redux_decode_lag_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E, S,
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
    rc = L.redux_decode_blocks_lag(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, S, hout.ctypes.data,
                                   hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [8]
    assert (hout[n:] == FILL).all()
    for f in clean:
        assert np.array_equal(hout[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_device_encoder_decoder_roundtrip_and_ranges(rx, E):
    import torch
    B, S = 4096, 3
    n = 4 * E * B + 3 * B + 5
    x = interleaved(n, S, E, seed=E)
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E, filter="lag", lag=S)
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, element_size=E, filter="lag", lag=S)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, filter="lag", lag=S)
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required, for E = 1 too
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_in)  # (the phases are the plain coder's)
    F = E * B
    ranges = [(2 * F - 7, 20), (3 * F - 1, 2)]  # two ranges, each across a frame boundary
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, ranges)
    torch.cuda.synchronize()
    h = got.cpu().numpy()
    for (s0, m), o in zip(ranges, where):
        assert np.array_equal(h[o: o + m], x[s0: s0 + m]), (E, s0, m)


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_with_the_filter(rx, tmp_path):
    from redux_amd import cli, container
    B = 4096
    x = channels(3, 2, 132).tobytes()  # three interleaved int16 walks: three frames and 300 elements
    src = tmp_path / "pcm.i16"
    src.write_bytes(x)
    zz, lg, back, part = tmp_path / "zigzag.rdxb", tmp_path / "lag.rdxb", tmp_path / "back.i16", tmp_path / "part.i16"
    common = ["-c", "-i", str(src), "--block-size", str(B), "--element-size", "2"]
    assert cli.main(common + ["-o", str(zz), "--filter", "zigzag"]) == 0
    assert cli.main(common + ["-o", str(lg), "--filter", "lag", "--lag", "3"]) == 0
    p11, p13 = zz.read_bytes(), lg.read_bytes()
    assert p11[4] == 11 and p13[4] == 13 and container.filter(p13) == "lag" and container.lag(p13) == 3
    assert container.element_size(p13) == 2
    print("3 interleaved int16 walks: --filter zigzag %d bytes, --filter lag --lag 3 %d bytes, %.3f x" % (len(p11), len(p13), len(p13) / len(p11)))
    assert len(p13) < len(p11)
    assert p13 == container.compress_bytes(x, B, element_size=2, filter="lag", lag=3)
    assert cli.main(["-d", "-i", str(lg), "-o", str(back)]) == 0
    assert back.read_bytes() == x
    F = 2 * B
    assert cli.main(["-d", "-i", str(lg), "-o", str(part), "--range", "%d:%d" % (2 * F + 100, 40)]) == 0  # inside the third frame
    assert part.read_bytes() == x[2 * F + 100: 2 * F + 140]
    assert container.decompress_range(p13, F - 3, 2 * F) == x[F - 3: 3 * F - 3]
    for checksum in (False, True):
        blob = container.compress_bytes(x, B, element_size=4, filter="lag", lag=4, checksum=checksum)
        assert blob[4] == (0x1D if checksum else 13) and container.lag(blob) == 4 and container.decompress_bytes(blob) == x
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, filter="lag", lag=4)) == b""
    assert cli.main(["-c", "-i", str(src), "-o", str(tmp_path / "x"), "--filter", "lag", "--lag", "3"]) == 1  # no block size


def test_cpp_lag_mirror(rx, tmp_path):
    import subprocess
    out = subprocess.run([build_lag_mirror_test(tmp_path), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lag mirror ok" in out.stdout, out.stdout + out.stderr
