"""Delta filter for integer series on the device: the fused and the general kernels against the numpy restatement, the
streams of every layer against the CPU oracle on the transformed bytes, the host pipeline over chunk sizes and contexts,
the device coder objects, damaged streams, checksums, and the container / CLI end to end."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_delta_cpu import delta_planes_ref, timestamps_i64
from test_planes_cpu import lengths, planes_ref
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


def series(n, seed=3):
    """n bytes of integer series: int64 timestamps, sorted int32 draws, an int16 random walk, and plain noise at the end"""
    rng = np.random.default_rng(seed)
    a = (1_700_000_000_000_000 + np.cumsum(rng.integers(900, 1100, n // 32 + 1))).astype("<u8").tobytes()[: n // 4]
    b = np.sort(rng.integers(0, 1 << 30, n // 16 + 1)).astype("<u4").tobytes()[: n // 4]
    c = np.cumsum(rng.normal(0, 50, n // 8 + 1)).astype(np.int64).astype("<i2").tobytes()[: n // 4]
    d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return np.frombuffer((a + b + c + d)[:n], dtype=np.uint8).copy()


def run_dev(rx, torch, x, E, B, inverse, so=0, do=0):
    """redux_delta_planes_dev of x between guarded buffers at the given byte offsets -> (result, guards intact)"""
    L = len(x)
    ts, src = guarded(torch, L, so)
    if L:
        src.copy_(torch.from_numpy(x).cuda())
    td, dst = guarded(torch, L, do)
    rx.delta_planes(src, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), guards_intact(td, L, do) and guards_intact(ts, L, so)


# ---- the kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [4096, 65536, 100, 48, 4688])   # (4688: 293 groups a frame: two iterations of the inverse,
def test_delta_planes_dev_matches_restatement(rx, E, B):      # the second a ragged wave; three frames and a short one do)
    import torch
    rng = np.random.default_rng(E * 7 + B)
    F, W = E * B, 1024 * E  # a frame; what one wave of the fused kernels covers
    lens = lengths(E, B) + [W - 1, W, W + 16 * E, 4 * W + 1, F + W, 2 * F - 1, 2 * F + W + E + 1, 5 * F, 5 * F + 3 * E + 1]
    if B == 4688:
        lens = [L for L in lens if L <= 3 * F + 5]
    for L in sorted(set(lens)):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for so, do in ((0, 0), (1, 0), (0, 1), (1, 1)):  # aligned, source / destination / both off by one byte
            for inverse in (False, True):
                got, intact = run_dev(rx, torch, x, E, B, inverse, so, do)
                assert np.array_equal(got, delta_planes_ref(x, E, B, inverse=inverse)), (E, B, L, so, do, inverse)
                assert intact, (E, B, L, so, do, inverse)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [65536, 100])
def test_delta_planes_dev_multi_mib(rx, E, B):
    import torch
    L = (3 << 20) + 5 * E + 3
    x = series(L, seed=E + B)
    for so, do in ((0, 0), (1, 1)):
        y, intact = run_dev(rx, torch, x, E, B, False, so, do)
        assert intact and np.array_equal(y, delta_planes_ref(x, E, B)), (E, B, so, do)
        back, intact = run_dev(rx, torch, y, E, B, True, do, so)
        assert intact and np.array_equal(back, x), (E, B, so, do)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_extreme_inputs(rx, E):
    import torch
    dt = np.dtype("<u%d" % E)
    top = (1 << 8 * E) - 1
    for B in (65536, 100):
        n = 3 * B + 17  # elements: three full frames and a short one
        cases = {"all 0xFF": np.full(n, top, dtype=dt),
                 "alternating 0 / max": np.where(np.arange(n) % 2 == 0, 0, top).astype(dt),
                 "alternating max / 0": np.where(np.arange(n) % 2 == 0, top, 0).astype(dt)}
        for name, v in cases.items():
            x = np.concatenate([v.view(np.uint8), np.arange(E - 1, dtype=np.uint8)])  # + trailing bytes
            for off in (0, 1):
                y, intact = run_dev(rx, torch, x, E, B, False, off, off)
                assert intact and np.array_equal(y, delta_planes_ref(x, E, B)), (E, B, name, off)
                back, intact = run_dev(rx, torch, y, E, B, True, off, off)
                assert intact and np.array_equal(back, x), (E, B, name, off)
                # the same bytes taken as DIFFERENCES: the running sum of a frame wraps B times and more
                s, intact = run_dev(rx, torch, x, E, B, True, off, off)
                assert intact and np.array_equal(s, delta_planes_ref(x, E, B, inverse=True)), (E, B, name, off)


def test_delta_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    assert L.redux_delta_planes_dev(pa, pb, 4096, 64, 3, 0, s) == lib.INVALID_INPUT
    assert L.redux_delta_planes_dev(pa, pb, 4096, 0, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_delta_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 0, s) == lib.INVALID_INPUT  # overlap
    assert L.redux_delta_planes_dev(pa, pb, 4096, 64, 1, 0, s) == lib.OK
    torch.cuda.synchronize()


# ---- streams: the plain coder on the transformed bytes, against the oracle ------------------------------------------------
@pytest.mark.parametrize("params", [(8, 30, 32), (8, 14, 16)])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_streams_equal_oracle_on_transformed_bytes(rx, params, E):
    import torch
    B = 65536
    x = series(2 * E * B + 3 * B + 77, seed=E)
    # (slot: a model of 14 frequency bits freezes inside a block and can cost 15 bits per symbol afterwards)
    want, wst = ox.compress_blocks(delta_planes_ref(x, E, B), B, params, slot=2 * B + 1024)
    assert not wst.any()
    out, offs, st = rx.compress_blocks(x, B, params, element_size=E, filter="delta")   # the host-pointer call
    assert not st.any() and split(out, offs) == want, (params, E)
    enc = rx.DeviceEncoder(params, B, len(x), element_size=E, filter="delta")           # the device call
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (params, E)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, params, element_size=E, length=len(x), filter="delta")
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)


def test_without_the_filter_nothing_changes(rx):
    import torch
    B = 65536
    x = series(3 * 4 * B + 999)
    for E in (1, 2, 4):
        a = rx.compress_blocks(x, B, element_size=E)
        b = rx.compress_blocks(x, B, element_size=E, filter=None)
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
        ref_out, ref_offs, _ = rx.compress_blocks(planes_ref(x, E, B), B)
        assert split(a[0], a[1]) == split(ref_out, ref_offs)
        d0, s0, _ = rx.decompress_blocks(a[0], a[1], B, element_size=E, length=len(x))
        d1, s1, _ = rx.decompress_blocks(a[0], a[1], B, element_size=E, length=len(x), filter=None)
        assert np.array_equal(d0, x) and np.array_equal(d1, x) and np.array_equal(s0, s1)
        d_in = torch.from_numpy(x).cuda()
        e0 = rx.DeviceEncoder((8, 30, 32), B, len(x), element_size=E)
        e1 = rx.DeviceEncoder((8, 30, 32), B, len(x), element_size=E, filter=None)
        o0, f0, _, _ = e0.encode(d_in)
        o1, f1, _, _ = e1.encode(d_in)
        torch.cuda.synchronize()
        assert e0.ws_bytes == e1.ws_bytes and torch.equal(f0, f1) and torch.equal(o0[: int(f0[-1])], o1[: int(f1[-1])])
        assert np.array_equal(o0[: int(f0[-1])].cpu().numpy(), a[0])


# ---- the host pipeline: chunks and contexts ---------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 8])
def test_host_pipeline_chunk_sizes_and_two_contexts(rx, E):
    B = 4096
    x = series(40 * 64 * B + 12345, seed=E)
    want = rx.compress_blocks(x, B, element_size=E, filter="delta")  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B)[1] == 1
    ref, _ = ox.compress_blocks(delta_planes_ref(x, E, B)[: 70 * B], B, (8, 30, 32))
    assert split(want[0], want[1])[:70] == ref
    plans = set()
    try:
        for chunk in (1, 1 << 20, 3 << 20, 16 << 20):  # 64, 256, 768 and 4096 blocks a chunk
            rx.host_set_chunk_bytes(chunk, chunk)
            plans.add(rx.host_chunk_plan(nb, B)[0])
            for devices in ([], [0, 0]):
                rx.host_set_devices(devices)
                got = rx.compress_blocks(x, B, element_size=E, filter="delta")
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (chunk, devices)
                back, sizes, st = rx.decompress_blocks(got[0], got[1], B, element_size=E, length=len(x), filter="delta")
                assert not st.any() and np.array_equal(back, x), (chunk, devices)
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)
    assert len(plans) == 4, plans


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_device_encoder_decoder_roundtrip(rx, E):
    import torch
    B = 65536
    n = 4 * E * B + 3 * B + 5
    x = series(n, seed=E)
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder((8, 30, 32), B, n, element_size=E, filter="delta")
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, element_size=E, filter="delta")
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder((8, 30, 32), B, nb, element_size=E, filter="delta")
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required, for E = 1 too
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_in)  # (the phases are the plain coder's)


# ---- damaged and truncated streams ------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2])
def test_damaged_streams_stay_in_bounds_and_spare_other_frames(rx, lib, E):
    import torch
    B, params = 4096, (8, 30, 32)
    nfull = 12 // E
    n = nfull * E * B + 1000  # 12 full blocks in nfull frames, then a short frame of one block of 1000 bytes
    x = series(n, seed=11)
    out, offs, _ = rx.compress_blocks(x, B, params, element_size=E, filter="delta")
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 13
    bad = list(streams)
    bad[3] = streams[-1]                         # a valid stream of the wrong length (1000 bytes, not B)
    bad[8] = streams[8][: len(streams[8]) // 3]  # truncated
    bad[nb - 1] = streams[nb - 1][:2]            # the short last frame: truncated
    hit = {3 // E, 8 // E}
    clean = [f for f in range(nfull) if f not in hit]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*params)
    wsb = L.redux_decode_delta_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    F = E * B
    for off in (0, 5):
        tg, d_out = guarded(torch, n, off)
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        st = L.redux_decode_delta_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E,
                                      C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()),
                                      C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(ws_ptr), wsb,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == lib.OK
        torch.cuda.synchronize()
        s = status.cpu().numpy()
        assert s[3] == lib.INVALID_INPUT and [b for b in range(nb) if s[b] != lib.OK] == [3, 8, nb - 1]
        first_bad, nbad = summary.cpu().tolist()
        assert nbad == 3 and first_bad in (int(s[3]), int(s[8]), int(s[nb - 1]))
        assert guards_intact(tg, n, off)
        got = d_out.cpu().numpy()
        for f in clean:  # the frames whose blocks are all OK hold the original bytes
            assert np.array_equal(got[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f
    # the host-pointer call: same statuses, only out[0 .. n) written
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs = np.zeros(nb, dtype=np.uint32)
    hst = np.zeros(nb, dtype=np.int32)
    hoffs = boffs.astype(np.uint64)
    rc = L.redux_decode_blocks_delta(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, hout.ctypes.data,
                                     hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [3, 8, nb - 1]
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
    out, offs, st = rx.compress_blocks(x, B, element_size=E, block_crc=crc, filter="delta")
    assert np.array_equal(crc, want)
    plain = rx.compress_blocks(x, B, element_size=E, filter="delta")
    assert np.array_equal(out, plain[0]) and np.array_equal(offs, plain[1])  # the streams do not depend on block_crc
    got = np.zeros(nb, dtype=np.uint32)
    back, _, st2 = rx.decompress_blocks(out, offs, B, element_size=E, length=len(x), block_crc=got, filter="delta")
    assert not st2.any() and np.array_equal(back, x) and np.array_equal(got, want)


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_with_the_filter(rx, tmp_path):
    from redux_amd import cli, container
    x = timestamps_i64()  # 2 MiB of int64 timestamps
    src = tmp_path / "t.i64"
    src.write_bytes(x.tobytes())
    planes, delta, back = tmp_path / "planes.rdxb", tmp_path / "delta.rdxb", tmp_path / "back.i64"
    assert cli.main(["-c", "-i", str(src), "-o", str(planes), "--block-size", "65536", "--element-size", "8"]) == 0
    assert cli.main(["-c", "-i", str(src), "-o", str(delta), "--block-size", "65536", "--element-size", "8", "--filter", "delta",
                     "--checksum"]) == 0
    p2, p6 = planes.read_bytes(), delta.read_bytes()
    assert p2[4] == 2 and p6[4] == 0x16 and container.filter(p6) == "delta" and container.element_size(p6) == 8
    assert container.filter(p2) is None
    assert len(p6) < 0.5 * len(p2), (len(p2), len(p6))
    assert cli.main(["-d", "-i", str(delta), "-o", str(back)]) == 0
    assert back.read_bytes() == x.tobytes()
    for E in (1, 2, 4, 8):
        y = x.tobytes()[: 5 * 65536 + 13]
        blob = container.compress_bytes(y, 4096, element_size=E, filter="delta")
        assert blob[4] == 6 and container.decompress_bytes(blob) == y
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, filter="delta")) == b""
    assert container.compress_bytes(x.tobytes()[:70000], 65536, element_size=8) == \
        container.compress_bytes(x.tobytes()[:70000], 65536, element_size=8, filter=None)
    assert cli.main(["-c", "-i", str(src), "-o", str(tmp_path / "x"), "--filter", "delta"]) == 1
