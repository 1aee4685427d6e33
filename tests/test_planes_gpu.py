"""Byte-plane layout of typed data on the device: k_planes against the numpy restatement, the streams of every layer
against the plain coder on the transformed bytes (and the CPU oracle), round trips through the host pipeline, the
device coder objects, damaged streams, and the container / CLI end to end."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_cpu import bf16_data, lengths, planes_ref

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def split(out, offs):
    return [out[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


def typed(n, seed=3):
    """a mix of bf16, fp32 and int64 patterns: the layout must not care what the bytes are"""
    rng = np.random.default_rng(seed)
    a = bf16_data(n // 4 + 1, seed).tobytes()[: n // 2]
    b = (rng.standard_normal(n // 16 + 1).astype(np.float32)).tobytes()[: n // 4]
    c = rng.integers(0, 1 << 20, n // 32 + 1, dtype=np.int64).tobytes()
    return np.frombuffer((a + b + c)[:n].ljust(n, b"\x07"), dtype=np.uint8).copy()


def guarded(torch, n, offset=0):
    """a device buffer of n bytes at byte offset `offset` from a 256-byte boundary, with FILL guard bands on both sides"""
    t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    return t, t[GUARD + offset: GUARD + offset + n]


def guards_intact(t, n, offset=0):
    h = t.cpu().numpy()
    return bool((h[: GUARD + offset] == FILL).all() and (h[GUARD + offset + n:] == FILL).all())


# ---- k_planes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 4, 8])
@pytest.mark.parametrize("B", [4, 16, 65536, 4688])   # (4688: 293 groups a frame, a whole row of 256 and a ragged wave)
def test_planes_dev_matches_restatement(rx, E, B):
    import torch
    rng = np.random.default_rng(E * 7 + B)
    lens = lengths(E, B) + ([5 * E * B, 5 * E * B + E * 3 + 1] if B == 65536 else [])
    for L in lens:
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for so, do in ((0, 0), (3, 0), (0, 5), (1, 9)):  # aligned, unaligned source, unaligned destination, both
            for inverse in (False, True):
                ts, src = guarded(torch, L, so)
                if L:
                    src.copy_(torch.from_numpy(x).cuda())
                td, dst = guarded(torch, L, do)
                rx.planes(src, E, B, inverse=inverse, out=dst)
                torch.cuda.synchronize()
                want = planes_ref(x, E, B, inverse=inverse)
                assert np.array_equal(dst.cpu().numpy(), want), (E, B, L, so, do, inverse)
                assert guards_intact(td, L, do), (E, B, L, so, do, inverse)
                assert guards_intact(ts, L, so)


def test_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    assert L.redux_planes_dev(pa, pb, 4096, 64, 3, 0, s) == lib.INVALID_INPUT
    assert L.redux_planes_dev(pa, pb, 4096, 0, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 0, s) == lib.INVALID_INPUT  # overlap
    assert L.redux_planes_dev(pa, pb, 4096, 64, 1, 0, s) == lib.OK
    torch.cuda.synchronize()


# ---- streams: the plain coder on the transformed bytes ------------------------------------------------------------
@pytest.mark.parametrize("params,B", [((8, 30, 32), 65536), ((8, 14, 16), 65536), ((4, 10, 16), 4096)])
@pytest.mark.parametrize("E", [2, 4, 8])
def test_streams_equal_plain_coder_on_planes(rx, params, B, E):
    x = typed(2 * E * B + 3 * B + 77)
    out, offs, st = rx.compress_blocks(x, B, params, element_size=E)
    ref_out, ref_offs, _ = rx.compress_blocks(planes_ref(x, E, B), B, params)
    assert not st.any()
    assert split(out, offs) == split(ref_out, ref_offs)
    nb = len(offs) - 1
    y = planes_ref(x, E, B)
    for b in sorted({0, E - 1, E, nb - 1}):
        want, _ = ox.compress(y[b * B: (b + 1) * B].tobytes(), params)
        assert split(out, offs)[b] == want, (params, E, b)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, params, element_size=E, length=len(x))
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)


def test_element_size_one_is_byte_identical(rx, lib):
    import torch
    B = 65536
    x = typed(3 * B + 999)
    a = rx.compress_blocks(x, B)
    b = rx.compress_blocks(x, B, element_size=1)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    out, offs, _ = a
    plain, psizes, _ = rx.decompress_blocks(out, offs, B)
    d1, s1, _ = rx.decompress_blocks(out, offs, B, element_size=1, length=len(x))
    assert np.array_equal(d1, plain[: len(x)]) and np.array_equal(s1, psizes)
    d_in = torch.from_numpy(x).cuda()
    e0 = rx.DeviceEncoder((8, 30, 32), B, len(x))
    e1 = rx.DeviceEncoder((8, 30, 32), B, len(x), element_size=1)
    o0, f0, _, _ = e0.encode(d_in)
    o1, f1, _, _ = e1.encode(d_in)
    torch.cuda.synchronize()
    assert torch.equal(f0, f1) and torch.equal(o0[: int(f0[-1])], o1[: int(f1[-1])])
    assert e1.ws_bytes == e0.ws_bytes


# ---- the host pipeline: chunks and contexts ---------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 8])
def test_host_pipeline_many_chunks_and_two_contexts(rx, E):
    B = 4096
    x = typed(40 * 64 * B + 12345)  # 41 chunks of 64 blocks once the chunks are made small
    want = rx.compress_blocks(x, B, element_size=E)  # one chunk
    assert rx.host_chunk_plan(len(want[1]) - 1, B)[1] == 1
    try:
        rx.host_set_chunk_bytes(1, 1)  # 64 blocks a chunk
        assert rx.host_chunk_plan(len(want[1]) - 1, B)[1] > 8
        for devices in ([], [0, 0]):
            rx.host_set_devices(devices)
            got = rx.compress_blocks(x, B, element_size=E)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), devices
            back, sizes, st = rx.decompress_blocks(got[0], got[1], B, element_size=E, length=len(x))
            assert not st.any() and np.array_equal(back, x), devices
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)
    back, _, st = rx.decompress_blocks(want[0], want[1], B, element_size=E, length=len(x))
    assert not st.any() and np.array_equal(back, x)


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 4, 8])
def test_device_encoder_decoder_roundtrip(rx, E):
    import torch
    B = 65536
    n = 4 * E * B + 3 * B + 5
    x = typed(n, seed=E)
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder((8, 30, 32), B, n, element_size=E)
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, element_size=E)
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder((8, 30, 32), B, nb, element_size=E)
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)  # the original length is required


# ---- damaged and truncated streams ------------------------------------------------------------------------------------
def test_damaged_streams_stay_in_bounds_and_spare_other_frames(rx, lib):
    import torch
    E, B, params = 2, 4096, (8, 30, 32)
    n = 6 * E * B + 1000  # frames 0..5 full, frame 6 short (1000 bytes: one block)
    x = typed(n, seed=11)
    out, offs, _ = rx.compress_blocks(x, B, params, element_size=E)
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 6 * E + 1
    bad = list(streams)
    bad[3] = streams[-1]                   # frame 1: a valid stream of the wrong length (1000 bytes, not B)
    bad[8] = streams[8][: len(streams[8]) // 3]  # frame 4: truncated
    bad[nb - 1] = streams[nb - 1][:2]      # the short last frame: truncated
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*params)
    wsb = L.redux_decode_planes_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    for off in (0, 5):
        tg, d_out = guarded(torch, n, off)
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        st = L.redux_decode_planes_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E,
                                       C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()),
                                       C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(ws_ptr), wsb,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == lib.OK
        torch.cuda.synchronize()
        s = status.cpu().numpy()
        assert s[3] == lib.INVALID_INPUT and s[8] != lib.OK and s[nb - 1] != lib.OK
        assert [b for b in range(nb) if s[b] != lib.OK] == [3, 8, nb - 1]
        first_bad, nbad = summary.cpu().tolist()
        assert nbad == 3 and first_bad in (int(s[3]), int(s[8]), int(s[nb - 1]))
        assert guards_intact(tg, n, off)
        got = d_out.cpu().numpy()
        F = E * B
        for f in (0, 2, 3, 5):  # the frames whose blocks are all OK hold the original bytes
            assert np.array_equal(got[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f
    # the host-pointer call: same statuses, only out[0 .. n) written
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs = np.zeros(nb, dtype=np.uint32)
    hst = np.zeros(nb, dtype=np.int32)
    hoffs = boffs.astype(np.uint64)
    rc = L.redux_decode_blocks_planes(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, hout.ctypes.data,
                                      hs.ctypes.data, hst.ctypes.data)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [3, 8, nb - 1]
    assert (hout[n:] == FILL).all()
    for f in (0, 2, 3, 5):
        assert np.array_equal(hout[f * E * B: (f + 1) * E * B], x[f * E * B: (f + 1) * E * B]), f


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_with_element_size(rx, tmp_path):
    from redux_amd import cli, container
    x = bf16_data(1 << 19, seed=5)  # 1 MiB of bf16
    src = tmp_path / "w.bf16"
    src.write_bytes(x.tobytes())
    plain, planes, back = tmp_path / "plain.rdxb", tmp_path / "planes.rdxb", tmp_path / "back.bf16"
    assert cli.main(["-c", "-i", str(src), "-o", str(plain), "--block-size", "65536"]) == 0
    assert cli.main(["-c", "-i", str(src), "-o", str(planes), "--block-size", "65536", "--element-size", "2"]) == 0
    p1, p2 = plain.read_bytes(), planes.read_bytes()
    assert p1[4] == 1 and p2[4] == 2 and container.element_size(p2) == 2
    assert len(p2) < 0.92 * len(p1), (len(p1), len(p2))
    assert cli.main(["-d", "-i", str(planes), "-o", str(back)]) == 0
    assert back.read_bytes() == x.tobytes()
    assert container.decompress_bytes(container.compress_bytes(x.tobytes()[:-7], 65536, element_size=8)) == x.tobytes()[:-7]
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4)) == b""
    assert cli.main(["-c", "-i", str(src), "-o", str(tmp_path / "x"), "--element-size", "2"]) == 1
