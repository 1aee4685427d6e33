"""Snapshot-stride filter on the device: the fused, the byte and the running-sum kernels against the numpy restatement, with
the kernel names telling the paths apart; one transform past 2^32 bytes checked on the device; the streams of both encode
calls against the CPU oracle on the transformed bytes, checksums, a damaged stream, the device coder objects, the container and
the CLI end to end."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_gpu import FILL, guarded, guards_intact, split
from test_stride_cpu import PARAMS, series, stride_planes_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def run_dev(rx, torch, x, E, B, S, inverse, so=0, do=0):
    """stride_planes of x between guarded buffers at the given byte offsets (FILL in front of the source: a predecessor read
    from there would show in the result) -> (result, guards and source intact, the kernels' names)"""
    L = len(x)
    ts, src = guarded(torch, L, so)
    src.copy_(torch.from_numpy(x).cuda())
    td, dst = guarded(torch, L, do)
    rx.stride_planes(src, E, B, S, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    intact = guards_intact(td, L, do) and guards_intact(ts, L, so) and np.array_equal(src.cpu().numpy(), x)
    return dst.cpu().numpy(), intact, rx.stride_kernel_name(L, B, E, S, inverse, src, dst)


def check(rx, torch, x, E, B, S, so=0, do=0):
    """forward against the restatement, and the inverse of the restatement's output against x -> the two name strings"""
    z = stride_planes_ref(x, E, S, B)
    got, intact, fwd = run_dev(rx, torch, x, E, B, S, False, so, do)
    assert intact, (E, B, S, len(x), so, do)
    if not np.array_equal(got, z):
        at = int(np.nonzero(got != z)[0][0])
        raise AssertionError(f"forward E={E} B={B} S={S} len={len(x)} offsets={(so, do)} [{fwd}]: first difference at byte {at}")
    back, intact, inv = run_dev(rx, torch, z, E, B, S, True, so, do)
    assert intact, (E, B, S, len(x), so, do)
    if not np.array_equal(back, x):
        at = int(np.nonzero(back != x)[0][0])
        raise AssertionError(f"inverse E={E} B={B} S={S} len={len(x)} offsets={(so, do)} [{inv}]: first difference at byte {at}")
    return fwd, inv


# ---- the transform, byte for byte against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("B", [4096, 65536, 100])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_stride_planes_dev_matches_restatement(rx, E, B):
    import torch
    rng = np.random.default_rng(E * 100003 + B)
    F = E * B
    L = 3 * F + 3 * E + (1 if E > 1 else 0)  # three frames, a short one of three elements, and a trailing byte
    n = L // E
    x = rng.integers(0, 256, L, dtype=np.uint8)
    # S*E below 16, 16, a 16-multiple, one element off it, one frame, one frame and an element, about 40 snapshots, 3, 2, 1
    strides = sorted({1, 3, max(16 // E, 1), 1024, 1025, B, B + 1, max(n // 40, 1), n // 2 - 1, n - 1, n, n + 7})
    for S in strides:
        fwd, inv = check(rx, torch, x, E, B, S)
        if B % 16 == 0:
            assert fwd == "k_stride_planes + k_stride_planes_bytes", (S, fwd)
            assert inv.startswith("copy" if E == 1 else "k_planes + k_planes_bytes"), (S, inv)
        else:
            assert fwd == "k_stride_planes_bytes" and inv.startswith("copy" if E == 1 else "k_planes_bytes"), (S, fwd, inv)
        if S >= n:
            assert "k_stride_sum" not in inv, (S, inv)
        elif S * E % 16 == 0:
            assert "k_stride_sum" in inv and "_bytes" not in inv.replace("k_planes_bytes", ""), (S, inv)
        else:
            assert "k_stride_sum_bytes" in inv, (S, inv)
    for S in (3, 1024, 1025, B, n - 1):  # source and destination a byte off, each alone and both
        for so, do in ((1, 0), (0, 1), (1, 1)):
            fwd, inv = check(rx, torch, x, E, B, S, so, do)
            assert fwd == "k_stride_planes_bytes", (S, so, do, fwd)
            if do and S < n:
                assert "k_stride_sum_bytes" in inv, (S, so, do, inv)
    # full frames only, and less than one frame
    check(rx, torch, x[: 2 * F], E, B, B)
    check(rx, torch, x[: F - E - 1], E, B, 5)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_time_segments_carry_across_every_edge(rx, E):
    """S = 3 over 100,003 elements (a column is an element) and S = 64 over 2^22 elements (a column is a chunk where 64*E is a
    16-byte multiple): both cut time into segments, and a wrong carry at any segment edge shows in everything behind it"""
    import torch
    rng = np.random.default_rng(E)
    for S, n, tail in ((3, 100003, 1), (64, 1 << 22, 0)):
        x = rng.integers(0, 256, n * E + (tail if E > 1 else 0), dtype=np.uint8)
        fwd, inv = check(rx, torch, x, E, 4096, S)
        if S == 3:
            assert "k_stride_totals_bytes + k_stride_scan_bytes + k_stride_sum_bytes" in inv, inv
        else:
            assert "k_stride_totals + k_stride_scan + k_stride_sum" in inv, inv


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_the_extremes_of_the_fold(rx, E):
    import torch
    B, n = 4096, 3 * 4096 + 17
    dt = np.dtype("<u%d" % E)
    top, half = (1 << 8 * E) - 1, 1 << (8 * E - 1)
    alternating = lambda a, b: np.array([a, b], dtype=dt)[np.arange(n) % 2]
    cases = {"zeros": np.zeros(n, dtype=dt), "all ones": np.full(n, top, dtype=dt), "0 / max": alternating(0, top),
             "half / 0": alternating(half, 0), "max / 1": alternating(top, 1)}
    for name, v in cases.items():
        x = v.view(np.uint8).copy()
        for S in (1, 3, 16, 1025):
            check(rx, torch, x, E, B, S)
        back, intact, _ = run_dev(rx, torch, x, E, B, 4, True)  # the same buffers taken as FOLDED input of the inverse
        assert intact and np.array_equal(back, stride_planes_ref(x, E, 4, B, inverse=True)), name


def test_stride_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    L = lib.lib()
    a = torch.full((8192,), 7, dtype=torch.uint8, device="cuda:0")
    b = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    call = lambda src, dst, n, B, E, S, inv=0, ws=None, wsb=0: L.redux_stride_planes_dev(src, dst, n, B, E, S, inv, ws, wsb, s)
    for E, S in ((0, 1), (3, 1), (16, 1), (4, 0)):
        assert call(v(a), v(b), 4096, 4096, E, S) == lib.INVALID_INPUT
    assert call(v(a), v(b), 4096, 0, 4, 1) == lib.INVALID_INPUT
    assert call(None, v(b), 4096, 4096, 4, 1) == lib.INVALID_INPUT and call(v(a), None, 4096, 4096, 4, 1) == lib.INVALID_INPUT
    assert call(v(a), v(a), 4096, 4096, 4, 1) == lib.INVALID_INPUT and call(v(a), v(a, 4095), 4096, 4096, 4, 1) == lib.INVALID_INPUT
    # the inverse at a small stride needs its workspace, and says so before it writes anything
    need = L.redux_stride_workspace_bytes(8192, 4, 1)
    assert need > 0 and call(v(a), v(b), 8192, 4096, 4, 1, 1) == lib.OUTPUT_TOO_SMALL
    torch.cuda.synchronize()
    assert bool((b == FILL).all())
    assert call(v(a), v(b), 0, 4096, 4, 1) == lib.OK and call(None, None, 0, 4096, 4, 1, 1) == lib.OK


# ---- one transform past 2^32 bytes, checked on the device ----------------------------------------------------------------
def test_transform_past_4gib_against_torch_on_the_device(rx):
    import torch
    n_bytes, E, B, S = (1 << 32) + (1 << 20) + 3, 4, 65536, (1 << 28) + 5
    free, _ = torch.cuda.mem_get_info()
    if free < 9 * n_bytes:
        print(f"skipped: {free} bytes of device memory free, the case wants {9 * n_bytes}")
        pytest.skip("not enough free device memory for the case past 2^32 bytes")
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    x = torch.randint(0, 256, (n_bytes,), dtype=torch.uint8, device="cuda:0", generator=g)
    n, F = n_bytes // E, E * B
    v = x[: n * E].view(torch.int32)
    want = x.clone()
    w = want[: n * E].view(torch.int32)
    d = v[S:] - v[:-S]
    w[S:] = (d << 1) ^ (d >> 31)
    del d
    nf = n_bytes // F
    ref = want.clone()
    ref[: nf * F] = want[: nf * F].view(nf, B, E).transpose(1, 2).reshape(-1)
    last = n_bytes - nf * F
    ref[nf * F: nf * F + last // E * E] = want[nf * F: nf * F + last // E * E].view(last // E, E).t().reshape(-1)
    del want, w
    got = rx.stride_planes(x, E, B, S)
    assert torch.equal(got, ref)
    assert rx.stride_kernel_name(n_bytes, B, E, S, False, x, got) == "k_stride_planes + k_stride_planes_bytes"
    del got
    back = rx.stride_planes(ref, E, B, S, inverse=True)
    assert torch.equal(back, x)
    assert "k_stride_sum_bytes" in rx.stride_kernel_name(n_bytes, B, E, S, True, ref, back)  # (S*E = 2^30 + 20: no 16-multiple)


# ---- the coder behind it -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trajectory():
    """the trajectory of the value claim, its streams on the CPU oracle behind the restatement, at B = 4096"""
    data, E, S = series()["trajectory"]
    x = np.frombuffer(data, dtype=np.uint8).copy()
    z = stride_planes_ref(x, E, S, 4096)
    want, _ = ox.compress_blocks(z.tobytes(), 4096, PARAMS)
    return x, E, S, 4096, want


def test_streams_of_both_encode_calls_equal_the_oracle_on_the_transformed_bytes(rx, trajectory):
    import torch
    x, E, S, B, want = trajectory
    nb = len(want)
    crc = np.zeros(nb, dtype=np.uint32)
    out, offs, status = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="stride", stride=S, block_crc=crc)
    assert not status.any() and split(out, offs) == want
    assert crc.tolist() == [zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)]
    dcrc = np.zeros(nb, dtype=np.uint32)
    back, sizes, st = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=len(x), filter="stride", stride=S, block_crc=dcrc)
    assert not st.any() and np.array_equal(back, x) and np.array_equal(dcrc, crc)
    # the device coder objects: redux_encode_stride_dev / redux_decode_stride_dev
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, len(x), element_size=E, filter="stride", stride=S)
    d_out, d_offs, d_status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and np.array_equal(d_offs.cpu().numpy().astype(np.uint64), offs)
    assert np.array_equal(d_out[: int(offs[-1])].cpu().numpy(), out)
    dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, filter="stride", stride=S)
    d_back, _, _, dsum = dec.decode(d_out[: int(offs[-1])], d_offs, length=len(x))
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(d_back, d_in)
    with pytest.raises(rx.InvalidInput):
        dec.decode(d_out, d_offs)  # the original length is required
    with pytest.raises(rx.Unsupported):
        dec.decode_ranges(d_out[: int(offs[-1])], offs, len(x), [(0, 16)])


@pytest.mark.parametrize("E,S", [(1, 5000), (4, 3), (2, 4096)])
def test_round_trips_at_small_and_odd_shapes(rx, E, S):
    """a small stride (the segmented sums behind the decoder), a stride of one frame, and element size 1, host and device"""
    import torch
    rng = np.random.default_rng(E + S)
    B = 4096
    n = 11 * E * B + 5 * E + (E > 1)
    x = np.cumsum(rng.integers(-3, 4, n), dtype=np.int64).astype(np.uint8)
    z = stride_planes_ref(x, E, S, B)
    want, _ = ox.compress_blocks(z.tobytes(), B, PARAMS)
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="stride", stride=S)
    assert split(out, offs) == want
    back, _, st = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=n, filter="stride", stride=S)
    assert not st.any() and np.array_equal(back, x)
    dec = rx.DeviceDecoder(PARAMS, B, len(want), element_size=E, filter="stride", stride=S)
    d_back, _, _, dsum = dec.decode(torch.from_numpy(out).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and np.array_equal(d_back.cpu().numpy(), x)


def test_a_damaged_stream_is_reported_and_stays_in_bounds(rx, lib):
    import torch
    E, B, S = 1, 4096, 3 * 4096  # (E = 1: block b holds bytes [b*B, (b+1)*B), so "the blocks before it" are bytes)
    rng = np.random.default_rng(77)
    n = 9 * B + 1000
    x = np.cumsum(rng.integers(-2, 3, n), dtype=np.int64).astype(np.uint8)
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="stride", stride=S)
    streams = split(out, offs)
    nb = len(streams)
    bad = list(streams)
    bad[4] = streams[4][: len(streams[4]) // 3]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*PARAMS)
    wsb = L.redux_decode_stride_workspace_bytes(C.byref(cp), n, B, E, S)
    assert wsb >= L.redux_decode_planes_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data, d_offs = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(boffs).cuda()
    for off in (0, 5):
        tg, d_out = guarded(torch, n, off)
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        args = (C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E, S, C.c_void_p(d_out.data_ptr()),
                C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(ws_ptr))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.redux_decode_stride_dev(*args, wsb - 256, stream) == lib.OUTPUT_TOO_SMALL  # (less than the size asked for)
        assert L.redux_decode_stride_dev(*args, wsb, stream) == lib.OK
        torch.cuda.synchronize()
        s = status.cpu().numpy()
        assert [b for b in range(nb) if s[b] != lib.OK] == [4] and summary.cpu().tolist()[1] == 1
        assert guards_intact(tg, n, off)
        got = d_out.cpu().numpy()
        assert np.array_equal(got[: 4 * B], x[: 4 * B])                    # the blocks before it
        assert np.array_equal(got[5 * B: 7 * B], x[5 * B: 7 * B])          # and what does not descend from it: S = 3 blocks
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs, hst = np.zeros(nb, dtype=np.uint32), np.zeros(nb, dtype=np.int32)
    hoffs = boffs.astype(np.uint64)
    rc = L.redux_decode_blocks_stride(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, S, hout.ctypes.data, hs.ctypes.data,
                                      hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [4]
    assert (hout[n:] == FILL).all() and np.array_equal(hout[: 4 * B], x[: 4 * B])


def test_host_pair_does_not_depend_on_the_chunk_size(rx, lib, trajectory):
    """the pair stages the whole buffer: the test hook that shrinks the chunks of every other host call changes nothing"""
    x, E, S, B, want = trajectory
    L = lib.lib()
    L.redux_host_set_chunk_bytes(64 * B, 64 * B)
    try:
        out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="stride", stride=S)
        back, _, st = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=len(x), filter="stride", stride=S)
    finally:
        L.redux_host_set_chunk_bytes(0, 0)
    assert split(out, offs) == want and not st.any() and np.array_equal(back, x)


# ---- container and CLI -----------------------------------------------------------------------------------------------------
def test_container_and_cli_end_to_end(rx, tmp_path, trajectory):
    from redux_amd import cli, container
    x, E, S, B, want = trajectory
    payload = sum(len(s) for s in want)
    for checksum in (False, True):
        buf = container.compress_bytes(x.tobytes(), B, PARAMS, element_size=E, filter="stride", stride=S, checksum=checksum)
        assert buf[4] == (0x1F if checksum else 0x0F) and container.stride(buf) == (E, S) and container.record(buf) is None
        nb = len(want)
        assert len(buf) == payload + container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="stride")
        assert container.decompress_bytes(buf) == x.tobytes()
    src, packed, back = tmp_path / "traj.f32", tmp_path / "traj.rdxb", tmp_path / "back.f32"
    src.write_bytes(x.tobytes())
    common = ["-c", "-i", str(src), "--block-size", str(B), "--filter", "stride", "--stride", str(S), "--element-size", str(E)]
    assert cli.main(common + ["-o", str(packed)]) == 0
    assert packed.read_bytes() == container.compress_bytes(x.tobytes(), B, PARAMS, element_size=E, filter="stride", stride=S)
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == x.tobytes()
    assert cli.main(common + ["-o", str(packed), "--checksum"]) == 0 and packed.read_bytes()[4] == 0x1F
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == x.tobytes()
    with pytest.raises(rx.Unsupported):
        container.decompress_range(packed.read_bytes(), 0, 16)
