"""Higher-order lagged differences on the device: the fused and the byte kernels against the numpy restatement for orders 1 to
3 and lags at every step of the inverse's scan and at either side of a 16-byte chunk, the lag kernels at order 1, the streams
of every layer against the CPU oracle on the transformed bytes, the host pipeline over chunks, a damaged stream, the device
coder objects and their range reads, and the container / CLI end to end."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox
from test_lag_gpu import interleaved
from test_lag_order_cpu import build_lag_order_mirror_test, lag_order_planes_ref, tones
from test_planes_gpu import FILL, GUARD, guarded, guards_intact, split

pytestmark = pytest.mark.gpu

PARAMS = (8, 30, 32)
# the scan's steps; j*S*E below, at and above 16 bytes; 3S at either side of 256 (85, 86); S = 30 with N = 64: 2S <= N < 3S
LAGS = [1, 2, 3, 5, 15, 16, 17, 30, 64, 85, 86, 255, 256]
FRONT = 8192  # poison in front of a source: more than the 3 * 256 * 8 bytes the farthest predecessor lies back


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def poisoned(torch, x, offset=0):
    """x on the device at byte offset `offset` from a 256-byte boundary, FRONT bytes of FILL in front of it and a guard
    band behind -> (whole buffer, view of x)"""
    n = len(x)
    t = torch.full((FRONT + n + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    v = t[FRONT + offset: FRONT + offset + n]
    if n:
        v.copy_(torch.from_numpy(x).cuda())
    return t, v


def poison_intact(t, n, offset=0):
    h = t.cpu().numpy()
    return bool((h[: FRONT + offset] == FILL).all() and (h[FRONT + offset + n:] == FILL).all())


def run_dev(torch, x, E, B, S, K, inverse, so=0, do=0, lag_only=False):
    """redux_lag_order_planes_dev (lag_only: redux_lag_planes_dev) of x between guarded buffers at the given byte offsets
    -> (result, guards intact)"""
    from redux_amd import api
    L = len(x)
    ts, src = poisoned(torch, x, so)
    td, dst = guarded(torch, L, do)
    if lag_only:
        api.lag_planes(src, E, B, S, inverse=inverse, out=dst)
    else:
        api.lag_order_planes(src, E, B, S, K, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), guards_intact(td, L, do) and poison_intact(ts, L, so)


# ---- the kernels ----------------------------------------------------------------------------------------------------
# B = 64: 4 groups a frame, N = 64; 4096: exactly one row of the inverse; 4112: a row and a group: the per-level carries;
# 8192: two full rows; 12304: three rows and a group: the carries again and, for lags that do not divide 4096, the moving chain
# phase; 100 and 4099: the byte kernels, the buffers also one byte off.  Two full frames, a short one and trailing bytes each;
# at 4099 also a short frame of E * B - 1 bytes, one byte less than a full one.
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [64, 4096, 4112, 8192, 12304, 100, 4099])
def test_lag_order_planes_dev_matches_restatement(rx, E, B, K):
    import torch
    rng = np.random.default_rng(E * 7 + B + K)
    L = 2 * E * B + (B // 3 + 1) * E + (E - 1)
    x = rng.integers(0, 256, L, dtype=np.uint8)
    offsets = ((0, 0), (1, 0), (0, 1)) if B in (100, 4099) else ((0, 0),)
    for S in LAGS:
        if B == 4099 and S in (1, 3, 255, 256):
            xs = x[: 3 * E * B - 1]
            for inverse in (False, True):
                got, intact = run_dev(torch, xs, E, B, S, K, inverse, 1, 0)
                assert intact and np.array_equal(got, lag_order_planes_ref(xs, E, B, S, K, inverse=inverse)), (E, B, S, K, inverse)
        want = {inverse: lag_order_planes_ref(x, E, B, S, K, inverse=inverse) for inverse in (False, True)}
        for so, do in offsets:
            for inverse in (False, True):
                got, intact = run_dev(torch, x, E, B, S, K, inverse, so, do)
                assert np.array_equal(got, want[inverse]), (E, B, S, K, so, do, inverse)
                assert intact, (E, B, S, K, so, do, inverse)
        if K == 1:  # order 1 is the lag filter, kernel against kernel on the same bytes
            for inverse in (False, True):
                g, _ = run_dev(torch, x, E, B, S, 1, inverse, lag_only=True)
                assert np.array_equal(g, want[inverse]), (E, B, S, inverse)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lag_order_kernels_on_extremes(rx, E):
    """all-ones elements and 0 alternating with the largest value: every coefficient of the sum wraps; and interleaved walks"""
    import torch
    dt = np.dtype("<u%d" % E)
    top = (1 << 8 * E) - 1
    for B in (4112, 100):
        n = 2 * B + 17
        cases = {"all max": np.full(n, top, dtype=dt), "0 / max": np.array([0, top], dtype=dt)[np.arange(n) % 2],
                 "walks": interleaved(n * E, 3, E).view(dt)}
        for name, v in cases.items():
            x = np.concatenate([v.view(np.uint8), np.arange(E - 1, dtype=np.uint8)])
            for K in (2, 3):
                for S in (1, 2, 3, 17):
                    y, intact = run_dev(torch, x, E, B, S, K, False)
                    assert intact and np.array_equal(y, lag_order_planes_ref(x, E, B, S, K)), (E, B, name, S, K)
                    back, intact = run_dev(torch, y, E, B, S, K, True)
                    assert intact and np.array_equal(back, x), (E, B, name, S, K)


def test_lag_order_planes_dev_rejects_bad_arguments(rx, lib):
    import torch
    from redux_amd import api
    L = lib.lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pa, pb = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr())
    for S, K in ((0, 2), (257, 2), (3, 0), (3, 4), (3, 1 << 20)):
        for inverse in (0, 1):
            assert L.redux_lag_order_planes_dev(pa, pb, 4096, 64, 2, S, K, inverse, s) == lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(pa, pb, 4096, 64, 3, 1, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(pa, pb, 4096, 0, 2, 1, 2, 0, s) == lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(pa, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 1, 2, 0, s) == lib.INVALID_INPUT  # overlap
    torch.cuda.synchronize()
    assert bool((b == FILL).all())  # nothing was written
    assert L.redux_lag_order_planes_dev(pa, pb, 4096, 64, 1, 256, 3, 0, s) == lib.OK
    torch.cuda.synchronize()
    with pytest.raises(rx.InvalidInput):
        api.lag_order_planes(a, 3, 64, 2, 2, out=b)


# ---- several frames per workgroup and per wave ------------------------------------------------------------------------
# The tests above give every input two full frames and a short one: no workgroup of the inverse kernels walks on to a second
# frame (carry[K][S], tot, last[K][2][256], par and the tile as the frame before left them), no wave of the forward kernel
# holds more than two frames (gi % frame_groups), and a frame has 4, 256, 257 or 769 groups.
def first_difference(got, want, E, B):
    at = int(np.nonzero(got != want)[0][0])
    return f"first difference at byte {at} (frame {at // (E * B)}, offset {at % (E * B)})"


# Frames of 1, 3, 5, 63 and 65 groups (N = B elements).  The lags: 1, 2, 3 and 17 always; for the three small frames S, 2S
# and 3S below, at (where N divides) and above N, up to S >= N where only the fold is left; for the two large ones 3S stays
# below N (S <= 256), so the scan's last steps, 3S at either side of 256 and a 16-byte chunk.
MANY_FRAMES_LAGS = {16: [1, 2, 3, 5, 6, 7, 8, 9, 15, 16, 17, 256], 48: [1, 2, 3, 15, 16, 17, 23, 24, 25, 47, 48, 49],
                    80: [1, 2, 3, 17, 26, 27, 39, 40, 41, 79, 80, 81], 1008: [1, 2, 3, 16, 17, 85, 86, 255, 256],
                    1040: [1, 2, 3, 16, 17, 85, 86, 255, 256]}


def test_the_lags_of_the_short_frames_lie_on_every_side_of_the_frame():
    for B, lags in MANY_FRAMES_LAGS.items():
        assert {1, 2, 3, 17} <= set(lags) and all(1 <= S <= 256 for S in lags) and B % 16 == 0
        for j in (1, 2, 3):
            sides = {(j * S > B) - (j * S < B) for S in lags}
            assert sides == ({-1} if 3 * 256 < B else {-1, 0, 1} if B % j == 0 else {-1, 1}), (B, j)
    assert [B // 16 for B in MANY_FRAMES_LAGS] == [1, 3, 5, 63, 65]


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", sorted(MANY_FRAMES_LAGS))
def test_lag_order_kernels_at_many_short_frames(rx, E, B, K):
    """203 full frames, a short one and E - 1 trailing bytes; frames of 1, 3 and 5 groups put up to 64 frames into one wave of
    k_lag_order_planes, 63 and 65 groups let every wave start at another group of its frame; both directions."""
    import torch
    nf = 203
    x = np.random.default_rng(E * 7 + B + K).integers(0, 256, nf * E * B + (B // 3 + 1) * E + (E - 1), dtype=np.uint8)
    for S in MANY_FRAMES_LAGS[B]:
        for inverse in (False, True):
            want = lag_order_planes_ref(x, E, B, S, K, inverse=inverse)
            got, intact = run_dev(torch, x, E, B, S, K, inverse)
            assert np.array_equal(got, want), f"E={E} B={B} S={S} K={K} inverse={inverse}: " + first_difference(got, want, E, B)
            assert intact, (E, B, S, K, inverse)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [65520, 65552, 100_000, 1 << 20])
def test_lag_order_kernels_at_frames_that_end_inside_a_turn(rx, E, B, K):
    """Three full frames and a short one (a third of a frame, five elements and E - 1 trailing bytes), as for the order-1
    kernels: uniform bytes, whose K-fold running sums wrap mod 2^(8E) every few elements, in the partial last turn of every
    frame too; and all-0xFF bytes.  S = 3, 255 and 256, both directions."""
    import torch
    rng = np.random.default_rng(E * 1000 + B % 997 + K)
    n = 3 * E * B + (B // 3 + 5) * E + E - 1
    for x in (rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0xFF, np.uint8)):
        for S in (3, 255, 256):
            for inverse in (False, True):
                want = lag_order_planes_ref(x, E, B, S, K, inverse=inverse)
                got, intact = run_dev(torch, x, E, B, S, K, inverse)
                assert np.array_equal(got, want), f"E={E} B={B} S={S} K={K} inverse={inverse}: " + first_difference(got, want, E, B)
                assert intact, (E, B, S, K, inverse)


def test_lag_order_kernels_at_one_very_long_frame(rx):
    """B = 2^22 + 16, E = 2, S = 5, K = 3: a frame of 2^18 + 1 groups, 1025 rows of the fused kernels with one group in the last
    row (the three carries and the tile are reused 1024 times inside one frame), then a short frame; both directions."""
    import torch
    E, B, S, K = 2, (1 << 22) + 16, 5, 3
    assert B // 16 == 1024 * 256 + 1
    x = np.random.default_rng(22).integers(0, 256, E * B + (B // 3 + 5) * E + 1, dtype=np.uint8)
    for inverse in (False, True):
        want = lag_order_planes_ref(x, E, B, S, K, inverse=inverse)
        got, intact = run_dev(torch, x, E, B, S, K, inverse)
        assert np.array_equal(got, want), f"inverse={inverse}: " + first_difference(got, want, E, B)
        assert intact, inverse


def on_device_poisoned(torch, n):
    """poisoned() for an input too large to pass through the host: (whole buffer, view of n bytes) with FRONT bytes of FILL in
    front and a guard band behind"""
    t = torch.full((FRONT + n + GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    return t, t[FRONT: FRONT + n]


def bands_intact(t, lo, n):
    return bool((t[:lo] == FILL).all()) and bool((t[lo + n:] == FILL).all())


@pytest.mark.parametrize("K", [2, 3])
def test_fused_lag_order_inverse_with_more_frames_than_workgroups(rx, K):
    """E = 1, B = 4112 (257 groups: two rows a frame, so the K carries are live), S = 3, 2^20 + 3 frames and a short one, past
    2^32 bytes: the grid-stride loop of k_lag_order_unplanes, where three workgroups go on to a second frame with carry[][],
    tot[][] and the tile as the first one left them.  The input is tiled on the device from 8 distinct frames in an aperiodic
    order (no period that divides the grid or 4), the expected output is the same tiling of the per-frame restatement,
    compared on the device; the forward kernel takes the result back to the input."""
    import torch
    from redux_amd import api
    E, B, S, nf, short = 1, 4112, 3, (1 << 20) + 3, 1237
    rng = np.random.default_rng(4112 + K)
    frames = rng.integers(0, 256, (8, B), dtype=np.uint8)
    last = rng.integers(0, 256, short, dtype=np.uint8)
    f = torch.arange(nf, device="cuda:0")
    idx = (f * f // 7 + f // 5 + f) % 8                                      # (no period)
    assert len(set(np.diff(np.nonzero((idx[:4096] == 0).cpu().numpy())[0]).tolist())) > 4
    assert len({int(idx[w]) for w in range(3)} | {int(idx[(1 << 20) + w]) for w in range(3)}) > 1
    n = nf * B + short
    assert n > 1 << 32
    ts, src = on_device_poisoned(torch, n)
    src[: nf * B].view(nf, B).copy_(torch.from_numpy(frames).cuda()[idx])
    src[nf * B:].copy_(torch.from_numpy(last).cuda())
    want = torch.from_numpy(np.stack([lag_order_planes_ref(fr, E, B, S, K, inverse=True) for fr in frames])).cuda()
    want_last = torch.from_numpy(lag_order_planes_ref(last, E, B, S, K, inverse=True)).cuda()
    td, dst = guarded(torch, n)
    api.lag_order_planes(src, E, B, S, K, inverse=True, out=dst)
    torch.cuda.synchronize()
    assert bands_intact(td, GUARD, n) and bands_intact(ts, FRONT, n)
    step = 1 << 17
    for f0 in range(0, nf, step):
        got = dst[f0 * B: min(f0 + step, nf) * B].view(-1, B)
        bad = (got != want[idx[f0: f0 + step]]).any(1)
        if bool(bad.any()):
            fr = f0 + int(bad.nonzero()[0])
            at = int((dst[fr * B: (fr + 1) * B] != want[idx[fr]]).nonzero()[0])
            raise AssertionError(f"K={K}: frame {fr} (distinct frame {int(idx[fr])}) differs at byte {at}")
    assert torch.equal(dst[nf * B:], want_last)
    tb, back = guarded(torch, n)
    api.lag_order_planes(dst, E, B, S, K, inverse=False, out=back)
    torch.cuda.synchronize()
    assert bands_intact(tb, GUARD, n) and bands_intact(td, GUARD, n)
    assert torch.equal(back, src)
    del ts, src, td, dst, tb, back, got, bad, want
    torch.cuda.synchronize()
    torch.cuda.empty_cache()                                                 # (three buffers of 4.3 GB)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("S", [3, 256])
def test_byte_lag_order_inverse_past_2_pow_20_frames(rx, S, K):
    """E = 1, B = 400 (no multiple of 16: the byte kernels; two iterations of 256 elements a frame, so the chains' carries in
    last[][][] are live, and par goes on from frame to frame), 2^20 + 3 frames and a short one of 77 bytes: the grid-stride
    loop of k_lag_order_unplanes_bytes.  (Nearly all of the time is numpy over the 419 MB of the restatement, K passes.)"""
    import torch
    E, B, nf, short = 1, 400, (1 << 20) + 3, 77
    x = np.random.default_rng(400 + S + K).integers(0, 256, nf * B + short, dtype=np.uint8)
    # the restatement, vectorised over the full frames (the per-frame loop of lag_order_planes_ref takes minutes here) ...
    body = x[: nf * B].reshape(nf, B)
    r = (body >> 1) ^ np.negative(body & 1)                             # unfold: (z >> 1) ^ (0 - (z & 1)) mod 256
    for _ in range(K):                                                   # the S running sums, K times
        if S < B // 2:
            for c in range(S):                                           # chain c: elements c, c + S, ...
                r[:, c::S] = np.cumsum(r[:, c::S], axis=1, dtype=np.uint8)
        else:
            r[:, S:] += r[:, : B - S]                                    # (chains of two elements at the most)
    want = np.concatenate([r.reshape(-1), lag_order_planes_ref(x[nf * B:], E, B, S, K, inverse=True)])
    # ... checked against lag_order_planes_ref on both ends
    k = 100 * B
    assert np.array_equal(want[:k], lag_order_planes_ref(x[:k], E, B, S, K, inverse=True))
    assert np.array_equal(want[-k - short:], lag_order_planes_ref(x[-k - short:], E, B, S, K, inverse=True))
    assert not np.array_equal(want[:k], lag_order_planes_ref(x[:k], E, B, S, K - 1, inverse=True))
    got, intact = run_dev(torch, x, E, B, S, K, True)
    assert np.array_equal(got, want), f"S={S} K={K}: " + first_difference(got, want, E, B)
    assert intact
    back, intact = run_dev(torch, got, E, B, S, K, False)
    assert intact and np.array_equal(back, x)


# ---- streams: the plain coder on the transformed bytes, against the oracle ------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("E", [2, 4])
@pytest.mark.parametrize("S", [2, 3])
def test_streams_equal_oracle_on_transformed_bytes(rx, E, S, K):
    import torch
    B = 4096
    x = interleaved(12 * B + 1000, S, E, seed=E + S)  # 13 blocks, the last one short
    f = {"element_size": E, "filter": "lag", "lag": S, "order": K}
    want, wst = ox.compress_blocks(lag_order_planes_ref(x, E, B, S, K), B, PARAMS)
    assert not wst.any() and len(want) == 13
    out, offs, st = rx.compress_blocks(x, B, PARAMS, **f)                       # the host-pointer call
    assert not st.any() and split(out, offs) == want, (E, S, K)
    enc = rx.DeviceEncoder(PARAMS, B, len(x), **f)                              # redux_encode_lag_order_dev
    assert enc.front.infix == "lag_order"
    d_out, d_offs, d_st, d_sum = enc.encode(torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert d_sum.tolist() == [0, 0]
    assert split(d_out.cpu().numpy(), d_offs.cpu().numpy()) == want, (E, S, K)
    dec = rx.DeviceDecoder(PARAMS, B, 13, **f)                                  # redux_decode_lag_order_dev
    back, sizes, dst, dsum = dec.decode(d_out[: int(offs[-1])], d_offs, length=len(x))
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and np.array_equal(back.cpu().numpy(), x)
    back, sizes, st2 = rx.decompress_blocks(out, offs, B, PARAMS, length=len(x), **f)
    assert not st2.any() and len(back) == len(x) and np.array_equal(back, x)
    lower = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S, order=K - 1)  # (the order reaches the kernel)
    assert not np.array_equal(lower[0], out)
    if K == 2:  # order 1 and no order are the lag filter's streams
        one = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S)
        assert np.array_equal(lower[0], one[0]) and np.array_equal(lower[1], one[1])


def test_host_pipeline_over_several_chunks(rx):
    B, E, S, K = 4096, 4, 3, 3
    x = interleaved(10 * 64 * B + 12345, S, E, seed=9)
    f = {"element_size": E, "filter": "lag", "lag": S, "order": K}
    want = rx.compress_blocks(x, B, **f)  # one chunk
    nb = len(want[1]) - 1
    assert rx.host_chunk_plan(nb, B)[1] == 1
    ref, _ = ox.compress_blocks(lag_order_planes_ref(x, E, B, S, K)[: 70 * B], B, PARAMS)
    assert split(want[0], want[1])[:70] == ref
    crc = np.zeros(nb, dtype=np.uint32)
    try:
        rx.host_set_chunk_bytes(1 << 20, 1 << 20)  # 256 blocks a chunk, cut at frame boundaries
        assert rx.host_chunk_plan(nb, B)[1] >= 2
        got = rx.compress_blocks(x, B, block_crc=crc, **f)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        back, sizes, st = rx.decompress_blocks(got[0], got[1], B, length=len(x), **f)
        assert not st.any() and np.array_equal(back, x)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    import zlib
    for b in (0, 1, 255, 256, nb - 1):  # block_crc is over the original bytes
        assert int(crc[b]) == zlib.crc32(x[b * B: (b + 1) * B].tobytes()), b


# ---- a damaged stream -------------------------------------------------------------------------------------------------
def test_damaged_stream_stays_in_bounds_and_spares_other_frames(rx, lib):
    import torch
    B, E, S, K = 4096, 2, 3, 2
    nfull = 6
    n = nfull * E * B + 1000  # 12 full blocks in 6 frames, then a short frame of one block of 1000 bytes
    F = E * B
    x = interleaved(n, S, E, seed=11)
    out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="lag", lag=S, order=K)
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
    wsb = L.redux_decode_lag_order_workspace_bytes(C.byref(cp), n, B, E)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    tg, d_out = guarded(torch, n, 5)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = L.redux_decode_lag_order_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, B, E, S, K,
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
    rc = L.redux_decode_blocks_lag_order(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, n, B, E, S, K, hout.ctypes.data,
                                         hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [8]
    assert (hout[n:] == FILL).all()
    for f in clean:
        assert np.array_equal(hout[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


# ---- device coder objects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_device_encoder_decoder_roundtrip_and_ranges(rx, E, K):
    import torch
    B, S = 4096, 3
    n = 4 * E * B + 3 * B + 5
    x = interleaved(n, S, E, seed=E)
    f = {"element_size": E, "filter": "lag", "lag": S, "order": K}
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
        dec.decode(out, offs)  # the original length is required, for E = 1 too
    F = E * B
    ranges = [(2 * F - 7, 20), (3 * F - 1, 2)]  # two ranges, each across a frame boundary
    got, where = dec.decode_ranges(out[: int(ref[1][-1])], offs, n, ranges)
    torch.cuda.synchronize()
    h = got.cpu().numpy()
    for (s0, m), o in zip(ranges, where):
        assert np.array_equal(h[o: o + m], x[s0: s0 + m]), (E, K, s0, m)


# ---- container and CLI ------------------------------------------------------------------------------------------------
def test_container_and_cli_with_the_order(rx, tmp_path):
    from redux_amd import cli, container
    B = 4096
    x = tones(2, 2, 7).tobytes()  # two interleaved int16 channels of tones: three frames and 200 elements
    src = tmp_path / "pcm.i16"
    src.write_bytes(x)
    names = {k: tmp_path / ("%s.rdxb" % k) for k in ("none", "1", "2", "3", "crc")}
    back, part = tmp_path / "back.i16", tmp_path / "part.i16"
    common = ["-c", "-i", str(src), "--block-size", str(B), "--element-size", "2", "--filter", "lag", "--lag", "2"]
    assert cli.main(common + ["-o", str(names["none"])]) == 0
    for K in ("1", "2", "3"):
        assert cli.main(common + ["-o", str(names[K]), "--order", K]) == 0
    blobs = {k: p.read_bytes() for k, p in names.items() if k != "crc"}
    assert blobs["1"] == blobs["none"] and blobs["1"][4] == 13 and container.order(blobs["1"]) == 1  # --order 1 writes version 13
    for K in (2, 3):
        p14 = blobs[str(K)]
        assert p14[4] == 14 and container.filter(p14) == "lag" and container.lag(p14) == 2 and container.order(p14) == K
        assert container.element_size(p14) == 2
        assert p14 == container.compress_bytes(x, B, element_size=2, filter="lag", lag=2, order=K)
        assert cli.main(["-d", "-i", str(names[str(K)]), "-o", str(back)]) == 0
        assert back.read_bytes() == x
    print("2 interleaved int16 tones: order 1 %d bytes, order 2 %d, order 3 %d" % tuple(len(blobs[k]) for k in ("1", "2", "3")))
    assert len(blobs["2"]) <= 0.80 * len(blobs["1"]) and len(blobs["3"]) < len(blobs["2"])  # (test_lag_order_cpu's claim, whole files)
    F = 2 * B
    assert cli.main(["-d", "-i", str(names["3"]), "-o", str(part), "--range", "%d:%d" % (2 * F + 100, 40)]) == 0  # inside the third frame
    assert part.read_bytes() == x[2 * F + 100: 2 * F + 140]
    assert container.decompress_range(blobs["2"], F - 3, 2 * F) == x[F - 3: 3 * F - 3]
    assert cli.main(common + ["-o", str(names["crc"]), "--order", "2", "--checksum"]) == 0
    p1e = names["crc"].read_bytes()
    assert p1e[4] == 0x1E and container.order(p1e) == 2 and len(container.block_crcs(p1e)) == -(-len(x) // B)
    assert cli.main(["-d", "-i", str(names["crc"]), "-o", str(back)]) == 0 and back.read_bytes() == x
    assert cli.main(["-d", "-i", str(names["crc"]), "-o", str(part), "--range", "%d:%d" % (F - 5, 11)]) == 0
    assert part.read_bytes() == x[F - 5: F + 6]
    for checksum in (False, True):
        blob = container.compress_bytes(x, B, element_size=4, filter="lag", lag=4, order=3, checksum=checksum)
        assert blob[4] == (0x1E if checksum else 14) and container.order(blob) == 3 and container.decompress_bytes(blob) == x
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, filter="lag", lag=4, order=2)) == b""
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(x, B, element_size=2, filter="lag", lag="auto", order=2)
    auto = container.compress_bytes(x, B, element_size=2, filter="lag", lag="auto", order=1)  # order 1 may stand with the count
    assert auto == container.compress_bytes(x, B, element_size=2, filter="lag", lag="auto") and auto[4] == 13


def test_cpp_lag_order_mirror(rx, tmp_path):
    import subprocess
    out = subprocess.run([build_lag_order_mirror_test(tmp_path), "--gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "lag order mirror ok" in out.stdout, out.stdout + out.stderr
