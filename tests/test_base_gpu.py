"""XOR-against-base filter on the device: the fused and the byte kernels against the numpy restatement
planes_ref(x ^ pad(y), E, B), the `_dev` coder calls against the byte-plane calls on the host-XORed input and against the
CPU oracle, the host-pointer pair over chunk sizes, damaged streams, and the Python API, the container and the CLI end to
end on a synthetic pair of fp32 snapshots."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_adaptive_instances_cpu import COOP
from test_adaptive_instances_gpu import FILL, guarded, guards_intact
from test_base_cpu import base_planes_ref, build_base_mirror_test, pad
from test_planes_cpu import planes_ref

pytestmark = pytest.mark.gpu

PARAMS = (8, 30, 32)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def _lib():
    from redux_amd import _lib as L
    return L


def _v(t):
    return C.c_void_p(t.data_ptr())


def split(out, offs):
    return [bytes(out[int(offs[i]): int(offs[i + 1])]) for i in range(len(offs) - 1)]


def on_device(a, align=0):
    """a copy of the numpy bytes `a` between guard bands, `align` bytes off a 16-byte boundary -> (whole tensor, view, lo)"""
    import torch
    t, view, lo = guarded(len(a), align)
    if len(a):
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return t, view, lo


def run_dev(rx, x, y, E, B, inverse, so=0, yo=0, do=0):
    """redux_base_planes_dev of x with base y between guarded buffers at the given byte offsets; asserts the guards"""
    import torch
    ts, src, slo = on_device(x, so)
    ty, base, ylo = on_device(y, yo)
    td, dst, dlo = guarded(len(x), do)
    rx.base_planes(src, base, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    assert guards_intact(td, dlo, len(x)) and guards_intact(ts, slo, len(x)) and guards_intact(ty, ylo, len(y)), (E, B, len(x), len(y))
    assert np.array_equal(src.cpu().numpy(), x) and np.array_equal(base.cpu().numpy(), y)   # the inputs are only read
    return dst.cpu().numpy()


def check(rx, x, y, E, B, so=0, yo=0, do=0):
    for inverse in (False, True):
        got = run_dev(rx, x, y, E, B, inverse, so, yo, do)
        want = base_planes_ref(x, y, E, B, inverse=inverse)
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"E={E} B={B} len={len(x)} base_len={len(y)} offsets={(so, yo, do)} inverse={inverse}: first "
                                 f"difference at byte {at} (frame {at // (E * B)}, offset {at % (E * B)})")


def base_lengths(L, E, B):
    """0, 1, len - 1, len, longer than the input, exactly two frames, and mid-frame and mid-element in the third"""
    return sorted({0, 1, max(L - 1, 0), L, L + 17, 2 * E * B, 2 * E * B + 7 * E + 1})


# ---- 1. the transform ---------------------------------------------------------------------------------------------------
# (1008: a frame ends inside a wave's turn of 64 groups; 4688: 293 groups a frame, a row of 256 and a ragged wave, three frames)
@pytest.mark.parametrize("B", [1, 16, 48, 100, 1008, 4096, 4688])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_base_planes_dev_matches_restatement(rx, E, B):
    rng = np.random.default_rng(E * 100003 + B)
    F = E * B
    last = (3 if B == 4688 else 5) * F + 3 * E + 1
    for L in (0, 1, F - 1, F, F + 1, last):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for yl in base_lengths(L, E, B):
            y = rng.integers(0, 256, yl, dtype=np.uint8)
            check(rx, x, y, E, B)                    # all three on 16-byte boundaries: the fused kernels where B allows
            check(rx, x, y, E, B, 1, 1, 1)
            if L == last:                            # each buffer alone, and all together, 1, 4 and 8 bytes off
                for off in (1, 4, 8):
                    for so, yo, do in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, off, off)):
                        check(rx, x, y, E, B, so, yo, do)
        assert not run_dev(rx, x, x.copy(), E, B, False).any()   # x == y: all-zero coder input


def test_base_planes_dev_past_the_grid_cap(rx):
    """B = 16, E = 2, 2^20 + 3 full frames of 32 bytes and a short one, the base ending inside frame 2^20 + 1: on 16-byte
    boundaries the fused kernels run 4097 workgroups and the byte kernels the last frames; one byte off, the byte kernels take
    everything in the grid-stride loop past their cap of 8192 workgroups."""
    E, B = 2, 16
    nf = (1 << 20) + 3
    rng = np.random.default_rng(20261018)
    x = rng.integers(0, 256, nf * E * B + 7, dtype=np.uint8)
    y = rng.integers(0, 256, (nf - 2) * E * B + 2 * E + 1, dtype=np.uint8)
    d = x ^ pad(y, len(x))
    # the restatement, vectorised over the full frames (the per-frame loop of planes_ref takes minutes here) ...
    want = np.concatenate([d[: nf * E * B].reshape(nf, B, E).transpose(0, 2, 1).reshape(-1), planes_ref(d[nf * E * B:], E, B)])
    # ... checked against planes_ref on both ends
    k = 100 * E * B
    assert np.array_equal(want[:k], planes_ref(d[:k], E, B)) and np.array_equal(want[-k - 7:], planes_ref(d[-k - 7:], E, B))
    for off in (0, 1):
        got = run_dev(rx, x, y, E, B, False, off, off, off)
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"forward, {off} off: first difference at byte {at} (frame {at // (E * B)})")
        back = run_dev(rx, want, y, E, B, True, off, off, off)
        if not np.array_equal(back, x):
            at = int(np.nonzero(back != x)[0][0])
            raise AssertionError(f"inverse, {off} off: first difference at byte {at} (frame {at // (E * B)})")


def test_base_planes_dev_rejects_bad_arguments(rx):
    import torch
    L, lib = _lib(), _lib().lib()
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    c = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.redux_base_planes_dev(_v(a), _v(b), 4096, _v(c), 4096, 64, 3, 0, s) == L.INVALID_INPUT
    assert lib.redux_base_planes_dev(_v(a), _v(b), 4096, _v(c), 4096, 0, 2, 0, s) == L.INVALID_INPUT
    assert lib.redux_base_planes_dev(_v(a), _v(b), 4096, C.c_void_p(a.data_ptr() + 16), 1024, 64, 2, 0, s) == L.INVALID_INPUT
    assert lib.redux_base_planes_dev(_v(a), _v(b), 4096, C.c_void_p(b.data_ptr() + 16), 1024, 64, 2, 0, s) == L.INVALID_INPUT
    assert lib.redux_base_planes_dev(_v(a), _v(b), 4096, _v(c), 4096, 64, 1, 0, s) == L.OK
    torch.cuda.synchronize()
    with pytest.raises(rx.InvalidInput):
        rx.base_planes(a, b, 3, 64)
    with pytest.raises(rx.InvalidInput):
        rx.base_planes(a, b, 2, 0)


# ---- 2. the `_dev` coder calls ------------------------------------------------------------------------------------------
def snapshots(n, seed):
    """n bytes of an fp32 pair: N(0, 0.02) weights and the same after an N(0, 2e-5) update"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n // 4 + 1) * 0.02).astype(np.float32)
    w2 = (w + np.float32(2e-5) * rng.standard_normal(len(w)).astype(np.float32)).astype(np.float32)
    return w2.view(np.uint8)[:n].copy(), w.view(np.uint8)[:n].copy()


def workspace(nbytes):
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    return t, C.c_void_p((t.data_ptr() + 255) // 256 * 256)


def encode_dev(d_in, n, d_base, base_len, E, B):
    """redux_encode_base_dev (d_base given) or redux_encode_planes_dev -> (out, offsets, status, summary), guards checked"""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    wsb = (lib.redux_encode_base_workspace_bytes if d_base is not None else lib.redux_encode_planes_workspace_bytes)(C.byref(cp), n, B, E)
    wst, wsp = workspace(wsb)
    cap = lib.redux_encode_bound(C.byref(cp), n, B)
    big, out, lo = guarded(cap)
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    if d_base is not None:
        rc = lib.redux_encode_base_dev(C.byref(cp), _v(d_in), n, _v(d_base), base_len, B, E, _v(out), cap, _v(offs), _v(status), _v(summ),
                                       wsp, wsb, None)
    else:
        rc = lib.redux_encode_planes_dev(C.byref(cp), _v(d_in), n, B, E, _v(out), cap, _v(offs), _v(status), _v(summ), wsp, wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, cap)
    return out, offs, status, summ


def decode_dev(d_streams, d_offs, d_base, base_len, n, E, B, off=0):
    """redux_decode_base_dev into a guarded buffer `off` bytes off a 16-byte boundary -> (out, sizes, status, summary)"""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    wsb = lib.redux_decode_base_workspace_bytes(C.byref(cp), n, B, E)
    wst, wsp = workspace(wsb)
    big, out, lo = guarded(n, off)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_decode_base_dev(C.byref(cp), _v(d_streams), _v(d_offs), _v(d_base), base_len, n, B, E, _v(out), _v(sizes), _v(status),
                                   _v(summ), wsp, wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, n)
    return out, sizes, status, summ


def truncated(streams, hit):
    """the streams with stream `hit` cut to a third -> (dense uint8, offsets int64)"""
    bad = list(streams)
    bad[hit] = bad[hit][: len(bad[hit]) // 3]
    offs = np.zeros(len(bad) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in bad])
    return np.frombuffer(b"".join(bad), dtype=np.uint8).copy(), offs


SHAPES = [(4096, 2, 388 * 4096 + 1001), (4096, 4, 388 * 4096 + 1001), (65536, 1, 70 * 65536), (65536, 2, 70 * 65536)]


@pytest.mark.parametrize("B,E,n", SHAPES)
def test_encode_base_dev_equals_planes_call_on_xored_input_and_the_oracle(rx, B, E, n):
    """389 blocks of 4096 bytes ending in a ragged frame (E = 2: one block of 1001 bytes; E = 4: the same, a frame of one
    block), the base ending mid-input, mid-frame and mid-element; and 70 blocks of 64 KiB with a base longer than the input.
    Both launches run the small-grid encoder k_coop_model + k_coop_chain<true> (at most 2048 blocks, code_bits 32) on the
    transformed copy in the workspace, and the lock-step decoder k_decode_lock<true> into the plane buffer."""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    assert nb == (389 if B == 4096 else 70)
    assert lib.redux_encode_kernel_name(C.byref(cp), C.c_void_p(4096), n, B).decode() == COOP[True]
    assert lib.redux_decode_kernel_name_n(C.byref(cp), C.c_void_p(4096), B, nb).decode().startswith("k_decode_lock<true>")
    x, y = snapshots(n, seed=B + E)
    y = y[: 200 * 4096 + 7 * E + 1] if B == 4096 else np.concatenate([y, y[:33]])
    d = x ^ pad(y, n)
    tx, d_x, xlo = on_device(x)
    ty, d_y, ylo = on_device(y)
    out, offs, status, summ = encode_dev(d_x, n, d_y, len(y), E, B)
    assert guards_intact(tx, xlo, n) and guards_intact(ty, ylo, len(y))
    td, d_d, dlo = on_device(d)
    out2, offs2, status2, summ2 = encode_dev(d_d, n, None, 0, E, B)
    assert summ.tolist() == [0, 0] and summ2.tolist() == [0, 0] and not bool(status.any())
    assert torch.equal(offs, offs2) and torch.equal(status, status2)
    total = int(offs[-1])
    assert torch.equal(out[:total], out2[:total])
    want, wst = ox.compress_blocks(planes_ref(d, E, B), B, PARAMS)
    assert not wst.any() and split(out[:total].cpu().numpy(), offs.cpu().numpy()) == want
    # the device's own output, decoded
    back, sizes, dstatus, dsum = decode_dev(out[:total], offs, d_y, len(y), n, E, B)
    assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
    assert sizes.tolist() == [min(B, n - b * B) for b in range(nb)]
    assert torch.equal(back, d_x)
    # one stream cut to a third: the frames whose blocks are all OK still hold x, and nothing outside out[0 .. n) is written
    hit = 5
    bad, boffs = truncated(want, hit)
    d_bad, d_boffs = torch.from_numpy(bad).cuda(), torch.from_numpy(boffs).cuda()
    for off in (0, 5):
        back, sizes, dstatus, dsum = decode_dev(d_bad, d_boffs, d_y, len(y), n, E, B, off)
        st = dstatus.cpu().numpy()
        assert np.nonzero(st)[0].tolist() == [hit] and dsum.tolist() == [int(st[hit]), 1]
        got = back.cpu().numpy()
        F = E * B
        for f in range(-(-n // F)):
            if f != hit // E:
                assert np.array_equal(got[f * F: (f + 1) * F], x[f * F: (f + 1) * F]), f


def test_device_coder_objects_with_a_base(rx):
    import torch
    B, E = 4096, 4
    n = 70 * B + 123
    x, y = snapshots(n, seed=9)
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y[: n - 4097]).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E, base=d_y)
    out, offs, status, summary = enc.encode(d_x)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    ref = rx.compress_blocks(x, B, PARAMS, element_size=E, base=y[: n - 4097])
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1]) and np.array_equal(out[: int(ref[1][-1])].cpu().numpy(), ref[0])
    nb = len(ref[1]) - 1
    dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, base=d_y)
    d_out, sizes, st, dsum = dec.decode(out[: int(ref[1][-1])], offs, length=n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and d_out.numel() == n and torch.equal(d_out, d_x)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out, offs)                                     # the original length is required
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_x)                                     # (the phases are the plain coder's)
    with pytest.raises(rx.InvalidInput):
        rx.DeviceEncoder(PARAMS, B, n, element_size=E, base=y)    # host bytes are not a device tensor
    # element size 1, and without a base nothing changes
    e1 = rx.DeviceEncoder(PARAMS, B, n, base=d_y)
    o1, f1, _, s1 = e1.encode(d_x)
    torch.cuda.synchronize()
    ref1 = rx.compress_blocks(x ^ pad(y[: n - 4097], n), B, PARAMS)
    assert s1.tolist() == [0, 0] and np.array_equal(o1[: int(ref1[1][-1])].cpu().numpy(), ref1[0])
    back1, _, _, bs1 = rx.DeviceDecoder(PARAMS, B, nb, base=d_y).decode(o1[: int(ref1[1][-1])], f1, length=n)
    torch.cuda.synchronize()
    assert bs1.tolist() == [0, 0] and torch.equal(back1, d_x)
    a, b = rx.compress_blocks(x, B, PARAMS, element_size=E), rx.compress_blocks(x, B, PARAMS, element_size=E, base=None)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


# ---- 3. the host-pointer pair -------------------------------------------------------------------------------------------
def test_host_pointer_pair_in_three_chunks_and_more_equals_the_dev_calls(rx):
    """B = 256, 200 blocks, E = 2, the base shorter than the input and ending inside the second chunk: chunks of 64 blocks
    (four of them) XOR their own share of the base, the last two have none."""
    import torch
    B, E, nb = 256, 2, 200
    n = nb * B - 77
    x, y = snapshots(n, seed=3)
    y = y[: 100 * B + 2 * E + 1]
    d_x, d_y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    out, offs, status, summ = encode_dev(d_x, n, d_y, len(y), E, B)
    assert summ.tolist() == [0, 0]
    total = int(offs[-1])
    want_out, want_offs = out[:total].cpu().numpy(), offs.cpu().numpy().astype(np.uint64)
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, n, B)]
    try:
        for chunk in (64 * B, 0):   # at least three chunks; then the default chunk size (one chunk)
            rx.host_set_chunk_bytes(chunk, chunk)
            assert (rx.host_chunk_plan(nb, B)[1] >= 3) == (chunk != 0)
            crc = np.zeros(nb, np.uint32)
            h_out, h_offs, h_st = rx.compress_blocks(x, B, PARAMS, element_size=E, block_crc=crc, base=y)
            assert not h_st.any() and crc.tolist() == want_crc
            assert np.array_equal(h_offs, want_offs) and np.array_equal(h_out, want_out)
            dcrc = np.zeros(nb, np.uint32)
            back, sizes, st = rx.decompress_blocks(h_out, h_offs, B, PARAMS, element_size=E, length=n, block_crc=dcrc, base=y)
            assert not st.any() and np.array_equal(back, x) and dcrc.tolist() == want_crc
            assert sizes.tolist() == [min(B, n - b * B) for b in range(nb)]
            # a longer base is used up to the input's length; another base decodes to other bytes
            back2, _, _ = rx.decompress_blocks(h_out, h_offs, B, PARAMS, element_size=E, length=n, base=np.concatenate([y, np.zeros(n, np.uint8)]))
            assert np.array_equal(back2, x)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    # the host-pointer decode of damaged streams writes only out[0 .. n)
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    bad, boffs = truncated(split(want_out, want_offs), 7)
    boffs = boffs.astype(np.uint64)
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs, hst = np.zeros(nb, np.uint32), np.zeros(nb, np.int32)
    rc = lib.redux_decode_blocks_base(C.byref(cp), bad.ctypes.data, boffs.ctypes.data, y.ctypes.data, len(y), n, B, E,
                                      hout.ctypes.data, hs.ctypes.data, hst.ctypes.data, None)
    assert rc != L.OK and np.nonzero(hst)[0].tolist() == [7] and (hout[n:] == FILL).all()
    F = E * B
    for f in range(-(-n // F)):
        if f != 7 // E:
            assert np.array_equal(hout[f * F: min((f + 1) * F, n)], x[f * F: (f + 1) * F]), f


def test_cpp_base_mirror(rx, tmp_path):
    import os
    import subprocess
    exe = build_base_mirror_test(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([exe, os.path.join(root, "tests", "golden", "corpora", "canterbury", "lcet10.txt")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "base mirror ok" in out.stdout, out.stdout + out.stderr


# ---- 4. Python, container and CLI end to end ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(20261018)
    n = 1 << 18
    w = (rng.standard_normal(n) * 0.02).astype(np.float32)
    w2 = (w + np.float32(2e-5) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return w.view(np.uint8), w2.view(np.uint8)


def test_container_with_a_base_pays_and_round_trips(rx, pair):
    """The cost identity gives 590,204 against 875,669 payload bytes for this pair (0.674); a stream is within a byte per
    block of it and the record costs 12 bytes: at most 0.72 of the container without the base."""
    from redux_amd import container
    w, w2 = pair
    plain = container.compress_bytes(w2, 65536, element_size=4)
    blob = container.compress_bytes(w2, 65536, element_size=4, base=w)
    print("fp32 pair, 1 MiB: %d bytes without the base, %d with it, %.4f" % (len(plain), len(blob), len(blob) / len(plain)))
    assert blob[4] == 8 and container.base(blob) == (len(w), zlib.crc32(w.tobytes())) and container.element_size(blob) == 4
    assert container.decompress_bytes(blob, base=w) == w2.tobytes()
    assert container.decompress_bytes(blob, base=w.tobytes() + b"more") == w2.tobytes()   # a longer base is fine
    assert len(blob) <= 0.72 * len(plain), (len(plain), len(blob))
    assert plain == container.compress_bytes(w2, 65536, element_size=4, base=None) and plain[4] == 2
    assert container.decompress_bytes(plain) == w2.tobytes()
    # an identical pair: a 64 KiB block of zeros costs about 300 bytes under (8, 30, 32)
    same = container.compress_bytes(w2, 65536, element_size=4, base=w2)
    print("identical pair: %d bytes, %.5f of the input" % (len(same), len(same) / len(w2)))
    assert len(same) <= 0.01 * len(w2) and container.decompress_bytes(same, base=w2) == w2.tobytes()
    # the refusals, with a real container
    other = w.copy()
    other[1000] ^= 1
    for bad in (None, other, w[:-1], b""):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(blob, base=bad)
    with pytest.raises(rx.InvalidInput):
        container.decompress_bytes(plain, base=w)
    # every element size, a base shorter than the data, checksums, and the empty input
    y = w2.tobytes()[: 5 * 65536 + 13]
    for E in (1, 2, 4, 8):
        b8 = container.compress_bytes(y, 4096, element_size=E, base=w[: 3 * 65536 + 5], checksum=True)
        assert b8[4] == 0x18 and container.base(b8)[0] == 3 * 65536 + 5 and container.decompress_bytes(b8, base=w) == y
        assert container.block_crcs(b8).tolist() == [zlib.crc32(y[o: o + 4096]) for o in range(0, len(y), 4096)]
    assert container.decompress_bytes(container.compress_bytes(b"", 65536, element_size=4, base=w), base=w) == b""
    assert container.decompress_bytes(container.compress_bytes(y, 65536, element_size=2, base=b""), base=b"") == y


def test_cli_with_a_base(rx, pair, tmp_path):
    from redux_amd import cli, container
    w, w2 = pair
    prev, cur, wrong = tmp_path / "step0.f32", tmp_path / "step1.f32", tmp_path / "wrong.f32"
    prev.write_bytes(w.tobytes())
    cur.write_bytes(w2.tobytes())
    wrong.write_bytes(w2.tobytes())
    plain, delta, back = tmp_path / "plain.rdxb", tmp_path / "base.rdxb", tmp_path / "back.f32"
    common = ["--block-size", "65536", "--element-size", "4"]
    assert cli.main(["-c", "-i", str(cur), "-o", str(plain)] + common) == 0
    assert cli.main(["-c", "-i", str(cur), "-o", str(delta), "--base", str(prev), "--checksum"] + common) == 0
    p2, p8 = plain.read_bytes(), delta.read_bytes()
    assert p2[4] == 2 and p8[4] == 0x18 and container.base(p8) == (len(w), zlib.crc32(w.tobytes())) and container.base(p2) is None
    assert len(container.block_crcs(p8)) == 16 and len(p8) <= 0.72 * len(p2)
    assert cli.main(["-d", "-i", str(delta), "-o", str(back), "--base", str(prev)]) == 0
    assert back.read_bytes() == w2.tobytes()
    assert cli.main(["-d", "-i", str(delta), "-o", str(back), "--base", str(wrong)]) == 3    # another file as base
    assert cli.main(["-d", "-i", str(delta), "-o", str(back)]) == 3                          # no base
    assert cli.main(["-d", "-i", str(plain), "-o", str(back), "--base", str(prev)]) == 3     # a base for another version
    assert cli.main(["-d", "-i", str(plain), "-o", str(back)]) == 0 and back.read_bytes() == w2.tobytes()
    # a damaged payload byte under --checksum: the block decodes to other bytes, or not at all; exit 3 either way
    hurt = bytearray(p8)
    hurt[len(hurt) // 2] ^= 0x10
    (tmp_path / "hurt.rdxb").write_bytes(bytes(hurt))
    assert cli.main(["-d", "-i", str(tmp_path / "hurt.rdxb"), "-o", str(back), "--base", str(prev)]) == 3
    assert cli.main(["-c", "-i", str(cur), "-o", str(tmp_path / "x"), "--base", str(prev)]) == 1   # no block size
