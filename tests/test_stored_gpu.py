"""Stored blocks on the device: payloads and flags against the CPU oracle and the rule for every element size and three
thresholds, round trips through the host-pointer and `_dev` calls (CRCs, small chunks, two contexts on one device), waves
that mix stored and coded blocks, 65,536 device-resident blocks of 64 KiB all stored, damaged flags, and the container and
CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_cpu import planes_ref
from test_stored_cpu import rule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P3 = (8, 30, 32)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def mixed(rx, B, seed=1):
    """iid, Zipf and constant blocks, then a ragged iid tail"""
    rng = np.random.default_rng(seed)
    zipf = rx.gen_zipf(3 * B, seed=seed).cpu().numpy()
    parts = [rng.integers(0, 256, 3 * B, dtype=np.uint8), zipf, np.full(2 * B, 7, np.uint8),
             rng.integers(0, 256, B // 2, dtype=np.uint8), zipf[: B], rng.integers(0, 256, B + B // 3 + 5, dtype=np.uint8)]
    return np.concatenate(parts)


def raw_len(n, B):
    return [min(B, n - o) for o in range(0, n, B)] or [0]


def encode(rx, x, B, E=1, t=65536, **kw):
    nb = max(1, -(-len(x) // B))
    flags = np.full(nb, 0xEE, dtype=np.uint8)
    out, offs, st = rx.compress_blocks(x, B, P3, element_size=E, stored=flags, store_ratio=t, **kw)
    return out, offs, st, flags


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_parity_with_oracle(rx, E):
    B = 16384
    for x in (mixed(rx, B, seed=E), np.array([0x5A], np.uint8), np.zeros(0, np.uint8)):
        xp = planes_ref(x, E, B) if E > 1 else x
        streams, ost = ox.compress_blocks(xp, B, P3)
        L = raw_len(len(x), B)
        sizes = [len(s) for s in streams]
        for t in (0, 65536, 64512):
            out, offs, st, flags = encode(rx, x, B, E, t)
            want = rule(ost, sizes, L, t).astype(np.uint8)
            assert flags.tolist() == want.tolist(), (E, t, len(x))
            assert (st == 0).all()
            for b in range(len(L)):
                got = out[int(offs[b]): int(offs[b + 1])].tobytes()
                exp = xp[b * B: b * B + L[b]].tobytes() if want[b] else streams[b]
                assert got == exp, (E, t, b)
            back, bs, bst = rx.decompress_blocks(out, offs, B, P3, element_size=E, length=len(x), stored=flags)
            assert back.tobytes() == x.tobytes() and bs.tolist() == L and (bst == 0).all()
            if t == 0:
                assert flags.all()
            if len(x) > B and E == 1:
                assert 0 < flags.sum() < len(flags) or t == 0


def test_host_round_trips_crc_small_chunks_two_contexts(rx):
    import zlib
    B = 65536
    x = mixed(rx, B, seed=11)
    nb = -(-len(x) // B)
    ref = encode(rx, x, B, 2)
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, len(x), B)]

    def run():
        crc = np.zeros(nb, np.uint32)
        out, offs, st, flags = encode(rx, x, B, 2, block_crc=crc)
        assert out.tobytes() == ref[0].tobytes() and flags.tolist() == ref[3].tolist() and crc.tolist() == want_crc
        dcrc = np.zeros(nb, np.uint32)
        back, _, _ = rx.decompress_blocks(out, offs, B, P3, element_size=2, length=len(x), stored=flags, block_crc=dcrc)
        assert back.tobytes() == x.tobytes() and dcrc.tolist() == want_crc

    run()
    rx.host_set_chunk_bytes(1, 1)
    try:
        run()
    finally:
        rx.host_set_chunk_bytes(0, 0)
    rx.host_set_devices([0, 0])
    try:
        rx.host_set_chunk_bytes(1, 1)
        try:
            run()
        finally:
            rx.host_set_chunk_bytes(0, 0)
    finally:
        rx.host_set_devices([])


def test_host_calls_several_chunks(rx):
    """chunks sized for a pipeline of several (no small-grid pairs area in their workspace)"""
    B = 65536
    x = rx.gen_iid(300 << 20, seed=21).cpu().numpy()
    x[5 * B: 9 * B] = 3  # four coded blocks
    out, offs, st, flags = encode(rx, x, B)
    assert int(flags.sum()) == len(flags) - 4 and int(offs[-1]) == len(x) - 4 * B + int(offs[9] - offs[5])
    back, _, _ = rx.decompress_blocks(out, offs, B, P3, length=len(x), stored=flags)
    assert back.tobytes() == x.tobytes()


def dev_encode(rx, d_in, B, E, t=65536):
    import torch
    from redux_amd import _lib
    L = _lib.lib()
    cp = _lib.Params(*P3)
    n = d_in.numel()
    nb = L.redux_block_count(n, B)
    cap = L.redux_encode_bound(C.byref(cp), n, B)
    ws_b = L.redux_encode_stored_workspace_bytes(C.byref(cp), n, B, E)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.empty(nb + 1, dtype=torch.int64, device="cuda:0")
    d_flags = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_st = torch.empty(nb, dtype=torch.int32, device="cuda:0")
    d_sum = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(ws_b, dtype=torch.uint8, device="cuda:0")
    v = lambda t_: C.c_void_p(t_.data_ptr())
    rc = L.redux_encode_stored_dev(C.byref(cp), C.c_void_p(d_in.data_ptr() if n else 0), n, B, E, t, v(d_out), cap, v(d_offs),
                                   v(d_flags), v(d_st), v(d_sum), v(ws), ws_b, None)
    assert rc == 0
    torch.cuda.synchronize()
    return d_out, d_offs, d_flags, d_st, d_sum


def dev_decode(rx, d_out, d_offs, d_flags, n, B, E, out_off=0):
    import torch
    from redux_amd import _lib
    L = _lib.lib()
    cp = _lib.Params(*P3)
    nb = L.redux_block_count(n, B)
    ws_b = L.redux_decode_stored_workspace_bytes(C.byref(cp), n, B, E)
    frame = torch.full((n + out_off + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_dst = frame[out_off: out_off + n]
    d_sz = torch.empty(nb, dtype=torch.int32, device="cuda:0")
    d_st = torch.empty(nb, dtype=torch.int32, device="cuda:0")
    d_sum = torch.full((2,), 9, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(ws_b + 256, dtype=torch.uint8, device="cuda:0")
    wsp = (ws.data_ptr() + 255) // 256 * 256
    v = lambda t_: C.c_void_p(t_.data_ptr())
    rc = L.redux_decode_stored_dev(C.byref(cp), v(d_out), v(d_offs), v(d_flags), n, B, E, C.c_void_p(d_dst.data_ptr()), n,
                                   v(d_sz), v(d_st), v(d_sum), C.c_void_p(wsp), ws_b, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert (frame[:out_off] == 0xA5).all() and (frame[out_off + n:] == 0xA5).all()  # nothing written outside
    return d_dst, d_sz, d_st, d_sum


@pytest.mark.parametrize("E,B,off", [(1, 65536, 0), (1, 1000, 3), (4, 16384, 5), (8, 4096, 0)])
def test_dev_calls_match_host_calls(rx, E, B, off):
    import torch
    x = mixed(rx, B, seed=B + E)
    base = torch.zeros(len(x) + 64, dtype=torch.uint8, device="cuda:0")
    d_in = base[off: off + len(x)]
    d_in.copy_(torch.from_numpy(x).cuda())
    out, offs, st, flags = encode(rx, x, B, E)
    d_out, d_offs, d_flags, d_st, d_sum = dev_encode(rx, d_in, B, E)
    assert d_sum.tolist() == [0, 0] and d_flags.cpu().numpy().tolist() == flags.tolist()
    assert d_offs.cpu().numpy().astype(np.uint64).tolist() == offs.tolist()
    assert d_out[: int(offs[-1])].cpu().numpy().tobytes() == out.tobytes()
    d_dst, d_sz, d_st2, d_sum2 = dev_decode(rx, d_out, d_offs, d_flags, len(x), B, E, out_off=off)
    assert d_sum2.tolist() == [0, 0] and torch.equal(d_dst, d_in)
    assert d_sz.cpu().tolist() == raw_len(len(x), B)


def test_mixed_waves(rx):
    """every other block stored: the coded blocks' table differs from block order in every wave"""
    import torch
    B = 65536
    rng = np.random.default_rng(5)
    nb = 192
    x = np.empty(nb * B - 100, np.uint8)
    for b in range(nb):
        blk = x[b * B: (b + 1) * B]
        blk[:] = rng.integers(0, 256, len(blk), dtype=np.uint8) if b % 2 == 0 else (np.arange(len(blk)) % 13).astype(np.uint8)
    out, offs, st, flags = encode(rx, x, B)
    assert flags.tolist() == [1 - b % 2 for b in range(nb)]
    back, sizes, bst = rx.decompress_blocks(out, offs, B, P3, length=len(x), stored=flags)
    assert back.tobytes() == x.tobytes()
    d_in = torch.from_numpy(x).cuda()
    d_out, d_offs, d_flags, _, _ = dev_encode(rx, d_in, B, 1)
    d_dst, _, _, d_sum = dev_decode(rx, d_out, d_offs, d_flags, len(x), B, 1)
    assert d_sum.tolist() == [0, 0] and torch.equal(d_dst, d_in)


def test_device_resident_4gib_iid_all_stored(rx):
    import torch
    B, nb = 65536, 65536
    d_in = rx.gen_iid(nb * B)
    d_out, d_offs, d_flags, d_st, d_sum = dev_encode(rx, d_in, B, 1)
    assert d_sum.tolist() == [0, 0] and bool((d_flags == 1).all()) and int(d_offs[-1]) == nb * B
    d_dst, d_sz, d_st2, d_sum2 = dev_decode(rx, d_out, d_offs, d_flags, nb * B, B, 1)
    assert d_sum2.tolist() == [0, 0] and torch.equal(d_dst, d_in)
    del d_out, d_dst
    torch.cuda.empty_cache()


def test_damaged_flags(rx):
    B = 16384
    x = mixed(rx, B, seed=3)
    out, offs, st, flags = encode(rx, x, B)
    coded = int(np.flatnonzero(flags == 0)[0])
    stored = int(np.flatnonzero(flags == 1)[0])
    f = flags.copy()
    f[coded] = 1  # a stream taken for raw bytes: shorter than its block
    _, sizes, bst = rx.decompress_blocks(out, offs, B, P3, check=False, length=len(x), stored=f)
    assert bst[coded] == rx.InvalidInput.status and (np.delete(bst, coded) == 0).all()
    f = flags.copy()
    f[stored] = 0  # raw bytes taken for a stream
    back, sizes, bst = rx.decompress_blocks(out, offs, B, P3, check=False, length=len(x), stored=f)
    assert bst[stored] != 0 or back[stored * B: (stored + 1) * B].tobytes() != x[stored * B: (stored + 1) * B].tobytes()
    f = flags.copy()
    f[stored] = 2
    _, sizes, bst = rx.decompress_blocks(out, offs, B, P3, check=False, length=len(x), stored=f)
    assert bst[stored] == rx.InvalidInput.status and sizes[stored] == 0
    # a checksummed container catches the stored block flagged coded
    from redux_amd import container
    blob = container.compress_bytes(x.tobytes(), B, P3, checksum=True, stored=True)
    assert blob[4] == 0x51 and container.decompress_bytes(blob) == x.tobytes()
    at = container.HEADER.size + 8 * len(flags) + stored // 8
    bad = blob[:at] + bytes([blob[at] & ~(1 << (stored % 8))]) + blob[at + 1:]
    with pytest.raises(rx.Error):
        container.decompress_bytes(bad)


def _cli(args, tmp_path, name):
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", *args], cwd=ROOT, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("kind", ["iid", "zipf", "bf16", "fp32"])
def test_container_and_cli(rx, tmp_path, kind):
    from redux_amd import container
    B = 65536
    rng = np.random.default_rng(9)
    E = {"bf16": 2, "fp32": 4}.get(kind, 1)
    if kind == "iid":
        x = rng.integers(0, 256, 40 * B + 1234, dtype=np.uint8).tobytes()
    elif kind == "zipf":
        x = rx.gen_zipf(20 * B + 99).cpu().numpy().tobytes()
    elif kind == "bf16":
        x = (rng.normal(0, 0.02, 20 * B).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()
    else:
        x = rng.normal(0, 1, 12 * B).astype(np.float32).tobytes()
    src, enc, dec = tmp_path / "in", tmp_path / "enc", tmp_path / "dec"
    src.write_bytes(x)
    _cli(["-c", "--stored", "--block-size", str(B), "--element-size", str(E), "-i", str(src), "-o", str(enc)], tmp_path, "c")
    blob = enc.read_bytes()
    assert blob[4] == (0x41 if E == 1 else 0x42)
    flags = container.block_stored(blob)
    nb = len(flags)
    if kind == "iid":
        assert flags.all() and len(blob) == container.HEADER.size + 4 * nb + (nb + 7) // 8 + len(x)
    if kind == "zipf":
        assert not flags.any()
    if kind == "fp32":  # the mantissa planes do not shrink
        assert flags.any() and not flags.all()
    _cli(["-d", "-i", str(enc), "-o", str(dec)], tmp_path, "d")
    assert dec.read_bytes() == x
    plain = container.compress_bytes(x, B, P3, E)
    assert len(blob) <= len(plain) + (nb + 7) // 8
