"""Constant blocks on the device: k_const_select against the numpy restatement const_ref in guarded buffers, the `_dev` coder
calls against the base / planes calls and the CPU oracle, damaged input to the decode call, the host-pointer pair over
chunk sizes and contexts, and the device coder objects, the container and the CLI end to end on a synthetic pair of fp32
snapshots whose middle frames are unchanged."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_adaptive_instances_gpu import FILL, guarded, guards_intact
from test_base_cpu import pad
from test_const_cpu import build_const_mirror_test, const_ref
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
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def split(out, offs):
    return [bytes(out[int(offs[i]): int(offs[i + 1])]) for i in range(len(offs) - 1)]


def on_device(a, align=0):
    import torch
    t, view, lo = guarded(len(a), align)
    if len(a):
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return t, view, lo


def workspace(nbytes):
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    return t, C.c_void_p((t.data_ptr() + 255) // 256 * 256)


# ---- 1. the detection -----------------------------------------------------------------------------------------------------
def detection_inputs(B, rng):
    """the inputs of one block size: (name, bytes)"""
    def blocks(kinds, last=None):
        """kinds: per block 'r' random (made non-constant), a byte value for a constant block, or ('x', value, offset): constant
        except the byte at offset; last: length of a short last block appended (random; for length 1 constant by the rule)"""
        out = []
        for k in kinds:
            if isinstance(k, str):
                blk = rng.integers(0, 256, B, dtype=np.uint8)
                if B > 1:
                    blk[B // 2] = blk[0] ^ 0x55   # never constant by chance
            elif isinstance(k, tuple):
                blk = np.full(B, k[1], dtype=np.uint8)
                blk[k[2]] ^= 0x80
            else:
                blk = np.full(B, k, dtype=np.uint8)
            out.append(blk)
        if last:
            tail = rng.integers(0, 256, last, dtype=np.uint8)
            if last > 1:
                tail[-1] = tail[0] ^ 1
            out.append(tail)
        return np.concatenate(out) if out else np.zeros(0, np.uint8)

    cases = [("empty", np.zeros(0, np.uint8)),
             ("none", blocks(["r"] * 5)),
             ("all", blocks([7] * 5)),
             ("alternating", blocks(["r", 0, "r", 255, "r"])),
             ("neighbours", blocks([1, 2, 2, 3, 0])),
             ("last one byte", blocks(["r", 9], last=1)),
             ("constant last one byte", np.concatenate([blocks([4, 4]), np.full(1, 4, np.uint8)]))]
    if B > 1:
        cases += [("first byte off", blocks([5, ("x", 5, 0), 5])),
                  ("last byte off", blocks([5, ("x", 5, B - 1), 5])),
                  ("last B - 1 bytes", blocks(["r", 9], last=B - 1)),
                  ("constant last B - 1 bytes", np.concatenate([blocks(["r"]), np.full(B - 1, 3, np.uint8)]))]
    for off in (15, 16, 17):
        if off < B - 1:
            cases.append((f"byte {off} off", blocks([0, ("x", 0, off), ("x", 200, off), 0])))
    for nb in (1, 63, 64, 65, 130):   # across a wave's 64 table entries and a workgroup's four blocks
        cases.append((f"{nb} blocks", blocks([(b % 251) if b % 3 else "r" for b in range(nb)])))
    return cases


@pytest.mark.parametrize("B", [1, 16, 48, 100, 1008, 4096])
def test_const_select_matches_restatement(rx, B):
    import torch
    rng = np.random.default_rng(B)
    for name, x in detection_inputs(B, rng):
        want = const_ref(x, B)
        for align in (0, 1, 4, 8):
            t, view, lo = on_device(x, align)
            nb = len(want)
            ft, flags, flo = guarded(nb)
            lib = _lib().lib()
            rc = lib.redux_const_blocks_dev(_v(view), len(x), B, C.c_void_p(flags.data_ptr()), None)
            assert rc == 0
            torch.cuda.synchronize()
            assert guards_intact(ft, flo, nb) and guards_intact(t, lo, len(x)), (name, align)
            assert np.array_equal(view.cpu().numpy(), x)
            got = flags.cpu().numpy()
            assert np.array_equal(got, want), (B, name, align, np.nonzero(got != want)[0][:8].tolist())
    # the Python wrapper: a device tensor gives a device tensor, bytes give numpy
    x = detection_inputs(B, rng)[3][1]
    assert np.array_equal(rx.api.constant_blocks(torch.from_numpy(x).cuda(), B).cpu().numpy(), const_ref(x, B))
    assert np.array_equal(rx.api.constant_blocks(x.tobytes(), B), const_ref(x, B))
    with pytest.raises(rx.InvalidInput):
        rx.api.constant_blocks(x.tobytes(), 0)


# ---- 2. the `_dev` coder calls ----------------------------------------------------------------------------------------------
def encode_ref_dev(d_in, n, d_base, base_len, E, B):
    """redux_encode_base_dev (base_len > 0) or redux_encode_planes_dev -> (out, offsets, status, summary)"""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    wsb = (lib.redux_encode_base_workspace_bytes if base_len else lib.redux_encode_planes_workspace_bytes)(C.byref(cp), n, B, E)
    wst, wsp = workspace(wsb)
    cap = lib.redux_encode_bound(C.byref(cp), n, B)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    if base_len:
        rc = lib.redux_encode_base_dev(C.byref(cp), _v(d_in), n, _v(d_base), base_len, B, E, _v(out), cap, _v(offs), _v(status), _v(summ),
                                       wsp, wsb, None)
    else:
        rc = lib.redux_encode_planes_dev(C.byref(cp), _v(d_in), n, B, E, _v(out), cap, _v(offs), _v(status), _v(summ), wsp, wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out, offs, status, summ


def encode_const_dev(d_in, n, d_base, base_len, E, B):
    """redux_encode_const_dev between guards -> (out, offsets, flags, status, summary)"""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    wsb = lib.redux_encode_const_workspace_bytes(C.byref(cp), n, B, E)
    assert wsb
    wst, wsp = workspace(wsb)
    cap = lib.redux_encode_bound(C.byref(cp), n, B)
    big, out, lo = guarded(cap)
    ft, flags, flo = guarded(nb)
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_encode_const_dev(C.byref(cp), _v(d_in), n, _v(d_base) if base_len else None, base_len, B, E,
                                    C.c_void_p(out.data_ptr()), cap, _v(offs), C.c_void_p(flags.data_ptr()), _v(status), _v(summ),
                                    wsp, wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, cap) and guards_intact(ft, flo, nb)
    return out, offs, flags, status, summ


def decode_const_dev(d_streams, d_offs, d_flags, d_base, base_len, n, E, B, off=0):
    """redux_decode_const_dev into a guarded buffer `off` bytes off a 16-byte boundary -> (out, sizes, status, summary)"""
    import torch
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    nb = lib.redux_block_count(n, B)
    wsb = lib.redux_decode_const_workspace_bytes(C.byref(cp), n, B, E)
    wst, wsp = workspace(wsb)
    big, out, lo = guarded(n, off)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.full((2,), -7, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_decode_const_dev(C.byref(cp), _v(d_streams), _v(d_offs), C.c_void_p(d_flags.data_ptr()),
                                    _v(d_base) if base_len else None, base_len, n, B, E, C.c_void_p(out.data_ptr()), _v(sizes),
                                    _v(status), _v(summ), wsp, wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, n), "the decode call wrote outside d_out[0 .. out_len)"
    return out, sizes, status, summ


def series(E, B, kind, seed):
    """(x, y or None): five frames and a short last one.  x: random bytes, its frame 1 zeros and its frame 3 one repeated
    element (so every plane of it is constant, each with its own value).  y by kind: none; equal to x; equal on frames 1 and
    2 only; x's first two frames and a few bytes."""
    rng = np.random.default_rng(seed)
    F = E * B
    n = 5 * F + F // 2 + 3
    x = rng.integers(0, 256, n, dtype=np.uint8)
    x[F: 2 * F] = 0
    x[3 * F: 4 * F] = np.tile(np.arange(1, E + 1, dtype=np.uint8), B)
    if kind == "none":
        return x, None
    if kind == "equal":
        return x, x.copy()
    if kind == "some":
        y = rng.integers(0, 256, n, dtype=np.uint8)
        y[F: 3 * F] = x[F: 3 * F]
        return x, y
    return x, x[: 2 * F + 3 * E + 1].copy()


def check_coding(x, y, E, B, align=0):
    import torch
    lib = _lib().lib()
    n = len(x)
    nb = lib.redux_block_count(n, B)
    ylen = 0 if y is None else len(y)
    xp = planes_ref(x ^ pad(y if y is not None else b"", n), E, B)
    want_flags = const_ref(xp, B)
    tx, d_x, xlo = on_device(x, align)
    ty, d_y, ylo = on_device(y if y is not None else np.zeros(0, np.uint8))
    out, offs, flags, status, summ = encode_const_dev(d_x, n, d_y, ylen, E, B)
    assert guards_intact(tx, xlo, n) and guards_intact(ty, ylo, ylen)
    assert np.array_equal(flags.cpu().numpy(), want_flags), (E, B, np.nonzero(flags.cpu().numpy() != want_flags)[0].tolist())
    assert summ.tolist() == [0, 0] and not bool(status.any())
    # the streams the call without the option writes, and the oracle's
    rout, roffs, rstatus, rsumm = encode_ref_dev(d_x, n, d_y, ylen, E, B)
    assert rsumm.tolist() == [0, 0]
    ref = split(rout.cpu().numpy(), roffs.cpu().numpy())
    oracle, ost = ox.compress_blocks(xp, B, PARAMS)
    assert not ost.any() and ref == oracle
    want = [bytes([xp[b * B]]) if want_flags[b] else ref[b] for b in range(nb)]
    got = split(out.cpu().numpy(), offs.cpu().numpy())
    assert got == want, [b for b in range(nb) if got[b] != want[b]][:8]
    total = int(offs[-1])
    for off in (0, 5):
        back, sizes, dstatus, dsum = decode_const_dev(out[:total], offs, flags, d_y, ylen, n, E, B, off)
        assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
        assert sizes.tolist() == [min(B, n - b * B) for b in range(nb)]
        assert torch.equal(back, d_x)
    return want_flags


@pytest.mark.parametrize("kind", ["none", "equal", "some", "shorter"])
@pytest.mark.parametrize("B", [48, 1008, 4096])   # (48 and 1008: the full-grid encoders' table form; 4096: the small-grid ones')
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_const_dev_calls_against_the_calls_without_the_option_and_the_oracle(rx, E, B, kind):
    x, y = series(E, B, kind, seed=E * 1000 + B)
    flags = check_coding(x, y, E, B)
    if kind == "equal":
        assert flags.all()                      # no block is left for the coder: every table entry idle
    else:
        assert flags.any() and not flags.all()


def test_const_dev_calls_with_no_constant_block_short_inputs_and_an_unaligned_input(rx):
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, 70 * 1008 + 17, dtype=np.uint8)
    assert not check_coding(x, None, 2, 1008).any()                 # nothing to skip: every block through the table form
    assert not check_coding(x[: 300 * 48], None, 1, 48, align=1).any()   # E = 1 reads the caller's buffer: off a 16-byte boundary
    flags = check_coding(np.concatenate([x[:4096], np.zeros(4096 + 1, np.uint8)]), None, 1, 4096, align=4)
    assert flags.tolist() == [0, 1, 1]                              # a last block of one byte is constant
    assert check_coding(x[:1], None, 4, 4096).tolist() == [1]
    assert check_coding(np.zeros(0, np.uint8), None, 2, 4096).tolist() == [0]             # the empty input
    assert check_coding(np.zeros(0, np.uint8), x[:100].copy(), 2, 4096).tolist() == [0]


# ---- 3. damaged input to decode ---------------------------------------------------------------------------------------------
def test_decode_const_dev_reports_damaged_input_per_block(rx):
    import torch
    L = _lib()
    B, E = 48, 1
    rng = np.random.default_rng(11)
    x = rng.integers(0, 256, 6 * B + 20, dtype=np.uint8)
    x[B: 2 * B] = 0x41
    x[4 * B: 5 * B] = 0
    n, nb = len(x), 7
    d_x = torch.from_numpy(x).cuda()
    out, offs, flags, status, summ = encode_const_dev(d_x, n, None, 0, E, B)
    assert flags.tolist() == [0, 1, 0, 0, 1, 0, 0]
    good = split(out.cpu().numpy(), offs.cpu().numpy())
    Lb = [min(B, n - b * B) for b in range(nb)]

    def run(streams, fl, hit, status_want):
        o = np.zeros(nb + 1, dtype=np.int64)
        o[1:] = np.cumsum([len(s) for s in streams])
        d_s = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\0", dtype=np.uint8).copy()).cuda()
        for off in (0, 3):
            back, sizes, dstatus, dsum = decode_const_dev(d_s, torch.from_numpy(o).cuda(), torch.tensor(fl, dtype=torch.uint8).cuda(),
                                                          None, 0, n, E, B, off)
            st = dstatus.tolist()
            assert [b for b in range(nb) if st[b]] == [hit], st
            if status_want is not None:
                assert st[hit] == status_want and sizes[hit].item() == 0
            assert dsum.tolist() == [st[hit], 1]
            got = back.cpu().numpy()
            for b in range(nb):
                if b != hit:
                    assert sizes[b].item() == Lb[b] and np.array_equal(got[b * B: b * B + Lb[b]], x[b * B: b * B + Lb[b]]), b
            if status_want is not None:   # nothing is written for that block
                assert (got[hit * B: hit * B + Lb[hit]] == FILL).all()

    fl = flags.tolist()
    run(good, fl[:1] + [2] + fl[2:], 1, L.INVALID_INPUT)                                   # a flag other than 0 / 1
    run(good, fl[:2] + [2] + fl[3:], 2, L.INVALID_INPUT)                                   # ... on a coded block
    run(good[:4] + [b""] + good[5:], fl, 4, L.INVALID_INPUT)                               # a constant block, 0-byte payload
    run(good[:4] + [b"\0\0"] + good[5:], fl, 4, L.INVALID_INPUT)                           # ... 2-byte payload
    run(good[:2] + [good[2][: len(good[2]) // 3]] + good[3:], fl, 2, None)                 # a damaged stream next to one
    # a constant flag on the empty input's block
    back, sizes, dstatus, dsum = decode_const_dev(torch.zeros(1, dtype=torch.uint8, device="cuda:0"),
                                                  torch.tensor([0, 1], dtype=torch.int64).cuda(),
                                                  torch.ones(1, dtype=torch.uint8, device="cuda:0"), None, 0, 0, 2, 4096)
    assert dstatus.tolist() == [L.INVALID_INPUT] and sizes.tolist() == [0] and dsum.tolist() == [L.INVALID_INPUT, 1]


# ---- 4. the host-pointer pair -----------------------------------------------------------------------------------------------
def test_host_pointer_pair_over_chunks_and_contexts_equals_the_one_chunk_call(rx):
    """B = 256, 200 blocks, E = 2, the base ending inside the second chunk of 64 blocks; unchanged frames in the first and the
    third chunk, constant input behind the base in the last."""
    B, E, nb = 256, 2, 200
    n = nb * B - 77
    rng = np.random.default_rng(3)
    x = rng.integers(0, 256, n, dtype=np.uint8)
    y = rng.integers(0, 256, 100 * B + 2 * E + 1, dtype=np.uint8)
    y[10 * B: 30 * B] = x[10 * B: 30 * B]
    y[70 * B: 80 * B] = x[70 * B: 80 * B]
    x[150 * B: 170 * B] = 0
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, n, B)]
    want_flags = const_ref(planes_ref(x ^ pad(y, n), E, B), B)
    assert 40 <= int(want_flags.sum()) < nb
    crc = np.zeros(nb, np.uint32)
    one = rx.compress_blocks(x, B, PARAMS, element_size=E, block_crc=crc, base=y, constant=True)
    assert rx.host_chunk_plan(nb, B)[1] == 1 and crc.tolist() == want_crc and np.array_equal(one[3], want_flags)
    plain = rx.compress_blocks(x, B, PARAMS, element_size=E, base=y)
    ref = split(plain[0], plain[1])
    assert split(one[0], one[1]) == [ref[b] if not want_flags[b] else bytes([0]) for b in range(nb)]
    nobase = rx.compress_blocks(x, B, PARAMS, element_size=E, constant=True)
    assert np.array_equal(nobase[3], const_ref(planes_ref(x, E, B), B)) and nobase[3].sum() == 20
    try:
        for devices in ([], [0, 0]):   # two contexts on one device
            rx.host_set_devices(devices)
            rx.host_set_chunk_bytes(64 * B, 64 * B)
            assert rx.host_chunk_plan(nb, B)[1] >= 3
            crc = np.zeros(nb, np.uint32)
            flags = np.full(nb, 9, np.uint8)
            h_out, h_offs, h_st = rx.compress_blocks(x, B, PARAMS, element_size=E, block_crc=crc, base=y, constant=flags)
            assert not h_st.any() and crc.tolist() == want_crc and np.array_equal(flags, want_flags)
            assert np.array_equal(h_offs, one[1]) and np.array_equal(h_out, one[0])
            dcrc = np.zeros(nb, np.uint32)
            back, sizes, st = rx.decompress_blocks(h_out, h_offs, B, PARAMS, element_size=E, length=n, block_crc=dcrc, base=y,
                                                   constant=flags)
            assert not st.any() and np.array_equal(back, x) and dcrc.tolist() == want_crc
            assert sizes.tolist() == [min(B, n - b * B) for b in range(nb)]
            back2, _, _ = rx.decompress_blocks(nobase[0], nobase[1], B, PARAMS, element_size=E, length=n, constant=nobase[3])
            assert np.array_equal(back2, x)
    finally:
        rx.host_set_chunk_bytes(0, 0)
        rx.host_set_devices([])
    # damaged flags through the host-pointer decode: reported, and only out[0 .. n) is written
    L, lib = _lib(), _lib().lib()
    cp = L.Params(*PARAMS)
    bad = want_flags.copy()
    bad[7] = 2
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs, hst = np.zeros(nb, np.uint32), np.zeros(nb, np.int32)
    offs = one[1].astype(np.uint64)
    rc = lib.redux_decode_blocks_const(C.byref(cp), one[0].ctypes.data, offs.ctypes.data, bad.ctypes.data, y.ctypes.data, len(y), n, B, E,
                                       hout.ctypes.data, hs.ctypes.data, hst.ctypes.data, None)
    assert rc == L.INVALID_INPUT and np.nonzero(hst)[0].tolist() == [7] and (hout[n:] == FILL).all()


def test_cpp_const_mirror(rx, tmp_path):
    import os
    import subprocess
    exe = build_const_mirror_test(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([exe, os.path.join(root, "tests", "golden", "corpora", "canterbury", "lcet10.txt")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and "const mirror ok" in out.stdout, out.stdout + out.stderr


# ---- 5. device coder objects, container and CLI end to end ------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """1 MiB of fp32 weights and the same after an update that left the middle half (frames 1 and 2 of four) alone"""
    rng = np.random.default_rng(20261018)
    n = 1 << 18
    w = (rng.standard_normal(n) * 0.02).astype(np.float32)
    w2 = (w + np.float32(2e-5) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    w2[n // 4: 3 * n // 4] = w[n // 4: 3 * n // 4]
    return w.view(np.uint8), w2.view(np.uint8)


def test_device_coder_objects_skip_constant_blocks(rx, pair):
    import torch
    w, w2 = pair
    B, E, n = 65536, 4, len(w2)
    d_w, d_w2 = torch.from_numpy(w).cuda(), torch.from_numpy(w2).cuda()
    enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E, base=d_w, constant=True)
    out, offs, status, summary, flags = enc.encode(d_w2)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and flags.tolist() == [0] * 4 + [1] * 8 + [0] * 4
    ref = rx.compress_blocks(w2, B, PARAMS, element_size=E, base=w, constant=True)
    total = int(ref[1][-1])
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1]) and np.array_equal(out[:total].cpu().numpy(), ref[0])
    dec = rx.DeviceDecoder(PARAMS, B, 16, element_size=E, base=d_w, constant=True)
    d_out, sizes, st, dsum = dec.decode(out[:total], offs, length=n, constant=flags)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(d_out, d_w2)
    with pytest.raises(rx.InvalidInput):
        dec.decode(out[:total], offs, length=n)                       # the flags are required
    with pytest.raises(rx.InvalidInput):
        dec.decode(out[:total], offs, constant=flags)                 # and the length
    with pytest.raises(rx.InvalidInput):
        rx.DeviceDecoder(PARAMS, B, 16, element_size=E, base=d_w).decode(out[:total], offs, length=n, constant=flags)
    with pytest.raises(rx.Unsupported):
        enc.encode_slots(d_w2)
    with pytest.raises(rx.Unsupported):
        rx.DeviceEncoder((4, 10, 16), B, n, constant=True)
    # without a base: the same object on constant input
    z = torch.zeros(3 * B + 5, dtype=torch.uint8, device="cuda:0")
    e1 = rx.DeviceEncoder(PARAMS, B, z.numel(), constant=True)
    o1, f1, _, s1, c1 = e1.encode(z)
    torch.cuda.synchronize()
    assert s1.tolist() == [0, 0] and c1.tolist() == [1] * 4 and f1.tolist() == [0, 1, 2, 3, 4]
    b1, _, _, bs1 = rx.DeviceDecoder(PARAMS, B, 4, constant=True).decode(o1[:4], f1, length=z.numel(), constant=c1)
    torch.cuda.synchronize()
    assert bs1.tolist() == [0, 0] and torch.equal(b1, z)
    # and without the option nothing changes
    a, b = rx.compress_blocks(w2, B, PARAMS, element_size=E, base=w), rx.compress_blocks(w2, B, PARAMS, element_size=E, base=w, constant=None)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def size_identity(container, with_, without):
    """len(with) == len(without) - sum over constant blocks of (s_b - 1) + ceil(nblocks / 8), s_b the sizes of `without`"""
    c = container._parse(with_)
    s = np.diff(container._parse(without).offsets.astype(np.int64))
    nb = len(s)
    assert len(with_) == len(without) - int((s[c.constant == 1] - 1).sum()) + (nb + 7) // 8, (len(with_), len(without))


def test_container_skips_constant_blocks_and_round_trips(rx, pair):
    from redux_amd import container
    w, w2 = pair
    v8 = container.compress_bytes(w2, 65536, element_size=4, base=w)
    v9 = container.compress_bytes(w2, 65536, element_size=4, base=w, skip_constant=True)
    print("fp32 pair, middle half unchanged: %d bytes without the option, %d with it" % (len(v8), len(v9)))
    assert v8[4] == 8 and v9[4] == 9 and int.from_bytes(v9[12:16], "little") == 0x90000014
    assert container.constant(v9).tolist() == [0] * 4 + [1] * 8 + [0] * 4 and container.base(v9) == container.base(v8)
    size_identity(container, v9, v8)
    assert container.decompress_bytes(v9, base=w) == w2.tobytes()
    assert v8 == container.compress_bytes(w2, 65536, element_size=4, base=w, skip_constant=False)
    for bad in (None, w[:-1], w2):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(v9, base=bad)
    # checksums; no base (F = 0) against version 2 / 1; every element size; a short last block; the empty input
    y = np.concatenate([w2[: 2 * 65536 + 13], np.zeros(3 * 65536, np.uint8), w2[:77]]).tobytes()
    for E in (1, 2, 4, 8):
        for base in (None, w[: 65536 + 5]):
            plain = container.compress_bytes(y, 4096, element_size=E, base=base, checksum=True)
            skip = container.compress_bytes(y, 4096, element_size=E, base=base, checksum=True, skip_constant=True)
            assert skip[4] == 0x19 and int.from_bytes(skip[12:16], "little") == 0x90000000 | (base is not None) << 4 | E
            size_identity(container, skip, plain)
            assert container.constant(skip).sum() >= 48 - E   # 48 blocks of zeros: every frame that lies wholly inside them
            assert container.decompress_bytes(skip, base=base) == y
            assert container.block_crcs(skip).tolist() == [zlib.crc32(y[o: o + 4096]) for o in range(0, len(y), 4096)]
    empty = container.compress_bytes(b"", 65536, element_size=4, skip_constant=True)
    assert container.constant(empty).tolist() == [0] and container.decompress_bytes(empty) == b""
    # a damaged bitmap under checksums: a coded block declared constant fails the size check of the parse, a constant one
    # declared coded decodes its byte as a stream
    hurt = bytearray(container.compress_bytes(w2, 65536, element_size=4, base=w, skip_constant=True, checksum=True))
    at = 32 + 12 + 64 + 64
    assert hurt[at: at + 2] == bytes([0xF0, 0x0F])
    hurt[at] = 0xE0
    with pytest.raises(rx.Error):
        container.decompress_bytes(bytes(hurt), base=w)


def test_cli_with_skip_constant(rx, pair, tmp_path):
    from redux_amd import cli, container
    w, w2 = pair
    prev, cur = tmp_path / "step0.f32", tmp_path / "step1.f32"
    prev.write_bytes(w.tobytes())
    cur.write_bytes(w2.tobytes())
    plain, skip, back = tmp_path / "base.rdxb", tmp_path / "skip.rdxb", tmp_path / "back.f32"
    common = ["--block-size", "65536", "--element-size", "4", "--base", str(prev), "--checksum"]
    assert cli.main(["-c", "-i", str(cur), "-o", str(plain)] + common) == 0
    assert cli.main(["-c", "-i", str(cur), "-o", str(skip), "--skip-constant"] + common) == 0
    p8, p9 = plain.read_bytes(), skip.read_bytes()
    assert p8[4] == 0x18 and p9[4] == 0x19 and container.constant(p9).sum() == 8
    size_identity(container, p9, p8)
    assert cli.main(["-d", "-i", str(skip), "-o", str(back), "--base", str(prev)]) == 0 and back.read_bytes() == w2.tobytes()
    assert cli.main(["-d", "-i", str(skip), "-o", str(back)]) == 3                          # no base
    assert cli.main(["-d", "-i", str(skip), "-o", str(back), "--base", str(cur)]) == 3      # another file as base
    # without a base
    assert cli.main(["-c", "-i", str(cur), "-o", str(skip), "--skip-constant", "--block-size", "65536"]) == 0
    assert skip.read_bytes()[4] == 9
    assert cli.main(["-d", "-i", str(skip), "-o", str(back)]) == 0 and back.read_bytes() == w2.tobytes()
