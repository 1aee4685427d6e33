"""Plane-static coding on the device: every stream against the CPU oracle under its plane's table, the device-built tables
against the numpy rule, every kernel instance, host-pointer calls against device calls, damage, E = 1, container / CLI."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT, corpus_files
from oracle import cbind as ox
from test_plane_static_cpu import plane_counts, tables_ref, typed
from test_planes_cpu import planes_ref
from test_static_gpu import guarded, guards_intact, oracle_decode_raw

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
TOTAL = 1 << 16


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def sp(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def data_of(kind, n, rx, seed=1):
    if n == 0:
        return np.zeros(0, np.uint8)
    if kind == "iid":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "zipf":
        return rx.gen_zipf(n, seed=seed).cpu().numpy()
    if kind == "bf16":
        return np.resize(typed("bf16", n + 2, seed), n)
    if kind == "one":
        return np.full(n, 0x3C, dtype=np.uint8)
    files = corpus_files("canterbury", "calgary")
    raw = np.frombuffer(open(files[seed % len(files)][1], "rb").read(), dtype=np.uint8)
    return np.resize(raw, n)


def to_dev(torch, host, off=0):
    buf = torch.zeros(host.size + 512, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 256 == 0
    d = buf[off: off + host.size]
    d.copy_(torch.from_numpy(host).cuda())
    return d


def coder_of(rx, torch, params, cums, E, B, n):
    d_cum = torch.from_numpy(np.ascontiguousarray(cums).view(np.int32).reshape(-1).copy()).cuda()
    return rx.DevicePlaneStaticCoder(params, d_cum, int(np.asarray(cums)[:, -1].max()), E, B, max(n, 1))


def check_streams(out, offs, xp, cums, E, B, params):
    """every block: the stream equals the oracle's for block b of x' under table b mod E"""
    o = offs.cpu().numpy()
    got = out[: int(o[-1])].cpu().numpy()
    nb = len(o) - 1
    for b in range(nb):
        want, _ = ox.compress_static(xp[b * B: (b + 1) * B], cums[b % E], params)
        g = got[int(o[b]): int(o[b + 1])].tobytes()
        assert g == want, f"block {b} of {nb} (table {b % E}): {len(g)} vs {len(want)} bytes"


def device_counts(torch, lib, d_x, B, E, cuts=()):
    counts = torch.zeros(E * 256, dtype=torch.int64, device="cuda:0")
    edges = [0] + list(cuts) + [d_x.numel()]
    for a, b in zip(edges, edges[1:]):
        # (a piece is whole frames, so its first block is a multiple of E: the counts pointer does not move)
        st = lib.lib().redux_plane_histogram_dev(C.c_void_p(d_x.data_ptr() + a) if b > a else None, b - a, B, E,
                                                 C.c_void_p(counts.data_ptr()), None, 0, sp(torch))
        assert st == lib.OK
    return counts.cpu().numpy().astype(np.uint64).reshape(E, 256)


def run_case(rx, lib, kind, n, E, B, params=P, total=TOTAL, in_off=0, seed=1):
    import torch
    x = data_of(kind, n, rx, seed)
    want_cums, xp = tables_ref(x, E, B, total)
    d_in = to_dev(torch, x, in_off)
    # the histogram: one call, and cut into calls at frame boundaries
    d_x = rx.planes(d_in, E, B) if n else d_in
    ref_counts = plane_counts(xp, E, B)
    assert np.array_equal(device_counts(torch, lib, d_x, B, E), ref_counts), (kind, n, E, B)
    F = E * B
    if n > 2 * F:
        assert np.array_equal(device_counts(torch, lib, d_x, B, E, cuts=(F, (n // F) * F)), ref_counts)
    if n > 16:  # an unaligned x' takes the byte-wise path
        d_u = to_dev(torch, xp, 3)
        assert np.array_equal(device_counts(torch, lib, d_u, B, E), ref_counts)
    coder = rx.DevicePlaneStaticCoder.from_data(d_in, params, E, B, max(n, 1), total=total)
    assert np.array_equal(coder.tables(), want_cums), (kind, n, E, B)
    assert np.array_equal(rx.plane_static_tables(d_in, E, B, params, total), want_cums)
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and not bool(status.any())
    check_streams(out, offs, xp, want_cums, E, B, params)
    o = offs.cpu().numpy()
    dec, sizes, dstatus, dsum = coder.decode(out[: int(o[-1])], offs, n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
    assert np.array_equal(dec.cpu().numpy(), x), (kind, n, E, B)
    return coder, x, xp, want_cums, out, offs


# ---- 6. bit-exactness -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4096, 65536, 100])
@pytest.mark.parametrize("E", [2, 4, 8])
def test_streams_tables_and_round_trip(rx, lib, E, B):
    lens = [0, 1, E * B - 1, 63 * B + 7, 64 * B, 65 * B + 1, (64 * E + 3) * B + 5]
    for i, kind in enumerate(["iid", "zipf", "bf16", "one", "corpus"]):
        for n in (lens if kind in ("bf16", "corpus") else lens[3:]):
            run_case(rx, lib, kind, n, E, B, seed=i + n % 7, in_off=(0 if n % 2 else 16))


def test_unaligned_input(rx, lib):
    run_case(rx, lib, "bf16", 70 * 4096 + 9, 2, 4096, in_off=5)


@pytest.mark.parametrize("E,B", [(2, 100), (8, 100), (2, 4096)])
def test_past_the_solo_boundary(rx, lib, E, B):
    """more than one wave per SIMD: the other encode / decode instances (names checked in test_every_kernel_instance)"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nb = 4 * cus * 64 + 64 * E + 3
    n = nb * B - 7
    cp = lib.Params(*P)
    assert b"one wave per SIMD" not in lib.lib().redux_plane_static_encode_kernel_name(C.byref(cp), TOTAL, n, B, E)
    assert b"one wave per SIMD" in lib.lib().redux_plane_static_encode_kernel_name(C.byref(cp), TOTAL, 4 * cus * 64 * B, B, E)
    run_case(rx, lib, "bf16", n, E, B)


# ---- 7. every kernel instance ---------------------------------------------------------------------------------------
def test_every_kernel_instance(rx, lib):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = lib.lib()
    seen_enc, seen_dec = set(), set()
    E = 2
    for params in (P, (8, 22, 24)):
        for total in (1 << 16, 100000, 1 << 17, (1 << 17) + 12345):
            for B, nb in ((4096, 64 * E + 3), (100, 4 * cus * 64 + 64 * E + 3)):
                n = nb * B - 3
                cp = lib.Params(*params)
                en = L.redux_plane_static_encode_kernel_name(C.byref(cp), total, n, B, E).decode()
                dn = L.redux_plane_static_decode_kernel_name(C.byref(cp), total, nb, E).decode()
                assert en.startswith("k_encode_segment_static<") and dn.startswith("k_decode_segment_static"), (en, dn)  # (one segment)
                # the instance is the one the one-table call picks for a launch of as many waves
                waves = E * (((nb + E - 1) // E + 63) // 64)
                ones = (C.c_uint32 * 258)(*([min(i, 256) * (total // 257) for i in range(257)] + [total]))
                assert L.redux_static_table_check(C.byref(cp), ones) == lib.OK
                assert en.replace("_segment_static", "_static") == L.redux_static_encode_kernel_name(C.byref(cp), ones, waves * 64 * B, B).decode()
                assert dn.replace("_segment_static", "_static") == L.redux_static_decode_kernel_name(C.byref(cp), ones, waves * 64).decode()
                assert ("fix-up" in en) == (total >= 1 << 17) and ("fix-up" in dn) == (total >= 1 << 17)
                assert ("lut" in dn) == (total <= 1 << 16)
                seen_enc.add(en)
                seen_dec.add(dn)
                run_case(rx, lib, "bf16", n, E, B, params=params, total=total, seed=total % 5)
    assert len(seen_enc) == 4 and len(seen_dec) == 9, (sorted(seen_enc), sorted(seen_dec))


# ---- 8. host-pointer calls ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 4, 8])
def test_host_calls_equal_device_calls_for_every_chunking(rx, lib, E):
    B = 4096
    n = (64 * 5 + 9) * B + 77
    coder, x, xp, cums, out, offs = run_case(rx, lib, "bf16", n, E, B)
    o = offs.cpu().numpy().astype(np.uint64)
    dev = out[: int(o[-1])].cpu().numpy()
    nb = len(o) - 1
    want_crc = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)], dtype=np.uint32)
    try:
        for chunk in (0, 64 * B, 128 * B):
            rx.host_set_chunk_bytes(chunk, chunk)
            assert np.array_equal(rx.plane_static_tables(x, E, B), cums), chunk
            m = rx.PlaneStaticModel.from_data(x, E, B)
            assert np.array_equal(m.cums, cums)
            for crc in (None, np.zeros(nb, dtype=np.uint32)):
                s, so, st = rx.compress_blocks(x, B, m, block_crc=crc)
                assert np.array_equal(so, o) and np.array_equal(s, dev) and not st.any(), chunk
                got = None if crc is None else np.zeros(nb, dtype=np.uint32)
                back, sizes, st = rx.decompress_blocks(s, so, B, m, length=n, element_size=E, block_crc=got)
                assert np.array_equal(back, x) and not st.any()
                if crc is not None:
                    assert np.array_equal(crc, want_crc) and np.array_equal(got, want_crc)
    finally:
        rx.host_set_chunk_bytes(0, 0)


# ---- 9. damage ------------------------------------------------------------------------------------------------------
def decode_guarded(rx, lib, coder, d_streams, d_offs, n, out_off=0, d_cum=None):
    import torch
    whole, d_out = guarded(torch, n, out_off)
    nb = d_offs.numel() - 1
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = lib.lib().redux_plane_static_decode_dev(
        C.byref(coder.cp), C.c_void_p((coder.d_cum if d_cum is None else d_cum).data_ptr()), coder.total,
        C.c_void_p(d_streams.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, coder.block_size, coder.E,
        C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()),
        C.c_void_p(summary.data_ptr()), coder._ws_ptr(), coder.ws_bytes, sp(torch))
    assert st == lib.OK
    torch.cuda.synchronize()
    assert guards_intact(whole, n, out_off)
    return d_out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy(), summary.tolist()


@pytest.mark.parametrize("E,B", [(2, 4096), (4, 100), (8, 4096)])
def test_damaged_streams(rx, lib, E, B):
    import torch
    n = (64 * E + 5) * B + 13
    coder, x, xp, cums, out, offs = run_case(rx, lib, "bf16", n, E, B)
    o = offs.cpu().numpy()
    nb = len(o) - 1
    streams = out[: int(o[-1])].cpu().numpy().copy()
    rng = np.random.default_rng(E)
    # bit flips and truncations: each block's status and size are the oracle's for that stream under its table, with the
    # planes path's length rule on top (an OK block of the wrong length is INVALID_INPUT)
    hurt = sorted(set(rng.integers(0, nb, 24).tolist()))
    dam, offs2 = streams.copy(), o.copy()
    for b in hurt[::2]:
        dam[int(o[b]) + int(rng.integers(0, o[b + 1] - o[b]))] ^= 1 << int(rng.integers(0, 8))
    parts = []
    for b in range(nb):
        s = dam[int(o[b]): int(o[b + 1])]
        parts.append(s[: max(0, len(s) - 3)] if b in hurt[1::2] else s)
        offs2[b + 1] = offs2[b] + len(parts[-1])
    dam2 = np.concatenate(parts)
    got, sizes, status, summary = decode_guarded(rx, lib, coder, torch.from_numpy(dam2).cuda(),
                                                 torch.from_numpy(offs2).cuda(), n, out_off=4)
    bad = 0
    for b in range(nb):
        want_len = min(B, n - b * B)
        st, raw = oracle_decode_raw(parts[b].tobytes(), B, cums[b % E], P)
        if st == 0 and len(raw) != want_len:
            st = lib.INVALID_INPUT
        assert status[b] == st, (b, status[b], st)
        if st == 0:
            assert sizes[b] == want_len
        bad += st != 0
    assert summary[1] == bad and bad > 0
    for b in set(range(nb)) - set(hurt):
        assert status[b] == 0
    # frames whose blocks are all OK hold the original bytes
    for f0 in range(0, nb, E):
        if not status[f0: f0 + E].any():
            assert np.array_equal(got[f0 * B: (f0 + E) * B], x[f0 * B: (f0 + E) * B])
    # offsets with slack: bytes after a stream are never read
    gaps = np.concatenate([np.concatenate([streams[int(o[b]): int(o[b + 1])], np.full(5, 0xEE, np.uint8)]) for b in range(nb)])
    loose = np.array([int(o[b]) + 5 * b for b in range(nb)] + [int(o[-1]) + 5 * nb], dtype=np.int64)
    got, sizes, status, summary = decode_guarded(rx, lib, coder, torch.from_numpy(gaps).cuda(), torch.from_numpy(loose).cuda(), n)
    assert summary == [0, 0] and np.array_equal(got, x)
    # the tables of the planes swapped: a table of another plane still decodes SOMETHING, within the plane buffer
    swapped = torch.from_numpy(np.ascontiguousarray(cums[::-1]).view(np.int32).reshape(-1).copy()).cuda()
    got, sizes, status, summary = decode_guarded(rx, lib, coder, out[: int(o[-1])], offs, n, d_cum=swapped)
    for b in range(0, nb, max(1, nb // 16)):
        st, raw = oracle_decode_raw(streams[int(o[b]): int(o[b + 1])].tobytes(), B, cums[::-1][b % E], P)
        if st == 0 and len(raw) != min(B, n - b * B):
            st = lib.INVALID_INPUT
        assert status[b] == st, b
    # a table the kernels must refuse: not increasing / another total
    broken = cums.copy()
    broken[1, 40] = broken[1, 39]
    d_broken = torch.from_numpy(broken.view(np.int32).reshape(-1).copy()).cuda()
    got, sizes, status, summary = decode_guarded(rx, lib, coder, out[: int(o[-1])], offs, n, d_cum=d_broken)
    assert all(status[b] == (lib.INVALID_INPUT if b % E == 1 else 0) for b in range(nb))
    assert summary == [lib.INVALID_INPUT, len(range(1, nb, E))]
    enc = coder_of(rx, torch, P, broken, E, B, n)
    _, _, est, esum = enc.encode(to_dev(torch, x))
    torch.cuda.synchronize()
    est = est.cpu().numpy()
    assert all(est[b] == (lib.INVALID_INPUT if b % E == 1 else 0) for b in range(nb)) and esum.tolist()[1] == len(range(1, nb, E))
    # out_cap too small for a block's stream: the encoder reports it, nothing is written past the output
    whole, d_small = guarded(torch, int(o[-1]) - 1, 0)
    eoffs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    estat = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    esum = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = lib.lib().redux_plane_static_encode_dev(
        C.byref(coder.cp), C.c_void_p(coder.d_cum.data_ptr()), coder.total, C.c_void_p(to_dev(torch, x).data_ptr()), n, B, E,
        C.c_void_p(d_small.data_ptr()), int(o[-1]) - 1, C.c_void_p(eoffs.data_ptr()), C.c_void_p(estat.data_ptr()),
        C.c_void_p(esum.data_ptr()), coder._ws_ptr(), coder.ws_bytes, sp(torch))
    torch.cuda.synchronize()
    assert st == lib.OK and guards_intact(whole, int(o[-1]) - 1, 0)
    assert esum.tolist()[0] == lib.OUTPUT_TOO_SMALL and estat.cpu().numpy()[-1] == lib.OUTPUT_TOO_SMALL
    # a workspace that is too small is refused before any launch
    assert lib.lib().redux_plane_static_decode_dev(
        C.byref(coder.cp), C.c_void_p(coder.d_cum.data_ptr()), coder.total, C.c_void_p(out.data_ptr()), C.c_void_p(offs.data_ptr()),
        n, B, E, C.c_void_p(d_small.data_ptr()), C.c_void_p(estat.data_ptr()), C.c_void_p(estat.data_ptr()), None,
        coder._ws_ptr(), 256, sp(torch)) == lib.OUTPUT_TOO_SMALL


# ---- 10. E = 1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nb", [(4096, 131), (100, 1000), (65536, 65)])
def test_one_table_through_the_new_calls_is_the_static_model(rx, lib, B, nb):
    import torch
    n = nb * B - 5
    x = data_of("zipf", n, rx, seed=nb)
    d_in = to_dev(torch, x)
    cum = rx.static_table(d_in, P)
    old = rx.DeviceStaticCoder(P, cum, B, n)
    o_out, o_offs, _, o_sum = old.encode(d_in)
    new = coder_of(rx, torch, P, cum.reshape(1, 258), 1, B, n)
    assert np.array_equal(rx.DevicePlaneStaticCoder.from_data(d_in, P, 1, B, n).tables()[0], cum)
    n_out, n_offs, _, n_sum = new.encode(d_in)
    torch.cuda.synchronize()
    assert o_sum.tolist() == [0, 0] and n_sum.tolist() == [0, 0]
    assert torch.equal(o_offs, n_offs)
    end = int(o_offs[-1])
    assert torch.equal(o_out[:end], n_out[:end])
    dec, _, _, dsum = new.decode(n_out[:end], n_offs, n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(dec, d_in)


# ---- 11. container and CLI ------------------------------------------------------------------------------------------
def test_container_and_cli_round_trip(rx, tmp_path):
    from redux_amd import container
    x = typed("bf16", 40 * 65536 + 6).tobytes() + b"xyz"
    for E, B in ((2, 65536), (4, 4096), (8, 1000)):
        for checksum in (False, True):
            blob = container.compress_bytes(x, B, P, element_size=E, model="plane-static", checksum=checksum)
            assert blob[4] == (0x14 if checksum else 4) and container.element_size(blob) == E
            cums, _ = tables_ref(np.frombuffer(x, np.uint8), E, B)
            assert np.array_equal(container.plane_static_tables(blob), cums)
            assert container.decompress_bytes(blob) == x
        planes_blob = container.compress_bytes(x, B, P, element_size=E)
        if (E, B) == (2, 65536):
            assert len(blob) < len(planes_blob)  # (bf16: the table per plane beats the adaptive coder on the same layout)
    # the CLI, with checksums: a damaged payload is a decompression error
    src, dst, out = tmp_path / "in.bin", tmp_path / "out.rdx", tmp_path / "back.bin"
    src.write_bytes(x)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", "-i", str(src), "-o", str(out), "--block-size", "65536",
                        "--model", "plane-static", "--element-size", "2", "--checksum"], env=env, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = out.read_bytes()
    assert blob[4] == 0x14
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-d", "-i", str(out), "-o", str(back_path(tmp_path))], env=env,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert back_path(tmp_path).read_bytes() == x
    bad = bytearray(blob)
    bad[-10] ^= 0x40
    out.write_bytes(bytes(bad))
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-d", "-i", str(out), "-o", str(back_path(tmp_path))], env=env,
                       capture_output=True, timeout=300)
    assert r.returncode == 3, r.stderr


def back_path(tmp_path):
    return tmp_path / "back.bin"
