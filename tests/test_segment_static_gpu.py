"""Segment-static coding on the device: every stream against the CPU oracle under the rule's table, the device-built tables
against the numpy rule, build + encode in one call, every kernel instance by name, host-pointer calls against device calls
for several chunkings and two contexts, CRCs, damaged tables and streams, container / CLI."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from oracle import cbind as ox
from test_plane_static_gpu import data_of, device_counts as plane_device_counts, sp, to_dev
from test_segment_static_cpu import mixed_bf16, nseg_of, segment_counts, segment_tables_ref
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


def data(kind, n, rx, seed=1):
    if kind == "mixed":
        return np.resize(mixed_bf16(n + 2, seed=seed, lo=9, hi=13), n) if n else np.zeros(0, np.uint8)
    return data_of(kind, n, rx, seed)


def check_streams(out, offs, xp, cums, E, B, G, params, every=1):
    """block b: the stream equals the oracle's for block b of x' under table (b // G) * E + b % E"""
    o = offs.cpu().numpy()
    got = out[: int(o[-1])].cpu().numpy()
    nb = len(o) - 1
    for b in range(0, nb, every):
        want, _ = ox.compress_static(xp[b * B: (b + 1) * B], cums[(b // G) * E + b % E], params)
        g = got[int(o[b]): int(o[b + 1])].tobytes()
        assert g == want, f"block {b} of {nb} (table {(b // G) * E + b % E}): {len(g)} vs {len(want)} bytes"


def device_counts(torch, lib, d_x, B, E, G):
    nt = lib.lib().redux_segment_static_table_count(max(1, -(-d_x.numel() // B)), E, G)
    counts = torch.zeros(nt * 256, dtype=torch.int64, device="cuda:0")
    st = lib.lib().redux_segment_histogram_dev(C.c_void_p(d_x.data_ptr()) if d_x.numel() else None, d_x.numel(), B, E, G,
                                               C.c_void_p(counts.data_ptr()), sp(torch))
    assert st == lib.OK
    return counts.cpu().numpy().astype(np.uint64).reshape(nt, 256)


def run_case(rx, lib, kind, n, E, B, k, params=P, total=TOTAL, in_off=0, seed=1):
    import torch
    G = 64 * E * k
    x = data(kind, n, rx, seed)
    want_cums, xp = segment_tables_ref(x, E, B, G, total)
    d_in = to_dev(torch, x, in_off)
    d_x = rx.planes(d_in, E, B) if n and E > 1 else d_in
    ref_counts = segment_counts(xp, E, B, G)
    assert np.array_equal(device_counts(torch, lib, d_x, B, E, G), ref_counts), (kind, n, E, B, k)
    if n > 16:  # an unaligned x' takes the byte-wise path
        assert np.array_equal(device_counts(torch, lib, to_dev(torch, xp, 3), B, E, G), ref_counts)
    assert np.array_equal(rx.segment_static_tables(d_in, E, B, G, params, total), want_cums)
    # build + encode in one call == tables, then encode
    coder = rx.DeviceSegmentStaticCoder.from_data(d_in, params, E, B, max(n, 1), G, total)
    torch.cuda.synchronize()
    assert coder.summary.tolist() == [0, 0]
    assert np.array_equal(coder.tables(n), want_cums), (kind, n, E, B, k)
    nb = max(1, -(-n // B))
    b_offs = coder.offsets[: nb + 1].clone()
    b_out = coder.out[: int(b_offs[-1])].clone()
    other = rx.DeviceSegmentStaticCoder(params, E, B, max(n, 1), G, total)
    other.set_tables(want_cums)
    out, offs, status, summary = other.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and not bool(status.any())
    assert torch.equal(offs, b_offs) and torch.equal(out[: int(offs[-1])], b_out)
    check_streams(out, offs, xp, want_cums, E, B, G, params)
    o = offs.cpu().numpy()
    dec, sizes, dstatus, dsum = other.decode(out[: int(o[-1])], offs, n)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
    assert np.array_equal(dec.cpu().numpy(), x), (kind, n, E, B, k)
    return other, x, xp, want_cums, out, offs


# ---- bit-exactness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_streams_tables_and_round_trip(rx, lib, E, k):
    G = 64 * E * k
    kinds = ["iid", "zipf", "one", "mixed"]
    # B = 100: empty, one byte, a multiple of G, not a multiple, a short last frame; B = 4096: two lengths on the data that moves
    for i, n in enumerate([0, 1, 2 * G * 100, (2 * G + E + 1) * 100 + 7, (G + 1) * 100 - 3]):
        run_case(rx, lib, kinds[(i + k) % 4], n, E, 100, k, seed=i + 1, in_off=(0 if n % 2 else 16))
    if k <= 2 or E == 1:
        run_case(rx, lib, "mixed", (G + 65) * 4096 + 5, E, 4096, k, seed=E)
        run_case(rx, lib, "mixed", 2 * G * 4096, E, 4096, k, seed=E + 1)


@pytest.mark.parametrize("E,k", [(1, 1), (1, 3), (2, 1)])
def test_large_blocks(rx, lib, E, k):
    G = 64 * E * k
    run_case(rx, lib, "mixed", (G + 3) * 65536 - 11, E, 65536, k, seed=k)


def test_unaligned_input(rx, lib):
    run_case(rx, lib, "mixed", 300 * 4096 + 9, 2, 4096, 1, in_off=5)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_one_segment_is_plane_static_and_static(rx, lib, E):
    import torch
    B, k = 4096, 2
    G = 64 * E * k
    n = G * B - 9
    x = data("mixed", n, rx, seed=E)
    d_in = to_dev(torch, x)
    seg = rx.DeviceSegmentStaticCoder.from_data(d_in, P, E, B, n, G)
    old = rx.DevicePlaneStaticCoder.from_data(d_in, P, E, B, n)
    o_out, o_offs, _, o_sum = old.encode(d_in)
    torch.cuda.synchronize()
    assert np.array_equal(seg.tables(n), old.tables())
    nb = o_offs.numel() - 1
    end = int(o_offs[-1])
    assert torch.equal(seg.offsets[: nb + 1], o_offs) and torch.equal(seg.out[:end], o_out[:end])
    if E == 1:
        one = rx.DeviceStaticCoder(P, rx.static_table(d_in, P), B, n)
        s_out, s_offs, _, _ = one.encode(d_in)
        torch.cuda.synchronize()
        assert torch.equal(s_offs, o_offs) and torch.equal(s_out[:end], o_out[:end])


@pytest.mark.parametrize("B", [100, 4096])
@pytest.mark.parametrize("E", [1, 2, 8])
def test_one_segment_equals_plane_static_call_for_call(rx, lib, E, B):
    """What lets plane-static run on the segment-static kernels: with one segment that holds every block, each segment call
    gives what its plane call gives (counts, tables, offsets, statuses, stream bytes), and each decoder reads the other's
    streams.  Once under the lookup decoder (total 2^16; its waves share a segment only if k % 4 == 0) and once under the
    lock-step one (total 2^16 + 1)."""
    import torch
    L = lib.lib()
    nb = 64 * E + 3
    n = nb * B - 3
    x = data_of("bf16", n, rx, seed=E)
    d_in = to_dev(torch, x)
    d_x = rx.planes(d_in, E, B) if E > 1 else d_in
    cp = lib.Params(*P)
    for total, k, form in ((1 << 16, 4, "_lut<"), ((1 << 16) + 1, 2, "_lock<")):
        G = 64 * E * k
        assert G >= nb
        assert form in L.redux_segment_static_decode_kernel_name(C.byref(cp), total, nb, E, G).decode()
        assert np.array_equal(device_counts(torch, lib, d_x, B, E, G), plane_device_counts(torch, lib, d_x, B, E))
        old = rx.DevicePlaneStaticCoder.from_data(d_in, P, E, B, n, total=total)
        cums = rx.segment_static_tables(d_in, E, B, G, P, total)
        assert np.array_equal(cums, old.tables())
        seg = rx.DeviceSegmentStaticCoder(P, E, B, n, G, total)
        seg.set_tables(cums)
        s_out, s_offs, s_st, s_sum = seg.encode(d_in)
        o_out, o_offs, o_st, o_sum = old.encode(d_in)
        torch.cuda.synchronize()
        end = int(o_offs[-1])
        assert torch.equal(s_offs, o_offs) and torch.equal(s_st, o_st) and s_sum.tolist() == o_sum.tolist() == [0, 0]
        assert torch.equal(s_out[:end], o_out[:end])
        for dec, (streams, offs) in ((seg, (o_out, o_offs)), (old, (s_out, s_offs))):
            back, sizes, dst, dsum = dec.decode(streams[:end], offs, n)
            torch.cuda.synchronize()
            assert dsum.tolist() == [0, 0] and not bool(dst.any())
            assert np.array_equal(back.cpu().numpy(), x), (E, B, total)


# ---- every kernel instance -------------------------------------------------------------------------------------------
def test_every_kernel_instance(rx, lib):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    L = lib.lib()
    seen_enc, seen_dec, seen = set(), set(), set()
    E = 2
    for params in (P, (8, 22, 24)):
        for total in (1 << 16, 100000, 1 << 17):
            for k in (1, 4, 8):
                for B, nb in ((4096, 64 * E * k + 3), (100, 4 * cus * 64 + 64 * E * k + 3)):
                    n = nb * B - 3
                    G = 64 * E * k
                    cp = lib.Params(*params)
                    en = L.redux_segment_static_encode_kernel_name(C.byref(cp), total, n, B, E, G).decode()
                    dn = L.redux_segment_static_decode_kernel_name(C.byref(cp), total, nb, E, G).decode()
                    assert en.startswith("k_encode_segment_static<") and dn.startswith("k_decode_segment_static"), (en, dn)
                    assert en == L.redux_plane_static_encode_kernel_name(C.byref(cp), total, n, B, E).decode()
                    assert ("fix-up" in en) == (total >= 1 << 17) and ("fix-up" in dn) == (total >= 1 << 17)
                    # the lookup decoder's waves share a segment: 8 waves need k % 8 == 0, 4 waves k % 4 == 0
                    solo = nb < 4 * cus * 64
                    if total <= 1 << 16:
                        want = "lut<%s, 8>" if k == 8 and not solo else "lut<%s, 4>" if k in (4, 8) else "lock<"
                        assert (want % ("true" if params[2] == 32 else "false") if "%" in want else want) in dn, (k, solo, dn)
                    else:
                        assert "lut" not in dn
                    seen_enc.add(en)
                    seen_dec.add(dn)
                    if (en, dn, k) in seen:  # (this pair of instances has run at this k)
                        continue
                    seen.add((en, dn, k))
                    run_case(rx, lib, "mixed", n, E, B, k, params=params, total=total, seed=total % 5 + k)
    assert len(seen_enc) == 4 and len(seen_dec) == 9, (sorted(seen_enc), sorted(seen_dec))


# ---- host-pointer calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,k", [(1, 1), (2, 1), (4, 2), (8, 1)])
def test_host_calls_equal_device_calls_for_every_chunking(rx, lib, E, k):
    B = 4096
    G = 64 * E * k
    n = (3 * G + 64 + 9) * B + 77
    coder, x, xp, cums, out, offs = run_case(rx, lib, "mixed", n, E, B, k)
    o = offs.cpu().numpy().astype(np.uint64)
    dev = out[: int(o[-1])].cpu().numpy()
    nb = len(o) - 1
    want_crc = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)], dtype=np.uint32)
    try:
        for devices in ([], [0, 0]):  # (two contexts on one device)
            rx.host_set_devices(devices)
            for chunk in (0, 64 * B, G * B, 2 * G * B + 64 * B):
                rx.host_set_chunk_bytes(chunk, chunk)
                for crc in (None, np.zeros(nb, dtype=np.uint32)):
                    m = rx.SegmentStaticModel.template(P, E, G)
                    s, so, st = rx.compress_blocks(x, B, m, block_crc=crc)
                    assert np.array_equal(m.cums, cums), (devices, chunk)
                    assert np.array_equal(so, o) and np.array_equal(s, dev) and not st.any(), (devices, chunk)
                    got = None if crc is None else np.zeros(nb, dtype=np.uint32)
                    back, sizes, st = rx.decompress_blocks(s, so, B, m, length=n, block_crc=got)
                    assert np.array_equal(back, x) and not st.any()
                    if crc is not None:
                        assert np.array_equal(crc, want_crc) and np.array_equal(got, want_crc)
                assert np.array_equal(rx.SegmentStaticModel.from_data(x, E, B, P, G).cums, cums)
    finally:
        rx.host_set_chunk_bytes(0, 0)
        rx.host_set_devices([])


# ---- damage ----------------------------------------------------------------------------------------------------------
def decode_guarded(rx, lib, coder, d_streams, d_offs, n, out_off=0, d_cum=None):
    import torch
    whole, d_out = guarded(torch, n, out_off)
    nb = d_offs.numel() - 1
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    st = lib.lib().redux_segment_static_decode_dev(
        C.byref(coder.cp), C.c_void_p((coder.d_cum if d_cum is None else d_cum).data_ptr()), coder.total,
        C.c_void_p(d_streams.data_ptr()), C.c_void_p(d_offs.data_ptr()), n, coder.block_size, coder.E, coder.G,
        C.c_void_p(d_out.data_ptr()), C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()),
        C.c_void_p(summary.data_ptr()), coder._ws_ptr(), coder.ws_bytes, sp(torch))
    assert st == lib.OK
    torch.cuda.synchronize()
    assert guards_intact(whole, n, out_off)
    return d_out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy(), summary.tolist()


@pytest.mark.parametrize("E,B,k,total", [(2, 4096, 1, TOTAL), (4, 100, 4, TOTAL), (2, 100, 8, TOTAL), (2, 100, 1, 1 << 17), (1, 4096, 2, 100000)])
def test_damaged_tables_and_streams(rx, lib, E, B, k, total):
    import torch
    G = 64 * E * k
    n = (2 * G + 64 * E + 5) * B + 13
    coder, x, xp, cums, out, offs = run_case(rx, lib, "mixed", n, E, B, k, total=total)
    o = offs.cpu().numpy()
    nb = len(o) - 1
    streams = out[: int(o[-1])].cpu().numpy().copy()
    # a table the kernels must refuse: exactly the blocks coded under it, b // G == 1 and b % E == E - 1; every workgroup
    # that loads it serves only such blocks, and the other segments decode
    broken = cums.copy()
    hit = 1 * E + E - 1
    broken[hit, 40] = broken[hit, 39]
    d_broken = torch.from_numpy(broken.view(np.int32).reshape(-1).copy()).cuda()
    got, sizes, status, summary = decode_guarded(rx, lib, coder, out[: int(o[-1])], offs, n, d_cum=d_broken)
    refused = [b for b in range(nb) if (b // G) * E + b % E == hit]
    assert len(refused) == G // E
    assert all(status[b] == (lib.INVALID_INPUT if b in set(refused) else 0) for b in range(nb))
    assert summary == [lib.INVALID_INPUT, len(refused)]
    for f0 in range(0, nb - nb % E, E):
        if f0 // G != 1:
            assert np.array_equal(got[f0 * B: (f0 + E) * B], x[f0 * B: (f0 + E) * B])
    enc = rx.DeviceSegmentStaticCoder(P, E, B, n, G, total)
    enc.set_tables(broken)
    _, _, est, esum = enc.encode(to_dev(torch, x))
    torch.cuda.synchronize()
    est = est.cpu().numpy()
    assert all(est[b] == (lib.INVALID_INPUT if b in set(refused) else 0) for b in range(nb)) and esum.tolist()[1] == len(refused)
    # bit flips and truncations: each block's status and size are the oracle's for that stream under its table, with the
    # planes path's length rule on top; nothing is written past out_len
    rng = np.random.default_rng(E + k)
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
        st, raw = oracle_decode_raw(parts[b].tobytes(), B, cums[(b // G) * E + b % E], P)
        if st == 0 and len(raw) != want_len:
            st = lib.INVALID_INPUT
        assert status[b] == st, (b, status[b], st)
        if st == 0:
            assert sizes[b] == want_len
        bad += st != 0
    assert summary[1] == bad and bad > 0
    # a workspace that is too small is refused before any launch
    assert lib.lib().redux_segment_static_decode_dev(
        C.byref(coder.cp), C.c_void_p(coder.d_cum.data_ptr()), coder.total, C.c_void_p(out.data_ptr()), C.c_void_p(offs.data_ptr()),
        n, B, E, G, C.c_void_p(out.data_ptr()), C.c_void_p(coder.status.data_ptr()), C.c_void_p(coder.status.data_ptr()), None,
        coder._ws_ptr(), 256 if E > 1 else 0, sp(torch)) == (lib.OUTPUT_TOO_SMALL if n else lib.OK)


# ---- container and CLI -----------------------------------------------------------------------------------------------
def test_container_and_cli_round_trip(rx, tmp_path):
    from redux_amd import container
    x = mixed_bf16(4 << 20).tobytes() + b"xyz"  # (tensors of 128 KiB to 1 MiB: the data moves from segment to segment)
    xa = np.frombuffer(x, np.uint8)
    for E, B, G in ((2, 4096, 128), (2, 4096, None), (1, 4096, 64), (4, 1000, 512), (8, 4096, 512)):
        for checksum in (False, True):
            blob = container.compress_bytes(x, B, P, element_size=E, model="segment-static", checksum=checksum, segment_blocks=G)
            g = rx.default_segment_blocks(E) if G is None else G
            assert blob[4] == (0x15 if checksum else 5) and container.element_size(blob) == E
            cums, _ = segment_tables_ref(xa, E, B, g)
            got, gg = container.segment_static_tables(blob)
            assert gg == g and np.array_equal(got, cums)
            assert container.decompress_bytes(blob) == x
        if G == 128:  # the case of test_segment_static_cpu's oracle test, end to end: smaller than one table per plane
            assert len(blob) < len(container.compress_bytes(x, B, P, element_size=E, model="plane-static", checksum=True))
    src, dst = tmp_path / "in.bin", tmp_path / "out.rdx"
    back = tmp_path / "back.bin"
    src.write_bytes(x)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", "-i", str(src), "-o", str(dst), "--block-size", "4096",
                        "--model", "segment-static", "--element-size", "2", "--segment-blocks", "256", "--checksum"], env=env,
                       capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    blob = dst.read_bytes()
    assert blob[4] == 0x15 and container.segment_static_tables(blob)[1] == 256
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-d", "-i", str(dst), "-o", str(back)], env=env, capture_output=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == x
    bad = bytearray(blob)
    bad[-10] ^= 0x40
    dst.write_bytes(bytes(bad))
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-d", "-i", str(dst), "-o", str(back)], env=env, capture_output=True,
                       timeout=300)
    assert r.returncode == 3, r.stderr
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", "-i", str(src), "-o", str(dst), "--block-size", "4096",
                        "--model", "segment-static", "--segment-blocks", "100"], env=env, capture_output=True, timeout=300)
    assert r.returncode == 1
