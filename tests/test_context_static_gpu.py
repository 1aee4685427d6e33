"""Context-static coding on the GPU (include/redux_hip.h, "context-static coding"): the pair histogram and the tables against
the numpy rule, every stream bit for bit against the reference model of test_context_static_cpu.py (oracle.redux_ref.Codec
with a model that answers from table ctx) and decoded back, refusals and damage inside guard bands, the host-pointer calls
against the device calls, and the container and CLI end to end.  Sizes are the smallest at which a lane, wave or workgroup
boundary can go wrong; the Python reference codes about 100,000 symbols a second."""
import ctypes as C
import functools
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from oracle import redux_ref as ref
from test_context_static_cpu import (P, TOTAL, ContextStaticModel, corpus, encode_ref, ideal_bits, pair_counts, table_section_bytes,
                                     tables_ref)
from test_context_static_instances_cpu import DEC, ENC, dec_name, enc_name

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def d_tables(cums):
    return dev(np.ascontiguousarray(cums, dtype=np.uint32).view(np.int32).reshape(-1))


@functools.lru_cache(maxsize=None)
def alice16k():
    return corpus("canterbury/alice29.txt")[:16384].copy()


@functools.lru_cache(maxsize=None)
def random64k():
    return np.random.default_rng(11).integers(0, 256, 65536).astype(np.uint8)


# ---- histogram and tables ------------------------------------------------------------------------------------------------
def device_counts(lib, pieces, B):
    """redux_context_histogram_dev over device tensors, added into one u64[256][256]"""
    import torch
    counts = torch.zeros(65536, dtype=torch.int64, device="cuda:0")
    for t in pieces:
        st = lib.lib().redux_context_histogram_dev(C.c_void_p(t.data_ptr()) if t.numel() else None, t.numel(), B,
                                                   C.c_void_p(counts.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == lib.OK
    torch.cuda.synchronize()
    return counts.cpu().numpy().astype(np.uint64).reshape(256, 256)


def boundary_data(n, B):
    """text in which every block ends in 0xEE and begins with 0xDD: the pair (0xEE, 0xDD) occurs only across boundaries"""
    x = np.resize(alice16k(), n).copy()
    x[B - 1::B] = 0xEE
    x[::B] = 0xDD
    return x


@pytest.mark.parametrize("B,n,offset", [(64, 64 * 300, 0), (64, 64 * 300 + 1, 0), (64, 64 * 300 + 37, 5), (257, 257 * 70 + 13, 1),
                                        (4096, 4096 * 9 + 4095, 0), (100000, 250007, 3), (64, 1, 0), (64, 15, 7), (64, 0, 0)])
def test_device_counts_equal_numpy(lib, B, n, offset):
    x = boundary_data(n, B) if n else np.zeros(0, dtype=np.uint8)
    whole = dev(np.concatenate([np.zeros(offset, dtype=np.uint8), x]))
    got = device_counts(lib, [whole[offset:]], B)
    want = pair_counts(x, B)
    assert np.array_equal(got, want)
    if n > 2 * B:
        assert got[0xEE, 0xDD] == 0 and got[0, 0xDD] == -(-n // B)  # boundary pairs are not counted; block starts count under 0


def test_device_counts_in_two_pieces_of_whole_blocks(lib):
    B, n = 257, 257 * 90 + 100
    x = boundary_data(n, B)
    d = dev(x)
    cut = 257 * 41
    assert np.array_equal(device_counts(lib, [d[:cut], d[cut:]], B), pair_counts(x, B))


@pytest.mark.parametrize("total", [65536, 4096])
def test_device_tables_equal_the_host_rule(rx, total):
    import torch
    for x, B in ((alice16k(), 4096), (random64k(), 65536), (np.zeros(5000, dtype=np.uint8), 64), (np.zeros(0, dtype=np.uint8), 64)):
        want = rx.context_static_tables_from_counts(pair_counts(x, B), P, total)
        assert np.array_equal(want, tables_ref(pair_counts(x, B), total))
        assert np.array_equal(rx.context_static_tables(dev(x) if len(x) else torch.zeros(0, dtype=torch.uint8, device="cuda:0"), B, P, total), want)
        assert np.array_equal(rx.context_static_tables(x, B, P, total), want)  # host pointers, through the pinned ring
    coder = rx.DeviceContextStaticCoder.from_data(dev(alice16k()), P, 4096, 16384, total)
    assert np.array_equal(coder.tables(), tables_ref(pair_counts(alice16k(), 4096), total))


def test_host_tables_do_not_depend_on_the_chunk_size(rx):
    x = np.resize(corpus("canterbury/alice29.txt"), 700001)
    want = tables_ref(pair_counts(x, 1000))
    try:
        rx.host_set_chunk_bytes(1, 1)  # 64 KiB chunks, rounded up to whole blocks
        assert np.array_equal(rx.context_static_tables(x, 1000), want)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    assert np.array_equal(rx.context_static_tables(x, 1000), want)


# ---- streams ---------------------------------------------------------------------------------------------------------------
def split(out, offs):
    return [out[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


def check_streams(rx, x, B, cums, params=P):
    """encode on the device == the reference model's streams; decoding gives x back"""
    import torch
    x = np.ascontiguousarray(x, dtype=np.uint8)
    coder = rx.DeviceContextStaticCoder(params, d_tables(cums), int(cums[0, 257]), B, max(len(x), 1))
    d_in = dev(x) if len(x) else torch.zeros(0, dtype=torch.uint8, device="cuda:0")
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and not status.cpu().numpy().any()
    offs_h = offs.cpu().numpy()
    got = split(out.cpu().numpy(), offs_h)
    want = encode_ref(x, B, cums, params)
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"block {b} of {len(want)} differs from the reference model"
    back, sizes, st, dsum = coder.decode(out[: int(offs_h[-1])], offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and not st.cpu().numpy().any()
    nb = len(want)
    lens = np.clip(len(x) - np.arange(nb) * B, 0, B)
    assert sizes.cpu().numpy().tolist() == lens.tolist()
    back = back.cpu().numpy()
    assert b"".join(back[b * B: b * B + int(lens[b])].tobytes() for b in range(nb)) == x.tobytes()
    return got


@pytest.mark.parametrize("B", [64, 257, 4096])
def test_lengths_around_a_block(rx, B):
    text = alice16k()
    cums = tables_ref(pair_counts(text, B))
    for n in (0, 1, B - 1, B, B + 1):
        check_streams(rx, text[:n], B, cums)


@pytest.mark.parametrize("params", [(8, 30, 32), (8, 22, 24)])
@pytest.mark.parametrize("B", [257, 4096])
def test_text_streams(rx, B, params):
    text = alice16k()
    check_streams(rx, text, B, tables_ref(pair_counts(text, B)), params)


@pytest.mark.parametrize("B,nblocks", [(64, 65), (257, 65), (4096, 65), (64, 64 * 8 + 1), (64, 64 * 16 + 1)])
def test_wave_and_workgroup_boundaries(rx, B, nblocks):
    """65 blocks: a second, nearly empty wave; 64 * 8 + 1 and 64 * 16 + 1 blocks: a third and a fifth workgroup's first lane.
    Every one of these shapes runs W = 4 waves per workgroup in both coders (a workgroup per CU comes before a deeper one;
    tests/test_context_static_instances_gpu.py has the shapes of 8 and 16 waves); the last block is short"""
    x = np.resize(alice16k() if B > 64 else random64k(), nblocks * B - 3)
    assert enc_name(P, len(x), B) == ENC[(True, 4)] and dec_name(P, nblocks) == DEC[4]
    check_streams(rx, x, B, tables_ref(pair_counts(x, B)))


@pytest.mark.parametrize("params", [(8, 30, 32), (8, 22, 24)])
def test_constant_and_random_inputs(rx, params):
    for x, B in ((np.zeros(16384, dtype=np.uint8), 4096), (np.full(16384, 0xFF, dtype=np.uint8), 4096), (random64k()[:16384], 4096)):
        check_streams(rx, x, B, tables_ref(pair_counts(x, B)), params)
    cums = tables_ref(pair_counts(random64k(), 65536))
    assert pair_counts(random64k(), 65536).any(axis=1).all()  # all 256 contexts occur
    check_streams(rx, random64k()[:20000], 257, cums, params)


def test_65536_random_bytes(rx):
    """all 256 contexts occur, and none of their tables is the substitute"""
    x = random64k()
    counts = pair_counts(x, 4096)
    assert counts.any(axis=1).all()
    check_streams(rx, x, 4096, tables_ref(counts))


def test_more_wave_slots_than_the_grid_holds(rx):
    """The coders are persistent: one workgroup per CU, at most 8 (encode) and 16 (decode) waves of 64 blocks each, and a
    wave that is done takes the slot a whole grid further on.  Blocks of 16 bytes put 64 * 16 * CUs + 1 blocks, what reaches
    that second round in both coders, into a few megabytes; the streams are held to a round trip and, for the first and
    the last blocks, to the reference model."""
    import torch
    B = 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblocks = 64 * 16 * cus + 1
    x = np.resize(corpus("canterbury/alice29.txt"), nblocks * B - 5)
    assert enc_name(P, len(x), B) == ENC[(True, 8)] and dec_name(P, nblocks) == DEC[16]
    cums = tables_ref(pair_counts(x, B))
    coder = rx.DeviceContextStaticCoder(P, d_tables(cums), TOTAL, B, len(x))
    d_in = dev(x)
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    offs_h = offs.cpu().numpy()
    out_h = out[: int(offs_h[-1])].cpu().numpy()
    assert split(out_h, offs_h[:41]) == encode_ref(x[: 40 * B], B, cums)
    assert split(out_h, offs_h[-41:]) == encode_ref(x[(nblocks - 40) * B:], B, cums)
    back, sizes, st, dsum = coder.decode(out[: int(offs_h[-1])], offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0]
    assert sizes[:-1].eq(B).all() and int(sizes[-1]) == B - 5
    assert torch.equal(back[: len(x)], d_in)


def test_two_symbol_alternation_under_total_4096(rx):
    x = np.tile(np.array([0x00, 0xFF], dtype=np.uint8), 8192)
    got = check_streams(rx, x, 4096, tables_ref(pair_counts(x, 4096), 4096))
    assert max(map(len, got)) < 80  # every symbol but the first costs about 0.09 bits (3840 / 4096)


@pytest.mark.parametrize("name,params", [("pending_80_8_30_32.bin", (8, 30, 32)), ("pending_80_8_22_24.bin", (8, 22, 24)),
                                         ("pending_7f_8_22_24.bin", (8, 22, 24))])
def test_long_carry_runs(rx, name, params):
    x = np.fromfile(os.path.join(ROOT, "tests", "golden", "adversarial", name), dtype=np.uint8)
    x = np.resize(x, 64 * 70)
    check_streams(rx, x, 64 * 35, tables_ref(pair_counts(x, 64 * 35)), params)
    # under tables in which 0x7F / 0x80 own almost nothing: long renormalisation shifts
    check_streams(rx, x, 1024, tables_ref(pair_counts(np.zeros(100000, dtype=np.uint8), 1 << 20)), params)


@pytest.mark.parametrize("params", [(8, 30, 32), (8, 22, 24)])
def test_tables_built_from_other_data(rx, params):
    """text tables code random bytes: most of the contexts that occur own the substitute table"""
    cums = tables_ref(pair_counts(alice16k(), 4096))
    x = random64k()[:8192 + 5]
    assert (~pair_counts(alice16k(), 4096).any(axis=1))[x].any()
    check_streams(rx, x, 4096, cums, params)
    check_streams(rx, x[:3000], 257, cums, params)


# ---- refusals and damage ---------------------------------------------------------------------------------------------------
def guarded(n, offset=0):
    import torch
    t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    return t, t[GUARD + offset: GUARD + offset + n]


def guards_intact(t, n, offset=0):
    h = t.cpu().numpy()
    return bool((h[: GUARD + offset] == FILL).all() and (h[GUARD + offset + n:] == FILL).all())


def ref_decode(stream, cums, cap, params=P):
    """the reference codec on one stream with room for cap bytes: (status, the bytes written before it was decided)"""
    codec = ref.Codec(ContextStaticModel(ref.Parameters(*params), cums))
    out = ref.BitWriter(cap)
    try:
        codec.decompress_stream(ref.BitReader(stream), out)
        return 0, bytes(out.out)
    except ref.Eof:
        return 1, bytes(out.out)
    except ref.IoError:
        return 4, bytes(out.out)


class Raw:
    """the _dev calls on caller-owned, guarded output buffers"""

    def __init__(self, lib, params, cums, total, B, n):
        import torch
        self.torch, self.lib, self.L = torch, lib, lib.lib()
        self.cp = lib.Params(*params)
        self.d_cum, self.total, self.B = d_tables(cums), total, B
        self.nb = self.L.redux_block_count(n, B)
        self.ws_bytes = max(self.L.redux_context_static_encode_workspace_bytes(C.byref(self.cp), n, B), 1 << 18)
        self.ws = torch.zeros(self.ws_bytes + 256, dtype=torch.uint8, device="cuda:0")
        self.ws_ptr = (self.ws.data_ptr() + 255) // 256 * 256
        self.cap = self.L.redux_context_static_encode_bound(C.byref(self.cp), n, B)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def encode(self, d_in):
        torch = self.torch
        whole, out = guarded(self.cap)
        offs = torch.zeros(self.nb + 1, dtype=torch.int64, device="cuda:0")
        status = torch.full((self.nb,), -1, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        st = self.L.redux_context_static_encode_dev(
            C.byref(self.cp), C.c_void_p(self.d_cum.data_ptr()), self.total, C.c_void_p(d_in.data_ptr()), d_in.numel(), self.B,
            C.c_void_p(out.data_ptr()), self.cap, C.c_void_p(offs.data_ptr()), C.c_void_p(status.data_ptr()),
            C.c_void_p(summary.data_ptr()), C.c_void_p(self.ws_ptr), self.ws_bytes, self.stream())
        torch.cuda.synchronize()
        return st, whole, out, offs, status.cpu().numpy(), summary.cpu().numpy()

    def decode(self, d_streams, d_offs, B=None, out_offset=0):
        torch = self.torch
        B = self.B if B is None else B
        nb = d_offs.numel() - 1
        whole, out = guarded(nb * B, out_offset)
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        status = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        st = self.L.redux_context_static_decode_dev(
            C.byref(self.cp), C.c_void_p(self.d_cum.data_ptr()), self.total, C.c_void_p(d_streams.data_ptr()),
            C.c_void_p(d_offs.data_ptr()), nb, B, C.c_void_p(out.data_ptr()), nb * B, C.c_void_p(sizes.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()), C.c_void_p(self.ws_ptr), self.ws_bytes, self.stream())
        torch.cuda.synchronize()
        assert guards_intact(whole, nb * B, out_offset), "the decoder wrote outside its output"
        return st, out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy(), summary.cpu().numpy()


def test_a_bad_table_on_the_device_refuses_every_block(lib):
    x = np.resize(alice16k(), 257 * 70)
    cums = tables_ref(pair_counts(x, 257))
    good = Raw(lib, P, cums, TOTAL, 257, len(x))
    st, _, out, offs, status, _ = good.encode(dev(x))
    assert st == lib.OK and not status.any()
    streams, d_offs = out[: int(offs[-1])].clone(), offs.clone()
    bad = cums.copy()
    bad[0x65, 100] = bad[0x65, 99]  # one row that does not increase, in a table no host code has checked
    r = Raw(lib, P, bad, TOTAL, 257, len(x))
    st, whole, out, offs, status, summary = r.encode(dev(x))
    assert st == lib.OK and (status == lib.INVALID_INPUT).all() and summary.tolist() == [lib.INVALID_INPUT, r.nb]
    assert guards_intact(whole, r.cap) and not offs.cpu().numpy().any()  # no stream, and nothing outside the output
    st, back, sizes, status, summary = r.decode(streams, d_offs)
    assert st == lib.OK and (status == lib.INVALID_INPUT).all() and not sizes.any() and (back == FILL).all()
    other = Raw(lib, P, cums, 4096, 257, len(x))  # good tables, another total than the launch's
    assert (other.encode(dev(x))[4] == lib.INVALID_INPUT).all()
    assert (other.decode(streams, d_offs)[3] == lib.INVALID_INPUT).all()


def test_total_above_2_16_is_unsupported(lib, rx):
    x = alice16k()
    r = Raw(lib, P, tables_ref(pair_counts(x, 4096)), 65537, 4096, len(x))
    st, whole, out, _, status, _ = r.encode(dev(x))
    assert st == lib.UNSUPPORTED and (status == -1).all() and (out.cpu().numpy() == FILL).all()
    assert r.decode(out[:8], dev(np.array([0, 8], dtype=np.int64)))[0] == lib.UNSUPPORTED
    import torch
    counts = torch.zeros(65536, dtype=torch.int64, device="cuda:0")
    assert lib.lib().redux_context_static_tables_dev(C.byref(r.cp), C.c_void_p(counts.data_ptr()), 65537, C.c_void_p(r.d_cum.data_ptr()),
                                                     None) == lib.UNSUPPORTED
    with pytest.raises(rx.Unsupported):
        rx.context_static_tables(x, 4096, P, 65537)


def test_damaged_streams_and_short_capacity(lib):
    B = 257
    x = np.resize(alice16k(), B * 66 + 100)
    cums = tables_ref(pair_counts(x, B))
    r = Raw(lib, P, cums, TOTAL, B, len(x))
    st, _, out, offs, status, _ = r.encode(dev(x))
    assert st == lib.OK and not status.any()
    offs_h = offs.cpu().numpy()
    streams = out[: int(offs_h[-1])].cpu().numpy()
    lens = np.clip(len(x) - np.arange(r.nb) * B, 0, B)
    # intact, at an output address that is no multiple of 4
    st, back, sizes, status, _ = r.decode(dev(streams), offs, out_offset=3)
    assert st == lib.OK and not status.any() and sizes.tolist() == lens.tolist()
    # truncated: every stream loses its last three bytes; status, size and bytes are the reference codec's
    cut = np.concatenate([streams[int(offs_h[b]): int(offs_h[b + 1]) - 3] for b in range(r.nb)])
    coffs = np.concatenate([[0], np.cumsum(np.diff(offs_h) - 3)]).astype(np.int64)
    st, back, sizes, status, summary = r.decode(dev(cut), dev(coffs))
    assert st == lib.OK
    for b in range(r.nb):
        want_st, want = ref_decode(cut[int(coffs[b]): int(coffs[b + 1])].tobytes(), cums, B)
        assert status[b] == want_st and sizes[b] == len(want) and back[b * B: b * B + len(want)].tobytes() == want, b
    assert (status == lib.EOF).sum() > r.nb // 2 and summary[1] == (status != 0).sum()
    # flipped bytes: a status or wrong bytes, never a write outside the block's range (r.decode checks the guards, and a
    # block's neighbours must still decode to their own bytes)
    rng = np.random.default_rng(5)
    hurt = streams.copy()
    victims = np.arange(0, r.nb, 2)
    for b in victims:
        at = int(offs_h[b]) + int(rng.integers(0, max(1, int(offs_h[b + 1] - offs_h[b]) - 4)))
        hurt[at] ^= 0xFF
    st, back, sizes, status, _ = r.decode(dev(hurt), offs)
    assert st == lib.OK and (sizes <= B).all()
    for b in range(r.nb):
        blk = x[b * B: b * B + int(lens[b])]
        same = status[b] == 0 and sizes[b] == lens[b] and back[b * B: b * B + int(lens[b])].tobytes() == blk.tobytes()
        assert same == (b not in victims), b
    # capacity one short: the symbol that does not fit is decoded, then OUTPUT_TOO_SMALL; a stream that ends before that
    # symbol's bits reports Eof instead, in the reference codec's order
    st, back, sizes, status, _ = r.decode(dev(streams), offs, B=B - 1)
    full = lens == B
    assert st == lib.OK and (status[full] == lib.OUTPUT_TOO_SMALL).all() and (sizes[full] == B - 1).all() and not status[~full].any()
    for b in list(np.flatnonzero(full)[:5]) + [r.nb - 1]:
        want_st, want = ref_decode(streams[int(offs_h[b]): int(offs_h[b + 1])].tobytes(), cums, B - 1)
        assert status[b] == want_st and back[b * (B - 1): b * (B - 1) + int(sizes[b])].tobytes() == want
    # a stream cut inside the symbol that would not fit, with room for one byte less than it holds: Eof, not OUTPUT_TOO_SMALL
    n3 = 3
    short = np.concatenate([streams[int(offs_h[b]): int(offs_h[b]) + n3] for b in range(r.nb)])
    st, _, sizes, status, _ = r.decode(dev(short), dev((np.arange(r.nb + 1) * n3).astype(np.int64)), B=1)
    assert st == lib.OK
    for b in range(0, r.nb, 13):
        assert status[b] == ref_decode(short[b * n3: (b + 1) * n3].tobytes(), cums, 1)[0] == lib.EOF


# ---- host-pointer calls -----------------------------------------------------------------------------------------------------
def test_host_calls_equal_the_device_calls(rx, lib):
    B = 1024
    x = np.resize(corpus("canterbury/alice29.txt"), B * 200 + 77)
    m = rx.ContextStaticModel.from_data(x, B)
    assert np.array_equal(m.cums, tables_ref(pair_counts(x, B)))
    import torch
    coder = rx.DeviceContextStaticCoder(P, d_tables(m.cums), m.total(), B, len(x))
    out, offs, _, summary = coder.encode(dev(x))
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    want_offs = offs.cpu().numpy().astype(np.uint64)
    want = out[: int(want_offs[-1])].cpu().numpy()
    assert split(want, want_offs)[:3] == encode_ref(x[: 3 * B], B, m.cums)
    crcs = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(len(want_offs) - 1)], dtype=np.uint32)
    assert np.array_equal(rx.crc32_blocks(x, B), crcs)
    try:
        for chunk in ((0, 0), (1, 1)):  # the default plan (one chunk), then 64 KiB chunks
            rx.host_set_chunk_bytes(*chunk)
            for devices in ([], [0, 0]):
                rx.host_set_devices(devices)
                crc = np.zeros(len(crcs), dtype=np.uint32)
                got, goffs, st = rx.compress_blocks(x, B, m, block_crc=crc)
                assert np.array_equal(got, want) and np.array_equal(goffs, want_offs) and not st.any(), (chunk, devices)
                assert np.array_equal(crc, crcs)
                crc[:] = 0
                back, sizes, st = rx.decompress_blocks(got, goffs, B, m, block_crc=crc)
                assert not st.any() and np.array_equal(crc, crcs), (chunk, devices)
                assert b"".join(back[b * B: b * B + int(sizes[b])].tobytes() for b in range(len(sizes))) == x.tobytes()
        assert rx.host_chunk_plan(len(crcs), B)[1] > 1
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)
    assert rx.compress_blocks(x, B, m)[0].tobytes() == want.tobytes() and rx.compress_blocks(b"", B, m)[1].tolist()[0] == 0


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["large/bible.txt", "large/world192.txt"])
def test_container_round_trip_and_size(rx, name):
    from redux_amd import container
    x = corpus(name)
    B = 65536
    buf = container.compress_bytes(x.tobytes(), B, P, model="context-static")
    assert buf[4] == 7 and container.decompress_bytes(buf) == x.tobytes()
    adaptive = container.compress_bytes(x.tobytes(), B, P)
    cums = container.context_static_tables(buf)
    assert np.array_equal(cums, tables_ref(pair_counts(x, B)))
    nb = -(-len(x) // B)
    ideal = ideal_bits(x, B, cums) / 8 + table_section_bytes(cums) + 4 * nb + 32
    print(f"{name}: context-static {len(buf)} ({len(buf) / len(x):.4f}), adaptive {len(adaptive)} ({len(adaptive) / len(x):.4f}), "
          f"ratio {len(buf) / len(adaptive):.4f}; ideal + sections {ideal:.0f}, container / ideal {len(buf) / ideal:.5f}")
    assert len(buf) <= 0.85 * len(adaptive)
    assert len(buf) <= 1.01 * ideal


def test_cli_round_trip_with_checksums(tmp_path):
    src = os.path.join(ROOT, "tests", "golden", "corpora", "calgary", "book1")
    packed, back = tmp_path / "book1.rdx", tmp_path / "book1.out"
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = lambda *a: subprocess.run([sys.executable, "-m", "redux_amd.cli", *a], cwd=ROOT, env=env, capture_output=True, timeout=300)
    r = run("-c", "-i", src, "-o", str(packed), "--block-size", "65536", "--model", "context-static", "--checksum")
    assert r.returncode == 0, r.stderr
    assert packed.read_bytes()[4] == 0x17
    r = run("-d", "-i", str(packed), "-o", str(back))
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == open(src, "rb").read()
    assert run("-c", "-i", src, "-o", str(packed), "--block-size", "65536", "--model", "context-static", "--stored").returncode == 1
