"""Every kernel instance of the static-table model against the CPU oracle (oracle/, OX_MODEL_STATIC).

redux_static_encode_blocks_dev / redux_static_decode_blocks_dev choose among 4 encoder and 9 decoder instances by the
table total, code_bits and the grid (at most one wave per SIMD, "solo", or more); inside each kernel the encoder picks
16-byte or byte loads and the decoders 16-byte, 4-byte or byte stores.  Each test first asserts, through
redux_static_*_kernel_name, the instance it targets -- a change of the dispatch fails here instead of quietly dropping
coverage -- and then holds the instance to the bar of every other kernel here: each block's stream is byte-identical to
the oracle's, decoding gives back the input, and for damaged streams each block's status, size and bytes equal the
oracle's.  Decoded output lands inside guard bands that must stay untouched."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_oracle_codec import static_tables
from test_static_cpu import worst_case_table

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5

E_FIX, E_CB32_SOLO, E_CB32, E_NARROW = ("k_encode_static<true, false>", "k_encode_static<false, true, true>",
                                        "k_encode_static<false, true>", "k_encode_static<false, false>")
D_FIX = "k_decode_static<true>"
D_LUT = {(True, True): "k_decode_static_lut<true, 4>", (False, True): "k_decode_static_lut<false, 4>",
         (True, False): "k_decode_static_lut<true, 8>", (False, False): "k_decode_static_lut<false, 8>"}
D_LOCK = {(True, True): "k_decode_static_lock<true, true>", (False, True): "k_decode_static_lock<false, true>",
          (True, False): "k_decode_static_lock<true, false>", (False, False): "k_decode_static_lock<false, false>"}


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def shaped(total, seed):
    """A table of exactly `total` with an uneven shape: 257 frequencies >= 1, the remainder on symbol 32."""
    base = [1 + ((i * i * 31 + i * seed) % 251) for i in range(257)]
    s = sum(base)
    f = [1 + (b - 1) * (total - 257) // (s - 257) for b in base]
    f[32] += total - sum(f)
    cum = [0]
    for x in f:
        cum.append(cum[-1] + x)
    assert cum[257] == total and min(f) >= 1
    return cum


@functools.lru_cache(None)
def tables():
    t = dict(static_tables())
    t["lock65537"] = ((8, 30, 32), shaped(65537, 3))          # the smallest table the LUT decoder does not take
    t["max17"] = ((8, 17, 20), shaped((1 << 17) - 1, 5))      # freq_max at 17 bits: the largest total without fix-up
    t["fix18"] = ((8, 18, 20), shaped(1 << 17, 7))            # the smallest fix-up table, code_bits < 32
    t["lock24"] = ((8, 22, 24), shaped(100003, 9))
    t["fix24"] = ((8, 22, 24), shaped(3000001, 11))
    t["worst30"] = ((8, 30, 32), worst_case_table((8, 30, 32)))  # ~30 bits per byte: ~60 bytes per 16-byte chunk
    t["worst22"] = ((8, 22, 24), worst_case_table((8, 22, 24)))
    return t


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def big_nblocks():
    """More than one wave per SIMD (4 x CUs waves of 64 blocks), a partial last wave, and a last 8-wave group of the
    LUT decoder with dead waves."""
    waves = 4 * cus() + 6
    assert waves % 8 != 0 and waves > 4 * cus()
    return 64 * (waves - 1) + 17


SOLO_NBLOCKS = 64 * 9 + 23   # 10 waves: partial last wave, partial last 4-wave LUT group


def enc_name(rx, params, cum, n, bs):
    from redux_amd import _lib
    p = _lib.Params(*params)
    return _lib.lib().redux_static_encode_kernel_name(C.byref(p), (C.c_uint32 * 258)(*cum), n, bs).decode()


def dec_name(rx, params, cum, nblocks):
    from redux_amd import _lib
    p = _lib.Params(*params)
    return _lib.lib().redux_static_decode_kernel_name(C.byref(p), (C.c_uint32 * 258)(*cum), nblocks).decode()


def expected_decoder(params, cum, solo):
    total, cb32 = cum[257], params[2] == 32
    if total >= 1 << 17:
        return D_FIX
    return (D_LUT if total <= 65536 else D_LOCK)[(cb32, solo)]


def expected_encoder(params, cum, solo):
    if cum[257] >= 1 << 17:
        return E_FIX
    if params[2] == 32:
        return E_CB32_SOLO if solo else E_CB32
    return E_NARROW


# ---- the oracle, one block per call --------------------------------------------------------------------------------
def _ox_fn(name):
    f = getattr(ox.lib(), name)
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    f.restype = C.c_int
    return f


def oracle_encode_blocks(host, bs, cum, params):
    """ox_compress_static of every block of `host`: (dense streams, offsets)."""
    f = _ox_fn("ox_compress_static")
    tab = np.ascontiguousarray(np.asarray(cum, dtype=np.uint64))
    cap = bs * 5 + 1024
    out = np.empty(cap, dtype=np.uint8)
    bi, bo = C.c_uint64(), C.c_uint64()
    n = host.size
    nb = max(1, (n + bs - 1) // bs)
    parts, offs = [], np.zeros(nb + 1, dtype=np.int64)
    for b in range(nb):
        ln = min(bs, n - b * bs)
        st = f(host.ctypes.data + b * bs, ln, out.ctypes.data, cap, params[0], params[1], params[2], tab.ctypes.data,
               C.byref(bi), C.byref(bo))
        assert st == 0
        parts.append(out[: bo.value].tobytes())
        offs[b + 1] = offs[b] + bo.value
    return b"".join(parts), offs


def oracle_decode_raw(stream, cap, cum, params):
    """ox_decompress_static without raising: (status, bytes written before the status was decided), the oracle's
    IoError (its writer fails where the block capacity ends) mapped to REDUX_OUTPUT_TOO_SMALL."""
    f = _ox_fn("ox_decompress_static")
    a = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    tab = np.ascontiguousarray(np.asarray(cum, dtype=np.uint64))
    bi, bo = C.c_uint64(), C.c_uint64()
    st = f(a.ctypes.data, len(stream), out.ctypes.data, cap, params[0], params[1], params[2], tab.ctypes.data,
           C.byref(bi), C.byref(bo))
    return (4 if st == ox.IO_ERROR else st), out[: bo.value].tobytes()


# ---- device helpers ------------------------------------------------------------------------------------------------
def guarded(torch, n, offset):
    """n bytes at `offset` from a 256-byte boundary, FILL guard bands on both sides: (whole buffer, view)"""
    t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    assert t.data_ptr() % 256 == 0
    return t, t[GUARD + offset: GUARD + offset + n]


def guards_intact(t, n, offset):
    h = t.cpu().numpy()
    return bool((h[: GUARD + offset] == FILL).all() and (h[GUARD + offset + n:] == FILL).all())


def block_data(nb, bs, n, seed):
    """n bytes in blocks of bs: mostly uniform bytes, with blocks of the last data symbol (next to EOF in the table),
    of symbol 0 and of a four-letter alphabet."""
    rng = np.random.default_rng(seed)
    host = rng.integers(0, 256, n, dtype=np.uint8)
    for b in range(nb):
        lo, hi = b * bs, min(n, (b + 1) * bs)
        if b % 7 == 3:
            host[lo:hi] = 255
        elif b % 11 == 5:
            host[lo:hi] = 0
        elif b % 13 == 6:
            host[lo:hi] = rng.integers(0, 4, hi - lo, dtype=np.uint8)
    return host


def encode_and_check(rx, params, cum, host, bs, in_off):
    """Encode host from a device buffer at byte offset in_off; every block's stream must equal the oracle's.
    Returns (device streams, device offsets)."""
    import torch
    n = host.size
    src = torch.zeros(n + 512, dtype=torch.uint8, device="cuda:0")
    assert src.data_ptr() % 256 == 0
    d_in = src[in_off: in_off + n]
    d_in.copy_(torch.from_numpy(host).cuda())
    coder = rx.DeviceStaticCoder(params, cum, bs, max(n, 1))
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and not bool(status.any())
    want, want_offs = oracle_encode_blocks(host, bs, cum, params)
    got_offs = offs.cpu().numpy()
    got = out[: int(got_offs[-1])].cpu().numpy().tobytes()
    if not (np.array_equal(got_offs, want_offs) and got == want):
        for b in range(len(want_offs) - 1):
            g = got[int(got_offs[b]): int(got_offs[b + 1])]
            w = want[int(want_offs[b]): int(want_offs[b + 1])]
            assert g == w, f"block {b} of {len(want_offs) - 1}: stream differs from the oracle ({len(g)} vs {len(w)} bytes)"
    return out[: int(got_offs[-1])].clone(), offs.clone()


def decode_raw(rx, params, cum, d_streams, d_offs, nb, bs, out_off):
    """redux_static_decode_blocks_dev into a guarded buffer at out_off: (out bytes, sizes, status, summary), host."""
    import torch
    from redux_amd import _lib
    whole, d_out = guarded(torch, nb * bs, out_off)
    sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -1, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    p = _lib.Params(*params)
    st = _lib.lib().redux_static_decode_blocks_dev(
        C.byref(p), (C.c_uint32 * 258)(*cum), C.c_void_p(d_streams.data_ptr()), C.c_void_p(d_offs.data_ptr()), nb, bs,
        C.c_void_p(d_out.data_ptr()), nb * bs, C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()),
        C.c_void_p(summary.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert st == 0
    assert guards_intact(whole, nb * bs, out_off), "the decoder wrote outside its output"
    return d_out.cpu().numpy(), sizes.cpu().numpy(), status.cpu().numpy(), summary.cpu().numpy()


# ---- 1. every instance: streams equal the oracle's, decode inverts them ---------------------------------------------
MATRIX = [("flat", True), ("flat", False), ("skewed", True), ("full16", True), ("full16", False), ("narrow16", True),
          ("narrow16", False), ("lock65537", True), ("mid17", True), ("mid17", False), ("max17", True), ("max17", False),
          ("lock24", True), ("lock24", False), ("fix18", True), ("fix18", False), ("wide", True), ("fix24", True),
          ("worst30", True), ("worst30", False), ("worst22", True)]
# (block size, d_in offset, d_out offset, last block's length): 16-byte loads and stores with a last block too short
# for a chunk / byte loads, 4-byte stores / byte loads and stores
LAYOUTS = {"a16": (48, 0, 0, 17), "a4": (44, 4, 4, 39), "u1": (47, 1, 1, 42)}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("name,solo", MATRIX, ids=[f"{n}-{'solo' if s else 'large'}" for n, s in MATRIX])
def test_static_instance_matches_oracle(rx, name, solo, layout):
    params, cum = tables()[name]
    bs, in_off, out_off, tail = LAYOUTS[layout]
    nb = SOLO_NBLOCKS if solo else big_nblocks()
    n = (nb - 1) * bs + tail
    assert enc_name(rx, params, cum, n, bs).startswith(expected_encoder(params, cum, solo) + " ")
    assert dec_name(rx, params, cum, nb).startswith(expected_decoder(params, cum, solo) + " ")
    host = block_data(nb, bs, n, seed=zlib.crc32(f"{name}/{layout}".encode()))
    d_streams, d_offs = encode_and_check(rx, params, cum, host, bs, in_off)
    got, sizes, status, summary = decode_raw(rx, params, cum, d_streams, d_offs, nb, bs, out_off)
    assert summary.tolist() == [0, 0] and not status.any()
    want_sizes = np.full(nb, bs)
    want_sizes[-1] = tail
    assert np.array_equal(sizes, want_sizes)
    bad = np.nonzero(got[:n] != host)[0]
    assert bad.size == 0, f"first wrong byte at {bad[0]} (block {bad[0] // bs})"


# ---- 2. unaligned input and output, block sizes off every store width ------------------------------------------------
ALIGN_TABLES = ["flat", "narrow16", "mid17", "max17", "wide", "fix18", "worst30"]
# (block size, d_in offset, last block's length): ragged last blocks shorter and longer than 32 bytes
ALIGN_SHAPES = [(1001, 1, 20), (1001, 8, 100), (4095, 4, 100), (4095, 1, 20), (4096, 0, 20), (4096, 0, 100),
                (4096, 8, 100), (4096, 4, 33)]


@pytest.mark.parametrize("name", ALIGN_TABLES)
def test_static_unaligned_buffers_match_oracle(rx, name):
    """d_in at byte offsets 0, 1, 4 and 8 from a 256-byte boundary and block sizes that are not multiples of 16, 4 or 2
    (byte loads in the encoder); d_out at offsets 0, 1, 4 and 8 (the decoders' 16-byte, 4-byte and byte stores)."""
    params, cum = tables()[name]
    nb = 70
    for i, (bs, in_off, tail) in enumerate(ALIGN_SHAPES):
        n = (nb - 1) * bs + tail
        assert enc_name(rx, params, cum, n, bs).startswith(expected_encoder(params, cum, True) + " ")
        assert dec_name(rx, params, cum, nb).startswith(expected_decoder(params, cum, True) + " ")
        host = block_data(nb, bs, n, seed=i)
        d_streams, d_offs = encode_and_check(rx, params, cum, host, bs, in_off)
        for out_off in (0, 1, 4, 8):
            got, sizes, status, summary = decode_raw(rx, params, cum, d_streams, d_offs, nb, bs, out_off)
            assert summary.tolist() == [0, 0] and not status.any(), (bs, in_off, out_off)
            assert sizes[:-1].tolist() == [bs] * (nb - 1) and sizes[-1] == tail, (bs, in_off, out_off)
            bad = np.nonzero(got[:n] != host)[0]
            assert bad.size == 0, (bs, in_off, out_off, f"first wrong byte at {bad[0]} (block {bad[0] // bs})")


# ---- 3. damaged streams on every decoder instance --------------------------------------------------------------------
DAMAGE_BS = 48


@functools.lru_cache(None)
def damaged_streams(name):
    """[(stream, oracle status, oracle bytes)] for blocks of DAMAGE_BS: every truncation of one stream of three blocks'
    worth of symbols, the whole of it, garbage, empty streams, intact streams with trailing bytes or a flipped bit."""
    params, cum = tables()[name]
    bs = DAMAGE_BS
    rng = np.random.default_rng(sum(cum) & 0xFFFFFFFF)
    long_src = rng.integers(0, 256, 3 * bs, dtype=np.uint8).tobytes()
    long_stream, _ = ox.compress_static(long_src, cum, params)
    streams = [long_stream[:cut] for cut in range(len(long_stream) + 1)]
    streams.append(long_stream + rng.integers(0, 256, 5, dtype=np.uint8).tobytes())
    for n in list(range(0, 24)) + [int(x) for x in rng.integers(24, 400, 40)]:
        streams.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    streams += [b"\x00" * n for n in (1, 4, 5, 64)] + [b"\xff" * n for n in (1, 4, 7, 64)] + [b""] * 3
    for i in range(30):
        good, _ = ox.compress_static(rng.integers(0, 256, int(rng.integers(0, bs + 1)), dtype=np.uint8).tobytes(), cum, params)
        b = bytearray(good)
        if i % 2:
            b += rng.integers(0, 256, int(rng.integers(1, 9)), dtype=np.uint8).tobytes()   # trailing bytes: still Ok
        else:
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))              # one flipped bit
        streams.append(bytes(b))
    out = [(s,) + oracle_decode_raw(s, bs, cum, params) for s in streams]
    seen = {(st, len(w) == bs) for _, st, w in out}
    # the sweep reaches Eof with a full block written (the stream runs dry in the renormalisation of the symbol after
    # the last one that fits) and, further on, the capacity error (that symbol decodes, writing it fails)
    assert {(1, True), (4, True), (1, False), (0, False)} <= seen, seen
    return out


@functools.lru_cache(None)
def intact_blocks(name, nb):
    params, cum = tables()[name]
    host = block_data(nb, DAMAGE_BS, nb * DAMAGE_BS, seed=nb)
    dense, offs = oracle_encode_blocks(host, DAMAGE_BS, cum, params)
    return host, [dense[int(offs[b]): int(offs[b + 1])] for b in range(nb)]


DAMAGE = ["flat", "narrow16", "mid17", "max17", "wide", "fix18"]


@pytest.mark.parametrize("out_off", [0, 1, 4])
@pytest.mark.parametrize("solo", [True, False], ids=["solo", "large"])
@pytest.mark.parametrize("name", DAMAGE)
def test_static_decoder_on_damaged_streams_matches_oracle(rx, name, solo, out_off):
    """One launch per instance: intact blocks with damaged ones scattered among them (the first wave, the solo
    threshold, the last full wave and the ragged tail included).  Status, decoded size and decoded bytes of every block
    equal the oracle's; intact blocks decode to their input; nothing is written outside the output."""
    import torch
    params, cum = tables()[name]
    bs = DAMAGE_BS
    damaged = damaged_streams(name)
    nb = 64 * (2 * len(damaged) // 64) + 17 if solo else big_nblocks()
    assert dec_name(rx, params, cum, nb).startswith(expected_decoder(params, cum, solo) + " ")
    host, intact = intact_blocks(name, nb)
    thr = 4 * cus() * 64
    forced = [b for b in {0, 1, 62, 63, 64, thr - 1, thr, thr + 1, nb - 18, nb - 17, nb - 2, nb - 1} if b < nb]
    rng = np.random.default_rng(nb + out_off)
    rest = rng.permutation(np.setdiff1d(np.arange(nb), forced))[: len(damaged) - len(forced)]
    where = dict(zip([int(b) for b in forced] + [int(b) for b in rest], range(len(damaged))))
    assert len(where) == len(damaged)
    streams = [damaged[where[b]][0] if b in where else intact[b] for b in range(nb)]
    offs = np.zeros(nb + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in streams])
    d_streams = torch.from_numpy(np.frombuffer(b"".join(streams), dtype=np.uint8).copy()).cuda()
    d_offs = torch.from_numpy(offs).cuda()
    got, sizes, status, summary = decode_raw(rx, params, cum, d_streams, d_offs, nb, bs, out_off)

    want_status = np.zeros(nb, dtype=np.int32)
    want_sizes = np.full(nb, bs, dtype=np.int64)
    want = host.copy()
    for b, k in where.items():
        _, st, w = damaged[k]
        want_status[b], want_sizes[b] = st, len(w)
        want[b * bs: b * bs + len(w)] = np.frombuffer(w, dtype=np.uint8)
    wrong = np.nonzero((status != want_status) | (sizes != want_sizes))[0]
    assert wrong.size == 0, [(int(b), where.get(int(b)), int(status[b]), int(want_status[b]), int(sizes[b]),
                              int(want_sizes[b])) for b in wrong[:8]]
    defined = np.arange(bs)[None, :] < want_sizes[:, None]
    bad = np.nonzero(((got.reshape(nb, bs) != want.reshape(nb, bs)) & defined).any(axis=1))[0]
    assert bad.size == 0, [(int(b), where.get(int(b))) for b in bad[:8]]
    failing = want_status != 0
    assert summary[1] == failing.sum() and summary[0] in set(want_status[failing].tolist())
