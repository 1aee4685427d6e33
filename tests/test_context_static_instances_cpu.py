"""Every context-static coder instance and the inputs that force the chunk redo (tests/test_context_static_instances_gpu.py):
the CPU side.

redux_context_static_encode_dev / redux_context_static_decode_dev choose among four encoder and three decoder instances by
the wave slots (64 blocks each) a launch has per CU: one workgroup per CU holds the 128 KiB image, so a launch is first
spread over the CUs and only then deepened, W = 4 waves per workgroup up to 4 slots per CU, 8 up to 8 (the encoder's
largest), 16 beyond (decoder only).  Here, without a GPU (the library then answers for 256 CUs):
  * ROWS: launch shapes as functions of the CU count, one per instance and reason, the thresholds from both sides; each maps
    to exactly its instance through redux_context_static_{encode,decode}_kernel_name, which share pick_context_encode_kernel /
    pick_context_decode_kernel with the launch code; the GPU file evaluates the same table with the device's CU count;
  * the table reaches all seven instances (a written-out list), and what the `_dev` calls refuse has no name;
  * REDO: per triple two blocks on which static_chunk (redux_static.hpp) must replay a 16-symbol chunk, certified with the
    Python restatement: a symbol inside the chunked region appends more than 32 bits, in a chunk whose last byte differs
    from the byte in front of the chunk (the context the replay restores is not the one the first pass ended with);
  * the closed form of the pair counts of the period-4 buffer the histogram's GPU test uses, against pair_counts."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import redux_ref as ref
from test_context_static_cpu import TOTAL, ContextStaticModel, corpus, pair_counts, tables_ref
from test_semistatic_cpu import rule_ref

P32, P24 = (8, 30, 32), (8, 22, 24)
TRIPLES = (P32, P24)
ENC = {(True, 4): "k_encode_context_static<true, 4> (code_bits 32, 4 waves per group)",
       (False, 4): "k_encode_context_static<false, 4> (code_bits < 32, 4 waves per group)",
       (True, 8): "k_encode_context_static<true, 8> (code_bits 32, 8 waves per group)",
       (False, 8): "k_encode_context_static<false, 8> (code_bits < 32, 8 waves per group)"}
DEC = {4: "k_decode_context_static<4> (4 waves per group)", 8: "k_decode_context_static<8> (8 waves per group)",
       16: "k_decode_context_static<16> (16 waves per group)"}
# the seven instances, written out: the coverage test compares what ROWS reaches with THIS list
ALL_INSTANCES = ["k_encode_context_static<true, 4> (code_bits 32, 4 waves per group)",
                 "k_encode_context_static<false, 4> (code_bits < 32, 4 waves per group)",
                 "k_encode_context_static<true, 8> (code_bits 32, 8 waves per group)",
                 "k_encode_context_static<false, 8> (code_bits < 32, 8 waves per group)",
                 "k_decode_context_static<4> (4 waves per group)",
                 "k_decode_context_static<8> (8 waves per group)",
                 "k_decode_context_static<16> (16 waves per group)"]
CUS_WITHOUT_A_DEVICE = 256


def library_cus():
    """the CU count the name calls answer for: HIP's current device, 256 where there is none"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else CUS_WITHOUT_A_DEVICE


# reason -> (wave slots of the launch as a function of the CU count, encoder W, decoder W).  A launch of s slots has
# 64 (s - 1) + 1 blocks: its last wave slot holds a single block.
SLOTS = {
    "one_slot": (lambda cus: 1, 4, 4),
    "one_slot_per_cu": (lambda cus: cus, 4, 4),
    "last_of_4_waves": (lambda cus: 4 * cus, 4, 4),                 # the last W = 4 shape of both coders
    "first_of_8_waves": (lambda cus: 4 * cus + 1, 8, 8),            # the threshold's other side: W = 8 in both
    "last_of_8_decoder_waves": (lambda cus: 8 * cus, 8, 8),
    "first_of_16_decoder_waves": (lambda cus: 8 * cus + 1, 8, 16),  # the encoder's largest is 8: its grid wraps once
    "second_round_of_16": (lambda cus: 16 * cus + 1, 8, 16),        # (test_more_wave_slots_than_the_grid_holds)
}
# id -> (params, reason, slots(cus), encoder name, decoder name)
ROWS = {f"{why}_{'_'.join(map(str, p))}": (p, why, fn, ENC[(p[2] == 32, we)], DEC[wd])
        for why, (fn, we, wd) in SLOTS.items() for p in TRIPLES}


def _lib():
    from redux_amd import _lib as L
    return L


def blocks_of(slots):
    return 64 * (slots - 1) + 1


def enc_name(params, in_len, block_size, total=TOTAL):
    L = _lib()
    return L.lib().redux_context_static_encode_kernel_name(C.byref(L.Params(*params)), total, in_len, block_size).decode()


def dec_name(params, nblocks, total=TOTAL):
    L = _lib()
    return L.lib().redux_context_static_decode_kernel_name(C.byref(L.Params(*params)), total, nblocks).decode()


def row_names(key, cus, block_size=48):
    """(encoder, decoder) the library names for the row's launch on a device of `cus` CUs; the last block is short"""
    params, _, fn, _, _ = ROWS[key]
    nb = blocks_of(fn(cus))
    return enc_name(params, nb * block_size - 5, block_size), dec_name(params, nb)


# ---- 1. the instance table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(ROWS))
def test_every_row_maps_to_its_instances(key):
    _, _, fn, enc, dec = ROWS[key]
    assert row_names(key, library_cus()) == (enc, dec)
    # the choice is by wave slots: a full last slot (63 blocks more) and other block sizes change nothing
    params = ROWS[key][0]
    nb = 64 * fn(library_cus())
    for bs in (16, 4096):
        assert enc_name(params, nb * bs, bs) == enc
    assert dec_name(params, nb) == dec


def test_the_table_reaches_all_seven_instances():
    got = {r[3] for r in ROWS.values()} | {r[4] for r in ROWS.values()}
    assert sorted(got) == sorted(ALL_INSTANCES) and len(ALL_INSTANCES) == 7
    assert sorted(ALL_INSTANCES) == sorted(list(ENC.values()) + list(DEC.values()))
    named = set()
    for key in ROWS:
        named |= set(row_names(key, library_cus()))
    assert sorted(named) == sorted(ALL_INSTANCES)
    # every reason under both code widths, the thresholds from both sides
    assert len(ROWS) == 2 * len(SLOTS) == 14
    for cus in (256, 304, 8):
        s = {why: fn(cus) for why, (fn, _, _) in SLOTS.items()}
        assert s["first_of_8_waves"] == s["last_of_4_waves"] + 1 == 4 * cus + 1
        assert s["first_of_16_decoder_waves"] == s["last_of_8_decoder_waves"] + 1 == 8 * cus + 1


def test_what_the_dev_calls_refuse_has_no_name():
    ok_e, ok_d = enc_name(P32, 100 * 4096, 4096), dec_name(P32, 100)
    assert ok_e == ENC[(True, 4)] and ok_d == DEC[4]
    assert enc_name(P32, 100 * 4096, 4096, total=65537) == "" and dec_name(P32, 100, total=65537) == ""   # UNSUPPORTED
    assert enc_name(P32, 100 * 4096, 0) == ""                                                              # block_size 0
    for any_triple in ((8, 24, 40), (13, 20, 32)):
        assert enc_name(any_triple, 100 * 4096, 4096) == "" and dec_name(any_triple, 100) == ""
    assert enc_name((8, 10, 32), 100 * 4096, 4096, total=4096) == ""     # a total above freq_max: INVALID_INPUT
    assert enc_name((8, 10, 32), 100 * 4096, 4096, total=1023) == ENC[(True, 4)]
    assert dec_name(P32, 0) == ""                                        # no blocks: the decode call launches nothing
    assert enc_name(P32, 0, 4096) == ENC[(True, 4)]                      # no bytes: one empty block is coded
    assert enc_name(P32, 1 << 40, 1 << 26) == ""                         # 64 blocks of a wave beyond a 32-bit lane offset
    L = _lib()
    assert L.lib().redux_context_static_encode_kernel_name(None, TOTAL, 4096, 4096) == b""
    assert L.lib().redux_context_static_decode_kernel_name(None, TOTAL, 1) == b""


def test_thresholds_in_blocks():
    """at 256 CUs 65,536 blocks are the last W = 4 launch of both coders, 131,072 the decoder's last W = 8 one"""
    n = library_cus()
    for p in TRIPLES:
        cb = p[2] == 32
        assert enc_name(p, 256 * n * 64, 64) == ENC[(cb, 4)] and enc_name(p, (256 * n + 1) * 64, 64) == ENC[(cb, 8)]
        assert enc_name(p, (1 << 24) * 64, 64) == ENC[(cb, 8)]
        assert dec_name(p, 256 * n) == DEC[4] and dec_name(p, 256 * n + 1) == DEC[8]
        assert dec_name(p, 512 * n) == DEC[8] and dec_name(p, 512 * n + 1) == DEC[16] and dec_name(p, 1 << 24) == DEC[16]
    # the older GPU test's shapes (tests/test_context_static_gpu.py): all W = 4 but the one deep launch
    for nb in (65, 64 * 8 + 1, 64 * 16 + 1):
        assert enc_name(P32, nb * 64 - 3, 64) == ENC[(True, 4)] and dec_name(P32, nb) == DEC[4]
    deep = 64 * 16 * n + 1
    assert enc_name(P32, deep * 16 - 5, 16) == ENC[(True, 8)] and dec_name(P32, deep) == DEC[16]


# ---- 2. inputs that force the redo of a chunk -------------------------------------------------------------------------
# static_chunk codes 16 symbols without looking and replays them from the saved coder state AND the saved model when a
# lane's append (the symbol's k shared leading bits and, with k > 0, the pending run in front of them) exceeded 32 bits.
# Decoding 80 00 00 ... (or 7F FF FF ...) keeps the interval astride the half for as long as one likes: the pending run
# grows by every symbol and nothing is written, so the decoded symbols ALONE never append anything before the EOF symbol,
# which is not coded in a chunk.  A block is therefore REDO_PREFIX decoded symbols and then text: its first byte that is
# not the symbol the stream would have decoded next ends the run.  A byte above that symbol writes 1 and the run as zeros
# (the stream 80 00 00 ...), one below it 0 and the run as ones (7F FF FF ...).
REDO_PREFIX = 20     # decoded symbols: the run passes 32 bits about half way
REDO_LEN = 64        # bytes of a block: four chunks, the append in the second


@functools.lru_cache(maxsize=None)
def redo_text():
    return corpus("canterbury/alice29.txt")[:16384].copy()


@functools.lru_cache(maxsize=None)
def redo_tables():
    """tables built from text: u32[256][258] for the context model, u32[258] for the one-table model"""
    text = redo_text()
    return tables_ref(pair_counts(text, 4096)), rule_ref(np.bincount(text, minlength=256).astype(np.uint64), TOTAL).astype(np.uint32)


def make_model(kind, params):
    cums, cum = redo_tables()
    p = ref.Parameters(*params)
    return ContextStaticModel(p, cums) if kind == "context" else ref.StaticModel(p, cum)


def decode_prefix(head, kind, params, nsym):
    """the first nsym symbols the reference codec decodes from `head` 00 00 ... / FF FF ... under the model"""
    fill = b"\x00" if head == 0x80 else b"\xff"
    out = ref.BitWriter(nsym)
    try:
        ref.Codec(make_model(kind, params)).decompress_stream(ref.BitReader(bytes([head]) + fill * (8 * nsym + 16)), out)
    except ref.IoError:      # the capacity reached: what is wanted
        pass
    return bytes(out.out)


def coding_trace(block, kind, params):
    """per data symbol of the block, coded by the reference codec: (pending run after it, bits it appended)"""
    codec = ref.Codec(make_model(kind, params))
    out = ref.BitWriter()
    rows = []
    for s in block:
        before = out.count * 8 + out.bits
        codec.compress_symbol(s, out)
        rows.append((codec.pending, out.count * 8 + out.bits - before))
    return rows


@functools.lru_cache(maxsize=None)
def redo_block(kind, params, head):
    """REDO_LEN bytes: REDO_PREFIX symbols decoded from head 00 .. / FF .., a byte on the other side of the symbol that
    would have come next (the most frequent one under the model at that point), then text"""
    pre = decode_prefix(head, kind, params, REDO_PREFIX + 1)
    assert len(pre) == REDO_PREFIX + 1       # (no EOF symbol among them)
    nxt, pre = pre[-1], pre[:-1]
    cums, cum = redo_tables()
    freq = np.diff((cums[pre[-1]] if kind == "context" else cum).astype(np.int64))[:256]
    side = np.arange(256) > nxt if head == 0x80 else np.arange(256) < nxt
    assert side.any()
    ender = int(np.argmax(np.where(side, freq, 0)))
    text = redo_text()[1000: 1000 + REDO_LEN - REDO_PREFIX - 1]
    return np.frombuffer(pre + bytes([ender]) + text.tobytes(), dtype=np.uint8).copy()


def certify(block, kind, params):
    """-> (position of the first symbol that appends more than 32 bits, the bits it appends, the longest pending run
    in front of it), asserting that the symbol lies in the chunked region of a block at least 32 bytes long, that its chunk
    holds two byte values or more and, under the context model, ends in another context than it began in"""
    n = len(block)
    assert n >= 32 and n % 16 == 0
    rows = coding_trace(block.tobytes(), kind, params)
    over = [i for i, (_, bits) in enumerate(rows) if bits > 32]
    assert over, max(bits for _, bits in rows)
    at = over[0]
    assert at < (n & ~15)                                           # static_encode_body's main_end for a wave of such blocks
    assert at > 0 and rows[at - 1][0] > 32 and rows[at][1] > rows[at - 1][0]   # the run in front of it is what is appended
    chunk = block[at & ~15: (at & ~15) + 16]
    assert len(set(chunk.tolist())) >= 2
    if kind == "context":                                           # (the one-table model has no state to restore)
        before = int(block[(at & ~15) - 1]) if at >= 16 else 0      # the context static_chunk saves, and restores
        assert int(chunk[15]) != before
    return at, rows[at][1], rows[at - 1][0]


REDO_CASES = [(kind, params, head) for kind in ("context", "static") for params in TRIPLES for head in (0x80, 0x7F)]


@pytest.mark.parametrize("kind,params,head", REDO_CASES)
def test_redo_blocks_append_more_than_32_bits_inside_a_chunk(kind, params, head):
    block = redo_block(kind, params, head)
    at, bits, run = certify(block, kind, params)
    print(kind, params, hex(head), "symbol", at, "appends", bits, "bits after a pending run of", run)
    assert at == REDO_PREFIX and 16 <= at < 32               # the second chunk: the first one is replayed by no lane
    # the run is written as the stream the prefix was decoded from
    stream = ref.compress(block.tobytes(), make_model(kind, params))[0]
    want = bytes([head]) + (b"\x00" if head == 0x80 else b"\xff") * 3
    assert stream[:4] == want
    assert ref.decompress(stream, make_model(kind, params))[0] == block.tobytes()


def test_the_decoded_symbols_alone_append_nothing():
    """why the blocks end in text: 200 symbols decoded from 80 00 00 ... append no bit at all when coded back (the run is
    written by the EOF symbol, outside the chunks), under both models and triples"""
    for kind in ("context", "static"):
        for params in TRIPLES:
            rows = coding_trace(decode_prefix(0x80, kind, params, 200), kind, params)
            assert len(rows) == 200 and max(bits for _, bits in rows) == 0 and rows[-1][0] > 32


# ---- 3. the histogram's period-4 buffer -------------------------------------------------------------------------------
def period4(n, a, b):
    return np.resize(np.array([a, b, a, b ^ 1], dtype=np.uint8), n)


def period4_counts(n, a, b, B):
    """pair_counts(period4(n, a, b), B) in closed form, for B a multiple of 4 or at least n, and 0, a, b, b ^ 1 distinct"""
    assert (B % 4 == 0 or B >= n) and len({0, a, b, b ^ 1}) == 4 and n >= 4
    at = lambda r: (n - r + 3) // 4          # positions i < n with i % 4 == r
    starts = -(-n // B)                      # block starts: all at i % 4 == 0, their context is 0
    want = np.zeros((256, 256), dtype=np.uint64)
    want[0, a] = starts
    want[a, b] = at(1)
    want[b, a] = at(2)
    want[a, b ^ 1] = at(3)
    want[b ^ 1, a] = at(0) - starts
    return want


@pytest.mark.parametrize("n,B", [(4, 64), (5, 64), (6, 64), (7, 4), (1000, 64), (1001, 1 << 20), (4099, 4096), (64 * 50 + 30, 64)])
def test_period4_closed_form(n, B):
    a, b = 0x41, 0x6A
    want = period4_counts(n, a, b, B)
    assert np.array_equal(want, pair_counts(period4(n, a, b), B)) and want.sum() == n
    assert (a * 256 + b) >> 1 == (a * 256 + (b ^ 1)) >> 1       # the two bins share a dword of packed counters
