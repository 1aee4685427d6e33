"""The static-table model without a GPU: which kernel instance each static call launches (the rules that do not depend
on the CU count) and the per-block cap of the encoder against the most expensive streams valid input can produce.
tests/test_static_gpu.py runs every instance on the device."""
import ctypes as C

import pytest

from oracle import cbind as ox
from redux_amd import _lib

FLAT = list(range(258))
HUGE_LEN = 1 << 36          # 48-byte blocks: ~2^30 blocks, ~2^24 waves -- more than 4 per SIMD of any device


def table(freq):
    """cum[258] of 257 frequencies (symbol 256 = EOF)."""
    cum = [0]
    for f in freq:
        cum.append(cum[-1] + f)
    return cum


def with_total(total, bulk=0):
    """A valid table with cum[257] == total: every symbol frequency 1, the rest on symbol `bulk`."""
    f = [1] * 257
    f[bulk] += total - 257
    return table(f)


def worst_case_table(params):
    """total = freq_max, all but 256 of it on symbol 0: every other symbol costs ~freq_bits bits."""
    return with_total((1 << params[1]) - 1)


def enc_name(params, cum, n, bs):
    p = _lib.Params(*params)
    return _lib.lib().redux_static_encode_kernel_name(C.byref(p), (C.c_uint32 * 258)(*cum), n, bs).decode()


def dec_name(params, cum, nblocks):
    p = _lib.Params(*params)
    return _lib.lib().redux_static_decode_kernel_name(C.byref(p), (C.c_uint32 * 258)(*cum), nblocks).decode()


def test_table_total_picks_the_decoder():
    P = (8, 30, 32)
    for nb in (1, 64):
        assert dec_name(P, with_total(65536), nb).startswith("k_decode_static_lut<true, 4>")
        assert dec_name(P, with_total(65537), nb).startswith("k_decode_static_lock<true, true>")
        assert dec_name(P, with_total((1 << 17) - 1), nb).startswith("k_decode_static_lock<true, true>")
        assert dec_name(P, with_total(1 << 17), nb).startswith("k_decode_static<true>")
    assert dec_name(P, FLAT, 1).startswith("k_decode_static_lut<true, 4>")
    assert dec_name(P, worst_case_table(P), 1).startswith("k_decode_static<true>")


def test_table_total_picks_the_encoder():
    P = (8, 30, 32)
    assert enc_name(P, with_total(65536), 4096, 4096).startswith("k_encode_static<false, true, true>")
    assert enc_name(P, with_total((1 << 17) - 1), 4096, 4096).startswith("k_encode_static<false, true, true>")
    assert enc_name(P, with_total(1 << 17), 4096, 4096).startswith("k_encode_static<true, false>")
    assert enc_name(P, worst_case_table(P), 0, 4096).startswith("k_encode_static<true, false>")


def test_code_bits_pick_different_instances():
    narrow = (8, 17, 20)
    lock = with_total((1 << 17) - 1)  # = freq_max at (8, 17, 20)
    assert enc_name(narrow, lock, 4096, 4096).startswith("k_encode_static<false, false>")
    assert dec_name(narrow, lock, 1).startswith("k_decode_static_lock<false, true>")
    assert dec_name(narrow, lock, HUGE_LEN // 48).startswith("k_decode_static_lock<false, false>")
    assert dec_name((8, 14, 16), FLAT, 1).startswith("k_decode_static_lut<false, 4>")
    assert dec_name((8, 14, 16), FLAT, HUGE_LEN // 48).startswith("k_decode_static_lut<false, 8>")
    assert dec_name((8, 18, 20), with_total(1 << 17), 1).startswith("k_decode_static<true>")
    assert enc_name((8, 18, 20), with_total(1 << 17), 4096, 4096).startswith("k_encode_static<true, false>")
    # code_bits 32 only: the encoder and the decoders have a second instance for grids above one wave per SIMD
    assert enc_name((8, 30, 32), FLAT, HUGE_LEN, 48).startswith("k_encode_static<false, true>")
    assert enc_name((8, 14, 16), FLAT, HUGE_LEN, 48).startswith("k_encode_static<false, false>")
    assert dec_name((8, 30, 32), FLAT, HUGE_LEN // 48).startswith("k_decode_static_lut<true, 8>")
    assert dec_name((8, 30, 32), with_total(65537), HUGE_LEN // 48).startswith("k_decode_static_lock<true, false>")
    assert dec_name((8, 30, 32), with_total(1 << 17), HUGE_LEN // 48).startswith("k_decode_static<true>")
    names = {enc_name(P, t, 4096, 4096) for P, t in (((8, 30, 32), FLAT), ((8, 14, 16), FLAT), ((8, 30, 32), with_total(1 << 17)))}
    assert len(names) == 3


def test_invalid_arguments_name_no_kernel():
    P = (8, 30, 32)
    bad = [FLAT[:100] + [FLAT[99]] + FLAT[101:],          # not strictly increasing
           [1] + FLAT[1:],                                 # cum[0] != 0
           [i * 100 for i in range(258)]]                  # total > freq_max at (8, 14, 16)
    for cum in bad:
        assert enc_name((8, 14, 16), cum, 4096, 4096) == "" and dec_name((8, 14, 16), cum, 1) == ""
    assert enc_name((12, 20, 32), FLAT, 4096, 4096) == "" and dec_name((12, 20, 32), FLAT, 1) == ""  # unsupported width
    assert enc_name((8, 9, 16), FLAT, 4096, 4096) == ""                                              # invalid parameters
    assert enc_name(P, FLAT, 4096, 0) == ""                                                          # block_size 0
    assert enc_name(P, FLAT, 1 << 30, 1 << 30) == ""   # 64 slots beyond a 32-bit lane offset: the call says UNSUPPORTED
    assert dec_name(P, FLAT, 0) == ""                   # no blocks: nothing is launched
    assert enc_name(P, with_total((1 << 30) - 1), 0, 4096) != ""
    assert enc_name(P, with_total(1 << 30), 0, 4096) == ""                                           # total > freq_max
    p = _lib.Params(*P)
    assert _lib.lib().redux_static_encode_kernel_name(C.byref(p), None, 4096, 4096) == b""
    assert _lib.lib().redux_static_decode_kernel_name(C.byref(p), None, 1) == b""


@pytest.mark.parametrize("params", [(8, 30, 32), (8, 22, 24), (8, 17, 20), (8, 14, 16)])
@pytest.mark.parametrize("bs", [48, 4096, 65536])
def test_worst_case_static_stream_fits_the_block_cap(params, bs):
    """The most expensive streams valid input can produce: a table of total freq_max with nearly all of it on one
    symbol, and a block of only a rare symbol.  Each byte costs ~freq_bits bits, so the stream expands -- and stays
    inside the per-block slot the encoder and redux_static_encode_bound reserve."""
    cum = worst_case_table(params)
    p = _lib.Params(*params)
    cap = _lib.lib().redux_static_encode_bound(C.byref(p), bs, bs)
    assert cap == _lib.lib().redux_static_encode_bound(C.byref(p), 7 * bs, bs) // 7   # one slot per block
    assert _lib.lib().redux_static_table_check(C.byref(p), (C.c_uint32 * 258)(*cum)) == 0
    stream, (bi, bo) = ox.compress_static(bytes([200]) * bs, cum, params, cap=2 * cap)
    assert bi == bs and bo == len(stream)
    assert bs < len(stream) <= cap, (len(stream), cap)
    bits_per_byte = 8 * len(stream) / bs
    assert params[1] - 0.5 < bits_per_byte < params[1] + 8 * (params[2] + 24) / bs, bits_per_byte
    back, _ = ox.decompress_static(stream, cum, params, cap=bs)
    assert back == bytes([200]) * bs
