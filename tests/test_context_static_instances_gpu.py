"""Every context-static coder instance, the histogram's fold path and the chunk redo on the GPU; the launch shapes, the
instance names and the certified redo blocks come from tests/test_context_static_instances_cpu.py.  Every test first asserts
the instance its shape reaches on this device, and every comparison is exact.

  1. every instance, every block: launches of 4 CUs, 4 CUs + 1 and 8 CUs + 1 wave slots (the last W = 4 shape; W = 8 in both
     coders; W = 16 in the decoder and a second round of the encoder's grid) under both code widths, blocks of 48 bytes (the
     16-byte chunk path and its line queue), a short last block alone in the last wave slot.  The input is periodic, K = 193
     distinct blocks of text (193 is prime: every distinct block meets every lane, wave and workgroup), so the reference
     model codes 193 blocks and the short one, and every stream, offset, status, size and decoded byte of the launch is
     compared with it.
  2. a bad table, streams cut by three bytes and a capacity one short on the 4 CUs + 1 and 8 CUs + 1 shapes, inside guard
     bands: the refusal loops and the status paths with more than one workgroup of 8 and 16 waves.
  3. k_context_hist with seven rows per workgroup (two folds inside the loop and the last one) on 15 + 7 * CUs * 16384 + 15
     bytes one byte past a 16-byte boundary, the "+ 30" of its invariant: constant buffers, where every byte of a workgroup
     meets one packed u16 counter (its low half, its high half), and a period-4 buffer whose two busy bins share a dword.
  4. the replay of a 16-symbol chunk from the saved coder state and model (static_chunk) on the certified blocks, in lane
     0, 37 and 63 of a wave whose other lanes hold text, under the context model and under the one-table model."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import redux_ref as ref
from test_context_static_cpu import TOTAL, corpus, encode_ref, pair_counts, tables_ref
from test_context_static_gpu import FILL, Raw, check_streams, d_tables, dev, device_counts, ref_decode
from test_context_static_instances_cpu import (DEC, ENC, P24, P32, REDO_LEN, ROWS, TRIPLES, blocks_of, certify, dec_name, enc_name,
                                               period4, period4_counts, redo_block, redo_tables, redo_text)

pytestmark = pytest.mark.gpu

K, B, SHORT = 193, 48, 29
SHAPES = ["last_of_4_waves", "first_of_8_waves", "first_of_16_decoder_waves"]
WIDE = SHAPES[1:]


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def key_of(why, params):
    return f"{why}_{'_'.join(map(str, params))}"


# ---- the periodic launch and its reference --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def period():
    """K distinct blocks of B bytes of text: uint8[K, B]"""
    rows = corpus("canterbury/alice29.txt")[20000: 20000 + K * B].reshape(K, B).copy()
    assert len({r.tobytes() for r in rows}) == K
    return rows


@functools.lru_cache(maxsize=None)
def period_tables():
    return tables_ref(pair_counts(period().reshape(-1), B))


@functools.lru_cache(maxsize=None)
def period_streams(params):
    return encode_ref(period().reshape(-1), B, period_tables(), params)


def launch_input(nblocks):
    """block b is distinct block b % K; the last one is its first SHORT bytes"""
    return np.resize(period().reshape(-1), nblocks * B)[: (nblocks - 1) * B + SHORT]


@functools.lru_cache(maxsize=None)
def expected(params, nblocks):
    """(streams of the whole launch, dense; offsets; streams of the K distinct blocks and of the short last one)"""
    streams = list(period_streams(params))
    assert len(streams) == K
    last = encode_ref(period()[(nblocks - 1) % K][:SHORT], B, period_tables(), params)[0]
    sizes = np.array([len(s) for s in streams], dtype=np.int64)[np.arange(nblocks) % K]
    sizes[-1] = len(last)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    full, rest = divmod(nblocks - 1, K)
    per = np.frombuffer(b"".join(streams), dtype=np.uint8)
    data = np.concatenate([np.tile(per, full), np.frombuffer(b"".join(streams[:rest]) + last, dtype=np.uint8)])
    assert len(data) == offs[-1]
    return data, offs, streams + [last]


def shape(why, params):
    """(blocks, input) of the row on this device, after asserting the instances the library names for it"""
    p, _, fn, enc, dec = ROWS[key_of(why, params)]
    nb = blocks_of(fn(cus()))
    x = launch_input(nb)
    assert enc_name(params, len(x), B) == enc and dec_name(params, nb) == dec
    return nb, x


def test_this_device_is_what_the_library_counts():
    """the names are answered for HIP's current device: its CU count moves the thresholds"""
    n = cus()
    print(f"{n} CUs: launches of {[blocks_of(ROWS[key_of(w, P32)][2](n)) for w in SHAPES]} blocks of {B} bytes, "
          f"histogram buffers of {hist_len()} bytes ({ROWS_PER_WG} rows per workgroup)")
    for p in TRIPLES:
        cb = p[2] == 32
        assert enc_name(p, 64 * 4 * n * B, B) == ENC[(cb, 4)] and enc_name(p, (64 * 4 * n + 1) * B, B) == ENC[(cb, 8)]
        assert dec_name(p, 64 * 4 * n) == DEC[4] and dec_name(p, 64 * 4 * n + 1) == DEC[8]
        assert dec_name(p, 64 * 8 * n) == DEC[8] and dec_name(p, 64 * 8 * n + 1) == DEC[16]


# ---- 1. every instance, every block ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", TRIPLES)
@pytest.mark.parametrize("why", SHAPES)
def test_every_block_of_every_instance(rx, why, params):
    import torch
    nb, x = shape(why, params)
    want, want_offs, _ = expected(params, nb)
    coder = rx.DeviceContextStaticCoder(params, d_tables(period_tables()), TOTAL, B, len(x))
    d_in = dev(x)
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and not bool(status.any()) and status.numel() == nb
    offs_h = offs.cpu().numpy()
    assert np.array_equal(offs_h, want_offs)
    got = out[: int(offs_h[-1])].cpu().numpy()
    if not np.array_equal(got, want):
        at = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"block {int(np.searchsorted(want_offs, at, side='right')) - 1} of {nb} differs from the reference model")
    back, sizes, st, dsum = coder.decode(out[: int(offs_h[-1])], offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and not bool(st.any()) and st.numel() == nb
    assert bool(sizes[:-1].eq(B).all()) and int(sizes[-1]) == SHORT
    assert torch.equal(back[: len(x)], d_in)


# ---- 2. refusal and damage on the wide instances ---------------------------------------------------------------------------
def reference_streams(params, nb):
    want, want_offs, _ = expected(params, nb)
    return dev(want), dev(want_offs)


@pytest.mark.parametrize("why,params", list(zip(WIDE, TRIPLES)) + list(zip(WIDE, TRIPLES[::-1])))
def test_a_bad_table_refuses_every_block_of_every_workgroup(lib, why, params):
    nb, x = shape(why, params)
    bad = period_tables().copy()
    bad[0x65, 100] = bad[0x65, 99]           # one row that does not increase
    r = Raw(lib, params, bad, TOTAL, B, len(x))
    assert r.nb == nb
    st, whole, out, offs, status, summary = r.encode(dev(x))
    assert st == lib.OK and (status == lib.INVALID_INPUT).all() and summary.tolist() == [lib.INVALID_INPUT, nb]
    assert not offs.cpu().numpy().any() and bool((whole == FILL).all())      # no stream, nothing in the output or its guards
    d_streams, d_offs = reference_streams(params, nb)
    st, back, sizes, status, summary = r.decode(d_streams, d_offs)            # (asserts the guards)
    assert st == lib.OK and (status == lib.INVALID_INPUT).all() and summary.tolist() == [lib.INVALID_INPUT, nb]
    assert not sizes.any() and (back == FILL).all()


@pytest.mark.parametrize("why,params", list(zip(WIDE, TRIPLES)))
def test_streams_cut_by_three_bytes(lib, why, params):
    """status, size and bytes of every block are the reference decoder's on the K distinct cut streams and the short one"""
    nb, x = shape(why, params)
    want, want_offs, streams = expected(params, nb)
    keep = np.ones(len(want), dtype=bool)
    for i in (1, 2, 3):
        keep[want_offs[1:] - i] = False
    cut, coffs = want[keep], want_offs - 3 * np.arange(nb + 1)
    assert min(map(len, streams)) > 3 and len(cut) == coffs[-1]
    refs = [ref_decode(s[:-3], period_tables(), B, params) for s in streams]
    idx = np.arange(nb) % K
    idx[-1] = K
    r = Raw(lib, params, period_tables(), TOTAL, B, len(x))
    st, back, sizes, status, summary = r.decode(dev(cut), dev(coffs))
    assert st == lib.OK
    assert np.array_equal(status, np.array([s for s, _ in refs], dtype=np.int32)[idx])
    assert np.array_equal(sizes, np.array([len(b) for _, b in refs], dtype=np.int32)[idx])
    ref_bytes = np.zeros((K + 1, B), dtype=np.uint8)
    for k, (_, b) in enumerate(refs):
        ref_bytes[k, : len(b)] = np.frombuffer(b, dtype=np.uint8)
    written = np.arange(B)[None, :] < sizes[:, None]
    assert np.array_equal(np.where(written, back.reshape(nb, B), 0), ref_bytes[idx])
    assert (status == lib.EOF).sum() > nb // 2 and summary[1] == (status != 0).sum()


@pytest.mark.parametrize("why,params", list(zip(WIDE, TRIPLES[::-1])))
def test_capacity_one_short(lib, why, params):
    """room for B - 1 bytes per block: the full blocks decode B - 1 bytes and report OUTPUT_TOO_SMALL, the short one is whole"""
    nb, x = shape(why, params)
    d_streams, d_offs = reference_streams(params, nb)
    r = Raw(lib, params, period_tables(), TOTAL, B, len(x))
    st, back, sizes, status, summary = r.decode(d_streams, d_offs, B=B - 1)  # (asserts the guards)
    assert st == lib.OK and (status[:-1] == lib.OUTPUT_TOO_SMALL).all() and (sizes[:-1] == B - 1).all()
    assert status[-1] == 0 and sizes[-1] == SHORT and summary.tolist() == [lib.OUTPUT_TOO_SMALL, nb - 1]
    blocks = np.resize(period().reshape(-1), nb * B).reshape(nb, B)
    got = back.reshape(nb, B - 1)
    assert np.array_equal(got[:-1], blocks[:-1, : B - 1]) and np.array_equal(got[-1, :SHORT], blocks[-1, :SHORT])


# ---- 3. k_context_hist at its invariant ------------------------------------------------------------------------------------
ROWS_PER_WG = 7        # kCtxHistSteps = 3: folds after rows 3 and 6, and the last one


def hist_len():
    return 15 + ROWS_PER_WG * cus() * 16384 + 15


def one_past_a_boundary(fill):
    """hist_len() bytes at an address 1 past a 16-byte boundary: a head of 15 bytes, whole rows for every workgroup, a tail
    of 15.  fill: a byte value, or a host array of that length"""
    import torch
    n = hist_len()
    t = torch.empty(n + 32, dtype=torch.uint8, device="cuda:0")
    v = t[1: 1 + n]
    assert t.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 1
    if isinstance(fill, int):
        v.fill_(fill)
    else:
        v.copy_(torch.from_numpy(fill))
    return v


def only(pairs):
    want = np.zeros((256, 256), dtype=np.uint64)
    for (c, s), n in pairs.items():
        want[c, s] = n
    return want


def test_constant_zeros_in_one_block(lib):
    """every byte of a workgroup in the low half of one dword: a carry out of it would show in counts[0][1]"""
    n = hist_len()
    assert n < 1 << 31
    got = device_counts(lib, [one_past_a_boundary(0)], n)
    assert got[0, 0] == n and np.array_equal(got, only({(0, 0): n}))


def test_constant_ff_in_one_block(lib):
    """... and in the high half of the last dword: what wraps there is lost"""
    n = hist_len()
    got = device_counts(lib, [one_past_a_boundary(0xFF)], n + 5)
    assert got[255, 255] == n - 1 and np.array_equal(got, only({(0, 255): 1, (255, 255): n - 1}))


def test_constant_zeros_in_blocks_of_64(lib):
    n = hist_len()
    assert np.array_equal(device_counts(lib, [one_past_a_boundary(0)], 64), only({(0, 0): n}))


def test_two_bins_of_one_dword_and_two_calls(lib):
    """a, b, a, b ^ 1: the bins (a, b) and (a, b ^ 1) are the halves of one dword and take a quarter of the bytes each; the
    same buffer counted in two calls of whole blocks adds up to the one call"""
    n, a, b = hist_len(), 0x41, 0x6A
    v = one_past_a_boundary(period4(n, a, b))
    got = device_counts(lib, [v], n)
    assert np.array_equal(got, period4_counts(n, a, b, n))
    want = period4_counts(n, a, b, 64)
    assert np.array_equal(device_counts(lib, [v], 64), want)
    cut = n // 2 // 64 * 64
    assert v[cut:].data_ptr() % 16 == 1
    assert np.array_equal(device_counts(lib, [v[:cut], v[cut:]], 64), want)


# ---- 4. the replay of a chunk ----------------------------------------------------------------------------------------------
REDO_LANES = (0, 37, 63)
REDO_BLOCKS = 65


def redo_input(block, lane):
    """65 blocks of REDO_LEN bytes of text, the last one 7 short, with the certified block in `lane` of the first wave"""
    x = redo_text()[2000: 2000 + REDO_BLOCKS * REDO_LEN].copy()
    x[lane * REDO_LEN: (lane + 1) * REDO_LEN] = block
    return x[:-7]


@pytest.mark.parametrize("head", [0x80, 0x7F])
@pytest.mark.parametrize("params", TRIPLES)
def test_chunk_replay_under_the_context_model(rx, params, head):
    """one lane raises the ballot, 63 lanes replay a chunk they did not need: streams bit for bit, and the round trip"""
    block = redo_block("context", params, head)
    assert certify(block, "context", params)[0] < (REDO_LEN & ~15)
    cums = redo_tables()[0]
    for lane in REDO_LANES:
        x = redo_input(block, lane)
        assert enc_name(params, len(x), REDO_LEN) == ENC[(params[2] == 32, 4)] and dec_name(params, REDO_BLOCKS) == DEC[4]
        check_streams(rx, x, REDO_LEN, cums, params)


STATIC_ENC = {P32: "k_encode_static<false, true, true> (code_bits 32, one wave per SIMD)", P24: "k_encode_static<false, false> (code_bits < 32)"}


@pytest.mark.parametrize("head", [0x80, 0x7F])
@pytest.mark.parametrize("params", TRIPLES)
def test_chunk_replay_under_the_one_table_model(rx, lib, params, head):
    """static_chunk is shared: the same on redux_static_encode_blocks_dev, whose model has no state to restore"""
    import torch
    block = redo_block("static", params, head)
    assert certify(block, "static", params)[0] < (REDO_LEN & ~15)
    cum = redo_tables()[1]
    p = ref.Parameters(*params)
    for lane in REDO_LANES:
        x = redo_input(block, lane)
        name = lib.lib().redux_static_encode_kernel_name(C.byref(lib.Params(*params)), (C.c_uint32 * 258)(*cum.tolist()), len(x), REDO_LEN)
        assert name.decode() == STATIC_ENC[params]
        coder = rx.DeviceStaticCoder(params, cum, REDO_LEN, len(x))
        d_in = dev(x)
        out, offs, status, summary = coder.encode(d_in)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0] and not bool(status.any())
        offs_h = offs.cpu().numpy()
        out_h = out[: int(offs_h[-1])].cpu().numpy()
        for b in range(REDO_BLOCKS):
            want = ref.compress(x[b * REDO_LEN: (b + 1) * REDO_LEN].tobytes(), ref.StaticModel(p, cum))[0]
            assert out_h[int(offs_h[b]): int(offs_h[b + 1])].tobytes() == want, f"block {b} (the certified one is {lane})"
        back, sizes, st, dsum = coder.decode(out[: int(offs_h[-1])], offs)
        torch.cuda.synchronize()
        assert dsum.tolist() == [0, 0] and sizes.tolist() == [REDO_LEN] * (REDO_BLOCKS - 1) + [REDO_LEN - 7]
        assert torch.equal(back[: len(x)], d_in)
