"""Byte planes, the delta filter and stored blocks on every adaptive coder instance below them
(tests/test_layered_instances_gpu.py): the CPU side.

redux_encode_planes_dev, redux_encode_delta_dev and redux_encode_stored_dev are a few lines each in front of
encode_slots_impl, and their decode calls in front of decode_blocks_dev_impl; what can go wrong is in the seams: which
buffer the coder and the compaction read (the caller's, possibly unaligned, input for E = 1 without a filter; the aligned
copy at the front of the workspace otherwise), the workspace that is left behind the copy (it decides small grid or full
grid), the store width of the table form, the selection kernel rewriting the sizes between coder and scan.  Here, without a
GPU:
  * ROWS: per layer one launch shape for every reason (REACH) an instance is reached under that layer; each maps to exactly
    its encoder and decoder, through the same name functions the launch code decides by, for the buffer, length and
    workspace the wrapper hands on (the copy it takes off the front is read off the workspace functions);
  * the table covers, per layer, every reason: removing a row fails test_the_table_covers_every_reason;
  * the table form of the decoders never names k_decode_cells<8> (redux_decode_kernel_name_table);
  * stored blocks with a triple other than 8-bit symbols and code_bits <= 32 are UNSUPPORTED, workspace 0;
  * the audit (run with -s): which instance each older GPU test of the three layers runs today.
Instance x layer pairs left out: the fix-up cell decoders of the widths below 8 (the plain table has them, the wrappers
add nothing width-dependent)."""
import ctypes as C

import numpy as np
import pytest

from test_adaptive_instances_cpu import COOP, ENC_ANY, PAIR, SINGLE16, SINGLE32, gen_enc
from test_stream_ranges_cpu import ANY, CELLS8, CELLS8_FIX, GENERIC32, LOCK, WAVE, WAVE_FIX, cells, dec_name

PLANES, DELTA, STORED = "planes", "delta", "stored"
LAYERS = (PLANES, DELTA, STORED)
P32, P24, P16 = (8, 30, 32), (8, 22, 24), (8, 14, 16)
GEN_LO, GEN_HI, ANY_P = (4, 10, 16), (10, 22, 32), (8, 24, 40)
BS64 = 65536
NB = 64 * 6 + 5                  # every launch: at least five whole waves of 64 blocks and a partial one
NB_FULL = 64 * 40 + 5            # above kCoopMaxBlocks (2048): the full-grid encoders
NB_MANY = 64 * 17 + 5            # above kWaveDecMaxBlocks (1024): no k_decode_wave
NB_4MIB = 64 * 16 + 5            # the decode-only launch of blocks above 4 MiB

# reason -> (params, B, nblocks, workspace, encoder, decoder for planes / delta, decoder for stored (the table form));
# encoder None: a decode-only launch (streams from the oracle); decoder None: the layer does not reach the reason
REACH = {
    "coop_whole_cb32": (P32, BS64, NB, "own", COOP[True], LOCK[True], LOCK[True]),
    "coop_whole_cb16": (P16, BS64, NB, "own", COOP[False], LOCK[False], LOCK[False]),
    "coop_windows_100k": (P32, 100_000, NB, "own", COOP[True], WAVE, WAVE),
    "coop_windows_150k": (P24, 150_000, NB, "own", COOP[False], WAVE_FIX, WAVE_FIX),
    "pair_by_blocks_cb32": (P32, 4096, NB_FULL, "own", PAIR[True], LOCK[True], LOCK[True]),
    "pair_by_blocks_cb16": (P16, 4096, NB_FULL, "own", PAIR[False], LOCK[False], LOCK[False]),
    "pair_by_workspace": (P32, BS64, NB, "tight", PAIR[True], LOCK[True], LOCK[True]),
    "pair_below_coop_min": (P16, 1008, NB, "own", PAIR[False], LOCK[False], LOCK[False]),
    "single16_by_block_size": (P32, 65528, NB, "tight", SINGLE16, LOCK[True], LOCK[True]),
    "single32_by_workspace": (P32, 65552, NB, "tight", SINGLE32, WAVE, WAVE),
    # planes and delta only
    "gen_below_8": (GEN_LO, 4096, NB, "own", gen_enc(4), cells(4), None),
    "gen_9_to_12": (GEN_HI, 4000, NB, "own", gen_enc(10), cells(10), None),
    "any": (ANY_P, 4096, NB, "own", ENC_ANY, ANY, None),
    "cells8": (P32, 100_000, NB_MANY, "own", COOP[True], CELLS8, None),
    "cells8_fix": (P24, 150_000, NB_MANY, "own", COOP[False], CELLS8_FIX, None),
    # stored only: x is the caller's buffer at E = 1; more than 1024 table entries above 64 KiB
    "single16_by_alignment": (P32, 4096, NB_FULL, "own", SINGLE16, None, LOCK[True]),
    "table_generic32": (P32, 65552, NB_MANY, "own", COOP[True], None, GENERIC32),
}
DECODE_ONLY = {"generic32_4mib": (P32, (1 << 22) + 16, NB_4MIB, "own", None, GENERIC32, None)}

# (layer, reason) -> (element size, input bytes off a 16-byte boundary).  The element sizes of a layer take turns; where
# the coder reads the wrapper's aligned copy an unaligned input must change nothing, so most rows are given one.
ELEMENT = {PLANES: (2, 8), DELTA: (1, 2, 8), STORED: (1, 4)}
PINNED = {(STORED, "single16_by_alignment"): (1, 4),      # the caller's buffer, 4 bytes off: no 16-byte loads
          (STORED, "pair_by_blocks_cb32"): (4, 4),        # ... the same shape at E = 4 reads the copy: the pair kernel
          (STORED, "pair_by_blocks_cb16"): (1, 0),
          (STORED, "pair_by_workspace"): (1, 0), (STORED, "pair_below_coop_min"): (1, 0),
          (DELTA, "pair_by_blocks_cb32"): (1, 4),         # delta alone copies at E = 1
          (PLANES, "generic32_4mib"): (2, 4)}             # (frames of 8 MiB: the oracle codes three of them)

# id -> (layer, params, E, B, nblocks, input offset, workspace, encoder name, decoder name, reason)
ROWS = {}
for _layer in LAYERS:
    _turn = 0
    for _why, (_p, _bs, _nb, _ws, _enc, _dec, _dec_t) in list(REACH.items()) + list(DECODE_ONLY.items()):
        _d = _dec_t if _layer == STORED else _dec
        if _d is None:
            continue
        _E, _off = PINNED.get((_layer, _why), (ELEMENT[_layer][_turn % len(ELEMENT[_layer])], 4 * (_turn % 2)))
        if _layer == STORED and _E == 1 and (_layer, _why) not in PINNED:
            _off = 0                                       # (an unaligned caller's buffer would select k_encode<true, false>)
        _turn += 1
        ROWS[f"{_layer}_e{_E}_{_why}"] = (_layer, _p, _E, _bs, _nb, _off, _ws, _enc, _d, _why)


def _lib():
    from redux_amd import _lib as L
    return L


def tail_len(params, bs):
    """The ragged last block: about two thirds of a block, an odd number of bytes (no multiple of an element size) that is
    a whole number of symbols (the gen and any coders drop a trailing partial symbol)."""
    t = bs * 2 // 3
    return t // 10 * 10 + 5 if params[0] % 5 == 0 else t | 1


def input_len(params, bs, nb):
    return (nb - 1) * bs + tail_len(params, bs)


def _ws_fn(layer):
    lib = _lib().lib()
    return {PLANES: lib.redux_encode_planes_workspace_bytes, DELTA: lib.redux_encode_delta_workspace_bytes,
            STORED: lib.redux_encode_stored_workspace_bytes}[layer]


def layer_ws_bytes(layer, params, E, bs, in_len, ws="own"):
    n = _ws_fn(layer)(C.byref(_lib().Params(*params)), in_len, bs, E)
    assert n > 0
    return n - 256 if ws == "tight" else n


def copy_bytes(layer, params, E, bs, in_len):
    """What the wrapper takes off the front of its workspace for the transformed copy: its own workspace call less the plain
    coder's."""
    L = _lib()
    return layer_ws_bytes(layer, params, E, bs, in_len) - L.lib().redux_encode_workspace_bytes(C.byref(L.Params(*params)), in_len, bs)


def layer_enc_name(layer, params, E, bs, nb, off=0, ws="own", in_len=None):
    """What the coder below the wrapper runs: it is given the copy (256-byte aligned, the workspace's front) or, where the
    wrapper makes none, the caller's buffer `off` bytes off a 16-byte boundary, and the workspace behind the copy."""
    L = _lib()
    in_len = input_len(params, bs, nb) if in_len is None else in_len
    copy = copy_bytes(layer, params, E, bs, in_len)
    return L.lib().redux_encode_kernel_name_ws(C.byref(L.Params(*params)), C.c_void_p(4096 + (0 if copy else off)), in_len, bs,
                                               layer_ws_bytes(layer, params, E, bs, in_len, ws) - copy).decode()


def table_name(params, bs, nentries):
    L = _lib()
    return L.lib().redux_decode_kernel_name_table(C.byref(L.Params(*params)), bs, nentries).decode()


def layer_dec_name(layer, params, bs, nb):
    """redux_decode_stored_dev hands decode_blocks_dev_impl a table of one entry per block; the other two none."""
    return table_name(params, bs, nb) if layer == STORED else dec_name(params, bs, nb)


# ---- 1. the instance table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(ROWS))
def test_every_row_maps_to_its_instances(key):
    layer, params, E, bs, nb, off, ws, enc, dec, _ = ROWS[key]
    in_len = input_len(params, bs, nb)
    L = _lib()
    plain = L.lib().redux_encode_workspace_bytes(C.byref(L.Params(*params)), in_len, bs)
    copy = copy_bytes(layer, params, E, bs, in_len)
    # the copy is the same for both workspaces, whole 256-byte lines, and absent exactly where the header says so
    assert layer_ws_bytes(layer, params, E, bs, in_len, "own") - copy == plain
    assert layer_ws_bytes(layer, params, E, bs, in_len, "tight") - copy == plain - 256
    assert copy % 256 == 0 and (copy >= in_len if E > 1 or layer == DELTA else copy == 0)
    if enc is not None:
        assert layer_enc_name(layer, params, E, bs, nb, off, ws) == enc
        if copy:       # the coder reads the copy: the caller's alignment selects nothing
            assert {layer_enc_name(layer, params, E, bs, nb, o, ws) for o in (0, 1, 4, 8)} == {enc}
    assert layer_dec_name(layer, params, bs, nb) == dec


def test_every_launch_has_the_waves_the_layout_needs():
    for key, (layer, params, E, bs, nb, off, ws, enc, dec, _) in ROWS.items():
        assert nb >= 64 * 5 + 2 and nb % 64 == 5, key
        assert 0 < tail_len(params, bs) < bs and tail_len(params, bs) * 8 % params[0] == 0 and tail_len(params, bs) % 2, key
        assert bs * 8 % params[0] == 0, key                # whole symbols: nothing is dropped at the end of a block


# The rows the table must hold, written out: the coverage test compares ROWS with THIS list, so a row (or a reason of REACH)
# that is removed fails it, whatever instances the remaining rows still reach.
_COMMON = ["coop_whole_cb32", "coop_whole_cb16", "coop_windows_100k", "coop_windows_150k", "pair_by_blocks_cb32",
           "pair_by_blocks_cb16", "pair_by_workspace", "pair_below_coop_min", "single16_by_block_size", "single32_by_workspace"]
_TYPED = _COMMON + ["gen_below_8", "gen_9_to_12", "any", "cells8", "cells8_fix", "generic32_4mib"]
WANT_ROWS = {PLANES: _TYPED, DELTA: _TYPED, STORED: _COMMON + ["single16_by_alignment", "table_generic32"]}


def test_the_table_covers_every_reason():
    """Per layer every reason of WANT_ROWS, once (16 + 16 + 12 rows); and per layer every instance."""
    got = sorted((r[0], r[9]) for r in ROWS.values())
    want = sorted((layer, why) for layer in LAYERS for why in WANT_ROWS[layer])
    assert got == want and len(ROWS) == len(want) == 44
    assert {layer: sum(r[0] == layer for r in ROWS.values()) for layer in LAYERS} == {PLANES: 16, DELTA: 16, STORED: 12}
    common_enc = set(PAIR.values()) | set(COOP.values()) | {SINGLE16, SINGLE32}
    for layer in LAYERS:
        rows = [r for r in ROWS.values() if r[0] == layer]
        encs, decs = {r[7] for r in rows} - {None}, {r[8] for r in rows}
        assert {r[2] for r in rows} == set(ELEMENT[layer])
        if layer == STORED:
            assert encs == common_enc and decs == set(LOCK.values()) | {WAVE, WAVE_FIX, GENERIC32}
        else:
            assert encs == common_enc | {gen_enc(4), gen_enc(10), ENC_ANY}
            want_dec = set(LOCK.values()) | {WAVE, WAVE_FIX, CELLS8, CELLS8_FIX, cells(4), cells(10), ANY}
            assert decs == want_dec | {GENERIC32}
        # the small-grid kernels on whole blocks and in windows; the pair kernel by block count, by workspace and below
        # kCoopMinBlock; both code widths of each
        for fam in (COOP, PAIR):
            assert {r[1][2] == 32 for r in rows if r[7] in fam.values()} == {True, False}
        assert {r[3] for r in rows if r[7] in COOP.values()} >= {BS64, 100_000, 150_000}
        assert {(r[3], r[6]) for r in rows if r[7] in PAIR.values()} == {(4096, "own"), (BS64, "tight"), (1008, "own")}
    # the seam of the buffer: stored at E = 1 reads the caller's buffer, stored at E = 4 and delta at E = 1 the copy
    a, b, c = (ROWS[k] for k in ("stored_e1_single16_by_alignment", "stored_e4_pair_by_blocks_cb32", "delta_e1_pair_by_blocks_cb32"))
    assert a[3:7] == b[3:7] == c[3:7] and a[5] == 4 and (a[7], b[7], c[7]) == (SINGLE16, PAIR[True], PAIR[True])


@pytest.mark.parametrize("params", [P32, P24, P16])
def test_the_table_form_never_names_the_cell_decoder(params):
    """cells8_takes(.., table = true) is false: above 64 KiB a table launch runs k_decode_wave up to 1024 entries (blocks of
    1 MiB too, which without a table leave it at 769), k_decode<false, true> beyond; up to 64 KiB the lock-step decoder."""
    cb = params[2] == 32
    sizes = sorted({s for k in range(8, 24) for s in ((1 << k) - 16, 1 << k, (1 << k) + 16)} | {65528, 65552, 100_000, 150_000})
    for bs in sizes:
        for n in (1, 64, 768, 769, 1024, 1025, 2048, 2049, 100_000):
            t, d = table_name(params, bs, n), dec_name(params, bs, n)
            assert t and "k_decode_cells" not in t, (bs, n, t)
            if d in (CELLS8, CELLS8_FIX):
                assert t == GENERIC32 if n > 1024 else t in (WAVE, WAVE_FIX), (bs, n, t)
            else:
                assert t == d, (bs, n, t, d)
            if bs <= BS64:
                assert t == LOCK[cb]
    assert table_name(params, 65552, 1024) == WAVE and table_name(params, 65552, 1025) == GENERIC32
    assert dec_name(params, 65552, 1025) == CELLS8
    assert table_name(params, 1 << 20, 1024).startswith("k_decode_wave") and table_name(params, 1 << 20, 1025) == GENERIC32
    assert dec_name(params, 1 << 20, 768).startswith("k_decode_wave") and dec_name(params, 1 << 20, 769).startswith("k_decode_cells<8>")
    assert table_name(params, BS64, 0) == "" and table_name(params, 0, 5) == ""


@pytest.mark.parametrize("params", [GEN_LO, GEN_HI, ANY_P, (13, 20, 32), (8, 30, 33)])
def test_stored_takes_8_bit_symbols_and_code_bits_up_to_32_only(params):
    """stored_check comes before any pointer is looked at: UNSUPPORTED from both `_dev` calls, 0 from both workspace calls,
    no name for the table form."""
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    assert L.UNSUPPORTED == 5
    for E in (1, 4):
        assert lib.redux_encode_stored_workspace_bytes(C.byref(cp), 10 * 4096, 4096, E) == 0
        assert lib.redux_decode_stored_workspace_bytes(C.byref(cp), 10 * 4096, 4096, E) == 0
        assert lib.redux_encode_stored_dev(C.byref(cp), None, 10 * 4096, 4096, E, 65536, None, 0, None, None, None, None, None, 0,
                                           None) == L.UNSUPPORTED
        assert lib.redux_decode_stored_dev(C.byref(cp), None, None, None, 10 * 4096, 4096, E, None, 0, None, None, None, None, 0,
                                           None) == L.UNSUPPORTED
    assert table_name(params, 4096, 10) == ""
    # planes and delta take them
    assert lib.redux_encode_planes_workspace_bytes(C.byref(cp), 10 * 4096, 4096, 2) > 0
    assert lib.redux_encode_delta_workspace_bytes(C.byref(cp), 10 * 4096, 4096, 2) > 0


# ---- the audit: what the older GPU tests of the three layers run today ---------------------------------------------------
def audit_rows():
    """(layer, test, shape, encoder, decoder): one row per launch shape of the older tests' device calls, from their code.
    Host-pointer calls of one chunk get the `_dev` call's own workspace; of several chunks, a workspace without the pairs
    area ("tight")."""
    def row(layer, test, params, E, bs, nb, ws="own", off=0):
        n = nb * bs
        return (layer, test, f"{params} E={E}: {nb} blocks of {bs}{', chunked' if ws == 'tight' else ''}",
                layer_enc_name(layer, params, E, bs, nb, off, ws, in_len=n).split(" (")[0], layer_dec_name(layer, params, bs, nb).split(" (")[0])
    rows = []
    for params in (P32, P16):
        for E in (2, 4, 8):
            rows.append(row(PLANES, "test_streams_equal_plain_coder_on_planes", params, E, BS64, 2 * E + 4))
        for E in (1, 2, 4, 8):
            rows.append(row(DELTA, "test_streams_equal_oracle_on_transformed_bytes", params, E, BS64, 2 * E + 4))
    rows.append(row(PLANES, "test_streams_equal_plain_coder_on_planes (gen)", GEN_LO, 2, 16384, 12))
    for E in (2, 8):
        rows.append(row(PLANES, "test_host_pipeline_many_chunks_and_two_contexts", P32, E, 4096, 64, "tight"))
    for E in (1, 8):
        rows.append(row(DELTA, "test_host_pipeline_chunk_sizes_and_two_contexts", P32, E, 4096, 2564))
        rows.append(row(DELTA, "test_host_pipeline_chunk_sizes_and_two_contexts", P32, E, 4096, 768, "tight"))
    for E in (1, 2, 4, 8):
        rows.append(row(DELTA, "test_device_encoder_decoder_roundtrip", P32, E, BS64, 4 * E + 4))
        rows.append(row(STORED, "test_parity_with_oracle", P32, E, 16384, 14))
    rows.append(row(STORED, "test_host_round_trips_crc_small_chunks_two_contexts", P32, 2, BS64, 64, "tight"))
    rows.append(row(STORED, "test_host_calls_several_chunks", P32, 1, BS64, 1600, "tight"))
    for E, bs, off in ((1, BS64, 0), (1, 1000, 3), (4, 16384, 5), (8, 4096, 0)):
        rows.append(row(STORED, "test_dev_calls_match_host_calls", P32, E, bs, 14, off=off))
    rows.append(row(STORED, "test_mixed_waves", P32, 1, BS64, 192))
    rows.append(row(STORED, "test_device_resident_4gib_iid_all_stored", P32, 1, BS64, 65536))
    return rows


def test_audit_of_the_older_layer_tests():
    """The before picture (python -m pytest -s prints it): the small-grid encoder and k_decode_lock nearly everywhere; the
    pair kernel only in the chunked host calls, in the all-stored 4 GiB launch and at B = 1000; no decoder but k_decode_lock
    (and one cell decoder); nothing above 64 KiB."""
    rows = audit_rows()
    for r in rows:
        print("%-7s %-52s %-44s %-28s %s" % r)
    for layer in LAYERS:
        decs = {r[4] for r in rows if r[0] == layer}
        assert decs <= {"k_decode_lock<true>", "k_decode_lock<false>", "k_decode_cells<4>"}, (layer, decs)
    encs = {(r[0], r[3]) for r in rows}
    assert {e for _, e in encs} == {"k_coop_model + k_coop_chain<true>", "k_coop_model + k_coop_chain<false>", "k_encode_pair<false, true>",
                                    "k_encode<true, false>", "k_encode_gen<4>"}
    # unchunked device calls on a full-grid encoder: the all-stored launch, and 1000-byte blocks 3 bytes off alignment
    full = [r for r in rows if not r[3].startswith("k_coop") and "chunked" not in r[2] and r[0] == STORED]
    assert sorted(r[1] for r in full) == ["test_dev_calls_match_host_calls", "test_device_resident_4gib_iid_all_stored"]
