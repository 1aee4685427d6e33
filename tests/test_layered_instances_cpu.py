"""Every layer in front of the adaptive coder on every coder instance below it (tests/test_layered_instances_gpu.py): the
CPU side.  The layers: byte planes, the delta filter and stored blocks; then constant blocks, the mixed layouts and the
zigzag, lag, base XOR and base folded-difference filters; then the higher-order lagged differences (lag order); then the
record layout for fixed-width structs.

Each layer's `_dev` calls are a few lines in front of encode_slots_impl / redux_encode_blocks_dev, and their decode calls
in front of decode_blocks_dev_impl; what can go wrong is in the seams: which buffer the coder and the compaction read (the
caller's, possibly unaligned, input for E = 1 without a filter or base; the aligned copy at the front of the workspace
otherwise), the workspace that is left behind what the wrapper takes off the front (it decides small grid or full grid),
the store width of the table form, the selection kernel rewriting the sizes between coder and scan; for constant blocks
the table the library builds itself (the coded blocks packed from entry 0, idle entries behind them) under the ENCODER's
table form, planned for nblocks * block_size bytes.  Here, without a GPU:
  * ROWS: per layer one launch shape for every reason (REACH) an instance is reached under that layer; each maps to exactly
    its encoder and decoder, through the same name functions the launch code decides by, for the buffer, length and
    workspace the wrapper hands on (what it takes off the front is read off the workspace functions: the copy; for
    constant blocks the copy and the table, always; for the mixed layouts the copy and the cost rows);

        layer                        reasons                                       E by turn     besides
        planes, delta                16 (REACH but the two of stored, + 4 MiB)     2, 8 / 1, 2, 8
        stored                       12 (the ten common, alignment, table_generic32)  1, 4
        const                        stored's 12                                   1, 2, 4, 8    base: none / whole / ends inside a frame
        mixed                        7 (MIXED_WHYS)                                (units of 8)  a dictated table of all 8 layouts
        zigzag, lag, base, base_sub  8 each (FILTER_WHYS)                          1, 2, 4, 8    lag 3, 2, 17, 256, 5, 64, 255, 16;
                                                                                                 base as const, once longer than x
        lag_order                    8 (FILTER_WHYS)                               1, 2, 4, 8    the same lags; order 2, 3, 3, 2, 3, 2, 2, 3:
                                                                                                 both orders at every element size
        record                       8 (FILTER_WHYS)                               (record size) R = the eight lags by turn in place of E; the byte delta
                                                                                                 off, off, on, on, ...: both at odd and even R
  * the table covers, per layer, every reason: removing a row fails test_the_table_covers_every_reason, which compares
    ROWS with a list written out per layer and asserts the encoders, decoders, element sizes, lags and kinds of base reached;
  * the table form of the decoders never names k_decode_cells<8> (redux_decode_kernel_name_table);
  * stored and constant blocks with a triple other than 8-bit symbols and code_bits <= 32 are UNSUPPORTED, workspace 0;
  * the inputs of the constant rows meet the flag pattern the GPU test asserts before it calls the device;
  * the audit (run with -s): which instance each older GPU test of the layers runs today.
Instance x layer pairs left out: the fix-up cell decoders of the widths below 8 (the plain table has them, the wrappers
add nothing width-dependent); under constant blocks the general-symbol coders (UNSUPPORTED, asserted); under the mixed
layouts, the four later filters and the lag order the reasons that differ from a row of theirs only in the code width or
in a decoder the same launch code reaches under delta (they share layout_stage and layout_decode_tail with it by
construction: the sixteen reasons of delta stay delta's), and the decode-only launch of 4 MiB blocks."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_adaptive_instances_cpu import COOP, ENC_ANY, PAIR, SINGLE16, SINGLE32, gen_enc
from test_stream_ranges_cpu import ANY, CELLS8, CELLS8_FIX, GENERIC32, LOCK, WAVE, WAVE_FIX, cells, dec_name

PLANES, DELTA, STORED = "planes", "delta", "stored"
CONST, MIXED, ZIGZAG, LAG, BASE, BASE_SUB = "const", "mixed", "zigzag", "lag", "base", "base_sub"
LAG_ORDER = "lag_order"                                   # (the infix of redux_encode_lag_order_workspace_bytes)
RECORD = "record"                                         # the record layout: a row's "E" is the record size, a frame E blocks
FIRST_LAYERS = (PLANES, DELTA, STORED)
FILTERS = (ZIGZAG, LAG, BASE, BASE_SUB, LAG_ORDER, RECORD)  # the filters of layout_stage / layout_decode_tail behind delta
WITH_LAG = (LAG, LAG_ORDER)                               # the calls that take a lag (the lag order: and an order behind it)
WITH_BASE = (CONST, BASE, BASE_SUB)                       # the calls that take (d_base, base_len)
LAYERS = FIRST_LAYERS + (CONST, MIXED) + FILTERS
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
for _layer in FIRST_LAYERS:
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

# ---- the layers that came after: constant blocks, mixed layouts, the zigzag, lag, base XOR and base folded-difference filters
# The reasons each is run for.  Constant blocks: the coders of stored blocks, and the table form of the decoders, so stored's
# twelve.  Mixed: the seven that differ in what lies behind the copy and the cost rows.  The filters share layout_stage and
# layout_decode_tail with delta by construction: eight reasons, one per encoder family and decoder the first layers' rows
# had not already paired with a filter's kind of copy.
_STORED_WHYS = [w for w, r in REACH.items() if r[6] is not None]
MIXED_WHYS = ["coop_whole_cb32", "coop_windows_100k", "pair_by_blocks_cb32", "pair_by_workspace", "single16_by_block_size",
              "single32_by_workspace", "cells8"]
FILTER_WHYS = ["coop_whole_cb16", "coop_windows_150k", "pair_by_blocks_cb32", "pair_below_coop_min", "single16_by_block_size",
               "single32_by_workspace", "gen_9_to_12", "cells8_fix"]
LATER_WHYS = {CONST: _STORED_WHYS, MIXED: MIXED_WHYS, **{f: FILTER_WHYS for f in FILTERS}}
MIXED_UNIT = 8                                             # REDUX_MIXED_UNIT_BLOCKS: a mixed row's "E" is the unit, in blocks
LAGS = (3, 2, 17, 256, 5, 64, 255, 16)                     # by turn, from the first row of the lag filter on
ELEMENT.update({CONST: (1, 2, 4, 8), MIXED: (MIXED_UNIT,), **{f: (1, 2, 4, 8) for f in FILTERS}, RECORD: LAGS})  # (record sizes)
ORDERS = (2, 3, 3, 2, 3, 2, 2, 3)                          # by turn: with E = 1, 2, 4, 8 by turn every element size meets both
# the base of a row, by turn: none (base_len 0), as long as the input, ending inside a frame at an odd byte; and one row
# of each base filter with a base longer than the input
BASE_KINDS = ("none", "full", "inside")
PINNED.update({(CONST, "single16_by_alignment"): (1, 4),   # E = 1 without a base: the caller's buffer, 4 bytes off
               (CONST, "pair_by_blocks_cb32"): (1, 4)})    # ... the same shape WITH a base reads the copy: the pair kernel
# the record layout: a row's "E" is its record size (LAGS by turn); these two keep their buffers aligned, so that the fast kernels
# run the tiles of 63 groups in column ranges (R = 256, B = 1008) and the 147 tiles a frame of B = 150,000
PINNED.update({(RECORD, "pair_below_coop_min"): (256, 0), (RECORD, "cells8_fix"): (16, 0)})
PINNED_BASE = {(CONST, "single16_by_alignment"): "none", (CONST, "pair_by_blocks_cb32"): "full",
               (BASE, "single32_by_workspace"): "longer", (BASE_SUB, "single32_by_workspace"): "longer"}
# id -> (lag or None, kind of base or None, order or None, the record layout's delta flag or None).  The flag alternates every
# two rows, so that the odd and the even record sizes (which alternate row by row) each meet both values
EXTRA = {}
for _layer in (CONST, MIXED) + FILTERS:
    for _turn, _why in enumerate(LATER_WHYS[_layer]):
        _p, _bs, _nb, _ws, _enc, _dec, _dec_t = REACH[_why]
        _E, _off = PINNED.get((_layer, _why), (ELEMENT[_layer][_turn % len(ELEMENT[_layer])], 4 * (_turn % 2)))
        _base = PINNED_BASE.get((_layer, _why), BASE_KINDS[_turn % 3]) if _layer in WITH_BASE else None
        if _layer == CONST and _E == 1 and _base == "none" and (_layer, _why) not in PINNED:
            _off = 0                                       # (as for stored: the caller's buffer is what the coder reads)
        _id = f"{_layer}_{_why}" if _layer == MIXED else f"{_layer}_r{_E}_{_why}" if _layer == RECORD else f"{_layer}_e{_E}_{_why}"
        ROWS[_id] = (_layer, _p, _E, _bs, _nb, _off, _ws, _enc, _dec_t if _layer == CONST else _dec, _why)
        EXTRA[_id] = (LAGS[_turn % len(LAGS)] if _layer in WITH_LAG else None, _base,
                      ORDERS[_turn % len(ORDERS)] if _layer == LAG_ORDER else None,
                      bool(_turn // 2 % 2) if _layer == RECORD else None)


def base_len_of(kind, in_len, E, bs):
    """The base_len of a row: 0; the input's length; two thirds of the way through the input, inside a frame, at an odd byte
    (inside an element for E > 1: its last byte is missing); 777 bytes more than the input."""
    if kind in (None, "none"):
        return 0
    if kind == "inside":
        F = E * bs
        return in_len // F * 2 // 3 * F + F // 2 - 1
    return {"full": in_len, "longer": in_len + 777}[kind]


def mixed_table(nunits):
    """The dictated unit table of the mixed rows: every layout, never the same twice in a row but for units 1 and 2, and a
    non-zero layout for the last unit."""
    t = np.array([(5 * u + u // 8) % 8 for u in range(nunits)], dtype=np.uint8)
    t[2] = t[1]
    t[-1] = t[-1] or 5
    return t


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
    if layer == MIXED:                                     # (no element size: the unit table holds one per unit)
        return lambda cp, in_len, bs, E: lib.redux_encode_mixed_workspace_bytes(cp, in_len, bs)
    return getattr(lib, f"redux_encode_{layer}_workspace_bytes")


def layer_ws_bytes(layer, params, E, bs, in_len, ws="own"):
    n = _ws_fn(layer)(C.byref(_lib().Params(*params)), in_len, bs, E)
    assert n > 0
    return n - 256 if ws == "tight" else n


def coded_len(layer, bs, in_len):
    """The bytes the coder's launch is planned for: the input's, but under constant blocks one table entry per block, so whole
    blocks (redux_encode_const_dev: encode_plan(p, nblocks * block_size, ...))."""
    return -(-in_len // bs) * bs if layer == CONST else in_len


def copy_bytes(layer, params, E, bs, in_len):
    """What the wrapper takes off the front of its workspace: its own workspace call less the plain coder's for the launch it
    plans.  The transformed copy; under constant blocks the copy and the table of the blocks left to code, under the mixed
    layouts the copy and the cost rows."""
    L = _lib()
    return layer_ws_bytes(layer, params, E, bs, in_len) - L.lib().redux_encode_workspace_bytes(C.byref(L.Params(*params)),
                                                                                               coded_len(layer, bs, in_len), bs)


def reads_copy(layer, E, base=None):
    """Whether the coder below the wrapper reads the copy at the workspace's front (else: the caller's buffer).  Byte planes
    at E = 1 are the identity, so planes, stored and, without a base, constant blocks make no copy there; every filter and the
    mixed layouts always do."""
    if layer in (PLANES, STORED):
        return E > 1
    return E > 1 or base not in (None, "none") if layer == CONST else True


def layer_enc_name(layer, params, E, bs, nb, off=0, ws="own", in_len=None, base=None):
    """What the coder below the wrapper runs: it is given the copy (256-byte aligned, the workspace's front) or, where the
    wrapper makes none, the caller's buffer `off` bytes off a 16-byte boundary, and the workspace behind the front."""
    L = _lib()
    in_len = input_len(params, bs, nb) if in_len is None else in_len
    front = copy_bytes(layer, params, E, bs, in_len)
    return L.lib().redux_encode_kernel_name_ws(C.byref(L.Params(*params)), C.c_void_p(4096 + (0 if reads_copy(layer, E, base) else off)),
                                               coded_len(layer, bs, in_len), bs,
                                               layer_ws_bytes(layer, params, E, bs, in_len, ws) - front).decode()


def table_name(params, bs, nentries):
    L = _lib()
    return L.lib().redux_decode_kernel_name_table(C.byref(L.Params(*params)), bs, nentries).decode()


def layer_dec_name(layer, params, bs, nb):
    """redux_decode_stored_dev and redux_decode_const_dev hand decode_blocks_dev_impl a table of one entry per block; the
    others none."""
    return table_name(params, bs, nb) if layer in (STORED, CONST) else dec_name(params, bs, nb)


# ---- 1. the instance table --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(ROWS))
def test_every_row_maps_to_its_instances(key):
    layer, params, E, bs, nb, off, ws, enc, dec, _ = ROWS[key]
    lag, base, order, delta = EXTRA.get(key, (None, None, None, None))
    in_len = input_len(params, bs, nb)
    L = _lib()
    plain = L.lib().redux_encode_workspace_bytes(C.byref(L.Params(*params)), coded_len(layer, bs, in_len), bs)
    copy = copy_bytes(layer, params, E, bs, in_len)
    # the front is the same for both workspaces, whole 256-byte lines, and absent exactly where the header says so
    assert layer_ws_bytes(layer, params, E, bs, in_len, "own") - copy == plain
    assert layer_ws_bytes(layer, params, E, bs, in_len, "tight") - copy == plain - 256
    assert copy % 256 == 0
    if layer in FIRST_LAYERS:
        assert (copy >= in_len if E > 1 or layer == DELTA else copy == 0) and reads_copy(layer, E) == bool(copy)
    elif layer == CONST:   # the copy and the table, for E = 1 without a base too: the size does not depend on the base
        table = copy - copy_bytes(DELTA, params, E, bs, in_len)
        assert table % 256 == 0 and table >= 8 * nb          # (an entry: at least an offset and a length)
    elif layer == MIXED:   # the copy and the cost rows f64[8][nblocks]
        assert copy == copy_bytes(DELTA, params, 1, bs, in_len) + (nb * 64 + 255) // 256 * 256
    else:                  # the filters: always a copy, of the planes call's size; lag, zigzag, base at E = 1 are no identity
        assert copy == copy_bytes(DELTA, params, 1 if layer == RECORD else E, bs, in_len) >= in_len   # (no element size there)
    assert (delta in (False, True) and 2 <= E <= 256 and in_len > E * bs) if layer == RECORD else delta is None
    if layer in WITH_BASE:
        n = base_len_of(base, in_len, E, bs)
        assert {"none": n == 0, "full": n == in_len, "longer": n > in_len,
                "inside": 0 < n < in_len - E * bs and n % 2 == 1 and 0 < n % (E * bs) < E * bs - 1 and n % E == E - 1}[base]
    else:
        assert base is None
    assert (1 <= lag <= 256) if layer in WITH_LAG else lag is None
    assert (order in (2, 3) and 3 * lag < bs) if layer == LAG_ORDER else order is None    # all K predecessors inside a frame
    if enc is not None:
        assert layer_enc_name(layer, params, E, bs, nb, off, ws, base=base) == enc
        if reads_copy(layer, E, base):       # the coder reads the copy: the caller's alignment selects nothing
            assert {layer_enc_name(layer, params, E, bs, nb, o, ws, base=base) for o in (0, 1, 4, 8)} == {enc}
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
_TABLE = _COMMON + ["single16_by_alignment", "table_generic32"]
_FILTER = ["coop_whole_cb16", "coop_windows_150k", "pair_by_blocks_cb32", "pair_below_coop_min", "single16_by_block_size",
           "single32_by_workspace", "gen_9_to_12", "cells8_fix"]
WANT_ROWS = {PLANES: _TYPED, DELTA: _TYPED, STORED: _TABLE, CONST: _TABLE,
             MIXED: ["coop_whole_cb32", "coop_windows_100k", "pair_by_blocks_cb32", "pair_by_workspace", "single16_by_block_size",
                     "single32_by_workspace", "cells8"],
             ZIGZAG: _FILTER, LAG: _FILTER, BASE: _FILTER, BASE_SUB: _FILTER, LAG_ORDER: _FILTER, RECORD: _FILTER}
WANT_COUNT = {PLANES: 16, DELTA: 16, STORED: 12, CONST: 12, MIXED: 7, ZIGZAG: 8, LAG: 8, BASE: 8, BASE_SUB: 8, LAG_ORDER: 8, RECORD: 8}
# the record layout's rows, written out: (record size, delta flag, block size) by reason
WANT_RECORD = {"coop_whole_cb16": (3, False, BS64), "coop_windows_150k": (2, False, 150_000), "pair_by_blocks_cb32": (17, True, 4096),
               "pair_below_coop_min": (256, True, 1008), "single16_by_block_size": (5, False, 65528),
               "single32_by_workspace": (64, False, 65552), "gen_9_to_12": (255, True, 4000), "cells8_fix": (16, True, 150_000)}
# the 95 rows the table held before the lag order came: none of their ids may change (CRC-32 of the sorted ids, one a line)
OLD_IDS, OLD_IDS_CRC = 95, 1587991626


def test_the_table_covers_every_reason():
    """Per layer every reason of WANT_ROWS, once (16 + 16 + 12 rows of the first layers, 12 + 7 + 4 * 8 of the later ones, 8
    of the lag order, 8 of the record layout); and per layer every instance, element size, lag, order and kind of base, and
    for the record layout every record size and both delta flags."""
    got = sorted((r[0], r[9]) for r in ROWS.values())
    want = sorted((layer, why) for layer in LAYERS for why in WANT_ROWS[layer])
    assert got == want and len(ROWS) == len(want) == 44 + 12 + 7 + 32 + 8 + 8 == 111
    # the 95 rows from before the lag order keep their ids (the checksum is of the sorted ids as they stood then) and lead the
    # table; the new ids are the lag order's and, behind them, the record layout's
    old = sorted(k for k, r in ROWS.items() if r[0] not in (LAG_ORDER, RECORD))
    assert len(old) == OLD_IDS and zlib.crc32("\n".join(old).encode()) == OLD_IDS_CRC and set(old) <= set(ROWS)
    assert sorted(list(ROWS)[:OLD_IDS]) == old
    assert list(ROWS)[OLD_IDS:] == [f"lag_order_e{(1, 2, 4, 8)[t % 4]}_{why}" for t, why in enumerate(FILTER_WHYS)] + \
        [f"record_r{R}_{why}" for why, (R, _, _) in WANT_RECORD.items()]
    assert all(len(x) == 4 for x in EXTRA.values())
    # the record layout: the rows written out in WANT_RECORD, the eight record sizes once each, both flags at odd and even sizes,
    # the byte path, tiles of 63 groups, general 10-bit symbols; no other layer carries the flag
    assert {r[9]: (r[2], EXTRA[k][3], r[3]) for k, r in ROWS.items() if r[0] == RECORD} == WANT_RECORD
    assert sorted(R for R, _, _ in WANT_RECORD.values()) == sorted(LAGS)
    assert {(R % 2, d) for R, d, _ in WANT_RECORD.values()} == {(o, d) for o in (0, 1) for d in (False, True)}
    assert {bs % 16 for _, _, bs in WANT_RECORD.values()} == {0, 8} and WANT_RECORD["pair_below_coop_min"][2] // 16 == 63
    assert ROWS["record_r255_gen_9_to_12"][1] == GEN_HI and all(reads_copy(RECORD, R) for R in LAGS)
    assert all(x[3] is None for k, x in EXTRA.items() if ROWS[k][0] != RECORD)
    # ... and which transform kernels a row's encode (caller's buffer -> workspace) and decode (workspace -> caller's buffer) run
    names = {}
    for k, r in ROWS.items():
        if r[0] == RECORD:
            n = input_len(r[1], r[3], r[4])
            names[r[9]] = tuple(_lib().lib().redux_record_kernel_name_at(*((4096, 8192 + r[5]) if inv else (8192 + r[5], 4096)), n, r[3], r[2],
                                                                         inv).decode().replace("k_record_", "") for inv in (0, 1))
    fast, byte = ("planes + planes_bytes", "unplanes + unplanes_bytes"), ("planes_bytes", "unplanes_bytes")
    assert names == {"coop_whole_cb16": fast, "coop_windows_150k": byte, "pair_by_blocks_cb32": fast, "pair_below_coop_min": fast,
                     "single16_by_block_size": byte, "single32_by_workspace": byte, "gen_9_to_12": fast, "cells8_fix": fast}
    from redux_amd import api
    _, p, R, bs, nb, *_ = ROWS["record_r256_pair_below_coop_min"]     # one frame: column ranges of 64, tiles of 512 and of 31 groups
    assert api.record_plan(input_len(p, bs, nb), bs, R, True, True, 256)[:2] == (9, 64) and bs % 512 // 16 == 31
    _, p, R, bs, nb, *_ = ROWS["record_r16_cells8_fix"]
    assert api.record_plan(input_len(p, bs, nb), bs, R, True, True, 256)[:2] == (10, 16) and -(-bs // 1024) == 147 and bs % 1024 // 16 == 31
    assert {layer: sum(r[0] == layer for r in ROWS.values()) for layer in LAYERS} == WANT_COUNT
    assert sorted(EXTRA) == sorted(k for k, r in ROWS.items() if r[0] not in FIRST_LAYERS)
    common_enc = set(PAIR.values()) | set(COOP.values()) | {SINGLE16, SINGLE32}
    table_dec = set(LOCK.values()) | {WAVE, WAVE_FIX, GENERIC32}
    for layer in LAYERS:
        rows = [r for r in ROWS.values() if r[0] == layer]
        extra = [EXTRA[k] for k, r in ROWS.items() if r[0] == layer and k in EXTRA]
        encs, decs = {r[7] for r in rows} - {None}, {r[8] for r in rows}
        assert {r[2] for r in rows} == set(ELEMENT[layer])
        if layer in (STORED, CONST):
            assert encs == common_enc and decs == table_dec
        elif layer in (PLANES, DELTA):
            assert encs == common_enc | {gen_enc(4), gen_enc(10), ENC_ANY}
            want_dec = set(LOCK.values()) | {WAVE, WAVE_FIX, CELLS8, CELLS8_FIX, cells(4), cells(10), ANY}
            assert decs == want_dec | {GENERIC32}
        elif layer == MIXED:   # one of every encoder family at code_bits 32, the lock-step, wave and cell decoders
            assert encs == {COOP[True], PAIR[True], SINGLE16, SINGLE32} and decs == {LOCK[True], WAVE, CELLS8}
            assert {(r[3], r[6]) for r in rows if r[7] == PAIR[True]} == {(4096, "own"), (BS64, "tight")}
            assert {r[3] for r in rows if r[7] == COOP[True]} == {BS64, 100_000}
        else:                  # a filter: both small-grid forms at the narrow widths, the pair kernel by count and below
            #                    kCoopMinBlock, both single-wave kernels, a general-symbol pair, the fix-up decoders
            assert encs == {COOP[False], PAIR[True], PAIR[False], SINGLE16, SINGLE32, gen_enc(10)}
            assert decs == {LOCK[True], LOCK[False], WAVE, WAVE_FIX, CELLS8_FIX, cells(10)}
            assert {r[1] for r in rows if r[7] == COOP[False]} == {P16, P24}
        if layer in FIRST_LAYERS + (CONST,):
            # the small-grid kernels on whole blocks and in windows; the pair kernel by block count, by workspace and below
            # kCoopMinBlock; both code widths of each
            for fam in (COOP, PAIR):
                assert {r[1][2] == 32 for r in rows if r[7] in fam.values()} == {True, False}
            assert {r[3] for r in rows if r[7] in COOP.values()} >= {BS64, 100_000, 150_000}
            assert {(r[3], r[6]) for r in rows if r[7] in PAIR.values()} == {(4096, "own"), (BS64, "tight"), (1008, "own")}
        # the lags: the eight, once each; the bases: every kind, and for constant blocks every kind at E = 1 and above
        assert sorted(x[0] for x in extra if x[0] is not None) == (sorted(LAGS) if layer in WITH_LAG else [])
        # the orders: 2 and 3 at every element size of the lag order, none anywhere else; all K predecessors inside a frame
        by = {(r[2], EXTRA[k][2]) for k, r in ROWS.items() if r[0] == layer and k in EXTRA}
        assert by == ({(E, K) for E in (1, 2, 4, 8) for K in (2, 3)} if layer == LAG_ORDER
                      else {(r[2], None) for r in rows if layer not in FIRST_LAYERS})
        if layer == LAG_ORDER:
            assert len(rows) == 8 and all(3 * EXTRA[k][0] < r[3] for k, r in ROWS.items() if r[0] == layer)
        kinds = {x[1] for x in extra} - {None}
        assert kinds == ({"none", "full", "inside"} if layer == CONST else {"none", "full", "inside", "longer"} if layer in (BASE, BASE_SUB)
                         else set())
        if layer == CONST:
            by = {(r[2] == 1, EXTRA[k][1]) for k, r in ROWS.items() if r[0] == CONST}
            assert by == {(e1, kind) for e1 in (True, False) for kind in BASE_KINDS}
    assert set(LAGS) == {3, 2, 17, 256, 5, 64, 255, 16} and len(LAGS) == 8
    assert ORDERS == (2, 3, 3, 2, 3, 2, 2, 3) and len(ORDERS) == len(FILTER_WHYS)
    # the seam of the buffer: stored at E = 1 reads the caller's buffer, stored at E = 4 and delta at E = 1 the copy
    a, b, c = (ROWS[k] for k in ("stored_e1_single16_by_alignment", "stored_e4_pair_by_blocks_cb32", "delta_e1_pair_by_blocks_cb32"))
    assert a[3:7] == b[3:7] == c[3:7] and a[5] == 4 and (a[7], b[7], c[7]) == (SINGLE16, PAIR[True], PAIR[True])
    # ... constant blocks at E = 1 read the caller's buffer without a base and the copy with one: the same shape, 4 bytes off
    a, b = ROWS["const_e1_single16_by_alignment"], ROWS["const_e1_pair_by_blocks_cb32"]
    assert a[2:7] == b[2:7] == (1, 4096, NB_FULL, 4, "own") and (a[7], b[7]) == (SINGLE16, PAIR[True])
    assert (EXTRA["const_e1_single16_by_alignment"][1], EXTRA["const_e1_pair_by_blocks_cb32"][1]) == ("none", "full")
    assert not reads_copy(CONST, 1, "none") and reads_copy(CONST, 1, "full") and reads_copy(CONST, 2, "none")


def test_the_mixed_rows_dictate_a_table_of_every_layout():
    for key, r in ROWS.items():
        if r[0] == MIXED:
            assert r[2] == MIXED_UNIT and r[4] % MIXED_UNIT == 5
            t = mixed_table(-(-r[4] // MIXED_UNIT))
            assert set(t.tolist()) == set(range(8)) and t[1] == t[2] and (t[3:] != t[2:-1]).all() and t[0] != t[1] and t[-1] != 0
    _, p, _, bs, nb, *_ = ROWS["mixed_single16_by_block_size"]       # no multiple of 16: the whole launch on the byte kernel
    lib = _lib().lib()
    assert lib.redux_mixed_kernel_name(input_len(p, bs, nb), bs, 0) == b"k_mixed_bytes<0>"
    assert lib.redux_mixed_kernel_name(input_len(p, bs, nb), bs, 1) == b"k_mixed_bytes<1>"
    _, p, _, bs, nb, *_ = ROWS["mixed_coop_whole_cb32"]
    assert lib.redux_mixed_kernel_name(input_len(p, bs, nb), bs, 0) == b"k_mixed_planes<0> + k_mixed_bytes<0>"


def test_the_constant_rows_inputs_meet_the_pattern():
    """The generators of the GPU file, without a device: for every constant-blocks row and both ragged blocks the flags of the
    numpy-restated coder input hold the pattern the GPU test asserts before it calls the device, the table has an idle wave
    and a wave of non-consecutive blocks, and a base ending inside a frame leaves units of their own behind it."""
    import test_layered_instances_gpu as G
    for key, r in ROWS.items():
        if r[0] != CONST:
            continue
        for ragged in "CS":
            X = G.Launch(*r[:5], G._seed(key), ragged, base=EXTRA[key][1], oracle=False)
            G.flag_pattern_holds(X, ragged)
            G.const_launch_is_what_the_row_is_for(X, EXTRA[key][1])


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
    no name for the table form.  The same for constant blocks: the rows of the general-symbol reasons are left out of that
    layer because the call answers UNSUPPORTED, which is asserted here."""
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
        # ... and constant blocks, whose coders are stored's (const_check): with and without a base
        assert lib.redux_encode_const_workspace_bytes(C.byref(cp), 10 * 4096, 4096, E) == 0
        assert lib.redux_decode_const_workspace_bytes(C.byref(cp), 10 * 4096, 4096, E) == 0
        for base_len in (0, 10 * 4096):
            assert lib.redux_encode_const_dev(C.byref(cp), None, 10 * 4096, None, base_len, 4096, E, None, 0, None, None, None, None,
                                              None, 0, None) == L.UNSUPPORTED
            assert lib.redux_decode_const_dev(C.byref(cp), None, None, None, None, base_len, 10 * 4096, 4096, E, None, None, None, None,
                                              None, 0, None) == L.UNSUPPORTED
    assert table_name(params, 4096, 10) == ""
    # planes, delta and the later filters take them; so does the mixed call's workspace
    for f in FILTERS:
        assert getattr(lib, f"redux_encode_{f}_workspace_bytes")(C.byref(cp), 10 * 4096, 4096, 2) > 0
    assert lib.redux_encode_mixed_workspace_bytes(C.byref(cp), 10 * 4096, 4096) > 0
    assert lib.redux_encode_planes_workspace_bytes(C.byref(cp), 10 * 4096, 4096, 2) > 0
    assert lib.redux_encode_delta_workspace_bytes(C.byref(cp), 10 * 4096, 4096, 2) > 0


# ---- the audit: what the older GPU tests of the three layers run today ---------------------------------------------------
def audit_rows():
    """(layer, test, shape, encoder, decoder): one row per launch shape of the older tests' device calls, from their code.
    Host-pointer calls of one chunk get the `_dev` call's own workspace; of several chunks, a workspace without the pairs
    area ("tight")."""
    def row(layer, test, params, E, bs, nb, ws="own", off=0, base=None):
        n = nb * bs
        what = f"E={E}" if layer != MIXED else "units of 8"
        return (layer, test, f"{params} {what}: {nb} blocks of {bs}{', chunked' if ws == 'tight' else ''}{', a base' if base else ''}",
                layer_enc_name(layer, params, E, bs, nb, off, ws, in_len=n, base=base).split(" (")[0],
                layer_dec_name(layer, params, bs, nb).split(" (")[0])
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
    # the layers that came after (tests/test_const_gpu.py, test_mixed_gpu.py, test_zigzag_gpu.py, test_lag_gpu.py, test_base_gpu.py,
    # test_base_sub_gpu.py)
    for E in (1, 2, 4, 8):
        for bs in (48, 1008, 4096):              # five frames and half a frame
            for base in (None, "full"):
                rows.append(row(CONST, "test_const_dev_calls_against_the_calls_without_the_option_and_the_oracle", P32, E, bs,
                                5 * E + E // 2 + 1, base=base))
    for E, bs, nb, off in ((2, 1008, 71, 0), (1, 48, 300, 1), (1, 4096, 3, 4)):
        rows.append(row(CONST, "test_const_dev_calls_with_no_constant_block_short_inputs_and_an_unaligned_input", P32, E, bs, nb, off=off))
    for bs, nb in ((4096, 20), (1000, 17)):
        rows.append(row(MIXED, "test_dictated_streams_are_those_of_the_spliced_transform", P32, MIXED_UNIT, bs, nb))
    rows.append(row(MIXED, "test_chosen_tables_round_trip_and_masks", P32, MIXED_UNIT, 4096, 44))
    rows.append(row(MIXED, "test_device_objects_round_trip", P32, MIXED_UNIT, 4096, 28))
    rows.append(row(MIXED, "test_several_chunks_give_the_single_chunk_result_and_crcs", P32, MIXED_UNIT, 1024, 272))
    rows.append(row(MIXED, "test_several_chunks_give_the_single_chunk_result_and_crcs", P32, MIXED_UNIT, 1024, 64, "tight"))
    for layer in (ZIGZAG, BASE_SUB):
        for params in (P32, P16):
            for E in (1, 2, 4, 8):
                rows.append(row(layer, "test_streams_equal_oracle_on_transformed_bytes", params, E, 4096, 2 * E + 4))
        for E in (1, 8):
            rows.append(row(layer, "test_host_pipeline_chunks_and_two_contexts", P32, E, 4096, 645 if layer == ZIGZAG else 772))
            rows.append(row(layer, "test_host_pipeline_chunks_and_two_contexts", P32, E, 4096, 64, "tight"))
    for E in (2, 4):
        rows.append(row(LAG, "test_streams_equal_oracle_on_transformed_bytes", P32, E, 4096, 13))
    rows.append(row(LAG, "test_host_pipeline_over_several_chunks", P32, 4, 4096, 645))
    rows.append(row(LAG, "test_host_pipeline_over_several_chunks", P32, 4, 4096, 64, "tight"))
    # the lag order (tests/test_lag_order_gpu.py): the lag filter's shapes; its container and CLI test codes 13 blocks at E = 2
    for E in (2, 4):
        rows.append(row(LAG_ORDER, "test_streams_equal_oracle_on_transformed_bytes", P32, E, 4096, 13))
    rows.append(row(LAG_ORDER, "test_host_pipeline_over_several_chunks", P32, 4, 4096, 644))
    rows.append(row(LAG_ORDER, "test_host_pipeline_over_several_chunks", P32, 4, 4096, 256, "tight"))
    rows.append(row(LAG_ORDER, "test_damaged_stream_stays_in_bounds_and_spares_other_frames", P32, 2, 4096, 13))
    rows.append(row(LAG_ORDER, "test_container_and_cli_with_the_order", P32, 2, 4096, 13))
    for layer in (ZIGZAG, LAG, BASE_SUB, LAG_ORDER):
        for E in (1, 2, 4, 8):
            rows.append(row(layer, "test_device_encoder_decoder_roundtrip_and_ranges", P32, E, 4096, 4 * E + 4))
    # the record layout (tests/test_record_gpu.py): "E" is the record size; 4096-byte blocks throughout
    for R in (3, 23):
        rows.append(row(RECORD, "test_streams_equal_oracle_on_transformed_bytes", P32, R, 4096, 2 * R + -(-(1000 * R + 2) // 4096)))
    rows.append(row(RECORD, "test_host_pipeline_over_several_chunks", P32, 23, 4096, 280))
    rows.append(row(RECORD, "test_host_pipeline_over_several_chunks", P32, 23, 4096, 69, "tight"))
    rows.append(row(RECORD, "test_damaged_stream_stays_in_bounds_and_spares_other_frames", P32, 3, 4096, 13))
    rows.append(row(RECORD, "test_device_encoder_decoder_roundtrip_and_ranges", P32, 23, 4096, 3 * 23 + 4))
    rows.append(row(RECORD, "test_container_and_cli_end_to_end", P32, 23, 4096, 2 * 23 + 4))
    for bs, E, nb in ((4096, 2, 389), (4096, 4, 389), (BS64, 1, 70), (BS64, 2, 70)):
        rows.append(row(BASE, "test_encode_base_dev_equals_planes_call_on_xored_input_and_the_oracle", P32, E, bs, nb))
    rows.append(row(BASE, "test_device_coder_objects_with_a_base", P32, 4, 4096, 71))
    rows.append(row(BASE, "test_host_pointer_pair_in_three_chunks_and_more_equals_the_dev_calls", P32, 2, 256, 64, "tight"))
    return rows


def test_audit_of_the_older_layer_tests():
    """The before picture (python -m pytest -s prints it): the small-grid encoder and k_decode_lock nearly everywhere; the
    pair kernel only in the chunked host calls, in the all-stored 4 GiB launch and at B = 1000; no decoder but k_decode_lock
    (and one cell decoder); nothing above 64 KiB.  The later layers the same: constant blocks add the pair kernel and
    k_encode<true, false> at 48- and 1008-byte blocks, in launches of at most 45 blocks (less than one wave's 64 table
    entries), one of 71 and one of 300 without a constant block; code_bits 32 everywhere but for two filters' 4 to 20
    blocks at 16.  The lag order and the record layout: the small-grid encoder (the pair kernel in the one chunked host call)
    and k_decode_lock<true> in every one of their tests."""
    rows = audit_rows()
    for r in rows:
        print("%-8s %-52s %-52s %-44s %s" % (r[0], r[1][:52], r[2], r[3], r[4]))
    assert {r[0] for r in rows} == set(LAYERS)
    for layer in LAYERS:
        decs = {r[4] for r in rows if r[0] == layer}
        assert decs <= {"k_decode_lock<true>", "k_decode_lock<false>", "k_decode_cells<4>"}, (layer, decs)
    first = {e for l, e in {(r[0], r[3]) for r in rows} if l in FIRST_LAYERS}
    assert first == {"k_coop_model + k_coop_chain<true>", "k_coop_model + k_coop_chain<false>", "k_encode_pair<false, true>",
                     "k_encode<true, false>", "k_encode_gen<4>"}
    # unchunked device calls on a full-grid encoder: the all-stored launch, and 1000-byte blocks 3 bytes off alignment
    full = [r for r in rows if not r[3].startswith("k_coop") and "chunked" not in r[2] and r[0] == STORED]
    assert sorted(r[1] for r in full) == ["test_dev_calls_match_host_calls", "test_device_resident_4gib_iid_all_stored"]
    # the later layers: no encoder the first layers' tests had not, no decoder but k_decode_lock; a full-grid encoder below
    # an unchunked call only at blocks below kCoopMinBlock (48, 1000, 1008 bytes)
    later = [r for r in rows if r[0] not in FIRST_LAYERS]
    assert {r[3] for r in later} == first - {"k_encode_gen<4>"} and {r[4] for r in later} == {"k_decode_lock<true>", "k_decode_lock<false>"}
    full = [r for r in later if not r[3].startswith("k_coop") and "chunked" not in r[2]]
    assert {r[0] for r in full} == {CONST, MIXED} and all(" of 48" in r[2] or " of 100" in r[2] for r in full)
    assert {r[4] for r in later if r[0] in (CONST, MIXED, LAG, BASE)} == {"k_decode_lock<true>"}
    for layer in (LAG_ORDER, RECORD):  # (the record layout: (8, 30, 32) at B = 4096 and at most 280 blocks, the same two)
        assert {(r[3], r[4], "chunked" in r[2]) for r in rows if r[0] == layer} == {
            ("k_coop_model + k_coop_chain<true>", "k_decode_lock<true>", False), ("k_encode_pair<false, true>", "k_decode_lock<true>", True)}
