"""Every adaptive coder instance and the rare-path inputs it is run on (tests/test_adaptive_instances_gpu.py): the CPU side.

The coder kernels have data-dependent slow paths that ordinary data never enters: a pending run that needs more than one
32-bit append (k_encode_pair's redo of a half from the saved state, encode_symbol_fast's careful path), low == high after
narrowing, rare symbols under a frozen model.  The inputs that force them were written when every launch ran the
full-grid kernels; since the small-grid kernels took the launches of at most 2048 blocks, most of them no longer reach
k_encode_pair or k_encode.  Here, without a GPU:
  * TARGETS: one launch shape per adaptive encode instance pick_encode_kernel can return, paired with the decoder its
    shape gets; each maps to exactly its instance, and the neighbour shape across every boundary to the other one;
  * no shape maps to a u16 kernel with the quotient fix-up (a u16 tree means at most 65,536 symbols: 257 + 65,536 < 2^17):
    those enumerators are gone, the sweep keeps them gone;
  * the audit (run with -s): which instance each older rare-path GPU test runs today;
  * rare-path inputs for every symbol width, built at import by decoding 80 00 00 ... / 7F FF FF ... with the C oracle:
    under its triple each has a pending run above 32 bits (Python restatement), for at least one triple of every width
    2 ... 12.  Width 1 is the exception: no triple tried passes 32 (WIDTH1_BIT_RUNS records 19, 19, 19 and 28); it still runs.
  * the low == high search of tests/golden/make_adversarial.py (saturate one symbol, then pick symbols whose interval is
    one code value) for (8, 14, 16), (4, 10, 12) and (12, 16, 18): each must yield hits
    ((4, 10, 16) and (12, 14, 16) yield none: the range never falls below twice the count there).
Families and widths left out: none besides the width-1 exception above."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cbind as ox
from oracle import redux_ref as rr
from test_gpu_parity import STRESS
from test_stream_ranges_cpu import ANY, CELLS8, CELLS8_FIX, GENERIC32, LOCK, WAVE, WAVE_FIX, cells, dec_name

# ---- the encode instances, by the names redux_encode_kernel_name gives them ------------------------------------------
PAIR = {True: "k_encode_pair<false, true> (u16 tree, model wave + coder wave, code_bits 32)",
        False: "k_encode_pair<false, false> (u16 tree, model wave + coder wave)"}
COOP = {True: "k_coop_model + k_coop_chain<true> (small grid: model by 64 lanes per block, chain wave + bit-writer wave, code_bits 32)",
        False: "k_coop_model + k_coop_chain<false> (small grid: model by 64 lanes per block, chain wave + bit-writer wave)"}
SINGLE16 = "k_encode<true, false> (u16 tree, one wave per 64 blocks)"
SINGLE32 = "k_encode<false, true> (u32 tree)"
ENC_ANY = "k_encode_any (general parameters, one lane per block)"


def gen_enc(sb):
    return f"k_encode_gen<{sb}>" if sb < 8 else f"k_encode_gen_pair<{sb}>"


P8 = [(8, 30, 32), (8, 22, 24), (8, 14, 16)]
BS64 = 65536
NB_PAIR = 64 * 40 + 5          # a true-shape full-grid launch: above kCoopMaxBlocks (2048), a partial last wave
NB_WIDE = 64 * 300 + 5         # 300 groups: more than one workgroup per CU of a 256-CU chip
NB_WS = 64 * 6 + 5             # "a few hundred 64 KiB blocks" on the full-grid kernels through the workspace they are given
NB_SMALL = 64 * 6 + 5          # every launch: at least five whole waves and a partial one (the GPU file's layout needs them)
NB_GEN = 64 * 6 + 5
GEN_TRIPLES = [(1, 25, 30), (2, 30, 32), (3, 29, 32), (4, 28, 32), (4, 10, 16), (5, 27, 32), (6, 26, 32), (7, 24, 30),
               (9, 20, 32), (10, 22, 32), (11, 21, 32), (12, 20, 32), (12, 14, 16)]

# id -> (params, block_size, nblocks, input alignment (bytes off 16), workspace, encoder name, decoder name).
# workspace: "own" = what redux_encode_workspace_bytes asks for the shape; "tight" = 256 bytes less, so no room for the
# small-grid pairs area (geometry_ws: the full-grid kernels, the path of every chunk of a multi-chunk host call).
# encoder name None: a decode-only launch (its streams come from the oracle).
TARGETS = {}
for _p in P8:
    _t, _cb = "_".join(map(str, _p)), _p[2] == 32
    TARGETS[f"pair_{_t}"] = (_p, BS64, NB_PAIR, 0, "own", PAIR[_cb], LOCK[_cb])
    TARGETS[f"pair_ws_{_t}"] = (_p, BS64, NB_WS, 0, "tight", PAIR[_cb], LOCK[_cb])
    TARGETS[f"single16_unaligned_{_t}"] = (_p, BS64, NB_PAIR, 4, "own", SINGLE16, LOCK[_cb])
    TARGETS[f"single16_bs65528_{_t}"] = (_p, 65528, NB_PAIR, 0, "own", SINGLE16, LOCK[_cb])
    TARGETS[f"coop_whole_{_t}"] = (_p, BS64, NB_SMALL, 0, "own", COOP[_cb], LOCK[_cb])
    TARGETS[f"coop_whole_4k_{_t}"] = (_p, 4096, 64 * 31 + 5, 0, "own", COOP[_cb], LOCK[_cb])
    TARGETS[f"coop_windows_{_t}"] = (_p, 100_000, NB_SMALL, 0, "own", COOP[_cb], WAVE)
TARGETS["pair_wide_8_30_32"] = ((8, 30, 32), BS64, NB_WIDE, 0, "own", PAIR[True], LOCK[True])
TARGETS["coop_windows_fix"] = ((8, 30, 32), 150_000, NB_SMALL, 4, "own", COOP[True], WAVE_FIX)
TARGETS["coop_windows_cells8"] = ((8, 30, 32), 100_000, 64 * 17 + 5, 0, "own", COOP[True], CELLS8)
TARGETS["coop_windows_cells8_fix"] = ((8, 22, 24), 150_000, 64 * 17 + 5, 0, "own", COOP[False], CELLS8_FIX)
TARGETS["single32_ws"] = ((8, 30, 32), 65552, NB_SMALL, 0, "tight", SINGLE32, WAVE)
TARGETS["single32_ws_8_14_16"] = ((8, 14, 16), 65552, NB_SMALL, 0, "tight", SINGLE32, WAVE)
# (k_encode runs its unrolled chunks, and with them encode_symbol_fast's careful path, for aligned input only: the ids
# above reach it; k_encode<true, false> is only ever chosen for unaligned input and codes symbol by symbol, as this one)
TARGETS["single32_ws_unaligned_8_22_24"] = ((8, 22, 24), 65552, NB_SMALL, 4, "tight", SINGLE32, WAVE)
TARGETS["dec_generic_u32"] = ((8, 30, 32), (1 << 22) + 16, 1025, 0, "own", None, GENERIC32)
for _p in GEN_TRIPLES:
    _t = "_".join(map(str, _p))
    TARGETS[f"gen_{_t}"] = (_p, 4096, NB_GEN, 0, "own", gen_enc(_p[0]), cells(_p[0]))
    if _p[0] < 8 and _p[1] > 17:            # the count passes 2^17 inside a block: the decoder's fix-up instance
        TARGETS[f"gen_{_t}_fix"] = (_p, 131072, NB_GEN, 4, "own", gen_enc(_p[0]), cells(_p[0], True))
TARGETS["gen_4_10_12"] = ((4, 10, 12), 4096, NB_GEN, 0, "own", gen_enc(4), cells(4))            # the low == high searches
TARGETS["gen_12_16_18"] = ((12, 16, 18), 98304, NB_GEN, 0, "own", gen_enc(12), cells(12))
TARGETS["any_8_24_40"] = ((8, 24, 40), 4096, NB_GEN, 0, "own", ENC_ANY, ANY)
TARGETS["any_13_20_32"] = ((13, 20, 32), 4096, NB_GEN, 4, "own", ENC_ANY, ANY)


def _lib():
    from redux_amd import _lib as L
    return L


def ws_bytes(params, bs, nb, ws="own"):
    L = _lib()
    n = L.lib().redux_encode_workspace_bytes(C.byref(L.Params(*params)), nb * bs, bs)
    return n - 256 if ws == "tight" else n


def enc_name(params, bs, nb, align=0, ws="own", in_len=None):
    """What a launch of nb blocks runs: input `align` bytes off a 16-byte boundary, workspace as TARGETS names it."""
    L = _lib()
    in_len = nb * bs if in_len is None else in_len
    return L.lib().redux_encode_kernel_name_ws(C.byref(L.Params(*params)), C.c_void_p(4096 + align), in_len, bs,
                                               ws_bytes(params, bs, nb, ws)).decode()


# ---- 1. the instance table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(TARGETS))
def test_every_target_maps_to_its_instances(key):
    params, bs, nb, align, ws, enc, dec = TARGETS[key]
    if enc is not None:
        assert enc_name(params, bs, nb, align, ws) == enc
    assert dec_name(params, bs, nb) == dec


def test_every_launch_has_the_waves_the_layout_needs():
    """Five whole waves and a partial one; without the partial wave (the GPU file's second form) still the same instances."""
    for key, (params, bs, nb, align, ws, enc, dec) in TARGETS.items():
        assert nb >= 64 * 5 + 2 and nb % 64 == 5 or enc is None, key
        if enc is not None:
            assert enc_name(params, bs, nb - 5, align, ws) == enc and dec_name(params, bs, nb - 5) == dec, key


def test_the_table_covers_every_adaptive_instance():
    encs = {t[5] for t in TARGETS.values()} - {None}
    decs = {t[6] for t in TARGETS.values()}
    want_enc = set(PAIR.values()) | set(COOP.values()) | {SINGLE16, SINGLE32, ENC_ANY} | {gen_enc(w) for w in range(1, 13) if w != 8}
    want_dec = set(LOCK.values()) | {WAVE, WAVE_FIX, CELLS8, CELLS8_FIX, GENERIC32, ANY}
    want_dec |= {cells(w) for w in range(1, 13) if w != 8} | {cells(w, True) for w in range(1, 8)}
    assert encs == want_enc
    assert decs == want_dec
    # the small-grid kernels on whole blocks and in windows, both code widths
    for cb in (True, False):
        assert {(t[1] <= BS64) for t in TARGETS.values() if t[5] == COOP[cb]} == {True, False}


@pytest.mark.parametrize("params", P8)
def test_boundaries_between_the_8_bit_encoders(params):
    cb = params[2] == 32
    # 2048 / 2049 blocks: the small-grid kernels end at kCoopMaxBlocks
    assert enc_name(params, BS64, 2048) == COOP[cb] and enc_name(params, BS64, 2049) == PAIR[cb]
    # aligned / unaligned input, block size a multiple of 16 or not: the pair kernel loads 16 bytes per lane
    assert enc_name(params, BS64, 2049, 0) == PAIR[cb] and enc_name(params, BS64, 2049, 4) == SINGLE16
    assert enc_name(params, 65520, 2049) == PAIR[cb] and enc_name(params, 65528, 2049) == SINGLE16
    # (the small-grid kernels take any alignment)
    assert enc_name(params, BS64, 2048, 4) == COOP[cb] and enc_name(params, 65528, 2048) == COOP[cb]
    # 1008 / 1024-byte blocks: kCoopMinBlock
    assert enc_name(params, 1008, 100) == PAIR[cb] and enc_name(params, 1024, 100) == COOP[cb]
    # 65,536 / 65,552-byte blocks: u16 / u32 tree nodes
    assert enc_name(params, BS64, 70, 0, "tight") == PAIR[cb] and enc_name(params, 65552, 70, 0, "tight") == SINGLE32
    assert enc_name(params, BS64, 70) == COOP[cb] and enc_name(params, 65552, 70) == COOP[cb]
    assert dec_name(params, BS64, 70) == LOCK[cb] and dec_name(params, 65552, 70) == WAVE
    # the workspace a launch is given: one byte short of the small-grid layout is the full-grid kernels
    L = _lib()
    cp = L.Params(*params)
    own = ws_bytes(params, BS64, 70)
    f = L.lib().redux_encode_kernel_name_ws
    assert f(C.byref(cp), None, 70 * BS64, BS64, own).decode() == COOP[cb]
    assert f(C.byref(cp), None, 70 * BS64, BS64, own - 1).decode() == PAIR[cb]
    assert f(C.byref(cp), None, 70 * BS64, BS64, 1 << 40).decode() == L.lib().redux_encode_kernel_name(C.byref(cp), None, 70 * BS64, BS64).decode()
    assert f(C.byref(cp), None, 70 * BS64, 0, own) == b""


def test_boundaries_of_the_other_widths():
    assert enc_name((7, 24, 30), 4096, 12) == gen_enc(7) and enc_name((9, 20, 32), 4096, 12) == gen_enc(9)
    assert enc_name((12, 20, 32), 4096, 12) == gen_enc(12) and enc_name((13, 20, 32), 4096, 12) == ENC_ANY
    assert enc_name((8, 30, 32), 4096, NB_GEN) == COOP[True] and enc_name((8, 30, 33), 4096, NB_GEN) == ENC_ANY
    assert enc_name((12, 20, 32), 95_230, 12) == gen_enc(12) and enc_name((12, 20, 32), 131072, 12) == ENC_ANY  # u16 nodes of the LDS tree


def test_no_u16_instance_takes_the_quotient_fixup():
    """SingleU16Fixup / GenericU16Fixup (k_encode<true, true>, k_decode<true, true>) were unreachable and are removed:
    every launch of blocks up to 64 KiB maps to a u16 instance without FIXUP, on every side of every constant."""
    sizes = sorted({s for k in range(0, 24) for s in ((1 << k) - 16, 1 << k, (1 << k) + 16) if 1 <= s <= (1 << 23)})
    counts = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 24575, 24576, 24577, 100_000]
    u16_enc = set(PAIR.values()) | set(COOP.values()) | {SINGLE16}
    seen = set()
    for params in P8:
        for bs in sizes:
            for nb in counts:
                d = dec_name(params, bs, nb)
                names = {enc_name(params, bs, nb, a, w) for a in (0, 4) for w in ("own", "tight")}
                names.add(enc_name(params, bs, nb, 0, "own", in_len=(nb - 1) * bs + 1))       # a ragged last block
                assert "" not in names and d != ""
                for n in names | {d}:
                    assert "true, true" not in n and "quotient fix-up" not in n, (params, bs, nb, n)
                if bs <= BS64:
                    assert names <= u16_enc and d == LOCK[params[2] == 32], (params, bs, nb, names, d)
                else:
                    assert not (names & (set(PAIR.values()) | {SINGLE16})) and d not in LOCK.values(), (params, bs, nb)
                seen |= names | {d}
    assert u16_enc | {SINGLE32, WAVE, WAVE_FIX, CELLS8, CELLS8_FIX, GENERIC32} <= seen


# ---- the audit: what the older rare-path GPU tests run today ----------------------------------------------------------
def adversarial_fixtures():
    adv = os.path.join(GOLDEN, "adversarial")
    out = {}
    for f in sorted(os.listdir(adv)):
        if f.endswith(".bin"):
            out[f[:-4]] = (tuple(int(x) for x in f[:-4].split("_")[-3:]), open(os.path.join(adv, f), "rb").read())
    return out


def audit_rows():
    """(test, shape, triple, instance): one row per launch shape of the older tests, from their code."""
    rows = []
    for w in P8 + [(8, 10, 16), (8, 16, 18), (8, 17, 19)]:
        rows.append(("test_stress_patterns", "1 block of 65536", w, enc_name(w, BS64, 1)))
    for name, (params, base) in adversarial_fixtures().items():
        for tail in (0, 300):
            bs = (len(base) + tail + 15) // 16 * 16
            for w in sorted({params, (8, 30, 32)}):
                rows.append(("test_adversarial_rare_paths", f"{name}{'+tail' if tail else ''}: 6 blocks of {bs}", w,
                             enc_name(w, bs, 6, in_len=5 * bs + len(base) + tail)))
    for w in ((8, 30, 32), (8, 14, 16)):
        rows.append(("test_every_byte_value_in_both_lane_halves", "128 blocks of 65536", w, enc_name(w, BS64, 128)))
    for nb in (64, 67):
        rows.append(("test_decode_full_wave_interval_collapse_narrow_codes", f"{nb} blocks of 65536", (8, 14, 16),
                     enc_name((8, 14, 16), BS64, nb)))
    return rows


def test_audit_of_the_older_rare_path_tests():
    """The before picture (python -m pytest -s prints it): only the inputs shorter than kCoopMinBlock still reach the pair
    kernel, in 6 lanes of one wave; everything else runs the small-grid kernels.  The GPU file carries the rest."""
    rows = audit_rows()
    for r in rows:
        print("%-55s %-45s %-12s %s" % (r[0], r[1], r[2], r[3].split(" (")[0]))
    by = {}
    for t, shape, w, inst in rows:
        by.setdefault(t, set()).add(inst.split("<")[0].split(" ")[0])
    assert by["test_stress_patterns"] == {"k_coop_model"}
    assert by["test_every_byte_value_in_both_lane_halves"] == {"k_coop_model"}
    assert by["test_decode_full_wave_interval_collapse_narrow_codes"] == {"k_coop_model"}
    pair = sorted({shape.split(":")[0].replace("+tail", "") for t, shape, w, inst in rows
                   if t == "test_adversarial_rare_paths" and inst.startswith("k_encode_pair")})
    coop = sorted({shape.split(":")[0].replace("+tail", "") for t, shape, w, inst in rows
                   if t == "test_adversarial_rare_paths" and inst.startswith("k_coop")})
    assert pair == ["pending_7f_8_14_16", "pending_7f_8_22_24", "pending_7f_8_30_32", "pending_80_8_30_32"]
    assert coop == ["pending_80_8_14_16", "pending_80_8_22_24", "width1_8_14_16"]
    assert not [r for r in rows if r[3].startswith("k_encode<")]


# ---- 2. rare-path inputs for every width ------------------------------------------------------------------------------
NSYM = 1200


def decode_prefix(head, params, nsym=NSYM):
    """The first nsym symbols (fewer if EOF comes first) the oracle decodes from `head` 00 00 ... / FF FF ...: whole bytes."""
    fill = b"\x00" if head == b"\x80" else b"\xff"
    cap = nsym * params[0] // 8
    st, out, _ = ox.decompress_raw(head + fill * 65536, cap, params)
    assert st in (ox.OK, ox.IO_ERROR)        # EOF symbol decoded, or the capacity reached
    return out


def symbols_of(data, sb):
    r = rr.BitReader(data)
    out = []
    for _ in range(len(data) * 8 // sb):
        out.append(r.read_bits(sb))
    return out


def pending_runs(data, params):
    """Coding `data` (its whole symbols, no EOF) with the Python restatement: (longest pending run, symbols that end with
    a run above 32 bits, symbols with low == high after narrowing)."""
    model = rr.AdaptiveTreeModel(rr.Parameters(*params))
    c = rr.Codec(model)
    out = rr.BitWriter()
    longest = over = hits = 0
    for sym in symbols_of(data, params[0]):
        count = model.total_frequency()
        lo, hi = model._range(sym)
        rng = c.high - c.low + 1
        hits += c.low + rng * hi // count - 1 == c.low + rng * lo // count
        c.compress_symbol(sym, out)
        longest = max(longest, c.pending)
        over += c.pending > 32
    return longest, over, hits


def width1_search(params, nsym, seed=20261003):
    """tests/golden/make_adversarial.py's search at any width: saturate symbol 0 until the model freezes, then pick
    symbols whose interval is a single code value (low == high after narrowing) whenever one exists.  (bytes, hits)"""
    import random
    P = rr.Parameters(*params)
    sb = params[0]
    model = rr.AdaptiveTreeModel(P)
    c = rr.Codec(model)
    out, data = rr.BitWriter(), rr.BitWriter()
    while model.total_frequency() < P.freq_max:
        c.compress_symbol(0, out)
        data.write_bits(0, sb)
    rnd = random.Random(seed)
    hits = 0
    for _ in range(nsym):
        count = model.total_frequency()
        rng = c.high - c.low + 1
        pick = 0 if rnd.random() < 0.7 else rnd.randrange(1, 1 << sb)
        if rng < 2 * count:
            for s in range(1, 1 << sb):
                lo, hi = model._range(s)
                if c.low + rng * hi // count - 1 == c.low + rng * lo // count:
                    pick, hits = s, hits + 1
                    break
        c.compress_symbol(pick, out)
        data.write_bits(pick, sb)
    while data.get_count() % 8 or (data.get_count() // 8) % 3:  # whole bytes and whole 12-bit symbols
        data.write_bits(0, sb)
    data.flush_bits()
    return bytes(data.out), hits


WIDTH1_TRIPLES = {(4, 10, 12): 3000, (12, 16, 18): 1500}      # triple -> symbols searched after the freeze
_FAMILIES = {}


def gen_families(params):
    """The rare-path inputs of a triple whose symbols are not bytes: name -> bytes (whole symbols, no tail)."""
    if params not in _FAMILIES:
        fam = {"pending_80": decode_prefix(b"\x80", params), "pending_7f": decode_prefix(b"\x7f", params)}
        if params in WIDTH1_TRIPLES:
            fam["width1"] = width1_search(params, WIDTH1_TRIPLES[params])[0]
        _FAMILIES[params] = {k: v for k, v in fam.items() if v}
    return _FAMILIES[params]


def byte_families():
    """The rare-path inputs of the 8-bit instances: the adversarial fixtures, the STRESS patterns, the soak block."""
    fam = {name: base for name, (_, base) in adversarial_fixtures().items()}
    fam.update({"stress_" + k: v for k, v in STRESS.items()})
    fam["soak_block_8_14_16"] = np.load(os.path.join(GOLDEN, "soak_block_8_14_16.npy")).tobytes()
    return fam


PENDING_TRIPLES = [p for p in GEN_TRIPLES if p[0] != 1]
WIDTH1_BIT_RUNS = {(1, 25, 30): 19, (1, 30, 32): 19, (1, 10, 32): 19, (1, 3, 32): 28}   # longest pending run, per 1-bit triple


@pytest.mark.parametrize("params", PENDING_TRIPLES)
def test_generated_inputs_have_pending_runs_past_32_bits(params):
    runs = {k: pending_runs(v, params) for k, v in gen_families(params).items()}
    print(params, {k: (len(v) * 8 // params[0],) + runs[k] for k, v in gen_families(params).items()})
    assert runs["pending_80"][0] > 32 and runs["pending_80"][1] > 0


def test_every_width_has_a_triple_with_a_long_pending_run():
    assert {p[0] for p in PENDING_TRIPLES} == set(range(2, 13)) - {8}
    for name, (params, base) in adversarial_fixtures().items():
        if name.startswith("pending"):
            assert pending_runs(base, params)[0] > 32, name


def test_width_1_reaches_no_run_past_32_bits():
    """The stated exception, recorded: the longest pending run of 1,200 decoded symbols under each 1-bit triple tried stays
    within one 32-bit append."""
    got = {params: pending_runs(decode_prefix(b"\x80", params), params)[0]
           for params in [(1, 25, 30), (1, 30, 32), (1, 10, 32), (1, 3, 32)]}
    print(got)
    assert got == WIDTH1_BIT_RUNS and max(got.values()) <= 32


def test_low_equals_high_inputs():
    base = adversarial_fixtures()["width1_8_14_16"][1]
    assert pending_runs(base, (8, 14, 16))[2] > 0
    assert pending_runs(np.load(os.path.join(GOLDEN, "soak_block_8_14_16.npy")).tobytes(), (8, 14, 16))[2] > 0
    for params, nsym in WIDTH1_TRIPLES.items():
        data, hits = width1_search(params, nsym)
        print(params, len(data), hits)
        assert hits > 0 and pending_runs(data, params)[2] >= hits
        assert data == gen_families(params)["width1"] and len(data) <= TARGETS["gen_" + "_".join(map(str, params))][1]
