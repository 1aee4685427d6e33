"""A block's input range may hold any number of bytes after its stream (include/redux_hip.h, "decode calls"): the CPU side.

redux::decompress reads its stream and ignores whatever follows it (lib.rs:113-120), and each decode call replaces one
redux::decompress call per block, so block b's range [in_offsets[b], in_offsets[b+1]) may be far longer than its
stream.  The lock-step decoders count a block's stream bits in 32 bits; they read a range only up to the bound every
stream with room for the block can reach (dec_range_bound, redux_decode.hpp).  Here, without a GPU:
  * every decode instance that tests/test_stream_ranges_gpu.py targets is the one the dispatch names for its shape,
    on both sides of each boundary that picks it;
  * the oracle ignores a range's tail: stream + 300 MiB decodes as the stream alone, with the same fetched bytes;
  * the bound holds: over garbage, the adversarial fixtures and streams built to be costly, the oracle never fetches
    more bytes than it, for every triple the GPU file uses."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cbind as ox

# ---- the instances, by the names redux_decode_kernel_name_n gives them ------------------------------------------------
LOCK = {True: "k_decode_lock<true> (u16 tree, one wave per 64 blocks, code_bits 32)",
        False: "k_decode_lock<false> (u16 tree, one wave per 64 blocks)"}
CELLS8 = "k_decode_cells<8> (u32 cells, blocks above 64 KiB, one wave per 64 blocks)"
CELLS8_FIX = "k_decode_cells<8> (u32 cells, blocks above 64 KiB, one wave per 64 blocks; fix-up: count past 2^17)"
WAVE = "k_decode_wave (one block per wave, cumulative table across the lanes)"
WAVE_FIX = "k_decode_wave (one block per wave, cumulative table across the lanes; fix-up: count past 2^17)"
GENERIC32 = "k_decode<false, true> (u32 tree)"
ANY = "k_decode_any (general parameters, one lane per block)"


def cells(sb, fix=False):
    if fix:
        return f"k_decode_cells<{sb}> (fix-up: count past 2^17)"
    return f"k_decode_cells<{sb}> " + ("(bottom cells in the workspace)" if sb >= 11 else "(cells in LDS)")


CELL_F = {1: 28, 2: 28, 3: 28, 4: 28, 5: 28, 6: 28, 7: 28, 9: 28, 10: 28, 11: 21, 12: 20}
FEW, MANY = 12, 1100           # blocks of a launch: the long ranges alone, or more than k_decode_wave takes (1024)

# id -> (params, block_size, nblocks, instance).  Every adaptive-model decode instance with a 32-bit bit count, and the
# controls, which count in 64 bits.
TARGETS = {"lock_cb32": ((8, 30, 32), 65536, FEW, LOCK[True]),
           "lock_cb24": ((8, 22, 24), 65536, FEW, LOCK[False])}
for _sb in (1, 2, 3, 4, 5, 6, 7, 9, 10):
    TARGETS[f"cells{_sb}"] = ((_sb, CELL_F[_sb], 32), 4096, FEW, cells(_sb))
for _sb in (1, 2, 3, 4, 5, 6, 7):
    TARGETS[f"cells{_sb}_fix"] = ((_sb, CELL_F[_sb], 32), 131072, FEW, cells(_sb, True))
for _sb in (11, 12):
    TARGETS[f"cells{_sb}"] = ((_sb, CELL_F[_sb], 32), 4096, FEW, cells(_sb))
TARGETS["cells8"] = ((8, 30, 32), 100_000, MANY, CELLS8)
TARGETS["cells8_fix"] = ((8, 30, 32), 150_000, MANY, CELLS8_FIX)
CONTROLS = {"wave": ((8, 30, 32), 100_000, FEW, WAVE),
            "wave_fix": ((8, 30, 32), 150_000, FEW, WAVE_FIX),
            "generic_u32": ((8, 30, 32), (1 << 22) + 16, 1025, GENERIC32),
            "any": ((8, 24, 40), 4096, FEW, ANY)}

# range lengths (stream + tail) of one launch, the 4 GiB one first: the blocks after it start past 4 GiB in d_in
LONG_RANGES = [(1 << 32) + 7, (1 << 28) - 1, (1 << 28) + 5, 3 << 27, (1 << 29) - 1, None]  # None: 2^29 + len(stream) - 1
HUGE_RANGE = (1 << 34) + 11                                                               # past rpo_last's 32-bit wrap


def range_lengths(stream_len):
    return [(1 << 29) + stream_len - 1 if n is None else n for n in LONG_RANGES]


def range_bound(params, capn):
    """dec_range_bound (redux_decode.hpp): the bytes of a range a block with room for capn bytes can make the reader fetch."""
    sb, _, cb = params
    return (cb * ((8 * capn + 7) // sb + 2) + 7) // 8


def dec_name(params, bs, nblocks):
    from redux_amd import _lib
    p = _lib.Params(*params)
    return _lib.lib().redux_decode_kernel_name_n(C.byref(p), None, bs, nblocks).decode()


def oracle_decode(stream, cap, params):
    """ox_decompress without raising: (status as the device reports it, decoded bytes, bytes fetched)."""
    st, out, fetched = ox.decompress_raw(stream, cap, params)
    return (4 if st == ox.IO_ERROR else st), out, fetched


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib.lib()


# ---- 1. which instance each target runs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(TARGETS) + sorted(CONTROLS))
def test_every_target_maps_to_its_instance(lib, key):
    params, bs, nb, want = {**TARGETS, **CONTROLS}[key]
    assert dec_name(params, bs, nb) == want


def _gen_needs_fixup(params, bs):  # redux_hip.hip gen_needs_fixup
    sb, f, _ = params
    updates = min(bs * 8 // sb, ((1 << f) - 1) - ((1 << sb) + 1))
    return (1 << sb) + 1 + updates > (1 << 17) + 64


@pytest.mark.parametrize("sb", [1, 2, 3, 4, 5, 6, 7])
def test_cell_fixup_boundary(lib, sb):
    """The last block size without the fix-up instance and the first with it."""
    params = (sb, CELL_F[sb], 32)
    lo, hi = 1, 1 << 22
    while hi - lo > 1:                                   # smallest block size that needs the fix-up
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if _gen_needs_fixup(params, mid) else (mid, hi)
    assert not _gen_needs_fixup(params, lo) and _gen_needs_fixup(params, hi)
    assert dec_name(params, lo, FEW) == cells(sb)
    assert dec_name(params, hi, FEW) == cells(sb, True)
    assert TARGETS[f"cells{sb}_fix"][1] >= hi and TARGETS[f"cells{sb}"][1] <= lo


def test_cells8_fixup_boundary(lib):
    """cells8_needs_fixup: 257 + min(block, freeze point) updates pass 2^17 + 64 from blocks of 130,880 bytes."""
    assert dec_name((8, 30, 32), 130_879, MANY) == CELLS8
    assert dec_name((8, 30, 32), 130_880, MANY) == CELLS8_FIX


@pytest.mark.parametrize("bs,wave", [(100_000, WAVE), (150_000, WAVE_FIX)])
def test_wave_decoder_takes_up_to_1024_blocks(lib, bs, wave):
    cells8 = CELLS8 if bs < 130_880 else CELLS8_FIX
    assert dec_name((8, 30, 32), bs, 1024) == wave
    assert dec_name((8, 30, 32), bs, 1025) == cells8


def test_wave_decoder_takes_up_to_768_blocks_of_1mib(lib):
    assert dec_name((8, 30, 32), 1 << 20, 768) == WAVE_FIX
    assert dec_name((8, 30, 32), 1 << 20, 769) == CELLS8_FIX


def test_lock_step_decoders_end_at_4mib(lib):
    """Above 4 MiB the 64-bit decoders take the blocks: the bound of every 32-bit one stays below 2^31 bits."""
    assert dec_name((8, 30, 32), 1 << 22, 1025) == CELLS8_FIX
    assert dec_name((8, 30, 32), (1 << 22) + 16, 1025) == GENERIC32
    for sb in (4, 7):
        assert dec_name((sb, CELL_F[sb], 32), 1 << 22, FEW) == cells(sb, True)
        assert dec_name((sb, CELL_F[sb], 32), (1 << 22) + 16, FEW) == ANY
    for key, (params, bs, _, _) in TARGETS.items():
        assert range_bound(params, bs) * 8 < 1 << 31, key
        assert range_bound(params, 1 << 22) * 8 < 1 << 31, key
    assert range_bound((8, 30, 32), 65536) * 8 < 1 << 31                  # static lock-step blocks of 64 KiB


# ---- 2. the oracle ignores a range's tail ---------------------------------------------------------------------------
def test_oracle_ignores_a_300mib_tail():
    rng = np.random.default_rng(11)
    src = (rng.integers(0, 256, 50_000, dtype=np.uint8) >> 2).tobytes()
    stream, _ = ox.compress(src, (8, 30, 32))
    buf = np.empty(len(stream) + (300 << 20), dtype=np.uint8)
    buf[: len(stream)] = np.frombuffer(stream, dtype=np.uint8)
    buf[len(stream):] = 0x5A
    buf[len(stream): len(stream) + 4096] = rng.integers(0, 256, 4096, dtype=np.uint8)
    alone = oracle_decode(stream, 65536, (8, 30, 32))
    whole = oracle_decode(buf, 65536, (8, 30, 32))
    assert alone == whole and alone[0] == 0 and alone[1] == src and alone[2] == len(stream)


# ---- 3. the bound the decoders clamp to holds ------------------------------------------------------------------------
def _triples():
    seen = {}
    for key, (params, bs, _, _) in TARGETS.items():
        seen.setdefault(params, set()).add(bs)
    seen.setdefault((8, 30, 32), set()).add(4096)        # the static-table decoders: blocks of 4 KiB, below
    return sorted((p, min(b)) for p, b in seen.items())


def _costly(params, cap, rng):
    """A source that trains the model on symbol 0, then sends only symbols it has not seen: each costs ~freq_bits bits."""
    sb = params[0]
    nsym = cap * 8 // sb
    syms = np.zeros(nsym, dtype=np.uint64)
    syms[nsym // 2:] = rng.integers(1, 1 << sb, nsym - nsym // 2)
    bits = ((syms[:, None] >> np.arange(sb - 1, -1, -1, dtype=np.uint64)) & 1).astype(np.uint8).ravel()
    return np.packbits(bits).tobytes()[:cap]


@pytest.mark.parametrize("params,cap", _triples())
def test_oracle_never_fetches_past_the_bound(params, cap):
    rng = np.random.default_rng(sum(params) + cap)
    bound = range_bound(params, cap)
    worst, reached = 0, 0
    cases = [rng.integers(0, 256, 2 * bound, dtype=np.uint8).tobytes() for _ in range(6)]        # garbage
    cases += [bytes(2 * bound), b"\xff" * (2 * bound)]
    for k in range(3):                                                                            # costly streams + a tail
        src = _costly(params, cap + 64 * k, rng)
        s, _ = ox.compress(src, params)
        cases.append(s + rng.integers(0, 256, 2 * bound, dtype=np.uint8).tobytes())
        cases.append(s[: len(s) * 2 // 3] + rng.integers(0, 256, 2 * bound, dtype=np.uint8).tobytes())
    if params in ((8, 22, 24), (8, 30, 32)):                                                      # adversarial fixtures
        tag = "_".join(map(str, params))
        for f in sorted(os.listdir(os.path.join(GOLDEN, "adversarial"))):
            if f.endswith(tag + ".bin"):
                data = open(os.path.join(GOLDEN, "adversarial", f), "rb").read()
                s, _ = ox.compress(data[:cap], params)
                cases.append(s + bytes(2 * bound))
    for c in cases:
        st, out, fetched = oracle_decode(c, cap, params)
        assert fetched <= bound, (len(c), st, fetched, bound)
        worst = max(worst, fetched)
        reached += st == 4
    assert reached > 0          # some of them fill the block: the bound is what they are measured against
    assert worst <= bound
