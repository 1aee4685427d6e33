"""The pair kernel's coder wave appends two symbols' bits at once (encode_pair_spec, redux_coder.hpp): integer restatements.

Per symbol the coder forms k (leading bits that low and high share), j (E3 steps), the pending count and the append: the
m = k + Pz bits of val = topk + ((2^Pz - 1) << (k - 1)), Pz = the pending bits this symbol flushes (encode_symbol,
redux_coder.hpp).  symbol_steps() restates that for a block at any (symbol_bits = 8, freq_bits, code_bits) and is checked
against the oracle's stream here; tests/test_pair_append_gpu.py imports it to prove what its inputs make the kernel do.

append_symbols() is the bit writer symbol by symbol (put_bits); append_pairs_spec() is the speculative pair form with the
kernel's register widths: V = (val_a << m_b) + val_b in 32 bits, M = m_a + m_b, a 64-bit accumulator shifted by M mod 64, at
most one dword stored per pair, nbm = (nbm + M) | -32.  For M <= 32 both give the same dwords and the same waiting bits; a
pair with M > 32 (the kernel's flag: the half is redone symbol by symbol) leaves garbage in the accumulator but never more
dwords than the true writer, at any pair of the run -- which is why the redo overwrites every stray store."""
import random

import numpy as np
import pytest

from oracle import cbind as ox

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def clz32(x):
    return 32 - x.bit_length()


def symbol_steps(data, params):
    """-> per symbol (data symbols, then EOF) a tuple (k, j, pend_before, m, val); val is exact, m may exceed 32"""
    sb, fb, cb = params
    assert sb == 8
    sh = 32 - cb
    nfreeze = (1 << fb) - 1 - 257
    counts = np.ones(257, dtype=np.int64)
    low = ihigh = pend = 0  # low and ~high left-aligned in 32 bits
    steps = []
    for p, s in enumerate(list(data) + [256]):
        c = 257 + min(p, nfreeze)
        lo = int(counts[:s].sum())
        hi = lo + int(counts[s])
        if p < nfreeze and s != 256:
            counts[s] += 1
        R1 = ((~(ihigh + low)) & M32) >> sh
        nlow = (low + (((R1 + 1) * lo // c) << sh)) & M32
        nihigh = ihigh if s == 256 else (-(low + (((R1 + 1) * hi // c) << sh))) & M32  # EOF: hi == c, high unchanged
        x = ~(nlow ^ nihigh) & M32
        k = clz32(x)
        sl = nlow << k
        topk, low2, ih2 = sl >> 32, sl & M32, (nihigh << k) & M32
        j = clz32(~((low2 & ih2) << 1) & M32)
        low, ihigh = (low2 << j) & 0x7FFFFFFF, (ih2 << j) & 0x7FFFFFFF
        Pz = pend if k else 0
        steps.append((k, j, pend, k + Pz, topk + ((((1 << Pz) - 1) << (k - 1)) if k else 0)))
        pend = pend - Pz + j
    return steps, low, pend


def stream_of(data, params):
    """the block's stream from symbol_steps: every append, the EOF tail (codec.rs:91-99), zero padding to a byte"""
    steps, low, pend = symbol_steps(data, params)
    bits = n = 0
    for _, _, _, m, val in steps:
        assert val < (1 << m) or m == 0 and val == 0
        bits, n = (bits << m) | val, n + m
    k, j = steps[-1][0], steps[-1][1]
    if k + j < params[2]:
        extra = params[2] - (k + j)
        b = low >> 31
        bits, n = (bits << 1) | b, n + 1
        bits, n = (bits << pend) | (((1 << pend) - 1) * (b ^ 1)), n + pend
        rest = extra - 1
        bits, n = (bits << rest) | (((low << 1) & M32) >> (32 - rest) if rest else 0), n + rest
    pad = -n % 8
    return ((bits << pad).to_bytes((n + pad) // 8, "big")) if n else b""


def pair_lengths(steps, nbytes):
    """M of every pair (2i, 2i + 1) below main_end, the part of a block that the unrolled chunks code"""
    main_end = (nbytes - 1) & ~15 if nbytes > 16 else 0
    return [(steps[i][3], steps[i + 1][3]) for i in range(0, main_end, 2)]


def append_symbols(acc, nb, seq):
    """put_bits for every (m, val) with m <= 32 -> (dwords, acc, nb)"""
    out = []
    for m, val in seq:
        assert m <= 32 and val < (1 << m)
        acc = ((acc << m) | val) & M64
        nb += m
        if nb >= 32:
            out.append((acc >> (nb - 32)) & M32)
        nb &= 31
    return out, acc, nb


def append_pairs_spec(acc, nb, seq):
    """encode_pair_spec's append for every two entries of seq -> (dwords after each pair, acc, nb, flagged)"""
    nbm = (nb - 32) & M32
    out, counts, flagged = [], [], False
    for (ma, va), (mb, vb) in zip(seq[0::2], seq[1::2]):
        M = ma + mb
        flagged |= M > 32
        V = ((((va & M32) << (mb & 31)) & M32) + (vb & M32)) & M32
        sa = (acc << (M & 63)) & M64
        acc = (sa & ~M32 & M64) | (((sa & M32) + V) & M32)
        nbv = (nbm + M) & M32
        if nbv < (1 << 31):
            out.append((acc >> (nbv & 63)) & M32)
        nbm = nbv | 0xFFFFFFE0
        counts.append(len(out))
    return out, counts, acc, (nbm + 32) & M32, flagged


def waiting(acc, nb):
    return acc & ((1 << nb) - 1)


def rand_val(rng, m):
    return rng.getrandbits(m) if m else 0


@pytest.mark.parametrize("seed", range(8))
def test_pairs_within_32_bits_equal_single_appends(seed):
    rng = random.Random(seed)
    for _ in range(200):
        nb0 = rng.randrange(32)
        acc0 = rng.getrandbits(nb0) if nb0 else 0
        seq = []
        for _ in range(rng.randrange(1, 9)):
            ma = rng.randrange(33)
            mb = rng.randrange(33 - ma)
            seq += [(ma, rand_val(rng, ma)), (mb, rand_val(rng, mb))]
        want, wacc, wnb = append_symbols(acc0, nb0, seq)
        got, _, gacc, gnb, flagged = append_pairs_spec(acc0, nb0, seq)
        assert not flagged and got == want and gnb == wnb and waiting(gacc, gnb) == waiting(wacc, wnb)


@pytest.mark.parametrize("ma,mb", [(32, 0), (0, 32), (16, 16), (1, 31), (31, 1), (0, 0), (0, 7), (7, 0), (0, 1), (1, 0)])
@pytest.mark.parametrize("ones", [False, True])
def test_edges_with_31_bits_waiting(ma, mb, ones):
    """M = 32 exactly, M = 0, m_a = 0, m_b = 0, behind 31 waiting bits (and behind none)"""
    for nb0 in (31, 0):
        acc0 = ((1 << nb0) - 1) if ones else (0x2AAAAAAA & ((1 << nb0) - 1))
        seq = [(ma, ((1 << ma) - 1) if ones else (0x9E3779B9 & ((1 << ma) - 1))),
               (mb, ((1 << mb) - 1) if ones else (0x7F4A7C15 & ((1 << mb) - 1)))]
        want, wacc, wnb = append_symbols(acc0, nb0, seq)
        got, _, gacc, gnb, flagged = append_pairs_spec(acc0, nb0, seq)
        assert not flagged and got == want and gnb == wnb and waiting(gacc, gnb) == waiting(wacc, wnb)
        assert len(got) == (1 if nb0 + ma + mb >= 32 else 0)


@pytest.mark.parametrize("seed", range(8))
def test_flagged_run_never_stores_more_than_the_true_one(seed):
    """a run with at least one M > 32: after EVERY pair the speculative writer has stored no more dwords than the true
    one, stores one exactly when the true one stores at least one, and its bit count stays the true one mod 32"""
    rng = random.Random(1000 + seed)
    for _ in range(200):
        nb0 = rng.randrange(32)
        acc0 = rng.getrandbits(nb0) if nb0 else 0
        seq = [(m, rand_val(rng, m)) for m in (rng.randrange(33) for _ in range(8))]
        at = 2 * rng.randrange(4)
        seq[at] = (rng.randrange(17, 33), 0)
        seq[at + 1] = (rng.randrange(17, 33), 1)
        _, counts, _, gnb, flagged = append_pairs_spec(acc0, nb0, seq)
        assert flagged
        acc, nb, true_count, before = acc0, nb0, 0, 0
        for i in range(4):
            d, acc, nb = append_symbols(acc, nb, seq[2 * i: 2 * i + 2])
            true_count += len(d)
            assert counts[i] <= true_count
            assert (counts[i] - before == 1) == (len(d) >= 1) and counts[i] - before <= len(d)
            before = counts[i]
        assert gnb == nb


def test_restatement_equals_the_oracle():
    rng = np.random.default_rng(5)
    zipf = np.minimum(rng.zipf(1.2, 3000) - 1, 255).astype(np.uint8)
    rare = np.concatenate([np.zeros(3001, np.uint8), np.arange(1, 256, dtype=np.uint8)])
    for params in ((8, 30, 32), (8, 22, 24), (8, 10, 16)):
        for data in (b"", b"\x00", bytes(rng.integers(0, 256, 1040, dtype=np.uint8)), zipf.tobytes(), rare.tobytes()):
            assert stream_of(data, params) == ox.compress(data, params)[0], (params, len(data))
