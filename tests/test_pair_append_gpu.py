"""k_encode_pair's coder wave appends two symbols at a time (encode_pair_spec) and redoes a half whose pair needs > 32 bits.

Written like tests/test_pair_input_feed_gpu.py: 2,112 blocks, so that the pair kernel runs (redux_encode_kernel_name is
asserted to say so); the dense bytes, the offsets, the status and the summary are compared with the CPU oracle, which codes
each distinct block once (the expected output is tiled from those).  What the inputs make the kernel do is asserted on the
CPU first, with the restatement of tests/test_pair_append_cpu.py (symbol_steps: k, j, pend, m per symbol; checked against
the oracle's stream for the rare blocks here):

  * A = 30,001 zeros, then 1 ... 255; B = 30,000 zeros, then 1 ... 255, then one zero.  After the run of zeros the interval
    is narrow and every new symbol is rare: appends of 13 to 26 bits follow each other, and several pairs (2i, 2i + 1) below
    main_end have m_a, m_b <= 32 but M = m_a + m_b > 32, at different positions of a half, while no single m exceeds 32: only
    the pair form's flag takes the redo.  B shifts the same run by one symbol, the other pair alignment.
  * iid blocks have no M > 32 at all.  Block b is A for b % 4 == 0, B for b % 4 == 1, else one of four iid blocks: every
    wave holds flagged and unflagged lanes in the same half.

Cases: (8, 30, 32) and (8, 22, 24) (the CB32 == false instance) on that mix; the zeros of A lengthened by 0, 2, 4, 6 (padded
to 30,272 bytes with zeros) so that the rare pairs land on each of the four pair positions of a half, in one launch;
(8, 10, 16) with 1,040-byte iid blocks for the frozen chunks.

No slot-limit case.  coder_chunk_checked takes over when some lane's stream is within kChunkBudget = 24 dwords of its slot's
capacity, 9 n / 8 + 1024 bytes for a block of n bytes whose model does not freeze (n (freq_bits + 2) / 8 + 1024 when it
does).  An adaptive add-one model codes ANY n symbols in at most n log2(256) + O(256 log n) bits, and a frozen one spends at
most freq_bits + 1 bits on a symbol, so a stream stays more than 96 bytes below that capacity at every block size: the slot
formula leaves no size at which a lane of these waves gets there."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbind as ox
from test_pair_append_cpu import pair_lengths, stream_of, symbol_steps

pytestmark = pytest.mark.gpu

P32, P24, PFREEZE = (8, 30, 32), (8, 22, 24), (8, 10, 16)
NB = 2112


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def rare_block(zeros, tail_zeros=0):
    return np.concatenate([np.zeros(zeros, np.uint8), np.arange(1, 256, dtype=np.uint8), np.zeros(tail_zeros, np.uint8)])


@functools.lru_cache(maxsize=None)
def iid_blocks(bs):
    # (about one iid block of 30,256 bytes in ten has a pair with M > 32, a pending run of 20 bits or more flushed next to
    # an ordinary symbol; these four have none at any size or parameter set used here, which every test asserts)
    rng = np.random.default_rng(12)
    return tuple(rng.integers(0, 256, bs, dtype=np.uint8) for _ in range(4))


@functools.lru_cache(maxsize=None)
def census(params, key):
    """(rare pairs [(first symbol, position in the half, m_a, m_b)], largest single m, restatement == oracle) of a block"""
    kind, arg = key
    d = {"A": lambda: rare_block(30001 + arg, 0), "B": lambda: rare_block(30000, 1), "pad": lambda: rare_block(30001 + arg, 30272 - 30256 - arg),
         "iid": lambda: iid_blocks(30256)[arg], "iid1040": lambda: iid_blocks(1040)[arg]}[kind]()
    steps, _, _ = symbol_steps(d.tobytes(), params)
    rare = [(2 * i, i % 4, a, b) for i, (a, b) in enumerate(pair_lengths(steps, len(d))) if a + b > 32]
    same = kind.startswith("iid") or stream_of(d.tobytes(), params) == ox.compress(d.tobytes(), params)[0]
    return rare, max(s[3] for s in steps[:-1]), same


def run(rx, params, distinct, pick):
    """distinct: equally long blocks; block b of the launch is distinct[pick(b)]"""
    import torch
    from redux_amd import _lib
    bs = len(distinct[0])
    assert bs % 16 == 0 and all(len(d) == bs for d in distinct)
    streams = [np.frombuffer(ox.compress(d.tobytes(), params)[0], np.uint8) for d in distinct]
    which = [pick(b) for b in range(NB)]
    a = np.concatenate([distinct[w] for w in which])
    dense = np.concatenate([streams[w] for w in which])
    want_offs = np.concatenate([[0], np.cumsum([len(streams[w]) for w in which])])
    name = _lib.lib().redux_encode_kernel_name(C.byref(_lib.Params(*params)), None, len(a), bs).decode()
    assert name.startswith("k_encode_pair<false, true>" if params[2] == 32 else "k_encode_pair<false, false>"), name
    d_in = torch.from_numpy(a).cuda()
    assert d_in.data_ptr() % 16 == 0
    enc = rx.DeviceEncoder(params, bs, len(a))
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    assert status.cpu().tolist() == [0] * NB
    assert offs.cpu().tolist() == want_offs.tolist()
    assert out[: len(dense)].cpu().numpy().tobytes() == dense.tobytes()


# ((8, 30, 32) first: the case that was run first, alone)
@pytest.mark.parametrize("params", [P32, P24])
def test_rare_pairs_in_every_wave(rx, params):
    for key in (("A", 0), ("B", 0)):
        rare, mmax, same = census(params, key)
        assert same, "the restatement's stream differs from the oracle's"
        assert len(rare) >= 1 and all(a <= 32 and b <= 32 for _, _, a, b in rare) and mmax <= 32, (key, rare, mmax)
    for q in range(4):
        assert census(params, ("iid", q))[0] == []
    blocks = [rare_block(30001), rare_block(30000, 1)] + list(iid_blocks(30256))
    run(rx, params, blocks, lambda b: b % 4 if b % 4 < 2 else 2 + (b // 4) % 4)


def test_rare_pair_at_every_position_of_a_half(rx):
    hit = []
    for extra in (0, 2, 4, 6):
        rare, mmax, same = census(P32, ("pad", extra))
        assert same and rare and mmax <= 32
        hit.append({pos for _, pos, _, _ in rare})
    # lengthening the zeros by two symbols moves the run by one pair; every variant hits several positions, and the first
    # rare pair of the four variants falls on positions 0, 3, 2 and 1
    assert [census(P32, ("pad", e))[0][0][1] for e in (0, 2, 4, 6)] == [0, 3, 2, 1]
    assert set.union(*hit) == {0, 1, 2, 3}
    blocks = [rare_block(30001 + e, 16 - e) for e in (0, 2, 4, 6)] + list(iid_blocks(30272))
    run(rx, P32, blocks, lambda b: b % 4 if b % 8 < 4 else 4 + (b // 8) % 4)


def test_frozen_chunks(rx):
    for q in range(4):
        assert census(PFREEZE, ("iid1040", q))[0] == []
    assert (1040 - 1) // 16 * 16 > (1 << 10) - 257 + 16  # frozen chunks behind the freeze-crossing one
    run(rx, PFREEZE, list(iid_blocks(1040)), lambda b: b % 4)
