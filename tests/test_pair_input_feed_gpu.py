"""k_encode_pair's input hand-over: the coder wave reads the input and passes it to the model wave through the ring.

The coder wave reads every lane's block a 128-byte line at a time and, while it codes chunk c (16 symbols), writes the 16 bytes
of chunk c + 2 into a ring slot that the model wave reads back right after the barrier closing chunk c (feed_slot,
redux_encode.hpp).  The model wave loads chunks 0 and 1 itself.  Every case codes 2,049 to 2,200 small blocks of iid bytes (the
pair kernel runs above 2,048 blocks; redux_encode_kernel_name is asserted to say so), each a multiple of 16 bytes from a
16-byte-aligned buffer, and compares the dense bytes, the offsets, the status and the summary with the CPU oracle.  The shapes
are the smallest at which the hand-over can go wrong (main chunks of a block of n bytes: (n - 1) // 16):

  * (8, 30, 32), 32 and 48 bytes: 1 and 2 main chunks, the hand-over is never used, or once;
  * 64 bytes: 3 chunks;
  * 128, 144, 160: the coder wave's first line swap at, just before and just after a chunk edge;
  * 256, 272, 400: the second line;   1040: several lines;
  * a last block of 17 bytes in a group of 52: that wave's shortest block gives one main chunk, its other lanes a long
    predicated tail;
  * 2,100 blocks: a partial last group (dead lanes);
  * (8, 10, 16), 784, 800, 1040: the model freezes after 767 symbols, so the rolled freeze-crossing chunk (symbols 752 to 767)
    is the last main chunk, is followed by one frozen chunk, by many;
  * (8, 22, 24), 272: the instance whose code values are narrower than 32 bits."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbind as ox

pytestmark = pytest.mark.gpu

P32, PFREEZE, P24 = (8, 30, 32), (8, 10, 16), (8, 22, 24)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@functools.lru_cache(maxsize=None)
def blocks(params, nb, bs, last=None):
    """nb blocks of bs iid bytes, the last one cut to `last` bytes -> (input, the oracle's streams end to end, offsets, status)"""
    rng = np.random.default_rng(bs * 4099 + nb)
    a = rng.integers(0, 256, nb * bs, dtype=np.uint8)[: (nb - 1) * bs + (bs if last is None else last)]
    out, sizes, status, slot = ox.compress_blocks_raw(a, bs, params)
    dense = np.concatenate([out[b * slot: b * slot + int(sizes[b])] for b in range(nb)])
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return a, dense, offs, status


def check(rx, params, nb, bs, last=None):
    import torch
    from redux_amd import _lib
    assert 2049 <= nb <= 2200 and bs % 16 == 0
    a, dense, want_offs, want_status = blocks(params, nb, bs, last)
    name = _lib.lib().redux_encode_kernel_name(C.byref(_lib.Params(*params)), None, len(a), bs).decode()
    assert name.startswith("k_encode_pair<false, true>" if params[2] == 32 else "k_encode_pair<false, false>"), name
    d_in = torch.from_numpy(a).cuda()
    assert d_in.data_ptr() % 16 == 0
    enc = rx.DeviceEncoder(params, bs, len(a))
    out, offs, status, summary = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    assert status.cpu().tolist() == want_status.tolist()
    assert offs.cpu().tolist() == want_offs.tolist()
    assert out[: len(dense)].cpu().numpy().tobytes() == dense.tobytes()


# (48 first: one hand-over, the least that uses every part of the protocol)
@pytest.mark.parametrize("bs", [48, 32, 64, 128, 144, 160, 256, 272, 400, 1040])
def test_whole_groups(rx, bs):
    check(rx, P32, 2112, bs)


def test_last_block_of_17_bytes(rx):
    """group 32 holds 52 blocks; its last one has 17 bytes: one main chunk for that wave, then 255 symbols of tail for 51 lanes"""
    check(rx, P32, 2100, 272, last=17)


def test_partial_last_group(rx):
    check(rx, P32, 2100, 272)


@pytest.mark.parametrize("bs", [784, 800, 1040])
def test_freeze_crossing_chunk(rx, bs):
    nfreeze = (1 << PFREEZE[1]) - 257
    main_end = (bs - 1) & ~15
    assert nfreeze == 767 and (nfreeze & ~15) + 16 <= main_end and (main_end - 768) // 16 == {784: 0, 800: 1, 1040: 16}[bs]
    check(rx, PFREEZE, 2112, bs)


def test_narrow_code_values(rx):
    check(rx, P24, 2112, 272)
