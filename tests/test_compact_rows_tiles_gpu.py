"""The encoder's row gather (k_compact_rows, redux_pack.hpp) at both tile heights: 64 rows and 256 rows.

Every case codes a small input through a kernel that leaves row-major group areas (k_encode_pair above 2048 blocks, the
k_coop_* kernels below; redux_encode_kernel_name says which), once per tile height, which redux_debug_compact_tile_rows
dictates, and compares the dense bytes, the offsets and the status with the CPU oracle.  The shapes are the smallest at which
a tile gather can go wrong:

  * 64, 65, 127 and 2,112 + 1 blocks: whole groups, a partial last group, group counts that are no multiple of 8 (the gather
    deals whole sets of 8 groups to the XCDs), a last block of one byte;
  * coded sizes on, one dword before and one dword after a tile edge: blocks of 2048 bytes whose first 108 bytes are zero code
    to 2048 bytes on average (an edge of both heights), blocks of 1280 bytes with 78 zeros to 1280 (an edge of the 64-row tile
    that is inside a 256-row tile); the sizes the oracle gives are asserted to hold edge - 4, edge and edge + 4;
  * all four dense alignments (offset & 3) in the first block of a group, and one group whose first four streams -- lanes of one
    store instruction -- have all four at once: asserted from the oracle's sizes;
  * blocks of one byte and of sixteen bytes (a table of ragged inputs; a plain call with block_size 16);
  * a table from redux_block_table_v with ragged tails and idle entries;
  * stored blocks mixed in (the gather skips them, k_compact copies them);
  * a dense buffer one byte short of the last block: OUTPUT_TOO_SMALL for that block, the others in place, nothing written
    from the last block's offset on (guard bytes behind the buffer included).

The oracle's answers are computed once per input and shared by both tile heights."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import cbind as ox
from test_stored_cpu import rule

pytestmark = pytest.mark.gpu

P3 = (8, 30, 32)
TILES = (64, 256)
GUARD = 4096


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(autouse=True)
def launch_chooses_again():
    yield
    from redux_amd import _lib
    assert _lib.lib().redux_debug_compact_tile_rows(0) == 0


def force(rows):
    from redux_amd import _lib
    assert _lib.lib().redux_debug_compact_tile_rows(rows) == 0


def kernel_name(nbytes, bs):
    from redux_amd import _lib
    return _lib.lib().redux_encode_kernel_name(C.byref(_lib.Params(*P3)), None, nbytes, bs).decode()


def row_major_kernel(nslots):
    """what leaves row-major group areas for a launch of this many slots (blocks of 1 KiB to 64 KiB, 16-byte multiples)"""
    return "k_encode_pair" if nslots > 2048 else "k_coop_"


@functools.lru_cache(maxsize=None)
def blocks(nb, bs, zeros, last=None, seed=1):
    """nb blocks of bs iid bytes, the first `zeros` of each zero (they set the coded size), the last block cut to `last` bytes;
    -> (input, the oracle's streams end to end, offsets, status)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (nb, bs), dtype=np.uint8)
    a[:, :zeros] = 0
    a = a.reshape(-1)[: (nb - 1) * bs + (bs if last is None else last)]
    out, sizes, status, slot = ox.compress_blocks_raw(a, bs, P3)
    dense = np.concatenate([out[b * slot: b * slot + int(sizes[b])] for b in range(nb)])
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    return a, dense, offs, status


def device_encode(rx, a, bs, rows, out_cap=None):
    """DeviceEncoder on a dense buffer of out_cap bytes (default: the bound) with guard bytes behind it
    -> (frame = buffer + guard, offsets, status, summary) on the host"""
    import torch
    assert row_major_kernel(-(-len(a) // bs)) in kernel_name(len(a), bs)
    enc = rx.DeviceEncoder(P3, bs, len(a))
    cap = enc.out_cap if out_cap is None else out_cap
    frame = torch.full((cap + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    enc.out, enc.out_cap = frame[:cap], cap
    force(rows)
    _, offs, status, summary = enc.encode(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    return frame.cpu().numpy(), offs.cpu().numpy(), status.cpu().numpy(), summary.tolist()


def check_plain(rx, nb, bs, zeros, rows, last=None):
    a, dense, want_offs, want_status = blocks(nb, bs, zeros, last)
    frame, offs, status, summary = device_encode(rx, a, bs, rows)
    assert summary == [0, 0] and status.tolist() == want_status.tolist()
    assert offs.tolist() == want_offs.tolist()
    assert frame[: len(dense)].tobytes() == dense.tobytes()
    assert (frame[len(dense):] == 0xA5).all()          # nothing behind the last stream
    return want_offs


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("nb", [64, 65, 127])
def test_small_launches(rx, nb, rows):
    check_plain(rx, nb, 2048, 108, rows)


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("bs,zeros", [(2048, 108), (1280, 78)])
def test_stream_ends_around_a_tile_edge_and_every_alignment(rx, bs, zeros, rows):
    """2,112 blocks and one of a single byte: 34 groups, the last of one stream"""
    offs = check_plain(rx, 2113, bs, zeros, rows, last=1)
    sizes = np.diff(offs)
    edge = bs                                          # 2048: 8 tiles of 64 rows, 2 of 256; 1280: 5 tiles of 64 rows
    assert edge % 256 == 0 and {edge - 4, edge, edge + 4} <= set(sizes.tolist())
    assert {int(o) & 3 for o in offs[:-1:64]} == {0, 1, 2, 3}
    assert any(sorted((offs[g: g + 4] & 3).tolist()) == [0, 1, 2, 3] for g in range(0, 2112, 64))


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("nb", [65, 2113])
def test_sixteen_byte_blocks(rx, nb, rows):
    a, dense, want_offs, want_status = blocks(nb, 16, 0, last=1)
    assert "k_encode_pair" in kernel_name(len(a), 16)
    import torch
    enc = rx.DeviceEncoder(P3, 16, len(a))
    force(rows)
    out, offs, status, summary = enc.encode(torch.from_numpy(a).cuda())
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and status.cpu().tolist() == want_status.tolist()
    assert offs.cpu().tolist() == want_offs.tolist()
    assert out[: len(dense)].cpu().numpy().tobytes() == dense.tobytes()


@functools.lru_cache(maxsize=None)
def ragged_inputs(repeat):
    """inputs of 1 byte, 16 bytes, no bytes, whole blocks and ragged tails -> (inputs, the oracle's streams end to end, offsets)"""
    bs = 2048
    rng = np.random.default_rng(repeat)
    lens = [1, 16, 3 * bs + 5, 100, bs, 2 * bs + 1, 17, 0, 5 * bs + 1000, 4] * repeat
    inputs = [rng.integers(0, 256, n, dtype=np.uint8) >> (i % 3) for i, n in enumerate(lens)]
    streams = [s for x in inputs for s in ox.compress_blocks(x, bs, P3)[0]]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])])
    return inputs, b"".join(streams), offs


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("repeat", [4, 110])
def test_block_table_with_ragged_tails_and_idle_entries(rx, repeat, rows):
    bs = 2048
    inputs, dense, want_offs = ragged_inputs(repeat)
    lens = [len(x) for x in inputs]
    tab = rx.block_table_v(np.concatenate([[0], np.cumsum(lens)[:-1]]), lens, bs)
    assert (tab["index"] == rx.BLOCK_IDLE).any() and (tab["length"][tab["index"] != rx.BLOCK_IDLE] < bs).any()
    assert {1, 16} <= set(tab["length"].tolist())
    assert row_major_kernel(len(tab)) in kernel_name(len(tab) * bs, bs) and (len(tab) > 2048) == (repeat == 110)
    force(rows)
    out, offs, status, first = rx.compress_blocks_v(inputs, bs, P3)
    assert not status.any() and offs.tolist() == want_offs.tolist()
    assert out.tobytes() == dense


@functools.lru_cache(maxsize=None)
def half_stored():
    """2,113 blocks of 2048 bytes, iid (stored: they code to more than 2048 bytes) and 6-bit (coded) in runs of 1 to 3
    -> (input, expected dense bytes, offsets, flags)"""
    bs, nb = 2048, 2113
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (nb, bs), dtype=np.uint8)
    soft = (np.cumsum(rng.integers(1, 4, nb)) // 3) % 2 == 0
    a[soft] >>= 2
    a = a.reshape(-1)
    out, sizes, status, slot = ox.compress_blocks_raw(a, bs, P3)
    flags = rule(status, [int(s) for s in sizes], [bs] * nb, 65536).astype(np.uint8)
    parts = [a[b * bs: (b + 1) * bs] if flags[b] else out[b * slot: b * slot + int(sizes[b])] for b in range(nb)]
    return a, np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]), flags


@pytest.mark.parametrize("rows", TILES)
def test_stored_blocks_mixed_in(rx, rows):
    a, dense, want_offs, want_flags = half_stored()
    assert 500 < int(want_flags.sum()) < 1600 and len({tuple(want_flags[g: g + 64]) for g in range(0, 2112, 64)}) > 8
    flags = np.full(len(want_flags), 0xEE, dtype=np.uint8)
    force(rows)
    out, offs, status = rx.compress_blocks(a, 2048, P3, stored=flags, store_ratio=65536)
    assert flags.tolist() == want_flags.tolist() and not status.any()
    assert offs.tolist() == want_offs.tolist() and out.tobytes() == dense.tobytes()


@pytest.mark.parametrize("rows", TILES)
@pytest.mark.parametrize("nb", [127, 2113])
def test_a_dense_buffer_one_byte_short_of_the_last_block(rx, nb, rows):
    from redux_amd import _lib
    a, dense, want_offs, want_status = blocks(nb, 2048, 108, None if nb == 127 else 1)
    frame, offs, status, summary = device_encode(rx, a, 2048, rows, out_cap=len(dense) - 1)
    assert summary == [_lib.OUTPUT_TOO_SMALL, 1]
    assert status.tolist() == [0] * (nb - 1) + [_lib.OUTPUT_TOO_SMALL]
    assert offs.tolist() == want_offs.tolist()
    start = int(want_offs[nb - 1])
    assert frame[:start].tobytes() == dense[:start].tobytes()
    assert (frame[start:] == 0xA5).all()               # reported, never written: the last block's bytes and the guard
