"""Every adaptive coder instance on the inputs that force its rare paths (the table and the inputs:
tests/test_adaptive_instances_cpu.py).

One launch per (instance id, input family).  A case first asserts, by name, that its launch runs the encode and decode
instance the id promises.  The launch is tiled on the device from four distinct blocks, each coded once by the oracle:
two ordinary blocks (seeded skewed bytes), the hard block H (the family's input + a seeded tail up to the block length: its
pending run is flushed inside the unrolled loop) and R, the family's exact input as the ragged last block of the launch
(flushed at EOF; the shortest block of its wave).  Every id runs in two forms: "partial", where R is the fifth lane of a
partial last wave, and "whole", five blocks fewer, where R is the last lane of a whole wave and ends that wave's unrolled
path.  Every launch has at least five whole spans of 64 blocks, and layout() asserts each placement.  H sits
  * alone in its wave at lane 0 of span 0, lane G/2 - 1 of span 1, lane G/2 of span 2 and lane G - 1 of span 3 (one bit of
    the redo / careful-path ballot, the other lanes repeating ordinary symbols), G = 64 blocks per wave, or 32 / 16 for
    k_encode_gen_pair<11> / <12>;
  * in all 64 blocks of span 4 (whole waves of hard blocks);
  * at the last lane of the last whole wave before R's and next to R; pair_wide also in groups 256 and 265 (a second
    workgroup of a CU).
Checked: offsets are the running sum of the oracle's stream sizes, every block's stream is byte-identical to the oracle's,
status all zero; the paired decoder gives the oracle's decode of each stream (for widths that do not divide the block the
oracle drops the trailing bits); neither call touches the 256-byte guard bands of 0xA5 around the input, the encode output
and the decode output.
Then the damaged form: H's stream with one flipped bit, cut at a third and with a damaged dword in lanes 5, 31 and 32 of a
wave of intact streams: status, size and bytes per block equal the oracle's."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox
from test_adaptive_instances_cpu import TARGETS, byte_families, dec_name, enc_name, gen_families, ws_bytes

pytestmark = pytest.mark.gpu

GUARD, FILL = 256, 0xA5
O1, O2, H, R = 0, 1, 2, 3


def _families(params):
    return byte_families() if params[0] == 8 else gen_families(params)


def _cases():
    out = []
    for key in sorted(TARGETS):
        for fam in sorted(_families(TARGETS[key][0])):
            out.append((key, fam))
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def _lib():
    from redux_amd import _lib as L
    return L


def _v(t):
    return C.c_void_p(t.data_ptr())


def guarded(n, align=0):
    """(whole tensor, view of n bytes `align` bytes off a 16-byte boundary) with GUARD bytes of FILL on either side"""
    import torch
    t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    lo = GUARD + align
    assert t.data_ptr() % 16 == 0
    return t, t[lo: lo + n], lo


def guards_intact(t, lo, n):
    return bool((t[:lo] == FILL).all()) and bool((t[lo + n:] == FILL).all())


def ordinary(n, seed):
    rng = np.random.default_rng(seed)
    return np.minimum(rng.standard_exponential(n) * 14, 255).astype(np.uint8).tobytes()


def distinct_blocks(base, bs, seed):
    """[O1, O2, H, R]: the four distinct blocks of a launch."""
    rng = np.random.default_rng(seed)
    h = base[:bs] + rng.integers(0, 256, max(0, bs - len(base)), dtype=np.uint8).tobytes()
    r = base if len(base) < bs else base[: bs * 2 // 3 + 1]
    return [ordinary(bs, seed + 1), ordinary(bs, seed + 2), h, r]


def group_width(params, enc):
    """Blocks that share a wave of the coder: 64, or 32 / 16 for k_encode_gen_pair<11> / <12> (GenTree::kBlocks)."""
    return {11: 32, 12: 16}.get(params[0], 64) if enc.startswith("k_encode_gen_pair") else 64


def layout(nb, G=64):
    """The kind of every block of a launch of nb blocks whose coder takes G blocks per wave.  Every placement the module
    docstring promises must exist: the launch has five whole spans of 64 blocks and more."""
    assert nb >= 64 * 5 + 2 and 64 % G == 0
    kinds = (np.arange(nb) % 2).astype(np.int64)
    alone = [64 * k + lane for k, lane in enumerate((0, G // 2 - 1, G // 2, G - 1))]   # one hard block in its wave (and span)
    wave = list(range(256, 320))                                                       # whole waves of hard blocks
    last = (nb - 1) // 64 * 64                                                         # first block of the last span
    ends = [last - 1] if nb % 64 else [last + 7]       # last lane of the last whole wave before R's; or beside R in a whole one
    ends += [nb - 2] if nb % 64 else []
    wide = [b for b in (256 * 64 + 17, 265 * 64 + 40) if b < last - 64]
    for b in alone + wave + ends + wide:
        assert 0 <= b < nb - 1
        kinds[b] = H
    kinds[nb - 1] = R
    for b in alone:                                    # alone: no other hard block in the same wave
        assert (kinds[b // G * G: b // G * G + G] == H).sum() == 1
    assert (kinds[256:320] == H).all()
    return kinds


def oracle_streams(blocks, params, bs):
    """Per distinct block: (stream, (status, decoded bytes) of the oracle's decode into a block of bs bytes)."""
    out = []
    for b in blocks:
        s, _ = ox.compress(b, params, cap=4 * len(b) + 4096)
        st, dec, used = ox.decompress_raw(s, bs, params)
        whole = len(b) * 8 // params[0] * params[0] // 8      # (a partial last symbol is never coded; its byte is zero-padded)
        assert st == 0 and used == len(s) and dec[:whole] == b[:whole] and whole <= len(dec) <= len(b)
        out.append((s, dec))
    return out


def first_difference(got, want):
    g, w = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
    n = min(len(g), len(w))
    d = np.nonzero(g[:n] != w[:n])[0]
    return int(d[0]) if len(d) else n


def compare_rows(flat, starts, want, what):
    """flat[starts[i]: starts[i] + len(want)] == want for every i (on the device, in chunks)."""
    import torch
    if not len(want) or not starts.numel():
        return
    e = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()
    ar = torch.arange(len(want), device="cuda:0")
    step = max(1, (16 << 20) // len(want))
    for i in range(0, starts.numel(), step):
        st = starts[i: i + step]
        got = flat[st[:, None] + ar[None, :]]
        bad = (got != e[None, :]).any(1)
        if bool(bad.any()):
            j = int(bad.nonzero()[0])
            row = got[j].cpu().numpy().tobytes()
            raise AssertionError(f"{what}: row {i + j} (start {int(st[j])}) differs at byte {first_difference(row, want)} of {len(want)}")


def encode_dev(params, bs, nb, align, ws, d_in, in_len):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    wsb = ws_bytes(params, bs, nb, ws)
    wst = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    wsp = (wst.data_ptr() + 255) // 256 * 256
    cap = lib.redux_encode_bound(C.byref(cp), in_len, bs)
    big, out, lo = guarded(cap)
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_encode_blocks_dev(C.byref(cp), _v(d_in), in_len, bs, _v(out), cap, _v(offs), _v(status), _v(summ), C.c_void_p(wsp),
                                     wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, cap)
    return out, offs, status, summ


def decode_dev(params, bs, nb, d_streams, d_offs):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    wsb = lib.redux_decode_workspace_bytes(C.byref(cp), nb, bs)
    wst = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    wsp = (wst.data_ptr() + 255) // 256 * 256
    big, out, lo = guarded(nb * bs)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_decode_blocks_dev(C.byref(cp), _v(d_streams), _v(d_offs), nb, bs, _v(out), nb * bs, _v(sizes), _v(status),
                                     _v(summ), C.c_void_p(wsp), wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, nb * bs)
    return out, sizes, status


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_the_comparison_sees_one_wrong_byte():
    """compare_rows over rows at uneven starts: equal rows pass, one changed byte in one row is reported with its place."""
    import torch
    want = ordinary(5000, 3)
    gaps = [0, 7, 1, 4096, 13] * 40
    starts = np.cumsum([g + len(want) for g in gaps]) - len(want)
    flat = np.full(int(starts[-1]) + len(want) + 9, FILL, dtype=np.uint8)
    for o in starts:
        flat[o: o + len(want)] = np.frombuffer(want, dtype=np.uint8)
    d = torch.from_numpy(flat).cuda()
    compare_rows(d, torch.from_numpy(starts).cuda(), want, "self-check")
    d[int(starts[133]) + 4321] ^= 0x10
    with pytest.raises(AssertionError, match="row 133 .* differs at byte 4321 of 5000"):
        compare_rows(d, torch.from_numpy(starts).cuda(), want, "self-check")


def _seed(key, fam):
    return sum(map(ord, key + fam))


# "partial": the table's block count, R in a partial last wave of 5 lanes; "whole": 5 blocks fewer, R the last lane of a
# whole wave (the gen kernels run their unrolled path in whole waves only: there R ends it).  pair_wide: partial only.
ENCODE_CASES = [(k, f, form) for k, f in CASES if TARGETS[k][5] is not None for form in ("partial", "whole")
                if not (form == "whole" and k == "pair_wide_8_30_32")]


@pytest.mark.parametrize("key,fam,form", ENCODE_CASES)
def test_instance_on_rare_path_input(rx, key, fam, form):
    import torch
    params, bs, nb, align, ws, enc, dec = TARGETS[key]
    nb -= 5 if form == "whole" else 0
    base = _families(params)[fam]
    blocks = distinct_blocks(base, bs, _seed(key, fam))
    kinds = layout(nb, group_width(params, enc))
    in_len = (nb - 1) * bs + len(blocks[R])
    big_in, d_in, lo_in = guarded(in_len, align)
    # the instance the id promises, for the very pointer, length and workspace of this launch
    L = _lib()
    name = L.lib().redux_encode_kernel_name_ws(C.byref(L.Params(*params)), _v(d_in), in_len, bs, ws_bytes(params, bs, nb, ws)).decode()
    assert name == enc == enc_name(params, bs, nb, align, ws, in_len=in_len)
    assert dec_name(params, bs, nb) == dec
    assert d_in.data_ptr() % 16 == align

    d_kinds = torch.from_numpy(kinds).cuda()
    full = torch.from_numpy(np.frombuffer(b"".join(blocks[:3]), dtype=np.uint8).copy()).cuda().view(3, bs)
    d_in[: (nb - 1) * bs].view(nb - 1, bs).copy_(full[d_kinds[:-1]])
    d_in[(nb - 1) * bs:].copy_(torch.from_numpy(np.frombuffer(blocks[R], dtype=np.uint8).copy()))
    del full
    want = oracle_streams(blocks, params, bs)

    out, offs, status, summ = encode_dev(params, bs, nb, align, ws, d_in, in_len)
    assert guards_intact(big_in, lo_in, in_len)
    assert summ.tolist() == [0, 0] and not bool(status.any())
    lens = torch.tensor([len(s) for s, _ in want], dtype=torch.int64, device="cuda:0")[d_kinds]
    exp_offs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(lens, 0)])
    if not torch.equal(offs, exp_offs):
        b = int(((offs[1:] - offs[:-1]) != lens).nonzero()[0])
        raise AssertionError(f"block {b} (kind {int(kinds[b])}): {int(offs[b + 1] - offs[b])} stream bytes, the oracle's has {int(lens[b])}")
    for k, (s, _) in enumerate(want):
        idx = (d_kinds == k).nonzero().flatten()
        compare_rows(out, exp_offs[idx], s, f"encode, kind {k}, blocks {idx[:4].tolist()}...")

    d_out, sizes, dstatus = decode_dev(params, bs, nb, out, offs)
    assert not bool(dstatus.any())
    dlens = torch.tensor([len(d) for _, d in want], dtype=torch.int32, device="cuda:0")[d_kinds]
    assert torch.equal(sizes, dlens)
    for k, (_, d) in enumerate(want):
        idx = (d_kinds == k).nonzero().flatten()
        compare_rows(d_out, idx * bs, d, f"decode, kind {k}")
    del big_in, d_in, out, d_out
    _free()


def damaged(stream, seed):
    rng = np.random.default_rng(seed)
    flip = bytearray(stream)
    flip[int(rng.integers(0, max(1, len(flip) // 3)))] ^= 1 << int(rng.integers(0, 8))
    cut = stream[: len(stream) // 3]
    dword = bytearray(stream)
    j = int(rng.integers(0, max(1, len(dword) - 4)))
    dword[j: j + 4] = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
    return [bytes(flip), cut, bytes(dword)]


@pytest.mark.parametrize("key,fam", CASES)
def test_decoder_on_damaged_rare_path_streams(rx, key, fam):
    import torch
    params, bs, nb, _, _, _, dec = TARGETS[key]
    nbd = nb if bs > 65536 else min(nb, 130)          # (the launch size picks the decoder of blocks above 64 KiB only)
    assert dec_name(params, bs, nbd) == dec
    blen = min(bs, 200_000)
    blocks = distinct_blocks(_families(params)[fam], blen, _seed(key, fam))
    good = [ox.compress(b, params, cap=4 * len(b) + 4096)[0] for b in blocks]
    bad = damaged(good[H], _seed(key, fam) + 5)
    streams = good + bad                                # kinds 0 .. 3 intact, 4 .. 6 damaged
    kinds = np.arange(nbd) % 2
    for lane, k in ((5, 4), (31, 5), (32, 6), (63, H), (0, H), (nbd - 1, R), (nbd - 2, 4)):
        if 0 <= lane < nbd:
            kinds[lane] = k
    expect = []
    for s in streams:
        st, d, _ = ox.decompress_raw(s, bs, params)
        expect.append((4 if st == ox.IO_ERROR else st, d))
    assert [e[0] for e in expect[:4]] == [0, 0, 0, 0]
    offs = np.zeros(nbd + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(streams[k]) for k in kinds])
    dense = np.frombuffer(b"".join(streams[k] for k in kinds), dtype=np.uint8).copy()
    big, d_in, lo = guarded(dense.size)
    d_in.copy_(torch.from_numpy(dense))
    d_out, sizes, status = decode_dev(params, bs, nbd, d_in, torch.from_numpy(offs).cuda())
    assert guards_intact(big, lo, dense.size)
    d_kinds = torch.from_numpy(kinds).cuda()
    want_st = torch.tensor([e[0] for e in expect], dtype=torch.int32, device="cuda:0")[d_kinds]
    want_sz = torch.tensor([len(e[1]) for e in expect], dtype=torch.int32, device="cuda:0")[d_kinds]
    if not (torch.equal(status, want_st) and torch.equal(sizes, want_sz)):
        b = int(((status != want_st) | (sizes != want_sz)).nonzero()[0])
        raise AssertionError(f"block {b} (kind {int(kinds[b])}): status {int(status[b])}, size {int(sizes[b])}; the oracle's "
                             f"{int(want_st[b])}, {int(want_sz[b])}")
    for k, (_, d) in enumerate(expect):
        idx = (d_kinds == k).nonzero().flatten()
        compare_rows(d_out, idx * bs, d, f"decode, kind {k}")
    del big, d_in, d_out
    _free()
