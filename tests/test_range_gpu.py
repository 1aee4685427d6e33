"""Range reads on the GPU: k_segment_copy against numpy at every pair of phases, container.Reader on every container kind the
writers produce, what damage a range read does and does not notice, DeviceDecoder.decode_ranges against slices of decode(), and
the command line's --range."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
B = 4096
FILL = 0xA5


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- k_segment_copy ----------------------------------------------------------------------------------------------------------
def copy_and_check(rx, segs, src_bytes, dst_bytes, so=0, do=0):
    """one call on buffers whose own addresses sit so / do bytes past a 16-byte boundary; the whole destination, guard bytes
    between and around the segments included, against numpy"""
    import torch
    rng = np.random.default_rng(len(segs) + src_bytes)
    src = rng.integers(0, 256, src_bytes, dtype=np.uint8)
    d_src = torch.empty(src_bytes + 32, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty(dst_bytes + 32, dtype=torch.uint8, device="cuda")
    d_src = d_src[(-d_src.data_ptr()) % 16 + so:][:src_bytes]
    d_dst = d_dst[(-d_dst.data_ptr()) % 16 + do:][:dst_bytes]
    d_src.copy_(torch.from_numpy(src))
    d_dst.fill_(FILL)
    want = np.full(dst_bytes, FILL, dtype=np.uint8)
    for s, d, n in segs:
        want[d: d + n] = src[s: s + n]
    assert rx.segment_copy(d_src, d_dst, segs) is d_dst
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8].tolist(), len(bad))


def test_every_pair_of_phases(rx):
    lens = (1, 15, 16, 17, 100, 4099)
    segs, at = [], 0
    for sp in range(16):
        for dp in range(16):
            for n in lens:
                segs.append((16 * (len(segs) % 61) + sp, at + 16 + dp, n))
                at += (16 + dp + n + 16 + 15) // 16 * 16  # (at least 16 guard bytes on either side)
    assert len(segs) == 16 * 16 * len(lens)
    copy_and_check(rx, segs, 16 * 61 + 16 + 4099, at + 16)
    copy_and_check(rx, segs[::7], 16 * 61 + 16 + 4099, at + 16, so=5, do=11)  # (buffers that are themselves misaligned)


def test_tile_seams(rx):
    segs, at = [], 0
    for n in (65535, 65536, 65537, 131071):
        for sp, dp in ((0, 0), (1, 0), (0, 1), (7, 13), (15, 3), (4, 8)):
            segs.append((sp + 32 * len(segs), at + 16 + dp, n))
            at += (16 + dp + n + 16 + 15) // 16 * 16
    assert len(rx.segment_tiles(segs)) > len(segs)
    copy_and_check(rx, segs, 131071 + 32 * len(segs) + 16, at + 16, so=3, do=9)


def test_a_thousand_random_segments_and_none(rx):
    rng = np.random.default_rng(1000)
    src_bytes = 1 << 20
    segs, at = [], 0
    for _ in range(1000):
        n = int(rng.integers(0, 3000)) if rng.integers(0, 8) else int(rng.integers(60000, 70000)) * int(rng.integers(0, 2))
        at += int(rng.integers(0, 40))
        segs.append((int(rng.integers(0, src_bytes - n + 1)), at, n))
        at += n
    order = rng.permutation(len(segs))
    copy_and_check(rx, [segs[i] for i in order], src_bytes, at + 7, so=1, do=2)
    copy_and_check(rx, [], 64, 64)
    copy_and_check(rx, [(3, 5, 0), (64, 64, 0)], 64, 64)
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for bad in ([(0, 0, 65)], [(0, 0, 8), (8, 7, 8)]):
        with pytest.raises(rx.InvalidInput):
            rx.segment_copy(torch.zeros(64, dtype=torch.uint8, device="cuda"), d, bad)
    with pytest.raises(rx.InvalidInput):
        rx.segment_copy(d[:32], d[16:], [(0, 0, 8)])  # (the buffers overlap)


# ---- container range reads ---------------------------------------------------------------------------------------------------
def typed(E, nbytes, seed):
    """a slowly varying integer series of element size E (so that every layout and filter has something to gain) whose third
    frame of E blocks of 4096 bytes, and 5 bytes more, is zero (so that some blocks are constant in every layout)"""
    rng = np.random.default_rng(seed)
    n = nbytes // E + 1
    v = np.cumsum(rng.integers(-40, 41, n)).astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[E])
    a = v.view(np.uint8)[:nbytes].copy()
    a[2 * E * B: 3 * E * B + 5] = 0
    return a


def mixed_data():
    """four parts of different dtype: 3 units + 5 blocks + 3 bytes"""
    cuts = (9 * B, 16 * B, 24 * B, 29 * B + 3)
    parts, lo = [], 0
    for E, hi in zip((2, 4, 8, 1), cuts):
        parts.append(typed(E, hi - lo, 40 + E))
        lo = hi
    return np.concatenate(parts)


KINDS = {
    "v1": dict(E=1), "v2": dict(E=4, element_size=4), "v3": dict(E=1, model="static"),
    "v4": dict(E=2, element_size=2, model="plane-static"), "v5": dict(E=1, model="segment-static", segment_blocks=64, B=1024),
    "v5e2": dict(E=2, element_size=2, model="segment-static", segment_blocks=128, B=1024),
    "v6": dict(E=4, element_size=4, filter="delta"), "v7": dict(E=1, model="context-static"),
    "v8": dict(E=2, element_size=2, base=True), "v9": dict(E=4, element_size=4, skip_constant=True),
    "v9base": dict(E=2, element_size=2, skip_constant=True, base=True), "v10": dict(E=1, layout="mixed", element_size=None),
    "0x41": dict(E=1, stored=True), "0x42": dict(E=2, element_size=2, stored=True),
    # the frame-local prefix-sum filters that came after the sweep: zigzag, the folded difference against a base, lag, lag order
    "v11": dict(E=2, element_size=2, filter="zigzag"), "v12": dict(E=4, element_size=4, base=True, base_op="sub"),
    "v13": dict(E=2, element_size=2, filter="lag", lag=3), "v14": dict(E=8, element_size=8, filter="lag", lag=2, order=3),
    # the record layout, with and without its byte delta: the granule is a frame of record_size blocks
    "v15": dict(E=1, record_size=23, filter="delta"), "v15plain": dict(E=1, record_size=5),
}
ALL_KINDS = list(KINDS) + [k + "+crc" for k in KINDS]  # (0x41 + 0x10 = 0x51, ...)
VERSION_BYTE = {"v11": 11, "v12": 12, "v13": 13, "v14": 14, "v15": 15, "v15plain": 15}  # (+crc: 0x1B, 0x1C, 0x1D, 0x1E, 0x1F)


@functools.lru_cache(maxsize=None)
def made(kind):
    """(container bytes, the data, the base or None, the granule's bytes F, the block size): compressed once per kind"""
    from redux_amd import container
    kw = dict(KINDS[kind.replace("+crc", "")])
    E, bs = kw.pop("E"), kw.pop("B", B)
    if "layout" in kw:
        data, F = mixed_data(), 8 * bs
    elif "segment_blocks" in kw:
        F = kw["segment_blocks"] * bs
        data = typed(E, 2 * F + 9 * bs + 3, 7)  # two segments and a short third
    else:
        F = kw.get("record_size", E) * bs       # (the record layout: E is 1, a frame is record_size blocks)
        data = typed(E, 5 * F + bs + 3, E)      # a short last frame of more than one block, with trailing bytes
    if kind.startswith("0x4"):                  # (bytes that do not shrink, so that blocks are stored)
        data[F: 3 * F] = np.random.default_rng(3).integers(0, 256, 2 * F, dtype=np.uint8)
    base = None
    if kw.pop("base", False):                   # an earlier snapshot, shorter than the data: the XOR ends inside a frame;
        base = data[: 3 * F + 100].copy()       # it differs in the first frame only, so the XOR of the next two is constant
        base[:F:997] ^= 0x10
    blob = container.compress_bytes(data.tobytes(), bs, P, checksum=kind.endswith("+crc"), base=None if base is None else base.tobytes(),
                                    **kw)
    return blob, data.tobytes(), None if base is None else base.tobytes(), F, bs


def the_ranges(total, F):
    """the issue's ranges; the last one is cut at the end of the data where the data has fewer than 4 F + 3 bytes (the mixed and
    the segment-static files: 3.6 and 2.1 granules)"""
    return [(0, 0), (0, 1), (0, total), (total - 1, 1), (total - 5, 5), (total, 0), (F - 1, 2), (F + 7, 1),
            (2 * F + 3, min(2 * F, total - 2 * F - 3))]


@pytest.mark.parametrize("kind", ALL_KINDS)
def test_every_container_kind_reads_by_range(rx, kind):
    from redux_amd import container
    blob, data, base, F, bs = made(kind)
    total = len(data)
    assert blob[4] & 0x10 == (0x10 if kind.endswith("+crc") else 0) and blob[4] & 0x40 == (0x40 if kind.startswith("0x4") else 0)
    if kind.replace("+crc", "") in VERSION_BYTE:
        assert blob[4] == VERSION_BYTE[kind.replace("+crc", "")] + (0x10 if kind.endswith("+crc") else 0)
    r = container.Reader(blob, base)
    assert (r.total, r.block_size, r.granule_blocks * bs) == (total, bs, F)
    ranges = the_ranges(total, F)
    for s, n in ranges:
        before = r.bytes_read
        assert r.read(s, n) == data[s: s + n], (s, n)
        assert n == 0 or r.bytes_read - before <= len(blob) - r.payload_offset
    # all together, unsorted, with a duplicate and an overlapping pair, in one call
    many = [ranges[i] for i in (8, 3, 0, 6, 2, 7, 4, 1, 5)] + [ranges[6], (F, 9)]
    assert r.read_many(many) == [data[s: s + n] for s, n in many]
    small = [(F + 7, 1), (total - 1, 1)]  # (two granules of the file: less than the whole payload is fetched)
    before = r.bytes_read
    assert r.read_many(small) == [data[s: s + n] for s, n in small] and r.bytes_read - before < len(blob) - r.payload_offset
    for s, n in ((total, 1), (2 ** 63, 2 ** 63)):
        with pytest.raises(rx.InvalidInput):
            r.read(s, n)
    assert container.decompress_range(blob, F - 1, 2, base=base) == data[F - 1: F + 1]


DAMAGED = ["v1+crc", "v2+crc", "v9base+crc", "v10+crc", "v12+crc", "v14+crc", "v15+crc", "v15plain+crc"]


@pytest.mark.parametrize("kind", DAMAGED)
def test_damage_matters_only_where_a_range_reads(rx, kind):
    from redux_amd import container
    blob, data, base, F, bs = made(kind)
    c = container._parse(blob)
    head = len(blob) - len(c.payload)
    g = F // bs
    rng_ = (F + 7, 9)                                   # granule 1: blocks g .. 2 g - 1
    far, near = 3 * g, g                                # (the first byte of a stream, or a constant block's one byte)
    bad = bytearray(blob)
    bad[head + int(c.offsets[far])] ^= 0xFF             # an uncovered block
    assert container.Reader(bytes(bad), base).read(*rng_) == data[F + 7: F + 16]
    with pytest.raises(rx.Error):
        container.decompress_bytes(bytes(bad), base)
    bad = bytearray(blob)
    bad[head + int(c.offsets[near])] ^= 0xFF            # a covered one
    with pytest.raises(rx.Error):
        container.Reader(bytes(bad), base).read(*rng_)
    assert container.Reader(blob, base).read(*rng_) == data[F + 7: F + 16]


# ---- streams resident in device memory ---------------------------------------------------------------------------------------
MODES = {"plain": dict(E=1), "planes": dict(E=4, element_size=4), "delta": dict(E=8, element_size=8, filter="delta"),
         "base": dict(E=2, element_size=2, base=True), "constant": dict(E=2, element_size=2, constant=True),
         "constant+base": dict(E=4, element_size=4, constant=True, base=True), "mixed": dict(E=1, mixed=True),
         # the gathered virtual input (covered granules concatenated, a short last frame, the gathered prefix of a base that
         # ends 100 bytes into a frame) behind the frame-local prefix-sum filters
         "zigzag": dict(E=1, filter="zigzag"), "base_sub": dict(E=8, element_size=8, base=True, base_op="sub"),
         "lag": dict(E=4, element_size=4, filter="lag", lag=5), "lag_order": dict(E=2, element_size=2, filter="lag", lag=3, order=2),
         # the record layout: frames of 23 blocks; the short last frame holds 178 records and 5 trailing bytes
         "record": dict(E=1, record_size=23, filter="delta")}


@pytest.mark.parametrize("mode", list(MODES))
def test_decode_ranges_equals_slices_of_decode(rx, mode):
    import torch
    kw = dict(MODES[mode])
    E = kw.pop("E")
    F = (8 if mode == "mixed" else kw.get("record_size", E)) * B
    x = mixed_data() if mode == "mixed" else typed(E, 5 * F + B + 3, 20 + E)
    n = len(x)
    d_in = torch.from_numpy(x).cuda()
    if kw.pop("base", False):
        y = x[: 3 * F + 100].copy()
        y[:F:501] ^= 3                                                             # (byte 0 differs: block 0 is no constant block)
        kw["base"] = torch.from_numpy(y).cuda()
    enc = rx.DeviceEncoder(P, B, n, **kw)
    res = enc.encode(d_in)
    out, offs, summary = res[0], res[1], res[3]
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    extra = {"constant": res[4]} if kw.get("constant") else {"unit_layouts": res[4]} if mode == "mixed" else {}
    if kw.get("constant"):
        assert 0 < int(res[4].sum()) < res[4].numel()
    d_streams = out[: int(offs[-1])].clone()
    nb = offs.numel() - 1
    dec = rx.DeviceDecoder(P, B, nb, **kw)
    whole = dec.decode(d_streams, offs, length=n, **extra)[0].clone()
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy(), x)
    ranges = the_ranges(n, F)
    ranges = [ranges[i] for i in (8, 3, 0, 6, 7, 4, 1, 5)] + [ranges[6], (F, 9)]  # (without the whole input: see below)
    total = sum(k for _, k in ranges)
    big = torch.full((total + 64,), FILL, dtype=torch.uint8, device="cuda")
    at = (-big.data_ptr()) % 16 + 17                                               # an odd byte offset
    got, where = dec.decode_ranges(d_streams, offs, n, ranges, out=big[at: at + total], **extra)
    torch.cuda.synchronize()
    assert got.data_ptr() == big.data_ptr() + at and where == np.cumsum([0] + [k for _, k in ranges])[:-1].tolist()
    h = big.cpu().numpy()
    assert (h[:at] == FILL).all() and (h[at + total:] == FILL).all()
    assert h[at: at + total].tobytes() == b"".join(x[s: s + k].tobytes() for s, k in ranges)
    # host offsets, a new output, the whole input among the ranges, and ranges without bytes
    got, where = dec.decode_ranges(d_streams, offs.cpu().numpy(), n, [(F + 7, 1), (0, n), (n - 5, 5)], **extra)
    torch.cuda.synchronize()
    assert where == [0, 1, n + 1] and got.cpu().numpy().tobytes() == x[F + 7: F + 8].tobytes() + x.tobytes() + x[n - 5:].tobytes()
    got, where = dec.decode_ranges(d_streams, offs, n, [(0, 0), (n, 0)], **extra)
    assert got.numel() == 0 and where == [0, 0]
    for bad in ([(n, 1)], [(2 ** 63, 2 ** 63)]):
        with pytest.raises(rx.InvalidInput):
            dec.decode_ranges(d_streams, offs, n, bad, **extra)
    # block 0 cut to one byte of its stream: a range that covers it raises, one that does not reads on
    h_offs = offs.cpu().numpy()
    cut = int(h_offs[1]) - 1
    assert cut > 0
    hurt = torch.cat([d_streams[:1], d_streams[int(h_offs[1]):]])
    hurt_offs = np.concatenate([[0], h_offs[1:] - cut])
    with pytest.raises(rx.Error):
        dec.decode_ranges(hurt, hurt_offs, n, [(3, 5)], **extra)
    ok, _ = dec.decode_ranges(hurt, hurt_offs, n, [(F + 7, 5)], **extra)
    assert ok.cpu().numpy().tobytes() == x[F + 7: F + 12].tobytes()
    small = rx.DeviceDecoder(P, B, F // B, **kw)                                  # room for one granule
    assert small.decode_ranges(d_streams, offs, n, [(F + 7, 5)], **extra)[0].cpu().numpy().tobytes() == x[F + 7: F + 12].tobytes()
    with pytest.raises(rx.InvalidInput):
        small.decode_ranges(d_streams, offs, n, [(F - 1, 2)], **extra)            # two granules


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_cli_range(rx, tmp_path, capsys):
    from redux_amd import cli
    blob, data, base, F, bs = made("v8+crc")
    src, basef, dst = tmp_path / "in.rdx", tmp_path / "base", tmp_path / "out"
    src.write_bytes(blob)
    basef.write_bytes(base)
    assert cli.main(["-d", "-i", str(src), "-o", str(dst), "--base", str(basef), "--range", "%d:%d" % (F + 7, 2 * F)]) == 0
    assert dst.read_bytes() == data[F + 7: 3 * F + 7]
    err = capsys.readouterr().err
    read = int(err.split(" bytes from ")[1].split()[0])
    assert err.startswith("Decompressed %d bytes from " % (2 * F)) and 32 < read < len(blob)
    assert cli.main(["-d", "-i", str(src), "-o", str(dst), "--base", str(basef), "--range", "%d:0" % len(data)]) == 0
    assert dst.read_bytes() == b""
    assert cli.main(["-d", "-i", str(src), "-o", str(dst), "--base", str(basef), "--range", "%d:1" % len(data)]) == 3  # past the end
    assert cli.main(["-d", "-i", str(src), "-o", str(dst), "--range", "0:1"]) == 3                                     # no base
    raw = tmp_path / "raw"
    assert cli.main(["-c", "-i", str(basef), "-o", str(raw)]) == 0                                                    # a raw stream
    assert cli.main(["-d", "-i", str(raw), "-o", str(dst), "--range", "0:1"]) == 3
    assert cli.main(["-d", "-i", str(tmp_path / "missing"), "--range", "0:1"]) == 2
