"""Range reads without a GPU: the plan of the covered granules (redux_range_plan) against a brute-force model, the tile cut of
the segmented copy and its host-side refusals, container.Reader on containers packed from oracle-coded blocks with the coder
call replaced by a recording stub, and the command line's --range."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from redux_amd import _lib, api, cli, container

PARAMS = (8, 30, 32)


# ---- redux_range_plan --------------------------------------------------------------------------------------------------
def plan_model(total, B, g, ranges):
    """mark the covered granules, cumulative-sum their sizes"""
    nb = max(1, -(-total // B))
    ng = -(-nb // g)
    size = np.array([min((j + 1) * g * B, total) - min(j * g * B, total) for j in range(ng)], dtype=np.int64)
    covered = np.zeros(ng, dtype=bool)
    for s, n in ranges:
        if n:
            covered[s // (g * B): (s + n - 1) // (g * B) + 1] = True
    before = np.concatenate([[0], np.cumsum(size * covered)])  # virtual bytes in front of granule j
    runs = []
    for j in np.flatnonzero(covered):
        if runs and runs[-1][0] + runs[-1][1] == j:
            runs[-1][1] += 1
        else:
            runs.append([int(j), 1])
    off = [int(before[s // (g * B)] + s - (s // (g * B)) * g * B) if n else 0 for s, n in ranges]
    return [tuple(r) for r in runs], off, int(before[-1])


def random_ranges(rng, total):
    k = int(rng.integers(0, 7))
    out = []
    for _ in range(k):
        s = int(rng.integers(0, total + 1))
        n = int(rng.integers(0, min(total - s, 3000) + 1)) if rng.integers(0, 5) else 0
        out.append((s, n))
    if out and rng.integers(0, 2):
        out.append(out[0])  # a duplicate
    if out and rng.integers(0, 2):
        s, n = out[-1]
        out.append((max(0, s - 5), min(total - max(0, s - 5), n + 9)))  # an overlapping one
    rng.shuffle(out)
    return [tuple(r) for r in out]


@pytest.mark.parametrize("g", [1, 2, 8, 64])
def test_plan_matches_the_brute_force_model(g):
    B = 16
    rng = np.random.default_rng(100 + g)
    for total in (4 * g * B, 4 * g * B + 1, 4 * g * B - 1, B - 3, 0):
        sets = [random_ranges(rng, total) for _ in range(40)]
        sets += [[], [(0, 0)], [(total, 0)], [(0, total)], [(total - 1, 1)] if total else []]
        for ranges in sets:
            runs, off, vlen = api.range_plan(total, B, g, ranges)
            assert (runs, off, vlen) == plan_model(total, B, g, ranges), (total, g, ranges)
            assert len(runs) <= len(ranges)


def test_plan_refusals_and_wide_values():
    L = _lib.lib()

    def call(total, B, g, starts, lens):
        s, n = np.array(starts, dtype=np.uint64), np.array(lens, dtype=np.uint64)
        f, c, o = (np.zeros(len(s) + 1, dtype=np.uint64) for _ in range(3))
        nr, vl = C.c_uint64(), C.c_uint64()
        return L.redux_range_plan(total, B, g, s.ctypes.data, n.ctypes.data, len(s), f.ctypes.data, c.ctypes.data, C.byref(nr),
                                  o.ctypes.data, C.byref(vl))
    assert call(100, 16, 2, [0, 100], [100, 0]) == _lib.OK
    assert call(100, 16, 2, [101], [0]) == _lib.INVALID_INPUT                  # start > total
    assert call(100, 16, 2, [90], [11]) == _lib.INVALID_INPUT                  # start + len > total
    assert call(2 ** 64 - 1, 16, 2, [2 ** 63], [2 ** 63]) == _lib.INVALID_INPUT  # ... by an overflowing sum
    assert call(100, 0, 2, [0], [1]) == _lib.INVALID_INPUT
    assert call(100, 16, 0, [0], [1]) == _lib.INVALID_INPUT
    for bad in ([(100, 1)], [(2 ** 63, 2 ** 63)], [(-1, 2)], [(0, 2 ** 64)], [(1,)], ["ab"]):
        with pytest.raises(api.InvalidInput):
            api.range_plan(100, 16, 2, bad)
    # granules as long as 64 bits hold: one granule, the whole input
    assert api.range_plan(2 ** 40, 2 ** 31, 2 ** 62, [(5, 7), (2 ** 39, 1)]) == ([(0, 1)], [5, 2 ** 39], 2 ** 40)
    assert api.range_plan(2 ** 50 + 3, 65536, 8, [(2 ** 50, 3)]) == ([(2 ** 31, 1)], [0], 3)


# ---- the tiles of the segmented copy ---------------------------------------------------------------------------------------
def test_tiles_cover_every_segment_in_order():
    rng = np.random.default_rng(7)
    segs = [(3, 5, 0), (1, 7, 1), (0, 16, 65536), (9, 100001, 65537), (5, 300003, 65535), (2, 500000, 131071),
            (11, 700013, 400000), (0, 1200000, 65536 * 3)]
    segs += [(int(rng.integers(0, 1 << 20)), 2000000 + 300000 * i + int(rng.integers(0, 16)), int(rng.integers(0, 250000)))
             for i in range(30)]
    tiles = api.segment_tiles(segs)
    assert tiles.dtype == api.SEGMENT_DTYPE and api.SEGMENT_DTYPE.itemsize == 24
    t = 0
    for src, dst, n in segs:
        done = 0
        while done < n:
            ts, td, tn = (int(v) for v in tiles[t])
            assert (ts, td) == (src + done, dst + done) and 0 < tn <= 65536 and done + tn <= n
            assert done == 0 or td % 16 == 0           # every tile but the segment's first: an aligned destination
            assert done + tn == n or tn >= 65536 - 15  # and no cut that is not needed
            done += tn
            t += 1
    assert t == len(tiles)
    L = _lib.lib()
    a = api._segments_arg(segs)
    assert L.redux_segment_copy_workspace_bytes(a.ctypes.data, len(a)) >= 24 * len(tiles)
    assert L.redux_segment_tiles(None, 0, None) == 0 and L.redux_segment_copy_workspace_bytes(None, 0) == 0
    assert L.redux_segment_copy_kernel_name() == b"k_segment_copy"


def test_segment_copy_refuses_bad_tables_on_the_host():
    """every refusal comes before any device call: this runs where there is no GPU, with addresses that are no memory"""
    L = _lib.lib()
    SRC, DST, WS = 0x10000000, 0x20000000, 0x30000000

    def call(segs, src=SRC, src_bytes=1 << 20, dst=DST, dst_bytes=1 << 20):
        a = api._segments_arg(segs)
        return L.redux_segment_copy_dev(src, src_bytes, dst, dst_bytes, a.ctypes.data, len(a), WS, 1 << 20, None)
    assert call([]) == _lib.OK and call([(5, 5, 0), (1 << 20, 1 << 20, 0)]) == _lib.OK  # (nothing to copy: no launch)
    assert call([((1 << 20) - 3, 0, 4)]) == _lib.INVALID_INPUT                 # src + len > src_bytes
    assert call([((1 << 20) + 1, 0, 0)]) == _lib.INVALID_INPUT
    assert call([(8, 0, 2 ** 64 - 4)]) == _lib.INVALID_INPUT                   # ... by overflow
    assert call([(0, (1 << 20) - 3, 4)]) == _lib.INVALID_INPUT                 # dst + len > dst_bytes
    assert call([(0, 2 ** 64 - 2, 4)], src_bytes=8) == _lib.INVALID_INPUT      # ... by overflow
    assert call([(0, 0, 10), (100, 9, 5)]) == _lib.INVALID_INPUT               # destinations overlap
    assert call([(0, 50, 10), (100, 40, 11)]) == _lib.INVALID_INPUT
    assert call([(0, 0, 10), (0, 0, 10)]) == _lib.INVALID_INPUT
    assert call([(0, 0, 4)], dst=SRC + (1 << 20) - 1) == _lib.INVALID_INPUT    # the buffers overlap
    assert call([(0, 0, 4)], dst=SRC) == _lib.INVALID_INPUT
    assert call([(0, 0, 4)], src=DST + 100, src_bytes=8) == _lib.INVALID_INPUT
    assert call([(0, 0, 4)], src=None) == _lib.INVALID_INPUT and call([(0, 0, 4)], dst=None) == _lib.INVALID_INPUT


# ---- container.Reader with the coder call recorded ---------------------------------------------------------------------------
B = 64


def _segment_tables(nseg, E):
    """valid static tables of a common total, every one different"""
    cums = np.zeros((nseg * E, 258), dtype=np.uint32)
    for t in range(nseg * E):
        f = np.ones(257, dtype=np.int64)
        f[t % 256] += (1 << 16) - 257
        cums[t, 1:] = np.cumsum(f)
    return cums


def build(kind):
    """(container bytes, the data, the streams' offsets, the keyword arguments pack() got, granule blocks, the base)"""
    rng = np.random.default_rng(sum(kind.encode()))
    nb, E, g = {"v1": (11, 1, 1), "0x12": (11, 2, 2), "v6": (22, 4, 4), "v9": (13, 2, 2), "v10": (29, 1, 8), "v5": (138, 1, 64)}[kind]
    total = nb * B - 57
    data = rng.integers(0, 7, total, dtype=np.uint8).tobytes()
    streams, _ = ox.compress_blocks(data, B, PARAMS)  # (oracle-coded blocks: real streams for version 1, stand-ins for the rest)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    kw, params, base = {}, PARAMS, None
    if kind == "0x12":
        kw = dict(element_size=2, block_crc=np.array([zlib.crc32(data[b * B:(b + 1) * B]) for b in range(nb)], dtype=np.uint32))
    elif kind == "v6":
        kw = dict(element_size=4, filter="delta")
    elif kind == "v9":
        flags = np.zeros(nb, dtype=np.uint8)
        flags[[1, 4, 5, 12]] = 1
        streams = [s[:1] if flags[b] else s for b, s in enumerate(streams)]
        offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
        base = rng.integers(0, 256, 5 * B + 10, dtype=np.uint8).tobytes() + b"tail the coder did not use"
        kw = dict(element_size=2, constant=flags, base=(5 * B + 10, zlib.crc32(base[: 5 * B + 10])))
    elif kind == "v10":
        kw = dict(unit_layouts=np.array([3, 0, 6, 1], dtype=np.uint8))
    elif kind == "v5":
        params = api.SegmentStaticModel(PARAMS, _segment_tables(3, 1), 1, 64)
    blob = container.pack(np.frombuffer(b"".join(streams), dtype=np.uint8), offs, params, B, total, **kw)
    return blob, data, offs, dict(kw, params=params), g, base


def covered_blocks(total, g, ranges):
    nb = -(-total // B)
    keep = np.zeros(nb, dtype=bool)
    for s, n in ranges:
        if n:
            keep[s // (g * B) * g: ((s + n - 1) // (g * B) + 1) * g] = True
    return np.flatnonzero(keep)


class Recorder:
    """stands for api.decompress_blocks: keeps what it was given and answers with the bytes of the virtual input"""

    def __init__(self, vdata):
        self.vdata, self.calls = vdata, []

    def __call__(self, streams, offsets, block_size, params=PARAMS, **kw):
        self.calls.append(dict(kw, streams=np.array(streams), offsets=np.array(offsets), block_size=block_size, params=params))
        nb = len(offsets) - 1
        sizes = np.array([len(self.vdata[b * B:(b + 1) * B]) for b in range(nb)], dtype=np.uint32)
        if kw.get("block_crc") is not None:
            kw["block_crc"][:] = [zlib.crc32(self.vdata[b * B:(b + 1) * B]) for b in range(nb)]
        out = np.zeros(nb * block_size, dtype=np.uint8)
        out[: len(self.vdata)] = np.frombuffer(self.vdata, dtype=np.uint8)
        return (out if kw.get("length") is None else out[: kw["length"]]), sizes, np.zeros(nb, dtype=np.int32)


RANGES = {"v1": [(3 * B + 5, 2 * B), (9 * B, 10), (3 * B + 9, 4)],
          "0x12": [(7 * B + 1, 3), (2 * B - 1, 2), (7 * B + 1, 3)],
          "v6": [(21 * B, 7), (0, 1), (9 * B - 1, 2)],
          "v9": [(4 * B + 3, 2 * B), (12 * B, 5), (0, 0)],
          "v10": [(28 * B, 7), (9 * B, 1)],
          "v5": [(130 * B, 100), (70 * B, 1)]}


@pytest.mark.parametrize("kind", list(RANGES))
def test_reader_hands_the_coder_the_covered_slices_once(kind, monkeypatch):
    blob, data, offs, kw, g, base = build(kind)
    ranges, total = RANGES[kind], len(data)
    sel = covered_blocks(total, g, ranges)
    vdata = b"".join(data[b * B:(b + 1) * B] for b in sel)
    rec = Recorder(vdata)
    monkeypatch.setattr(api, "decompress_blocks", rec)
    src = io.BytesIO(blob)
    r = container.Reader(src, base)
    assert (r.total, r.block_size, r.nblocks, r.version, r.granule_blocks) == (total, B, len(offs) - 1, blob[4], g)
    assert r.payload_offset == len(blob) - int(offs[-1]) and r.bytes_read == r.payload_offset  # (the index, not the payload)
    got = r.read_many(ranges)
    assert got == [data[s: s + n] for s, n in ranges]
    assert len(rec.calls) == 1
    c = rec.calls[0]
    payload = b"".join(blob[r.payload_offset + int(offs[b]): r.payload_offset + int(offs[b + 1])] for b in sel)
    assert c["streams"].tobytes() == payload and r.bytes_read == r.payload_offset + len(payload)
    assert c["offsets"].tolist() == np.concatenate([[0], np.cumsum(offs[sel + 1] - offs[sel])]).tolist()
    assert c["block_size"] == (B if kind != "v1" or len(vdata) >= B else len(vdata))
    if kind == "v1":
        assert "length" not in c and c["params"].triple() == PARAMS
    else:
        assert c["length"] == len(vdata)
    if kind == "0x12":
        assert c["element_size"] == 2 and c["block_crc"].tolist() == kw["block_crc"][sel].tolist() and c["stored"] is None
    if kind == "v6":
        assert c["element_size"] == 4 and c["filter"] == "delta" and c["base"] is None and c["constant"] is None
    if kind == "v9":
        assert c["element_size"] == 2 and c["constant"].tolist() == kw["constant"][sel].tolist()
        used = base[: 5 * B + 10]
        assert bytes(c["base"]) == b"".join(used[b * B:(b + 1) * B] for b in sel)
        assert 0 < len(c["base"]) < len(vdata)
    if kind == "v10":
        assert c["unit_layouts"].tolist() == kw["unit_layouts"][np.unique(sel // 8)].tolist()
    if kind == "v5":
        m = c["params"]
        assert isinstance(m, api.SegmentStaticModel) and (m.element_size, m.segment_blocks) == (1, 64)
        assert np.array_equal(m.cums, kw["params"].cums[np.unique(sel // 64)])
    # the one-liner, from bytes; ranges without bytes: no coder call at all
    rec.vdata = b"".join(data[b * B:(b + 1) * B] for b in covered_blocks(total, g, ranges[:1]))
    assert container.decompress_range(blob, *ranges[0], base=base) == data[ranges[0][0]: ranges[0][0] + ranges[0][1]]
    n = len(rec.calls)
    assert r.read_many([(0, 0), (total, 0)]) == [b"", b""] and r.read_many([]) == [] and len(rec.calls) == n
    for bad in ((total, 1), (2 ** 63, 2 ** 63), (total + 1, 0)):
        with pytest.raises(api.InvalidInput):
            r.read(*bad)


def test_reader_needs_only_the_covered_payload(monkeypatch):
    blob, data, offs, kw, g, _ = build("0x12")
    ranges = [(2 * B + 1, B)]
    sel = covered_blocks(len(data), g, ranges)
    monkeypatch.setattr(api, "decompress_blocks", Recorder(b"".join(data[b * B:(b + 1) * B] for b in sel)))
    head = len(blob) - int(offs[-1])
    end = head + int(offs[sel[-1] + 1])
    assert container.Reader(io.BytesIO(blob[:end])).read(*ranges[0]) == data[2 * B + 1: 3 * B + 1]  # cut just behind the covered streams
    assert container.Reader(blob[:end]).read(*ranges[0]) == data[2 * B + 1: 3 * B + 1]
    with pytest.raises(api.Eof):
        container.decompress_bytes(blob[:end])
    for cut in (end - 1, head + int(offs[sel[0]]) + 1, head):
        with pytest.raises(api.Eof):
            container.Reader(io.BytesIO(blob[:cut])).read(*ranges[0])                              # cut inside them
    for cut in (head - 1, 40, 31, 0):
        with pytest.raises(api.Eof):
            container.Reader(io.BytesIO(blob[:cut]))                                               # cut inside the index
    # damage in blocks no range covers does not matter; a wrong recorded CRC of a covered block does
    bad = bytearray(blob)
    bad[end + 3] ^= 0x55
    assert container.Reader(bytes(bad)).read(*ranges[0]) == data[2 * B + 1: 3 * B + 1]
    bad = bytearray(blob)
    bad[32 + 4 * (len(offs) - 1) + 4 * int(sel[0])] ^= 1
    with pytest.raises(api.InvalidInput):
        container.Reader(bytes(bad)).read(*ranges[0])


def test_reader_checks_the_base_at_open():
    blob, data, offs, kw, g, base = build("v9")
    for wrong in (None, base[:100], bytes(len(base))):
        with pytest.raises(api.InvalidInput):
            container.Reader(blob, wrong)
    with pytest.raises(api.InvalidInput):
        container.Reader(build("v1")[0], base)
    assert container.Reader(blob, base).read(0, 0) == b""


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_cli_parse_range():
    assert cli.parse(["-d", "--range", "0:0"]) == {"compress": False, "input": None, "output": None, "block_size": 0, "range": (0, 0)}
    assert cli.parse(["-d", "-i", "a", "--range", "5:7"]) == {"compress": False, "input": "a", "output": None, "block_size": 0,
                                                              "range": (5, 7)}
    assert "range" not in cli.parse(["-d"])
    for bad in (["-c", "--range", "0:1"], ["-d", "--range", "5"], ["-d", "--range", "-1:2"], ["-d", "--range", "a:b"],
                ["-d", "--range"], ["-d", "--range", "1:"], ["-d", "--range", ":1"], ["-d", "--range", "1:2:3"],
                ["--range", "1:2"]):
        assert cli.parse(bad) is None, bad
    assert "--range" in cli.USAGE and "--range" in cli.__doc__
    assert cli.main(["-d", "--range"]) == 1


def test_the_gpu_sweeps_hold_every_container_kind_and_mode():
    """The tables of tests/test_range_gpu.py against lists written out here: a kind, a mode or a damaged kind that is removed
    fails this test.  The record layout's kinds are container version 15 with and without the byte delta, their granule a
    frame of record_size blocks, and the file's ranges reach its short last frame and that frame's trailing bytes."""
    import test_range_gpu as G
    kinds = ["v1", "v2", "v3", "v4", "v5", "v5e2", "v6", "v7", "v8", "v9", "v9base", "v10", "0x41", "0x42", "v11", "v12", "v13", "v14",
             "v15", "v15plain"]
    assert list(G.KINDS) == kinds and G.ALL_KINDS == kinds + [k + "+crc" for k in kinds]
    assert list(G.MODES) == ["plain", "planes", "delta", "base", "constant", "constant+base", "mixed", "zigzag", "base_sub", "lag",
                             "lag_order", "record"]
    assert G.DAMAGED == ["v1+crc", "v2+crc", "v9base+crc", "v10+crc", "v12+crc", "v14+crc", "v15+crc", "v15plain+crc"]
    assert G.KINDS["v15"] == dict(E=1, record_size=23, filter="delta") and G.KINDS["v15plain"] == dict(E=1, record_size=5)
    assert G.MODES["record"] == dict(E=1, record_size=23, filter="delta")
    assert G.VERSION_BYTE == {"v11": 11, "v12": 12, "v13": 13, "v14": 14, "v15": 15, "v15plain": 15}
    for R in (23, 5):
        F, total = R * G.B, 5 * R * G.B + G.B + 3
        short = total - 5 * F                            # the short last frame: whole records and trailing bytes
        assert 0 < short % R < short and short > G.B
        ranges = G.the_ranges(total, F)
        # (total - 5, 5) lies in the short frame and ends in its 5 (R = 23) or 4 (R = 5) trailing bytes; (0, total) reads its records
        assert 0 < short % R <= 5 and (total - 5, 5) in ranges and (total - 1, 1) in ranges and (0, total) in ranges
        runs, virt_off, virt_len = api.range_plan(total, G.B, R, [(total - 5, 5)])
        assert [tuple(r) for r in runs] == [(5, 1)] and virt_len == short
