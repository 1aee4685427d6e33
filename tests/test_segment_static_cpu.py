"""Segment-static coding (include/redux_hip.h, "segment-static coding") without a GPU: the rule restated in numpy against the
host-only parts of the ABI, container version 5, the CLI parse table, and the reason for the feature on the CPU oracle."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from conftest import ROOT
from oracle import cbind as ox
from test_plane_static_cpu import plane_counts, tables_ref, typed
from test_planes_cpu import planes_ref
from test_semistatic_cpu import rule_ref

P = (8, 30, 32)
TOTAL = 1 << 16


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def nseg_of(nblocks, G):
    return max(1, -(-nblocks // G))


def segment_counts(xp, E, B, G):
    """u64[nseg * E][256]: the bytes of block b of x' counted for table (b // G) * E + b % E"""
    nb = max(1, -(-len(xp) // B))
    counts = np.zeros((nseg_of(nb, G) * E, 256), dtype=np.uint64)
    for b in range(nb):
        counts[(b // G) * E + b % E] += np.bincount(xp[b * B: (b + 1) * B], minlength=256).astype(np.uint64)
    return counts


def segment_tables_ref(x, E, B, G, total=TOTAL):
    """the rule: layout by planes_ref, counts per (b // G, b % E), the semi-static rule per table"""
    xp = planes_ref(x, E, B) if E > 1 else np.asarray(x, dtype=np.uint8)
    return np.stack([rule_ref(c, total) for c in segment_counts(xp, E, B, G)]), xp


def mixed_bf16(nbytes, seed=7, lo=16, hi=19):
    """a checkpoint: bf16 tensors (the high halves of fp32) of 2^lo .. 2^hi elements, sigma log-uniform in [0.002, 0.5]"""
    rng = np.random.default_rng(seed)
    parts, n = [], 0
    while n < nbytes // 2:
        m = int(2 ** rng.uniform(lo, hi))
        sigma = float(np.exp(rng.uniform(np.log(0.002), np.log(0.5))))
        v = rng.normal(0, sigma, m).astype(np.float32)
        parts.append((v.view(np.uint32) >> 16).astype(np.uint16))
        n += m
    return np.concatenate(parts)[: nbytes // 2].view(np.uint8).copy()


def skewed(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, n) * (rng.integers(0, 4, n) == 0)).astype(np.uint8)


# ---- the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_rule_against_the_host_abi(lib, E, k):
    L = lib.lib()
    cp = lib.Params(*P)
    B, G = 16, 64 * E * k
    # empty, one block, a t without bytes, whole segments, a partial last segment, a short last frame
    for nb_bytes in (0, 1, B, G * B, 2 * G * B, 2 * G * B + B + 3, 3 * G * B - 5, G * B + (E - 1) * B + 1):
        x = skewed(nb_bytes, nb_bytes + E)
        want, xp = segment_tables_ref(x, E, B, G)
        nb = max(1, -(-nb_bytes // B))
        nt = L.redux_segment_static_table_count(nb, E, G)
        assert nt == nseg_of(nb, G) * E == len(want)
        counts = np.ascontiguousarray(segment_counts(xp, E, B, G))
        cum = np.zeros((nt, 258), dtype=np.uint32)
        assert L.redux_segment_static_tables_from_counts(C.byref(cp), counts.ctypes.data, nb, E, G, TOTAL, cum.ctypes.data) == lib.OK
        assert np.array_equal(cum, want), (E, k, nb_bytes)
        assert L.redux_segment_static_table_check(C.byref(cp), cum.ctypes.data, nt, nb, E, G) == lib.OK
        for i in range(nt):  # a pair without bytes: all ones, total 257
            owns = counts[i].sum() > 0
            assert int(cum[i, 257]) == (TOTAL if owns else 257)
            assert owns or np.array_equal(cum[i], np.arange(258, dtype=np.uint32))
        assert L.redux_segment_static_total(cum.ctypes.data, nt) == (TOTAL if nb_bytes else 257)
    assert any(c.sum() == 0 for c in segment_counts(planes_ref(skewed(G * B + 1, 1), E, B) if E > 1 else skewed(G * B + 1, 1), E, B, G)) == (E > 1)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_one_segment_is_plane_static_and_static(lib, E):
    L = lib.lib()
    cp = lib.Params(*P)
    B, G = 100, 64 * E * 2
    x = skewed(G * B - 7, E)
    xp = planes_ref(x, E, B) if E > 1 else x
    nb = -(-len(x) // B)
    assert nb <= G
    counts = np.ascontiguousarray(segment_counts(xp, E, B, G))
    assert np.array_equal(counts, plane_counts(xp, E, B))
    seg = np.zeros((E, 258), dtype=np.uint32)
    assert L.redux_segment_static_tables_from_counts(C.byref(cp), counts.ctypes.data, nb, E, G, TOTAL, seg.ctypes.data) == lib.OK
    plane = np.zeros((E, 258), dtype=np.uint32)
    assert L.redux_plane_static_tables_from_counts(C.byref(cp), counts.ctypes.data, E, TOTAL, plane.ctypes.data) == lib.OK
    assert np.array_equal(seg, plane)
    if E == 1:
        one = np.zeros(258, dtype=np.uint32)
        assert L.redux_static_table_from_counts(C.byref(cp), counts.ctypes.data, TOTAL, one.ctypes.data) == lib.OK
        assert np.array_equal(seg[0], one)


def test_table_check_rejects_what_the_rule_cannot_give(lib, rx):
    L = lib.lib()
    cp = lib.Params(*P)
    E, B, G = 2, 64, 128
    x = mixed_bf16(3 * G * B - 10, lo=8, hi=10)
    cum, _ = segment_tables_ref(x, E, B, G)
    nb = -(-len(x) // B)
    ok = lambda c, nblocks=nb, e=E, g=G: L.redux_segment_static_table_check(
        C.byref(cp), np.ascontiguousarray(c).ctypes.data, len(c), nblocks, e, g)
    assert len(cum) == 6 and ok(cum) == lib.OK
    bad = cum.copy()
    bad[3, 100] = bad[3, 99]  # not strictly increasing
    assert ok(bad) == lib.INVALID_INPUT
    other, _ = segment_tables_ref(x, E, B, G, total=1 << 15)
    mixed = cum.copy()
    mixed[4] = other[4]  # totals differ
    assert ok(mixed) == lib.INVALID_INPUT
    ones = cum.copy()
    ones[5] = np.arange(258, dtype=np.uint32)  # the table of a pair without bytes goes with any total
    assert ok(ones) == lib.OK
    assert ok(cum, g=0) == lib.INVALID_INPUT  # k = 0
    assert ok(cum, g=64) == lib.INVALID_INPUT  # not a multiple of 64 E
    assert ok(cum, e=3) == lib.INVALID_INPUT
    assert ok(cum, nblocks=2 * G) == lib.INVALID_INPUT and ok(cum, nblocks=3 * G + 1) == lib.INVALID_INPUT  # the table count
    assert ok(cum[:4]) == lib.INVALID_INPUT and ok(cum[:4], nblocks=2 * G) == lib.OK
    assert L.redux_segment_static_table_check(C.byref(cp), None, 6, nb, E, G) == lib.INVALID_INPUT
    assert L.redux_segment_static_table_check(C.byref(lib.Params(12, 14, 16)), cum.ctypes.data, 6, nb, E, G) == lib.UNSUPPORTED
    assert L.redux_segment_static_table_count(nb, E, 0) == 0 and L.redux_segment_static_table_count(nb, 3, 192) == 0
    # the Python model
    m = rx.SegmentStaticModel(P, cum, E, G)
    assert m.element_size == 2 and m.segment_blocks == G and m.total() == TOTAL and m.parameters().triple() == P
    m.check(nb)
    with pytest.raises(rx.InvalidInput):
        m.check(2 * G)
    for c, e, g in ((cum, 2, 0), (cum, 2, 64), (cum, 3, 192), (cum[:5], 2, G), (bad, 2, G), (np.zeros((2, 257)), 2, G)):
        with pytest.raises(rx.InvalidInput):
            rx.SegmentStaticModel(P, c, e, g)
    assert rx.default_segment_blocks(2) == 64 * 2 * 4


def test_host_only_geometry(lib):
    L = lib.lib()
    cp = lib.Params(*P)
    n, B = 10 * 65536 + 3, 65536
    assert L.redux_segment_static_encode_bound(C.byref(cp), n, B) == L.redux_static_encode_bound(C.byref(cp), n, B)
    for E in (1, 2, 4, 8):
        enc = L.redux_plane_static_encode_workspace_bytes(C.byref(cp), n, B, E)
        assert L.redux_segment_static_encode_workspace_bytes(C.byref(cp), n, B, E) == enc
        assert L.redux_segment_static_decode_workspace_bytes(C.byref(cp), n, B, E) == L.redux_plane_static_decode_workspace_bytes(C.byref(cp), n, B, E)
        assert L.redux_segment_static_build_encode_workspace_bytes(C.byref(cp), n, B, E, 64 * E) >= enc + E * 2048
        assert L.redux_segment_static_build_encode_workspace_bytes(C.byref(cp), n, B, E, 63 * E) == 0
    assert L.redux_segment_static_encode_workspace_bytes(C.byref(lib.Params(12, 14, 16)), n, B, 2) == 0
    assert L.redux_segment_static_encode_kernel_name(C.byref(cp), TOTAL, n, B, 2, 64) == b""
    assert L.redux_segment_static_decode_kernel_name(C.byref(cp), TOTAL, 0, 2, 128) == b""


# ---- container version 5 -----------------------------------------------------------------------------------------------
def fake_streams(nb):
    sizes = (np.arange(nb) % 7 + 1).astype(np.uint64)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    return (np.arange(int(offs[-1])) % 251).astype(np.uint8), offs


def v5(rx, E=2, k=1, nb=300, B=64, crc=False):
    from redux_amd import container
    G = 64 * E * k
    total = nb * B - 3
    cum, _ = segment_tables_ref(skewed(total, nb), E, B, G)
    m = rx.SegmentStaticModel(P, cum, E, G)
    streams, offs = fake_streams(nb)
    crcs = np.arange(nb, dtype=np.uint32) if crc else None
    return container.pack(streams, offs, m, B, total, block_crc=crcs), m, streams, offs, total


@pytest.mark.parametrize("E,k", [(1, 1), (2, 1), (2, 3), (4, 2), (8, 1)])
@pytest.mark.parametrize("crc", [False, True])
def test_container_pack_unpack_identity(rx, E, k, crc):
    from redux_amd import container
    nb, B = 64 * E * k * 2 + 5, 64
    blob, m, streams, offs, total = v5(rx, E, k, nb, B, crc)
    assert blob[4] == (0x15 if crc else 5)
    assert struct.unpack_from("<I", blob, 12)[0] == 0x50000000 | k << 4 | E
    params, bs, tot, o, payload = container.unpack(blob)
    assert params.triple() == P and bs == B and tot == total and np.array_equal(o, offs) and np.array_equal(payload, streams)
    cums, G = container.segment_static_tables(blob)
    assert G == m.segment_blocks and np.array_equal(cums, m.cums) and container.element_size(blob) == E
    assert container.header_is_wellformed(blob)
    assert (container.block_crcs(blob) is not None) == crc
    assert container.plane_static_tables(blob) is None and container.static_table(blob) is None
    # the documented layout, byte for byte
    want = struct.pack("<4sBBBBIIQQ", b"RDXB", 0x15 if crc else 5, 8, 30, 32, B, 0x50000000 | k << 4 | E, nb, total) \
        + m.cums.astype("<u4").tobytes() + np.diff(offs.astype(np.int64)).astype("<u4").tobytes() \
        + (np.arange(nb, dtype="<u4").tobytes() if crc else b"") + streams.tobytes()
    assert blob == want


def test_container_header_word_and_table_count(rx):
    from redux_amd import container
    E, k, nb, B = 2, 2, 600, 64
    blob, m, streams, offs, total = v5(rx, E, k, nb, B)
    word = 0x50000000 | k << 4 | E

    def with_word(w):
        b = bytearray(blob)
        struct.pack_into("<I", b, 12, w)
        return bytes(b)

    assert container.unpack(with_word(word))[1] == B
    # each wrong marker, E or k: the words of the other versions, another marker nibble, E = 0 / 3 / 16-bit, k = 0
    for w in (0, 2, 4, 8, 0x00020002, k << 4 | E, 0x40000000 | k << 4 | E, 0x60000000 | k << 4 | E, 0xD0000000 | k << 4 | E,
              0x50000000 | k << 4, 0x50000000 | k << 4 | 3, 0x50000000 | k << 4 | 5, 0x50000000 | E):
        with pytest.raises(rx.InvalidInput):
            container.unpack(with_word(w))
        assert not container.header_is_wellformed(with_word(w))
    # a wrong nseg: the word says another k (or E) than the tables were built for, so the table count no longer matches
    # the file -- the sections behind the tables move and the file reads as damaged or truncated, never as another input
    for w in (0x50000000 | 1 << 4 | E, 0x50000000 | 5 << 4 | E, 0x50000000 | k << 4 | 4):
        with pytest.raises((rx.InvalidInput, rx.Eof)):
            container.decompress_bytes(with_word(w))
    # pack refuses a model whose table count is not that of the streams
    with pytest.raises(rx.InvalidInput):
        container.pack(streams[: int(offs[100])], offs[:101], m, B, 100 * B)
    # stored blocks do not exist for version 5
    for ver in (0x45, 0x55):
        b = bytearray(blob)
        b[4] = ver
        with pytest.raises(rx.InvalidInput):
            container.unpack(bytes(b))
    # a table the check rejects
    b = bytearray(blob)
    struct.pack_into("<I", b, 32 + 1032 * 3 + 4 * 50, struct.unpack_from("<I", b, 32 + 1032 * 3 + 4 * 49)[0])
    with pytest.raises(rx.InvalidInput):
        container.unpack(bytes(b))


def test_container_truncations(rx):
    from redux_amd import container
    E, k, nb, B = 2, 1, 200, 64
    blob, m, streams, offs, total = v5(rx, E, k, nb, B, crc=True)
    tables = len(m.cums) * 1032
    edges = [31, 32, 32 + 1032, 32 + tables - 1, 32 + tables, 32 + tables + 4 * nb - 1, 32 + tables + 4 * nb,
             32 + tables + 8 * nb - 1, 32 + tables + 8 * nb, len(blob) - 1]
    for cut in edges:
        with pytest.raises(rx.Eof):
            container.unpack(blob[:cut])
    container.unpack(blob)


def test_earlier_versions_are_packed_as_documented(rx):
    from redux_amd import container
    nb, B = 130, 64
    total = nb * B - 3
    streams, offs = fake_streams(nb)
    sizes = np.diff(offs.astype(np.int64)).astype("<u4").tobytes()
    head = lambda ver, res: struct.pack("<4sBBBBIIQQ", b"RDXB", ver, 8, 30, 32, B, res, nb, total)
    x = skewed(total, 3)
    assert container.pack(streams, offs, P, B, total) == head(1, 0) + sizes + streams.tobytes()
    assert container.pack(streams, offs, P, B, total, element_size=4) == head(2, 4) + sizes + streams.tobytes()
    cum = rule_ref(np.bincount(x, minlength=256).astype(np.uint64), TOTAL)
    assert container.pack(streams, offs, rx.StaticModel(P, cum), B, total) == head(3, 0) + cum.astype("<u4").tobytes() + sizes + streams.tobytes()
    cums, _ = tables_ref(x, 2, B)
    assert container.pack(streams, offs, rx.PlaneStaticModel(P, cums), B, total) \
        == head(4, 0x00020002) + cums.astype("<u4").tobytes() + sizes + streams.tobytes()
    crcs = np.arange(nb, dtype=np.uint32)
    assert container.pack(streams, offs, P, B, total, block_crc=crcs) == head(0x11, 0) + sizes + crcs.astype("<u4").tobytes() + streams.tobytes()


# ---- CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_parse():
    from redux_amd import cli
    ok = cli.parse(["-c", "--block-size", "4096", "--model", "segment-static"])
    assert ok and ok["model"] == "segment-static" and "segment_blocks" not in ok
    ok = cli.parse(["-c", "--block-size", "4096", "--model", "segment-static", "--element-size", "4", "--segment-blocks", "512",
                    "--checksum"])
    assert ok and ok["segment_blocks"] == 512 and ok["element_size"] == 4
    assert cli.parse(["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks", "64"])
    for bad in (["-c", "--model", "segment-static"],  # no block size
                ["-c", "--block-size", "4096", "--model", "segment-static", "--stored"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks", "0"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks", "100"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--element-size", "2", "--segment-blocks", "64"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks", "x"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks"],
                ["-c", "--block-size", "4096", "--model", "segment-static", "--segment-blocks", str(64 << 24)],
                ["-c", "--block-size", "4096", "--model", "plane-static", "--element-size", "2", "--segment-blocks", "128"],
                ["-c", "--block-size", "4096", "--segment-blocks", "128"]):
        assert cli.parse(bad) is None, bad
    assert "segment-static" in cli.USAGE and "--segment-blocks" in cli.USAGE and "segment-static" in cli.__doc__


# ---- the reason for the feature, on the oracle ---------------------------------------------------------------------------
def coded_bytes(xp, B, table_of):
    """sum of the oracle's static streams of the blocks of x', block b under table_of(b)"""
    return sum(len(ox.compress_static(xp[b * B: (b + 1) * B], table_of(b), P)[0]) for b in range(-(-len(xp) // B)))


def test_segment_tables_beat_one_table_per_plane_on_drifting_data():
    """Measured here (oracle streams + 1,032 bytes per table, over the input size): the issue's 8 MiB mixed-sigma bf16
    input 0.6882 against 0.7225 for plane-static; kennedy.xls 0.4443 against 0.4488 for one table."""
    B, E, G = 4096, 2, 128
    x = mixed_bf16(8 << 20)
    seg, xp = segment_tables_ref(x, E, B, G)
    plane, _ = tables_ref(x, E, B)
    s = coded_bytes(xp, B, lambda b: seg[(b // G) * E + b % E]) + 1032 * len(seg)
    p = coded_bytes(xp, B, lambda b: plane[b % E]) + 1032 * len(plane)
    print("mixed-sigma bf16, 8 MiB: segment-static %.4f (%d tables), plane-static %.4f" % (s / len(x), len(seg), p / len(x)))
    assert s < p

    x = np.frombuffer(open(os.path.join(ROOT, "tests", "golden", "corpora", "canterbury", "kennedy.xls"), "rb").read(), dtype=np.uint8)
    G = 64
    seg, _ = segment_tables_ref(x, 1, B, G)
    one = rule_ref(np.bincount(x, minlength=256).astype(np.uint64), TOTAL)
    s = coded_bytes(x, B, lambda b: seg[b // G]) + 1032 * len(seg)
    p = coded_bytes(x, B, lambda b: one) + 1032
    print("kennedy.xls: segment-static %.4f (%d tables), one table %.4f" % (s / len(x), len(seg), p / len(x)))
    assert s < p
