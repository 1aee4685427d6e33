"""Plane-static coding (include/redux_hip.h, "plane-static coding") without a GPU: the rule restated in numpy against the
host-only parts of the ABI, container version 4, the CLI parse table, and the value claim on the CPU oracle."""
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_cpu import lengths, planes_ref
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


def plane_counts(xp, E, B):
    """u64[E][256]: the bytes of block b of x' counted for table b mod E (no special case for the short last frame)"""
    counts = np.zeros((E, 256), dtype=np.uint64)
    for b in range(max(1, -(-len(xp) // B))):
        counts[b % E] += np.bincount(xp[b * B: (b + 1) * B], minlength=256).astype(np.uint64)
    return counts


def tables_ref(x, E, B, total=TOTAL):
    """the rule: layout by planes_ref, counts per b mod E, the semi-static rule per t"""
    xp = planes_ref(x, E, B)
    return np.stack([rule_ref(c, total) for c in plane_counts(xp, E, B)]), xp


def typed(kind, n, seed=5):
    """the data of the issue's table: bf16 = N(0, 0.02) as the high halves of fp32, fp32 = N(0, 1)"""
    rng = np.random.default_rng(seed)
    if kind == "bf16":
        v = rng.normal(0, 0.02, n // 2).astype(np.float32)
        return (v.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)
    return rng.normal(0, 1, n // 4).astype(np.float32).view(np.uint8)


# ---- the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [2, 4, 8])
@pytest.mark.parametrize("B", [16, 100, 65536])
def test_rule_against_the_host_abi(lib, E, B):
    L = lib.lib()
    cp = lib.Params(*P)
    for n in lengths(E, B):
        rng = np.random.default_rng(n + E)
        x = (rng.integers(0, 256, n) * (rng.integers(0, 4, n) == 0)).astype(np.uint8)  # skewed: zeros dominate
        want, xp = tables_ref(x, E, B)
        counts = np.ascontiguousarray(plane_counts(xp, E, B))
        cum = np.zeros((E, 258), dtype=np.uint32)
        assert L.redux_plane_static_tables_from_counts(C.byref(cp), counts.ctypes.data, E, TOTAL, cum.ctypes.data) == lib.OK
        assert np.array_equal(cum, want), (E, B, n)
        assert L.redux_plane_static_table_check(C.byref(cp), cum.ctypes.data, E) == lib.OK
        nb = max(1, -(-n // B))
        for t in range(E):  # a t that owns no bytes: all ones, total 257; every other table has the call's total
            owns = n > t * B
            assert int(cum[t, 257]) == (TOTAL if owns else 257), (E, B, n, t)
            assert owns or np.array_equal(cum[t], np.arange(258, dtype=np.uint32))
        assert any(n <= t * B for t in range(E)) == (nb < E)
        assert L.redux_plane_static_total(cum.ctypes.data, E) == (TOTAL if n else 257)


def test_table_check_rejects_what_the_rule_cannot_give(lib, rx):
    L = lib.lib()
    cp = lib.Params(*P)
    x = typed("bf16", 1 << 16)
    cum, _ = tables_ref(x, 2, 4096)
    ok = lambda c, E: L.redux_plane_static_table_check(C.byref(cp), np.ascontiguousarray(c).ctypes.data, E)
    assert ok(cum, 2) == lib.OK and ok(cum[:1], 1) == lib.OK
    assert ok(cum, 3) == lib.INVALID_INPUT
    bad = cum.copy()
    bad[1, 100] = bad[1, 99]  # not strictly increasing
    assert ok(bad, 2) == lib.INVALID_INPUT
    other, _ = tables_ref(x, 2, 4096, total=1 << 15)
    assert ok(np.stack([cum[0], other[1]]), 2) == lib.INVALID_INPUT  # totals differ
    ones = np.arange(258, dtype=np.uint32)
    assert ok(np.stack([cum[0], ones]), 2) == lib.OK  # the table of a plane without bytes goes with any total
    assert L.redux_plane_static_table_check(C.byref(cp), None, 2) == lib.INVALID_INPUT
    assert L.redux_plane_static_table_check(C.byref(lib.Params(12, 14, 16)), cum.ctypes.data, 2) == lib.UNSUPPORTED
    # the Python model
    m = rx.PlaneStaticModel(P, cum)
    assert m.element_size == 2 and m.total() == TOTAL and m.parameters().triple() == P
    for c in (cum[0], cum[:1], np.zeros((3, 258)), np.zeros((2, 257)), bad):
        with pytest.raises(rx.InvalidInput):
            rx.PlaneStaticModel(P, c)


def test_host_only_geometry(lib):
    L = lib.lib()
    cp = lib.Params(*P)
    n, B = 10 * 65536 + 3, 65536
    assert L.redux_plane_static_encode_bound(C.byref(cp), n, B) == L.redux_static_encode_bound(C.byref(cp), n, B)
    plain = L.redux_static_encode_workspace_bytes(C.byref(cp), n, B)
    assert L.redux_plane_static_encode_workspace_bytes(C.byref(cp), n, B, 1) == plain
    for E in (2, 4, 8):
        assert L.redux_plane_static_encode_workspace_bytes(C.byref(cp), n, B, E) >= plain + n
        assert L.redux_plane_static_decode_workspace_bytes(C.byref(cp), n, B, E) >= 11 * B
    assert L.redux_plane_static_encode_workspace_bytes(C.byref(cp), n, B, 3) == 0
    assert L.redux_plane_static_decode_workspace_bytes(C.byref(cp), n, B, 3) == 0
    assert L.redux_plane_histogram_workspace_bytes(n) == 0
    # the calls refuse what the plain static model refuses before anything is launched
    assert L.redux_plane_static_tables_dev(C.byref(cp), None, 2, TOTAL, None, None) == lib.INVALID_INPUT
    assert L.redux_plane_static_tables_dev(C.byref(cp), None, 2, 256, None, None) == lib.INVALID_INPUT
    assert L.redux_plane_static_encode_dev(C.byref(cp), None, TOTAL, None, 0, B, 3, None, 0, None, None, None, None, 0,
                                           None) == lib.INVALID_INPUT
    assert L.redux_plane_static_encode_kernel_name(C.byref(cp), TOTAL, n, B, 3) == b""
    assert L.redux_plane_static_decode_kernel_name(C.byref(cp), TOTAL, 0, 2) == b""


def test_api_refusals_stay(rx):
    x = typed("bf16", 1 << 14)
    cum, _ = tables_ref(x, 2, 4096)
    m = rx.PlaneStaticModel(P, cum)
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(x, 4096, m, element_size=4)
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(x, 4096, m, stored=np.zeros(4, np.uint8))
    with pytest.raises(rx.InvalidInput):
        rx.decompress_blocks(b"\0", [0, 1], 4096, m)  # no length
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(x, 4096, rx.StaticModel(P, cum[0]), element_size=2)  # one table, planes: still refused
    with pytest.raises(rx.InvalidInput):
        rx.plane_static_tables(x, 1, 4096)
    with pytest.raises(rx.InvalidInput):
        rx.plane_static_tables(x, 2, 0)


# ---- container version 4 -----------------------------------------------------------------------------------------------
def made_up(nb, seed=3):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 40, nb)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return rng.integers(0, 256, int(offs[-1]), dtype=np.uint8), offs


@pytest.mark.parametrize("E", [2, 4, 8])
def test_container_version_4_round_trip(rx, E):
    from redux_amd import container
    B, total_len = 64, 64 * 9 + 5
    x = np.random.default_rng(E).integers(0, 7, total_len).astype(np.uint8)
    cum, _ = tables_ref(x, E, B)
    m = rx.PlaneStaticModel(P, cum)
    streams, offs = made_up(10)
    for crc in (None, np.arange(10, dtype=np.uint32) * 7919):
        for es in (1, E):  # (the model's element size is used either way)
            blob = container.pack(streams, offs, m, B, total_len, element_size=es, block_crc=crc)
            assert blob[4] == (0x14 if crc is not None else 4)
            assert struct.unpack_from("<I", blob, 12)[0] == E << 16 | E
            assert len(blob) == 32 + E * 1032 + 40 + (40 if crc is not None else 0) + len(streams)
            Pp, bs, tl, o, payload = container.unpack(blob)
            assert (Pp.triple(), bs, tl) == (P, B, total_len)
            assert np.array_equal(o, offs) and np.array_equal(payload, streams)
            assert container.element_size(blob) == E
            assert np.array_equal(container.plane_static_tables(blob), cum)
            assert container.static_table(blob) is None and container.block_stored(blob) is None
            got = container.block_crcs(blob)
            assert (got is None) if crc is None else np.array_equal(got, crc)
            assert container.header_is_wellformed(blob)
    with pytest.raises(rx.InvalidInput):
        container.pack(streams, offs, m, B, total_len, element_size=E * 2 if E < 8 else 2)
    with pytest.raises(rx.InvalidInput):
        container.pack(streams, offs, m, B, total_len, stored=np.zeros(10, np.uint8))


def test_container_earlier_versions_are_byte_identical(rx):
    """what pack wrote for versions 1, 2, 3 before version 4 existed, restated from the documented layout"""
    from redux_amd import container
    streams, offs = made_up(5)
    sizes = np.diff(offs.astype(np.int64)).astype("<u4").tobytes()
    head = lambda ver, res: struct.pack("<4sBBBBIIQQ", b"RDXB", ver, 8, 30, 32, 64, res, 5, 300)
    assert container.pack(streams, offs, P, 64, 300) == head(1, 0) + sizes + streams.tobytes()
    assert container.pack(streams, offs, P, 64, 300, element_size=4) == head(2, 4) + sizes + streams.tobytes()
    cum = rule_ref(np.arange(256), TOTAL)
    m = rx.StaticModel(P, cum)
    assert container.pack(streams, offs, m, 64, 300) == head(3, 0) + cum.astype("<u4").tobytes() + sizes + streams.tobytes()
    crc = np.arange(5, dtype=np.uint32)
    assert container.pack(streams, offs, P, 64, 300, block_crc=crc) == head(0x11, 0) + sizes + crc.tobytes() + streams.tobytes()
    for blob in (head(1, 0), head(2, 4), head(3, 0)):
        assert container.plane_static_tables(blob + cum.astype("<u4").tobytes() + sizes + streams.tobytes()) is None


def test_container_version_4_damage(rx):
    from redux_amd import container
    E, B, total_len = 2, 64, 64 * 9 + 5
    x = np.random.default_rng(1).integers(0, 7, total_len).astype(np.uint8)
    cum, _ = tables_ref(x, E, B)
    streams, offs = made_up(10)
    blob = bytearray(container.pack(streams, offs, rx.PlaneStaticModel(P, cum), B, total_len))
    assert container.unpack(bytes(blob))

    def with_word(w, ver=4):
        b = bytearray(blob)
        b[4] = ver
        struct.pack_into("<I", b, 12, w)
        return bytes(b)

    # the word at offset 12: element size and table count must both be E in {2, 4, 8}
    for w in (0, 1, 2, 4, 8, 16, 0x80000000, 0x00020004, 0x00040002, 0x00010001, 0x00030003, 0x00100010, 0x00020000):
        assert not container.header_is_wellformed(with_word(w)), hex(w)
        with pytest.raises(rx.InvalidInput):
            container.unpack(with_word(w))
    for ver in (0x44, 0x54, 0x24, 0x84, 5, 0x15):  # no stored blocks, no other flags, no version 5
        with pytest.raises(rx.InvalidInput):
            container.unpack(with_word(0x00020002, ver))
    assert container.header_is_wellformed(with_word(0x00040004))  # (then needs four tables: this body is damaged)
    # a bad table
    for t in range(E):
        b = bytearray(blob)
        at = 32 + 1032 * t + 4 * 50
        b[at: at + 4] = b[at - 4: at]  # cum[50] = cum[49]
        with pytest.raises(rx.InvalidInput):
            container.unpack(bytes(b))
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(bytes(b))
    b = bytearray(blob)
    struct.pack_into("<I", b, 32 + 1032 + 4 * 257, 1 << 15)  # table 1's total differs (and is not increasing)
    with pytest.raises(rx.InvalidInput):
        container.unpack(bytes(b))
    # truncated tables, sizes, payload
    for cut in (32, 33, 32 + 1032, 32 + 2 * 1032 - 1, 32 + 2 * 1032 + 39, len(blob) - 1):
        with pytest.raises(rx.Eof):
            container.unpack(bytes(blob[:cut]))
    with pytest.raises(rx.Eof):
        container.plane_static_tables(bytes(blob[:100]))


# ---- CLI ---------------------------------------------------------------------------------------------------------------
def test_cli_parse_table():
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    for E in (2, 4, 8):
        assert cli.parse(["-c", "--block-size", "65536", "--element-size", str(E), "--model", "plane-static"]) == \
            dict(base, element_size=E, model="plane-static")
    assert cli.parse(["-c", "--block-size", "65536", "--element-size", "2", "--model", "plane-static", "--checksum"]) == \
        dict(base, element_size=2, model="plane-static", checksum=True)
    for bad in (["-c", "--element-size", "2", "--model", "plane-static"],
                ["-c", "--block-size", "0", "--element-size", "2", "--model", "plane-static"],
                ["-c", "--block-size", "65536", "--model", "plane-static"],
                ["-c", "--block-size", "65536", "--element-size", "1", "--model", "plane-static"],
                ["-c", "--block-size", "65536", "--element-size", "2", "--model", "plane-static", "--stored"],
                ["-c", "--block-size", "65536", "--element-size", "3", "--model", "plane-static"],
                ["-c", "--block-size", "65536", "--element-size", "2", "--model", "planestatic"],
                # the old refusals
                ["-c", "--block-size", "65536", "--element-size", "2", "--model", "static"],
                ["-c", "--model", "static"], ["-c", "--block-size", "65536", "--model", "static", "--stored"]):
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
    assert "plane-static" in cli.USAGE and "plane-static" in cli.__doc__


def test_compress_bytes_refusals(rx):
    from redux_amd import container
    for kw in (dict(model="plane-static"), dict(model="plane-static", element_size=1),
               dict(model="plane-static", element_size=2, stored=True), dict(model="plane-static", element_size=3),
               dict(model="static", element_size=2), dict(model="planes")):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(b"abcd" * 100, 64, **kw)


# ---- the value claim, on the CPU oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E", [("bf16", 2), ("fp32", 4)])
def test_plane_tables_beat_one_table_on_the_oracle(kind, E):
    """64 blocks of 64 KiB: the streams under E tables are smaller than those under ONE static table over the same x'
    (the byte-plane layout's gain survives only with a table per plane), and no larger than the adaptive coder's on x'."""
    B, nb = 65536, 64
    x = typed(kind, nb * B)
    cums, xp = tables_ref(x, E, B)
    one = rule_ref(np.bincount(xp, minlength=256), TOTAL)
    per_plane = sum(len(ox.compress_static(xp[b * B: (b + 1) * B], cums[b % E], P)[0]) for b in range(nb))
    single = sum(len(ox.compress_static(xp[b * B: (b + 1) * B], one, P)[0]) for b in range(nb))
    adaptive = sum(len(ox.compress(xp[b * B: (b + 1) * B], P)[0]) for b in range(nb))
    print(f"{kind}: E tables {per_plane / len(x):.4f}, one table {single / len(x):.4f}, adaptive planes {adaptive / len(x):.4f}")
    assert per_plane + E * 1032 < single
    assert per_plane < adaptive
    # every stream decodes under its plane's table
    for b in (0, 1, E - 1, nb - 1):
        s, _ = ox.compress_static(xp[b * B: (b + 1) * B], cums[b % E], P)
        assert ox.decompress_static(s, cums[b % E], P, cap=B)[0] == xp[b * B: (b + 1) * B].tobytes()
