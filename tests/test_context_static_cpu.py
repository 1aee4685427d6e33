"""Context-static coding (include/redux_hip.h, "context-static coding") without a GPU: the rule restated in numpy against the
host-only parts of the ABI, the reference model for oracle.redux_ref.Codec (used by the GPU tests as well), container
version 7, the CLI parse table, and the value claim as ideal code lengths."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from oracle import redux_ref as ref
from test_semistatic_cpu import rule_ref

P = (8, 30, 32)
TOTAL = 1 << 16
CORPORA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corpora")


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def corpus(name):
    return np.fromfile(os.path.join(CORPORA, name), dtype=np.uint8)


# ---- the rule in numpy ---------------------------------------------------------------------------------------------------
def contexts(x, B):
    """rule 1: the context of byte i is byte i - 1, 0 at the start of every block of B bytes"""
    x = np.asarray(x, dtype=np.uint8)
    ctx = np.zeros(len(x), dtype=np.int64)
    ctx[1:] = x[:-1]
    ctx[::B] = 0
    return ctx


def pair_counts(x, B):
    """rule 2: u64[256][256], counts[c][s] = bytes s whose context is c"""
    x = np.asarray(x, dtype=np.uint8)
    return np.bincount(contexts(x, B) * 256 + x, minlength=65536).reshape(256, 256).astype(np.uint64)


def tables_ref(counts, total=TOTAL):
    """rule 3: the semi-static rule per context; a context without bytes is counted as one of every byte value"""
    ones = np.ones(256, dtype=np.uint64)
    return np.stack([rule_ref(c if c.any() else ones, total) for c in counts]).astype(np.uint32)


class ContextStaticModel:
    """The reference model of rule 5 for oracle.redux_ref.Codec: get_frequency / get_symbol answer from table ctx and then
    advance ctx.  One instance codes one block."""

    def __init__(self, p, cums):
        self.params = p
        self.cums = [[int(v) for v in row] for row in cums]
        self.total = self.cums[0][-1]
        self.ctx = 0

    def parameters(self):
        return self.params

    def total_frequency(self):
        return self.total

    def get_frequency(self, symbol):
        row = self.cums[self.ctx]
        if symbol < 256:
            self.ctx = symbol
        return (row[symbol], row[symbol + 1])

    def get_symbol(self, value):
        row = self.cums[self.ctx]
        s = int(np.searchsorted(row, value, side="right")) - 1
        if s < 256:
            self.ctx = s
        return (s, row[s], row[s + 1])


def encode_ref(x, B, cums, params=P):
    """the streams of every block of x under the tables, by the reference codec: a list of bytes"""
    p = ref.Parameters(*params)
    x = np.asarray(x, dtype=np.uint8)
    return [ref.compress(x[b * B: (b + 1) * B].tobytes(), ContextStaticModel(p, cums))[0]
            for b in range(max(1, -(-len(x) // B)))]


def ideal_bits(x, B, cums):
    """the ideal code length of x under the tables, the EOF symbols included"""
    x = np.asarray(x, dtype=np.uint8)
    f = np.diff(cums.astype(np.int64), axis=1)  # [256, 257]
    total = float(cums[0, 257])
    bits = -np.log2(f[contexts(x, B), x] / total).sum()
    nb = max(1, -(-len(x) // B))
    last = [int(x[min((b + 1) * B, len(x)) - 1]) if len(x) > b * B else 0 for b in range(nb)]
    return bits - np.log2(f[last, 256] / total).sum()


def table_section_bytes(cums):
    """container version 7's table section: total, mask, 512 bytes per table that is not the substitute"""
    sub = tables_ref(np.zeros((1, 256), dtype=np.uint64), int(cums[0, 257]))[0]
    return 4 + 32 + 512 * int((cums != sub).any(axis=1).sum())


def test_reference_model_round_trips():
    x = corpus("canterbury/alice29.txt")[:3000]
    cums = tables_ref(pair_counts(x, 1000))
    p = ref.Parameters(*P)
    for b, s in enumerate(encode_ref(x, 1000, cums)):
        assert ref.decompress(s, ContextStaticModel(p, cums))[0] == x[b * 1000: (b + 1) * 1000].tobytes()
    assert sum(map(len, encode_ref(x, 1000, cums))) < 0.8 * sum(
        len(ref.compress(x[b * 1000: (b + 1) * 1000].tobytes(), ref.StaticModel(p, rule_ref(np.bincount(x, minlength=256).astype(np.uint64), TOTAL)))[0])
        for b in range(3))


# ---- the host rule -------------------------------------------------------------------------------------------------------
def every_context(n=1 << 17, seed=3):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)


RULE_INPUTS = {
    "text": lambda: corpus("canterbury/alice29.txt")[:50000],
    "zeros": lambda: np.zeros(5000, dtype=np.uint8),  # (two blocks)
    "two contexts": lambda: np.full(7777, 0x41, dtype=np.uint8),  # 0 at the block's start, then 0x41
    "every context": every_context,
    "one context": lambda: np.zeros(7777, dtype=np.uint8),  # one block of zeros: every byte's context is 0
    "empty": lambda: np.zeros(0, dtype=np.uint8),
}


@pytest.mark.parametrize("total", [65536, 4096])
@pytest.mark.parametrize("name", list(RULE_INPUTS))
def test_host_rule_equals_numpy(lib, rx, name, total):
    L = lib.lib()
    cp = lib.Params(*P)
    x = RULE_INPUTS[name]()
    B = 1 << 30 if name == "one context" else 4096
    counts = pair_counts(x, B)
    want = tables_ref(counts, total)
    cums = np.zeros((256, 258), dtype=np.uint32)
    assert L.redux_context_static_tables_from_counts(C.byref(cp), counts.ctypes.data, total, cums.ctypes.data) == lib.OK
    assert np.array_equal(cums, want), name
    assert (cums[:, 257] == total).all() and (cums[:, 0] == 0).all() and (np.diff(cums.astype(np.int64), axis=1) > 0).all()
    assert L.redux_context_static_table_check(C.byref(cp), cums.ctypes.data) == lib.OK
    assert L.redux_context_static_total(cums.ctypes.data) == total
    assert np.array_equal(rx.context_static_tables_from_counts(counts, P, total), want)
    present = int(counts.any(axis=1).sum())
    assert present == {"text": present, "zeros": 1, "two contexts": 2, "every context": 256, "one context": 1, "empty": 0}[name]
    sub = tables_ref(np.zeros((1, 256), dtype=np.uint64), total)[0]
    for c in np.flatnonzero(~counts.any(axis=1)):
        assert np.array_equal(cums[c], sub)


def test_counts_skip_the_pair_across_a_block_boundary():
    x = np.array([1, 2, 3, 4, 5, 6, 7], dtype=np.uint8)
    c = pair_counts(x, 3)
    assert c[0, 1] == 1 and c[0, 4] == 1 and c[0, 7] == 1 and c[3, 4] == 0 and c[6, 7] == 0 and c[1, 2] == 1 and c.sum() == 7


def test_total_and_table_checks(lib, rx):
    L = lib.lib()
    cp = lib.Params(*P)
    counts = pair_counts(corpus("canterbury/alice29.txt")[:20000], 4096)
    cums = np.zeros((256, 258), dtype=np.uint32)
    f = lambda total, params=cp: L.redux_context_static_tables_from_counts(C.byref(params), counts.ctypes.data, total, cums.ctypes.data)
    assert f(65537) == lib.UNSUPPORTED and f(1 << 20) == lib.UNSUPPORTED
    assert f(256) == lib.INVALID_INPUT
    assert f(4096, lib.Params(8, 10, 32)) == lib.INVALID_INPUT  # above freq_max = 1023
    assert f(1023, lib.Params(8, 10, 32)) == lib.OK
    assert f(4096, lib.Params(12, 14, 16)) == lib.UNSUPPORTED
    assert f(65536) == lib.OK
    ok = lambda c: L.redux_context_static_table_check(C.byref(cp), np.ascontiguousarray(c).ctypes.data)
    assert ok(cums) == lib.OK
    bad = cums.copy()
    bad[200, 100] = bad[200, 99]
    assert ok(bad) == lib.INVALID_INPUT
    other = tables_ref(counts, 4096)
    mixed = cums.copy()
    mixed[7] = other[7]
    assert ok(mixed) == lib.INVALID_INPUT  # totals differ
    assert L.redux_context_static_table_check(C.byref(cp), None) == lib.INVALID_INPUT
    big = np.tile(rule_ref(np.bincount(np.arange(256), minlength=256).astype(np.uint64), 1 << 17), (256, 1)).astype(np.uint32)
    assert ok(big) == lib.UNSUPPORTED
    m = rx.ContextStaticModel(P, cums)
    assert m.total() == TOTAL and m.parameters().triple() == P
    for c in (cums[0], cums[:255], np.zeros((256, 257)), bad, mixed):
        with pytest.raises(rx.InvalidInput):
            rx.ContextStaticModel(P, c)
    # host-only geometry: the static coder's bound, and a workspace that also holds the 128 KiB image
    n, B = 10 * 65536 + 3, 65536
    assert L.redux_context_static_encode_bound(C.byref(cp), n, B) == L.redux_static_encode_bound(C.byref(cp), n, B)
    assert L.redux_context_static_encode_workspace_bytes(C.byref(cp), n, B) >= L.redux_static_encode_workspace_bytes(C.byref(cp), n, B) + (1 << 17)
    assert L.redux_context_static_decode_workspace_bytes(C.byref(cp), 11, B) >= 1 << 17
    assert L.redux_context_static_encode_workspace_bytes(C.byref(cp), n, 0) == 0


def test_python_refuses_what_the_model_does_not_combine_with(rx):
    """before the library's coders are touched: no GPU here, and InvalidInput all the same"""
    x = corpus("canterbury/alice29.txt")[:20000]
    m = rx.ContextStaticModel(P, tables_ref(pair_counts(x, 4096)))
    for kw in ({"element_size": 2}, {"filter": "delta"}, {"stored": np.zeros(5, dtype=np.uint8)}):
        with pytest.raises(rx.InvalidInput):
            rx.compress_blocks(x, 4096, m, **kw)
    offs = np.arange(6, dtype=np.uint64)
    for kw in ({"element_size": 2, "length": 20000}, {"filter": "delta", "length": 20000}, {"length": 20000},
               {"stored": np.zeros(5, dtype=np.uint8), "length": 20000}):
        with pytest.raises(rx.InvalidInput):
            rx.decompress_blocks(np.zeros(5, dtype=np.uint8), offs, 4096, m, **kw)
    import io
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks_v([x.tobytes()], 4096, m)
    with pytest.raises(rx.InvalidInput):
        rx.decompress_blocks_v(np.zeros(5, dtype=np.uint8), offs, [20000], 4096, m)
    with pytest.raises(rx.InvalidInput):
        rx.compress(io.BytesIO(x.tobytes()), io.BytesIO(), m)
    with pytest.raises(rx.InvalidInput):
        rx.decompress(io.BytesIO(b"abc"), io.BytesIO(), m)
    from redux_amd import container
    for kw in ({"element_size": 2}, {"stored": True}, {"filter": "delta"}):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(x.tobytes(), 4096, P, model="context-static", **kw)


# ---- container version 7 -------------------------------------------------------------------------------------------------
def make_container(rx, x, B, total=TOTAL, crc=False):
    from redux_amd import container
    cums = tables_ref(pair_counts(x, B), total)
    m = rx.ContextStaticModel(P, cums)
    streams = encode_ref(x, B, cums)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    payload = np.frombuffer(b"".join(streams), dtype=np.uint8)
    crcs = None
    if crc:
        import zlib
        crcs = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(len(streams))], dtype=np.uint32)
    return container.pack(payload, offs, m, B, len(x), block_crc=crcs), cums, offs, payload


@pytest.mark.parametrize("total", [65536, 4096])
@pytest.mark.parametrize("crc", [False, True])
def test_container_version_7_round_trip(rx, total, crc):
    from redux_amd import container
    x = corpus("canterbury/alice29.txt")[:6000]
    buf, cums, offs, payload = make_container(rx, x, 2048, total, crc)
    assert buf[4] == (0x17 if crc else 7) and struct.unpack_from("<I", buf, 12)[0] == 0x70000000
    present = int(pair_counts(x, 2048).any(axis=1).sum())
    assert 0 < present < 100
    assert struct.unpack_from("<I", buf, 32)[0] == total
    assert sum(bin(v).count("1") for v in buf[36:68]) == present  # the other 256 - present tables were dropped ...
    assert len(buf) == 32 + 4 + 32 + 512 * present + 4 * 3 * (2 if crc else 1) + len(payload)
    assert table_section_bytes(cums) == 36 + 512 * present
    assert np.array_equal(container.context_static_tables(buf), cums)  # ... and are rebuilt
    Pp, B, n, o, pl = container.unpack(buf)
    assert Pp.triple() == P and B == 2048 and n == 6000 and np.array_equal(o, offs) and np.array_equal(pl, payload)
    assert container.static_table(buf) is None and container.plane_static_tables(buf) is None
    assert container.segment_static_tables(buf) is None and container.element_size(buf) == 1 and container.filter(buf) is None
    assert (container.block_crcs(buf) is not None) == crc and container.block_stored(buf) is None


def test_container_keeps_a_table_that_differs_from_the_substitute(rx):
    """all 256 contexts present: nothing is dropped, and the section is the full 128 KiB"""
    from redux_amd import container
    x = every_context(1 << 16)
    cums = tables_ref(pair_counts(x, 1 << 16))
    buf = container.pack(np.zeros(1, dtype=np.uint8), np.array([0, 1], dtype=np.uint64), rx.ContextStaticModel(P, cums), 1 << 16, len(x))
    assert buf[36:68] == b"\xff" * 32 and len(buf) == 32 + 36 + 256 * 512 + 4 + 1
    assert np.array_equal(container.context_static_tables(buf), cums)


def test_container_version_7_damage_is_invalid_input(rx):
    from redux_amd import container
    x = corpus("canterbury/alice29.txt")[:6000]
    buf, cums, _, _ = make_container(rx, x, 2048)
    present = np.flatnonzero(pair_counts(x, 2048).any(axis=1))
    rows = 68  # the first recorded row

    def damaged(edit):
        b = bytearray(buf)
        edit(b)
        with pytest.raises(rx.InvalidInput):
            container.unpack(bytes(b))

    first = np.frombuffer(buf, dtype="<u2", count=256, offset=rows).astype(np.int64)
    j = int(np.argmax(first))  # a frequency above 1 to take from

    def zero_frequency(b):  # the row still sums to total - 1
        k = int(np.flatnonzero(first == 1)[0])
        struct.pack_into("<H", b, rows + 2 * k, 0)
        struct.pack_into("<H", b, rows + 2 * j, int(first[j]) + 1)

    damaged(zero_frequency)
    damaged(lambda b: struct.pack_into("<H", b, rows + 2 * j, int(first[j]) - 1))  # a row that sums to total - 2
    for total in (0, 256, 65537, 1 << 20):
        damaged(lambda b, t=total: struct.pack_into("<I", b, 32, t))
    damaged(lambda b: struct.pack_into("<I", b, 32, 4096))  # another total than the rows sum to
    damaged(lambda b: b.__setitem__(5 + 1, 10) or struct.pack_into("<I", b, 32, 4096))  # (freq_bits 10: total above freq_max)
    for cut in (33, 40, 68, 68 + 100, 68 + 512 * len(present) - 1):  # a short table section
        with pytest.raises(rx.InvalidInput):
            container.unpack(buf[:cut])
    # a mask that claims more rows than the file has
    absent = int(np.flatnonzero(~pair_counts(x, 2048).any(axis=1))[-1])
    with pytest.raises((rx.InvalidInput, rx.Eof)):
        b = bytearray(buf)
        b[36 + absent // 8] |= 1 << (absent % 8)
        container.unpack(bytes(b))
    for ver in (0x47, 0x57):  # no stored blocks
        damaged(lambda b, v=ver: b.__setitem__(4, v))
    for word in (0, 0x70000001, 0x60000001, 1):  # the marker is required
        damaged(lambda b, w=word: struct.pack_into("<I", b, 12, w))
    with pytest.raises(rx.Eof):  # the sections behind the tables keep the other versions' Eof
        container.unpack(buf[:-1])


def test_versions_1_to_6_parse_as_before(rx):
    """the word 0x70000000 is refused under every other version, version 7 takes no other word, and what pack writes for
    versions 1 and 3 is byte for byte what it was (tests/test_container_cpu.py holds the recorded outcomes of versions
    1 to 6 and stays as it is)"""
    from redux_amd import container
    head = lambda ver, res: container.HEADER.pack(b"RDXB", ver, 8, 30, 32, 4096, res, 1, 100) + b"\0" * 64
    for ver in (1, 2, 3, 4, 5, 6, 0x11, 0x41):
        assert not container.header_is_wellformed(head(ver, 0x70000000))
    assert container.header_is_wellformed(head(1, 0)) and container.header_is_wellformed(head(2, 4))
    assert container.header_is_wellformed(head(7, 0x70000000)) and container.header_is_wellformed(head(0x17, 0x70000000))
    # versions 1 and 3 written by pack are byte for byte what they were: no new section, no new flag
    offs = np.array([0, 3], dtype=np.uint64)
    b1 = container.pack(np.arange(3, dtype=np.uint8), offs, P, 4096, 100)
    assert b1 == container.HEADER.pack(b"RDXB", 1, 8, 30, 32, 4096, 0, 1, 100) + struct.pack("<I", 3) + bytes([0, 1, 2])
    cum = rule_ref(np.bincount(np.arange(256), minlength=256).astype(np.uint64), TOTAL)
    b3 = container.pack(np.arange(3, dtype=np.uint8), offs, rx.StaticModel(P, cum), 4096, 100)
    assert b3[4] == 3 and len(b3) == 32 + 1032 + 4 + 3 and container.context_static_tables(b3) is None


# ---- CLI -------------------------------------------------------------------------------------------------------------------
def test_cli_usage_errors():
    from redux_amd import cli
    ok = cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--checksum"])
    assert ok is not None and ok["model"] == "context-static" and ok["checksum"]
    assert cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--element-size", "1"]) is not None
    assert cli.parse(["-c", "--model", "context-static"]) is None  # --block-size 0
    assert cli.parse(["-c", "--block-size", "0", "--model", "context-static"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--stored"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--filter", "delta"]) is None
    for e in ("2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--element-size", e]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "context-static", "--segment-blocks", "64"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "context"]) is None
    assert cli.parse(["-d"]) is not None  # -d reads the model from the container
    assert "context-static" in cli.USAGE


# ---- the value, as ideal code lengths ------------------------------------------------------------------------------------
def order0_fraction(x, B=65536):
    c = np.bincount(x, minlength=256).astype(np.uint64)
    f = np.diff(rule_ref(c, TOTAL).astype(np.int64))
    nb = max(1, -(-len(x) // B))
    bits = -(np.log2(f[:256] / TOTAL) * c).sum() - nb * np.log2(f[256] / TOTAL)
    return (bits / 8 + 1032) / len(x)


def context_fraction(x, B=65536):
    cums = tables_ref(pair_counts(x, B))
    return (ideal_bits(x, B, cums) / 8 + table_section_bytes(cums)) / len(x)


@pytest.mark.parametrize("name,computed", [("large/bible.txt", 0.768), ("large/world192.txt", 0.791)])
def test_value_on_large_text(name, computed):
    x = corpus(name)
    o0, o1 = order0_fraction(x), context_fraction(x)
    print(f"{name}: order 0 {o0:.4f}, context-static {o1:.4f}, ratio {o1 / o0:.3f}")
    assert o1 <= 0.82 * o0
    assert abs(o1 / o0 - computed) < 0.002  # what the issue's table and DESIGN.md 6i quote


def test_no_value_on_kennedy_xls():
    """all 256 contexts occur in a megabyte of spreadsheet: the 128 KiB of tables cost more than they save"""
    x = corpus("canterbury/kennedy.xls")
    o0, o1 = order0_fraction(x), context_fraction(x)
    print(f"kennedy.xls: order 0 {o0:.4f}, context-static {o1:.4f}")
    assert o1 > o0
