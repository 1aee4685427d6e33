"""Folded difference against a base (include/redux_hip.h, "folded difference against a base"): the numpy restatement of the
rule against hand-written expectations, the value claim on the CPU oracle (synthetic pairs only: no real checkpoint series
was measured), container version 12 and its damaged forms, the argument checks of the Python API before the library is
touched, the CLI flag, the host-only ABI helpers, the C++ mirror's refusals and the range reader.  No GPU call."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_base_cpu import STREAMS, OFFS, TOTAL, base_planes_ref, header_parse_only, no_library, pad
from test_planes_cpu import planes_ref

PARAMS = (8, 30, 32)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- the rule, restated ---------------------------------------------------------------------------------------------------
def base_sub_ref(x, y, E, B, inverse=False):
    """The filter alone, in the interleaved order: every element of a frame whose E bytes all lie below U = min(len(x),
    len(y)) becomes fold(x - y mod 2^(8E)) (inverse: unfold(z) + y); every other byte is XORed with pad(y)."""
    x = np.ascontiguousarray(x, np.uint8)
    n, F, dt = len(x), E * B, np.dtype("<u%d" % E)
    U, yp = min(n, len(y)), pad(y, n)
    out = x ^ yp
    one = dt.type(1)
    for f0 in range(0, n, F):
        N = min(F, n - f0) // E                       # the frame's elements
        K = min(N, max(0, U - f0) // E)               # of which the base covers the first K
        if K == 0:
            continue
        a, b = x[f0: f0 + K * E].copy().view(dt), yp[f0: f0 + K * E].copy().view(dt)
        if inverse:
            r = ((a >> one) ^ (dt.type(0) - (a & one))) + b
        else:
            d = a - b
            r = (d << one) ^ (dt.type(0) - (d >> dt.type(8 * E - 1)))
        out[f0: f0 + K * E] = r.astype(dt).view(np.uint8)
    return out


def base_sub_planes_ref(x, y, E, B, inverse=False):
    """what redux_base_sub_planes_dev computes: planes_ref(base_sub_ref(x, y)); the inverse undoes the layout first"""
    if inverse:
        return base_sub_ref(planes_ref(np.ascontiguousarray(x, np.uint8), E, B, inverse=True), y, E, B, inverse=True)
    return planes_ref(base_sub_ref(x, y, E, B), E, B)


def words(values, E):
    return np.array([v % (1 << 8 * E) for v in values], dtype="<u%d" % E).view(np.uint8)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_restatement_against_hand_written_expectations(rx, E):
    """x - y = 0, +1, -1, 2^(8E-1) (the most negative), a wrap (1 - max = 2), and a trailing odd byte; one frame (B = 8)"""
    top, full = 1 << (8 * E - 1), (1 << 8 * E) - 1
    y = words([5, 5, 5, 5, full, 7], E)
    x = words([5, 6, 4, 5 + top, 1, 7 - 3], E)
    z = words([0, 2, 1, full, 4, 5], E)
    tail = [] if E == 1 else [0xA5]
    ytail = [] if E == 1 else [0x0F]
    ztail = [] if E == 1 else [0xAA]
    xs, ys, zs = (np.concatenate([a, np.array(t, np.uint8)]) for a, t in ((x, tail), (y, ytail), (z, ztail)))
    assert base_sub_ref(xs, ys, E, 8).tolist() == zs.tolist()
    assert base_sub_ref(zs, ys, E, 8, inverse=True).tolist() == xs.tolist()
    assert base_sub_planes_ref(xs, ys, E, 8).tolist() == planes_ref(zs, E, 8).tolist()
    # B = 2: three frames of two elements and the short last frame that is the odd byte alone
    assert base_sub_ref(xs, ys, E, 2).tolist() == zs.tolist()


@pytest.mark.parametrize("E", [2, 4, 8])
def test_restatement_where_the_base_ends(rx, E):
    B = 4
    F = E * B
    rng = np.random.default_rng(E)
    x = rng.integers(0, 256, 2 * F + 3, dtype=np.uint8)
    y = rng.integers(0, 256, 3 * F, dtype=np.uint8)
    whole = base_sub_ref(x, y, E, B)
    # inside an element: elements 0 and 1 folded, the bytes of element 2 XORed with what the base has of them, the rest x
    U = 2 * E + 1
    got = base_sub_ref(x, y[:U], E, B)
    assert got[: 2 * E].tolist() == whole[: 2 * E].tolist()
    assert got[2 * E] == x[2 * E] ^ y[2 * E] and got[2 * E + 1:].tolist() == x[2 * E + 1:].tolist()
    # at an element boundary inside a frame, and exactly at a frame's end
    for U in (2 * E, F):
        got = base_sub_ref(x, y[:U], E, B)
        assert got[:U].tolist() == whole[:U].tolist() and got[U:].tolist() == x[U:].tolist()
    # the short last frame of 3 bytes: E = 2 one element and a trailing byte, E = 4 and 8 trailing bytes alone
    tail = whole[2 * F:]
    if E == 2:
        assert tail[:2].tolist() == base_sub_ref(x[2 * F: 2 * F + 2], y[2 * F: 2 * F + 2], 2, B).tolist()
        assert tail[2] == x[2 * F + 2] ^ y[2 * F + 2]
    else:
        assert tail.tolist() == (x[2 * F:] ^ y[2 * F: 2 * F + 3]).tolist()


def lengths(E, B):
    F = E * B
    return (0, 1, F - 1, F, F + 1, 3 * F + E + 1)


@pytest.mark.parametrize("B", [4, 100, 4096])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_restatement_round_trips(rx, E, B):
    assert callable(rx.base_sub_planes)
    rng = np.random.default_rng(E * 7 + B)
    for L in lengths(E, B):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for yl in sorted({0, 1, E - 1, max(L - 1, 0), L, L + 7}):
            y = rng.integers(0, 256, yl, dtype=np.uint8)
            d = base_sub_planes_ref(x, y, E, B)
            assert np.array_equal(base_sub_planes_ref(d, y, E, B, inverse=True), x), (E, B, L, yl)
            k = min(L, yl)
            assert np.array_equal(planes_ref(d, E, B, inverse=True)[k:], x[k:])        # past the base: x as it is
        assert not base_sub_planes_ref(x, x, E, B).any()                                # x == y: all-zero coder input
        assert np.array_equal(base_sub_planes_ref(x, b"", E, B), planes_ref(x, E, B))   # no base: the layout alone


# ---- the value claim, on the CPU oracle -------------------------------------------------------------------------------------
def as_bytes(w, dtype):
    """fp32 values -> the bytes of their fp32 or bf16 (round to nearest even) form"""
    u = w.astype("<f4").view(np.uint32)
    if dtype == "fp32":
        return u.view(np.uint8)
    return ((u + np.uint32(0x7FFF) + (u >> np.uint32(16) & np.uint32(1))) >> np.uint32(16)).astype("<u2").view(np.uint8)


def pairs(n_elements, seed=20261018):
    """tools/base_table.py's pairs(), restated: (name, dtype, E, base bytes, snapshot bytes) of every synthetic pair"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
    out = []
    for dtype, E in (("fp32", 4), ("bf16", 2)):
        for r in (1e-2, 1e-3, 1e-4):
            w2 = (w * (1 + np.float32(r) * rng.standard_normal(n_elements).astype(np.float32))).astype(np.float32)
            out.append((f"relative update {r:g}", dtype, E, as_bytes(w, dtype), as_bytes(w2, dtype)))
        out.append(("identical pair", dtype, E, as_bytes(w, dtype), as_bytes(w, dtype)))
        other = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
        out.append(("unrelated pair", dtype, E, as_bytes(other, dtype), as_bytes(w, dtype)))
    return out


def stream_bytes(planes, B):
    streams, status = ox.compress_blocks(planes, B, PARAMS)
    assert not np.asarray(status).any()
    return sum(len(s) for s in streams)


def test_folded_difference_is_smaller_than_xor_on_related_pairs_and_no_worse_on_unrelated_ones(rx):
    """B = 4096, 3 * 4096 + 100 elements, stream bytes of the CPU oracle behind either operation.  Measured: fp32 1e-3 0.944,
    bf16 1e-2 0.845, unrelated 1.004 / 1.009.  Synthetic pairs: no real checkpoint series was measured."""
    B = 4096
    bounds = {("relative update 0.001", "fp32"): 0.96, ("relative update 0.01", "bf16"): 0.88,
              ("unrelated pair", "fp32"): 1.02, ("unrelated pair", "bf16"): 1.02}
    seen = set()
    for name, dtype, E, y, x in pairs(3 * 4096 + 100):
        xor = stream_bytes(base_planes_ref(x, y, E, B), B)
        sub = stream_bytes(base_sub_planes_ref(x, y, E, B), B)
        print(f"{name} | {dtype} | XOR {xor} | folded difference {sub} | {sub / xor:.3f}")
        if name == "identical pair":
            assert sub == xor
            seen.add((name, dtype))
        if (name, dtype) in bounds:
            assert sub <= bounds[(name, dtype)] * xor, (name, dtype, xor, sub)
            seen.add((name, dtype))
    assert len(seen) == 6


# ---- container version 12 -----------------------------------------------------------------------------------------------
def test_container_v12_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    v1 = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL)
    assert container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, base_op="xor") == v1
    assert container.base_op(v1) is None
    crc = np.array([1, 2, 3], dtype=np.uint32)
    record = (12345, 0xDEADBEEF)
    for E in (1, 2, 4, 8):
        v8 = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=E, base=record)
        assert container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=E, base=record, base_op="xor") == v8
        v12 = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=E, base=record, base_op="sub")
        assert v12[4] == 12 and int.from_bytes(v12[12:16], "little") == 0xC0000000 | E
        assert v12[:4] + v12[5:12] + v12[16:] == v8[:4] + v8[5:12] + v8[16:]   # version 8 but for the version byte and the word
        c = container._parse(v12)
        assert c.params.triple() == PARAMS and c.block_size == 65536 and c.total == TOTAL and c.element_size == E
        assert c.base == record and c.base_op == "sub" and c.filter is None and c.static is None and c.crcs is None
        assert c.stored is None and c.constant is None and c.unit_layouts is None
        assert c.offsets.tolist() == OFFS.tolist() and c.payload.tobytes() == STREAMS.tobytes()
        assert container.base(v12) == record and container.base_op(v12) == "sub" and container.base_op(v8) == "xor"
        assert container.element_size(v12) == E and container.header_is_wellformed(v12) and container.filter(v12) is None
        v1c = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=E, block_crc=crc, base=record, base_op="sub")
        v18 = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=E, block_crc=crc, base=record)
        assert v1c[4] == 0x1C and container.base(v1c) == record and container.block_crcs(v1c).tolist() == [1, 2, 3]
        assert container.base_op(v1c) == "sub" and container._parse(v1c).payload.tobytes() == STREAMS.tobytes()
        assert v1c[:4] + v1c[5:12] + v1c[16:] == v18[:4] + v18[5:12] + v18[16:]
        nb = len(OFFS) - 1
        assert len(v12) - len(STREAMS) == container.overhead_bytes("adaptive", nb, E, base=True)
        assert len(v1c) - len(STREAMS) == container.overhead_bytes("adaptive", nb, E, checksum=True, base=True)
    assert container.overhead_bytes("adaptive", 3) == container.overhead_bytes("adaptive", 3, base=True) - 12
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("static", 3, base=True)


def test_container_base_op_of_every_version(rx):
    from redux_amd import container
    flags = np.array([0, 0, 0], np.uint8)
    pk = lambda **kw: container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, **kw)
    assert container.base_op(pk()) is None and container.base_op(pk(element_size=2)) is None
    assert container.base_op(pk(filter="delta")) is None and container.base_op(pk(filter="zigzag")) is None
    assert container.base_op(pk(base=(5, 6))) == "xor"
    assert container.base_op(pk(constant=flags)) is None
    assert container.base_op(pk(constant=flags, base=(5, 6))) == "xor"
    assert container.base_op(pk(base=(5, 6), base_op="sub", element_size=4)) == "sub"


def test_container_v12_truncated_is_eof_and_a_record_beyond_the_total_invalid(rx):
    from redux_amd import container
    crc = np.array([1, 2, 3], dtype=np.uint32)
    v = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=2, block_crc=crc, base=(9, 9), base_op="sub")
    assert len(v) == 32 + 12 + 12 + 12 + 10
    for cut in (31, 32, 33, 43, 44, 45, 55, 56, 57, 67, 68, 69, len(v) - 1):
        with pytest.raises(rx.Eof):
            container._parse(v[:cut])
        with pytest.raises(rx.Eof):
            container.base_op(v[:cut])
    container._parse(v)
    over = bytearray(v)
    over[32:40] = (TOTAL + 1).to_bytes(8, "little")  # more of the base than there is data
    with pytest.raises(rx.InvalidInput):
        container._parse(bytes(over))


def test_container_v12_takes_its_word_alone_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, PARAMS, 65536, 10, element_size=2, base=(10, 1), base_op="sub")
    assert container.header_is_wellformed(good) and good[4] == 12
    for ver in [v for v in range(1, 12)] + [0x10 | v for v in range(1, 12)] + [0x4C, 0x5C, 0x2C, 0x8C, 13, 0x1D]:
        bad = bytearray(good)   # no other version takes version 12's word, and it has no stored blocks
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), hex(ver)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    for word in (0, 2, 0x00020002, 0x50000012, 0x60000002, 0x70000000, 0x80000002, 0x90000002, 0x90000012, 0xA0000000, 0xB0000002,
                 0xC0000000, 0xC0000003, 0xC0000010, 0xC0000102, 0xD0000002):
        for ver in (12, 0x1C):   # nor does version 12 take another version's word
            bad = bytearray(good)
            bad[4] = ver
            bad[12:16] = word.to_bytes(4, "little")
            assert not container.header_is_wellformed(bytes(bad)), hex(word)
            with pytest.raises(rx.InvalidInput):
                container._parse(bytes(bad))
    flags = np.zeros(1, np.uint8)
    for kw in ({"element_size": 3}, {"stored": flags}, {"filter": "delta"}, {"filter": "zigzag"}, {"constant": flags}, {"base": None},
               {"base": (11, 1)}, {"base_op": "add"}, {"base_op": None}, {"unit_layouts": flags}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, PARAMS, 65536, 10, **{"base": (10, 1), "base_op": "sub", **kw})
    for model in (rx.StaticModel(PARAMS, np.arange(258)), rx.PlaneStaticModel(PARAMS, np.tile(np.arange(258), (2, 1))),
                  rx.SegmentStaticModel.template(PARAMS, 2)):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, model, 65536, 10, base=(10, 1), base_op="sub")


def test_decompress_bytes_checks_the_base_of_version_12_before_any_library_call(rx, monkeypatch):
    from redux_amd import container
    y = bytes(range(200)) * 3
    v12 = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=2, base=(500, zlib.crc32(y[:500])), base_op="sub")
    wrong = bytearray(y)
    wrong[499] ^= 1
    header_parse_only(monkeypatch)
    for bad in (None, y[:499], b"", bytes(wrong)):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(v12, base=bad)
        with pytest.raises(rx.InvalidInput):
            container.decompress_range(v12, 0, 10, base=bad)
    for ok in (y[:500], y):
        with pytest.raises(AssertionError, match="the library was loaded"):
            container.decompress_bytes(v12, base=ok)


# ---- refusals before the library is touched ---------------------------------------------------------------------------------
def test_python_api_refuses_base_op_before_any_library_call(rx, monkeypatch):
    from redux_amd import api, container
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    static = rx.StaticModel(PARAMS, np.arange(258))
    no_library(monkeypatch)
    y = b"abcd"
    calls = []
    for op in ("add", "SUB", "", None, 1, b"sub", "auto"):   # any other value, with and without a base
        calls += [lambda op=op: rx.compress_blocks(b"abcd", 4, base=y, base_op=op),
                  lambda op=op: rx.compress_blocks(b"abcd", 4, base_op=op),
                  lambda op=op: rx.decompress_blocks(b"\0", offs, 4, length=4, base=y, base_op=op),
                  lambda op=op: rx.DeviceEncoder(PARAMS, 4096, 4096, base=y, base_op=op),
                  lambda op=op: rx.DeviceDecoder(PARAMS, 4096, 1, base=y, base_op=op),
                  lambda op=op: container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, base=(1, 1), base_op=op)]
        if op != "auto":
            calls += [lambda op=op: container.compress_bytes(b"abcd" * 4, 16, base=y, base_op=op)]
    calls += [lambda: rx.compress_blocks(b"abcd", 4, base_op="sub"),                                    # "sub" without a base
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, base_op="sub"),
              lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, base_op="sub"),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, base_op="auto"),
              lambda: container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, base_op="sub"),
              lambda: rx.compress_blocks(b"abcd", 4, base=y, constant=True, base_op="sub"),             # "sub" with constant=
              lambda: rx.compress_blocks(b"abcd", 4, base=y, constant=flags, base_op="sub"),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, base=y, constant=flags, base_op="sub"),
              lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, base=y, constant=True, base_op="sub"),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, base=y, constant=True, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, base=y, skip_constant=True, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, base=y, skip_constant=True, base_op="auto"),
              # and wherever the base itself is refused
              lambda: rx.compress_blocks(b"abcd", 4, static, base=y, base_op="sub"),
              lambda: rx.compress_blocks(b"abcd", 4, filter="delta", base=y, base_op="sub"),
              lambda: rx.compress_blocks(b"abcd", 4, stored=flags, base=y, base_op="sub"),
              lambda: rx.compress_blocks(b"abcd", 4, unit_layouts=True, base=y, base_op="sub"),
              lambda: rx.decompress_blocks(b"\0", offs, 4, base=y, base_op="sub"),                      # the base needs the length
              lambda: container.compress_bytes(b"abcd" * 4, 16, model="static", base=y, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, layout="auto", base=y, base_op="sub"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, filter="zigzag", base=y, base_op="auto")]
    for i, call in enumerate(calls):
        with pytest.raises(rx.InvalidInput):
            call()
    front = lambda op, base, constant=None: api._resolve_front(None, base=base, base_op=op, constant=constant).front.infix
    assert front("xor", None) == "planes" and front("xor", y) == "base" and front("sub", y) == "base_sub"
    assert front("xor", y, True) == "base" and front("sub", y, False) == "base_sub"
    # base_op is the last keyword wherever base= is taken
    import inspect
    for f in (rx.compress_blocks, rx.decompress_blocks, rx.DeviceEncoder.__init__, rx.DeviceDecoder.__init__, container.compress_bytes,
              container.pack):
        assert list(inspect.signature(f).parameters)[-1] == "base_op", f
        assert inspect.signature(f).parameters["base_op"].default == "xor", f


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_base_op_flag(rx):
    from redux_amd import cli
    want = {"compress": True, "input": None, "output": None, "block_size": 65536, "base": "prev.bin"}
    for op in ("xor", "sub", "auto"):
        assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin", "--base-op", op]) == {**want, "base_op": op}
        assert cli.parse(["-c", "--base-op", op, "--block-size", "65536", "--base", "prev.bin", "--checksum"]) == \
            {**want, "base_op": op, "checksum": True}
        assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin", "--base-op", op, "--model", "adaptive"]) == \
            {**want, "base_op": op, "model": "adaptive"}
        for E in ("1", "2", "4", "8"):
            got = cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--base", "b", "--base-op", op])
            assert got["element_size"] == int(E) and got["base_op"] == op
    assert cli.parse(["-c", "--block-size", "65536", "--base", "b", "--base-op", "xor", "--skip-constant"])["skip_constant"]
    assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin"]) == want      # without the flag: as before
    assert cli.parse(["-d", "--base", "prev.bin"]) == {"compress": False, "input": None, "output": None, "block_size": 0,
                                                       "base": "prev.bin"}
    assert cli.parse(["-d", "--base", "prev.bin", "--range", "5:7"])["range"] == (5, 7)
    bads = [["-d", "--base", "b", "--base-op", "sub"], ["-d", "--base", "b", "--base-op", "xor"], ["-d", "--base-op", "sub"],
            ["-d", "--base", "b", "--range", "0:1", "--base-op", "sub"],
            ["-c", "--block-size", "65536", "--base-op", "sub"], ["-c", "--block-size", "65536", "--base-op", "xor"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op"], ["-c", "--block-size", "65536", "--base", "b", "--base-op", "add"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "SUB"],
            ["-c", "--base", "b", "--base-op", "sub"], ["-c", "--block-size", "0", "--base", "b", "--base-op", "sub"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--skip-constant"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "auto", "--skip-constant"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--stored"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--filter", "delta"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "auto", "--filter", "zigzag"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--layout", "auto"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--layout", "mixed"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--model", "static"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--model", "auto"],
            ["-c", "--block-size", "65536", "--base", "b", "--base-op", "sub", "--model", "segment-static"],
            ["--base", "b", "--base-op", "sub"]]
    for bad in bads:
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
    assert "--base-op" in cli.USAGE and "xor|sub|auto" in cli.USAGE and "--base-op sub" in cli.__doc__ and "version 12" in cli.__doc__


def test_cli_decode_of_version_12_exits_3_on_a_missing_or_wrong_base(rx, tmp_path, capsys):
    from redux_amd import cli, container
    y = tmp_path / "y.bin"
    y.write_bytes(bytes(600))
    v12 = tmp_path / "v12.rdxb"
    v12.write_bytes(container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=2, base=(600, zlib.crc32(bytes(600)) ^ 1),
                                   base_op="sub"))
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(599))
    capsys.readouterr()
    for argv in (["-d", "-i", str(v12), "-o", str(tmp_path / "o")],
                 ["-d", "-i", str(v12), "-o", str(tmp_path / "o"), "--base", str(short)],
                 ["-d", "-i", str(v12), "-o", str(tmp_path / "o"), "--base", str(y)],
                 ["-d", "-i", str(v12), "-o", str(tmp_path / "o"), "--base", str(y), "--range", "0:10"]):
        assert cli.main(argv) == 3, argv
        assert capsys.readouterr().err.startswith("Decompression error"), argv


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_base_sub_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        assert L.redux_base_sub_check(E) == (_lib.OK if E in (1, 2, 4, 8) else _lib.INVALID_INPUT), E
    assert L.redux_base_sub_check(0xFFFFFFFF) == _lib.INVALID_INPUT
    for params in (PARAMS, (8, 14, 16), (4, 10, 16), (8, 9, 16)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            for E in (0, 1, 2, 3, 4, 8, 16):
                assert L.redux_encode_base_sub_workspace_bytes(C.byref(p), n, B, E) == L.redux_encode_base_workspace_bytes(C.byref(p), n, B, E)
                assert L.redux_decode_base_sub_workspace_bytes(C.byref(p), n, B, E) == L.redux_decode_base_workspace_bytes(C.byref(p), n, B, E)
    for name in ("redux_base_sub_check", "redux_base_sub_planes_dev", "redux_encode_base_sub_workspace_bytes",
                 "redux_decode_base_sub_workspace_bytes", "redux_encode_base_sub_dev", "redux_decode_base_sub_dev",
                 "redux_encode_blocks_base_sub", "redux_decode_blocks_base_sub"):
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("base_sub", "base")], name


def test_base_sub_argument_checks_come_before_any_device_work(rx):
    from redux_amd import _lib
    L = _lib.lib()
    ok = _lib.Params(*PARAMS)
    V = C.c_void_p
    src, base, dst = V(1 << 20), V(2 << 20), V(3 << 20)
    dev = L.redux_base_sub_planes_dev
    assert dev(src, base, 16, dst, 16, 4, 3, 0, None) == _lib.INVALID_INPUT          # bad E
    assert dev(src, base, 16, dst, 16, 0, 2, 0, None) == _lib.INVALID_INPUT          # block size 0
    assert dev(None, base, 16, dst, 16, 4, 2, 0, None) == _lib.INVALID_INPUT         # null pointers with nonzero lengths
    assert dev(src, base, 16, None, 16, 4, 2, 0, None) == _lib.INVALID_INPUT
    assert dev(src, None, 16, dst, 16, 4, 2, 0, None) == _lib.INVALID_INPUT
    assert dev(src, None, 1, dst, 0, 4, 2, 0, None) == _lib.INVALID_INPUT
    for inverse in (0, 1):
        assert dev(src, base, 16, V((1 << 20) + 8), 16, 4, 2, inverse, None) == _lib.INVALID_INPUT    # dst overlaps src
        assert dev(src, base, 16, V((1 << 20) - 8), 16, 4, 2, inverse, None) == _lib.INVALID_INPUT
        assert dev(src, base, 16, V((2 << 20) + 8), 16, 4, 2, inverse, None) == _lib.INVALID_INPUT    # dst overlaps base
        assert dev(src, base, 16, V((2 << 20) - 8), 16, 4, 2, inverse, None) == _lib.INVALID_INPUT
        assert dev(src, base, 1 << 30, V((2 << 20) + 15), 16, 4, 2, inverse, None) == _lib.INVALID_INPUT  # (a long base: its first len bytes)
    assert dev(None, None, 0, None, 0, 4, 2, 0, None) == _lib.OK                     # len == 0
    assert dev(None, base, 16, None, 0, 4, 2, 0, None) == _lib.OK
    enc, dec = L.redux_encode_blocks_base_sub, L.redux_decode_blocks_base_sub
    x = np.zeros(16, np.uint8)
    out = np.zeros(64, np.uint8)
    offs = np.zeros(5, np.uint64)
    sizes = np.zeros(4, np.uint32)
    px, po, pf, ps = x.ctypes.data, out.ctypes.data, offs.ctypes.data, sizes.ctypes.data
    assert enc(C.byref(ok), px, 16, px, 16, 4, 3, po, 64, pf, None, None) == _lib.INVALID_INPUT      # bad E
    assert enc(C.byref(ok), px, 16, px, 16, 0, 2, po, 64, pf, None, None) == _lib.INVALID_INPUT      # block size 0
    assert enc(C.byref(ok), None, 16, px, 16, 4, 2, po, 64, pf, None, None) == _lib.INVALID_INPUT    # null input
    assert enc(C.byref(ok), px, 16, None, 16, 4, 2, po, 64, pf, None, None) == _lib.INVALID_INPUT    # null base with a length
    assert enc(C.byref(ok), px, 16, px, 16, 4, 2, None, 64, pf, None, None) == _lib.INVALID_INPUT
    assert enc(C.byref(ok), px, 16, px, 16, 4, 2, po, 64, None, None, None) == _lib.INVALID_INPUT
    assert enc(C.byref(_lib.Params(8, 9, 16)), px, 16, px, 16, 4, 2, po, 64, pf, None, None) == _lib.INVALID_INPUT
    assert dec(C.byref(ok), po, pf, px, 16, 16, 4, 3, px, ps, None, None) == _lib.INVALID_INPUT      # bad E
    assert dec(C.byref(ok), po, pf, px, 16, 16, 0, 2, px, ps, None, None) == _lib.INVALID_INPUT      # block size 0
    assert dec(C.byref(ok), po, pf, None, 16, 16, 4, 2, px, ps, None, None) == _lib.INVALID_INPUT    # null base with a length
    assert dec(C.byref(ok), po, None, px, 16, 16, 4, 2, px, ps, None, None) == _lib.INVALID_INPUT
    assert dec(C.byref(ok), po, pf, px, 16, 16, 4, 2, None, ps, None, None) == _lib.INVALID_INPUT
    assert dec(C.byref(ok), po, pf, px, 16, 16, 4, 2, px, None, None, None) == _lib.INVALID_INPUT


# ---- range reads ---------------------------------------------------------------------------------------------------------
class RecordingSource:
    """a seekable source that records what was fetched from it"""

    def __init__(self, data):
        self.data, self.at, self.reads = bytes(data), 0, []

    def seek(self, at, whence=0):
        self.at = at if whence == 0 else len(self.data) + at
        return self.at

    def read(self, n):
        self.reads.append((self.at, n))
        got = self.data[self.at: self.at + n]
        self.at += len(got)
        return got


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_reader_reports_the_operation_and_a_granule_of_a_frame(rx, E):
    from redux_amd import container
    nb, B = 19, 4096
    streams = np.arange(3 * nb, dtype=np.uint8)
    offs = np.arange(0, 3 * nb + 1, 3).astype(np.uint64)
    total = nb * B - 7
    y = bytes(range(256)) * 4
    record = (len(y), zlib.crc32(y))
    for crc in (None, np.arange(nb, dtype=np.uint32)):
        buf = container.pack(streams, offs, PARAMS, B, total, element_size=E, block_crc=crc, base=record, base_op="sub")
        src = RecordingSource(buf)
        r = container.Reader(src, y)
        assert r.base_op == "sub" and r.filter is None and r.granule_blocks == E and r.version == (12 if crc is None else 0x1C)
        assert r.total == total and r.block_size == B and r.nblocks == nb
        assert r.payload_offset == len(buf) - len(streams) and r.bytes_read == r.payload_offset
        assert sum(n for _, n in src.reads) == r.payload_offset          # the header, the record and the index, no payload
        assert r.read(5, 0) == b"" and r.bytes_read == r.payload_offset  # no bytes asked for: no coder call
        x = container.Reader(container.pack(streams, offs, PARAMS, B, total, element_size=E, block_crc=crc, base=record), y)
        assert x.base_op == "xor" and x.granule_blocks == E and x.payload_offset == r.payload_offset
        with pytest.raises(rx.InvalidInput):
            container.Reader(buf)                                        # no base
        with pytest.raises(rx.InvalidInput):
            container.Reader(buf, y[:-1])
    assert container.Reader(container.pack(streams, offs, PARAMS, B, total, element_size=E)).base_op is None


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_base_sub_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "base_sub_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "base_sub_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_base_sub_mirror_compiles_and_refuses(rx, tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_base_sub_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "base sub mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
