"""Delta filter for integer series (include/redux_hip.h, "delta filter"): the numpy restatement of the rule against
hand-written expectations, the value claim on the CPU oracle, container version 6, the CLI flag, the Python argument
checks and the host-only ABI helpers.  No GPU call.

The value claim rests on GENERATED integer series: nothing in the corpus fixtures benefits from the filter."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_cpu import bf16_data, lengths, oracle_bytes, planes_ref


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def delta_ref(x, E, B, inverse=False):
    """The rule: frames of E*B bytes (the last may be shorter); a frame of L bytes holds N = L // E little-endian unsigned
    elements, d[0] = x[0], d[i] = x[i] - x[i-1] mod 2^(8E), the L - N*E trailing bytes unchanged.  inverse=True takes the
    running sum mod 2^(8E) inside each frame.  (The byte-plane layout is planes_ref's, applied behind this.)"""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    out = x.copy()
    dt = np.dtype("<u%d" % E)
    F = E * B
    for f0 in range(0, len(x), F):
        fr = x[f0: f0 + F]
        N = len(fr) // E
        if N:
            v = fr[: N * E].copy().view(dt)
            if inverse:
                r = np.cumsum(v, dtype=dt)  # (wraps mod 2^(8E))
            else:
                r = v.copy()
                r[1:] = v[1:] - v[:-1]
            out[f0: f0 + N * E] = r.view(np.uint8)
    return out


def delta_planes_ref(x, E, B, inverse=False):
    """what redux_delta_planes_dev computes: the filter, then the layout; the inverse the other way round"""
    if inverse:
        return delta_ref(planes_ref(x, E, B, inverse=True), E, B, inverse=True)
    return planes_ref(delta_ref(x, E, B), E, B)


# x[k] = 3 k + 1 (no byte reaches 256, no borrow between bytes); the filter by hand for B = 4.  Neighbouring elements
# differ by 3 (E = 1), 6 in both bytes (E = 2), 12 in all four bytes (E = 4).
HAND = {
    (1, 0): [], (1, 1): [1], (1, 3): [1, 3, 3], (1, 4): [1, 3, 3, 3], (1, 5): [1, 3, 3, 3, 13],
    (1, 17): [1, 3, 3, 3, 13, 3, 3, 3, 25, 3, 3, 3, 37, 3, 3, 3, 49],
    (2, 0): [], (2, 1): [1],
    (2, 7): [1, 4, 6, 6, 6, 6, 19],                               # 3 elements + 1 trailing byte
    (2, 8): [1, 4] + [6] * 6, (2, 9): [1, 4] + [6] * 6 + [25],
    (2, 29): [1, 4] + [6] * 6 + [25, 28] + [6] * 6 + [49, 52] + [6] * 6 + [73, 76, 6, 6, 85],
    (4, 0): [], (4, 1): [1], (4, 3): [1, 4, 7],
    (4, 15): [1, 4, 7, 10] + [12] * 8 + [37, 40, 43],             # 3 elements + 3 trailing bytes
    (4, 16): [1, 4, 7, 10] + [12] * 12, (4, 17): [1, 4, 7, 10] + [12] * 12 + [49],
    (4, 53): [1, 4, 7, 10] + [12] * 12 + [49, 52, 55, 58] + [12] * 12 + [97, 100, 103, 106] + [12] * 12
             + [145, 148, 151, 154, 157],                         # last frame: 1 element + 1 trailing byte
}


@pytest.mark.parametrize("E", [1, 2, 4])
def test_filter_matches_hand_written_expectations(E):
    B = 4
    for L in lengths(E, B):
        x = (3 * np.arange(L) + 1).astype(np.uint8)
        got = delta_ref(x, E, B)
        assert got.tolist() == HAND[(E, L)], (E, L)
        assert delta_ref(got, E, B, inverse=True).tolist() == x.tolist(), (E, L)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_wrap_around_both_ways(E):
    dt = np.dtype("<u%d" % E)
    top = (1 << 8 * E) - 1
    x = np.array([top, 0, top], dtype=dt).view(np.uint8)            # 0 - 0xFF..F = 1, 0xFF..F - 0 = 0xFF..F
    d = delta_ref(x, E, 16)
    assert d.view(dt).tolist() == [top, 1, top]
    assert delta_ref(d, E, 16, inverse=True).view(dt).tolist() == [top, 0, top]   # 0xFF..F + 1 = 0
    # a frame is a fresh start: with B = 1 every element is a frame of its own
    assert delta_ref(x, E, 1).tolist() == x.tolist()
    if E > 1:  # no borrow from an element into its neighbour in memory
        lo = (1 << 8 * (E - 1))
        y = np.array([lo, lo - 1, lo - 1, 0], dtype=dt).view(np.uint8)
        assert delta_ref(y, E, 16).view(dt).tolist() == [lo, top, 0, top - lo + 2]


@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [4, 100, 4096])
def test_inverse_of_forward_is_identity(E, B):
    rng = np.random.default_rng(E * 10000 + B)
    for L in lengths(E, B):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        y = delta_planes_ref(x, E, B)
        assert len(y) == L
        assert np.array_equal(delta_planes_ref(y, E, B, inverse=True), x), (E, B, L)
        assert np.array_equal(delta_ref(delta_ref(x, E, B), E, B, inverse=True), x), (E, B, L)
        N = min(L, E * B) // E
        if N:  # the first element of a frame travels as it is
            assert np.array_equal(delta_ref(x, E, B)[:E], x[:E])


# ---- the value claim, on the CPU oracle --------------------------------------------------------------------------------
# Generated integer series, 2 MiB each (the int16 one 1 MiB), B = 65536, params (8, 30, 32).  The bounds are the issue's;
# measured with these generators: timestamps 0.338, sorted 0.464, tones 0.635 of the byte planes' size; bf16 1.055.
def timestamps_i64(seed=11):
    rng = np.random.default_rng(seed)
    return (1_700_000_000_000_000 + np.cumsum(rng.integers(900, 1100, 262144))).astype("<u8").view(np.uint8)


def sorted_i32(seed=12):
    return np.sort(np.random.default_rng(seed).integers(0, 1 << 30, 524288)).astype("<u4").view(np.uint8)


def tones_i16(seed=13):
    t = np.arange(524288)
    s = 9000 * np.sin(2 * np.pi * t / 600.0) + 5000 * np.sin(2 * np.pi * t / 173.0) \
        + np.random.default_rng(seed).normal(0, 20, len(t))
    return np.round(s).astype("<i2").view(np.uint8)


@pytest.mark.parametrize("name,gen,E,bound", [("int64 timestamps", timestamps_i64, 8, 0.5), ("sorted int32", sorted_i32, 4, 0.6),
                                              ("int16 tones", tones_i16, 2, 0.75)])
def test_filter_pays_on_integer_series(name, gen, E, bound):
    B = 65536
    x = gen()
    planes = oracle_bytes(planes_ref(x, E, B), B)
    delta = oracle_bytes(delta_planes_ref(x, E, B), B)
    print("%s: byte planes %.4f, delta + byte planes %.4f of the input, %.3f x" % (name, planes / len(x), delta / len(x), delta / planes))
    assert delta <= bound * planes, (name, planes, delta)


def test_filter_costs_on_bf16_which_is_why_it_is_not_a_default():
    B = 65536
    x = bf16_data(8 * B // 2)
    planes = oracle_bytes(planes_ref(x, 2, B), B)
    delta = oracle_bytes(delta_planes_ref(x, 2, B), B)
    print("bf16 N(0, 0.02): byte planes %.4f, delta + byte planes %.4f of the input, %.3f x" % (planes / len(x), delta / len(x), delta / planes))
    assert delta > planes, (planes, delta)


# ---- container version 6 ------------------------------------------------------------------------------------------------
def test_container_v6_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    v1 = container.pack(streams, offs, (8, 30, 32), 65536, total)
    assert container.pack(streams, offs, (8, 30, 32), 65536, total, filter=None) == v1   # no filter: today's bytes
    assert container.filter(v1) is None
    crc = np.array([1, 2, 3], dtype=np.uint32)
    for E in (1, 2, 4, 8):
        plain = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E)
        assert container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, filter=None) == plain
        assert container.filter(plain) is None
        v6 = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, filter="delta")
        assert v6[4] == 6 and int.from_bytes(v6[12:16], "little") == 0x60000000 | E
        assert v6[:4] + v6[5:12] + v6[16:] == v1[:4] + v1[5:12] + v1[16:]  # version 2's sections
        c = container._parse(v6)
        assert c.params.triple() == (8, 30, 32) and c.block_size == 65536 and c.total == total and c.element_size == E
        assert c.filter == "delta" and c.static is None and c.crcs is None and c.stored is None
        assert c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == streams.tobytes()
        assert container.filter(v6) == "delta" and container.element_size(v6) == E and container.header_is_wellformed(v6)
        v16 = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, block_crc=crc, filter="delta")
        assert v16[4] == 0x16 and container.filter(v16) == "delta" and container.block_crcs(v16).tolist() == [1, 2, 3]
        assert container._parse(v16).payload.tobytes() == streams.tobytes()
        for cut in (len(v16) - 1, len(v16) - 11, 32 + 12 + 11, 32 + 11, 33):  # payload, CRC table, size table
            with pytest.raises(rx.Eof):
                container._parse(v16[:cut])
        with pytest.raises(rx.Eof):
            container._parse(v6[:31])


def test_container_v6_requires_its_marker_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=2, filter="delta")
    for word in (0, 2, 0x50000012, 0x60000000, 0x60000003, 0x60000010, 0x60000102, 0x70000002):
        bad = bytearray(good)
        bad[12:16] = word.to_bytes(4, "little")
        assert not container.header_is_wellformed(bytes(bad)), hex(word)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
        with pytest.raises(rx.InvalidInput):
            container.filter(bytes(bad))
    for ver in (0x46, 0x56, 0x26, 0x86):
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), hex(ver)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    for ver in (1, 2, 3, 4, 5):  # no other version takes version 6's word
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), ver
    flags = np.zeros(1, np.uint8)
    for kw in ({"element_size": 3}, {"stored": flags}, {"filter": "xor"}, {"filter": True}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, (8, 30, 32), 65536, 10, **{"filter": "delta", **kw})
    static = rx.StaticModel((8, 30, 32), np.arange(258))
    with pytest.raises(rx.InvalidInput):
        container.pack(streams, offs, static, 65536, 10, filter="delta")
    for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"}, {"stored": True}):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(b"abcd" * 4, 16, filter="delta", **kw)
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(b"abcd" * 4, 16, filter="xor")


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_filter_flag(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "delta"]) == {**base, "filter": "delta"}
    assert cli.parse(["-c", "--block-size", "65536"]) == base
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "delta"])["element_size"] == int(E)
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "delta", "--model", "adaptive", "--checksum"])["filter"] == "delta"
    for bad in (["-c", "--filter", "delta"], ["-c", "--block-size", "0", "--filter", "delta"],
                ["-c", "--block-size", "65536", "--filter", "delta", "--stored"],
                ["-c", "--block-size", "65536", "--filter", "delta", "--model", "static"],
                ["-c", "--block-size", "65536", "--element-size", "2", "--filter", "delta", "--model", "plane-static"],
                ["-c", "--block-size", "65536", "--filter", "delta", "--model", "segment-static"],
                ["-c", "--block-size", "65536", "--filter", "xor"], ["-c", "--block-size", "65536", "--filter"]):
        assert cli.parse(bad) is None, bad
    assert cli.main(["-c", "--filter", "delta"]) == 1
    assert cli.main(["-c", "--block-size", "65536", "--filter", "delta", "--stored"]) == 1
    assert "--filter" in cli.USAGE and "--filter delta" in cli.__doc__


# ---- Python argument checks ----------------------------------------------------------------------------------------------
def test_python_api_refuses_the_filter_where_it_is_not_available_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api
    static = rx.StaticModel((8, 30, 32), np.arange(258))
    plane = rx.PlaneStaticModel((8, 30, 32), np.tile(np.arange(258), (2, 1)))
    segment = rx.SegmentStaticModel.template((8, 30, 32), 2)
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    adaptive = rx.AdaptiveTreeModel.new(rx.Parameters(8, 30, 32))

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    import io
    calls = [lambda m=m: rx.compress_blocks(b"abcd", 4, m, filter="delta") for m in (static, plane, segment)]
    calls += [lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, filter="delta") for m in (static, plane, segment)]
    calls += [lambda: rx.compress_blocks(b"abcd", 4, stored=flags, filter="delta"),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, stored=flags, filter="delta"),
              lambda: rx.decompress_blocks(b"\0", offs, 4, filter="delta"),                  # the filter needs the length
              lambda: rx.compress_blocks(b"abcd", 4, filter="xor"), lambda: rx.compress_blocks(b"abcd", 4, filter=1),
              lambda: rx.compress_blocks_v([b"abcd"], 4, filter="delta"),
              lambda: rx.decompress_blocks_v(b"\0", offs, [4], 4, filter="delta"),
              lambda: rx.compress(io.BytesIO(b"abcd"), io.BytesIO(), adaptive, filter="delta"),
              lambda: rx.decompress(io.BytesIO(b"\0"), io.BytesIO(), adaptive, filter="delta"),
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter="xor"),
              lambda: rx.DeviceDecoder((8, 30, 32), 4096, 1, filter="xor")]
    for i, call in enumerate(calls):
        with pytest.raises(rx.InvalidInput):
            call()
    assert api._resolve_front(None).front.infix == "planes" and api._resolve_front(None, filter="delta").front.infix == "delta"


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_delta_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        assert L.redux_delta_check(E) == (_lib.OK if E in (1, 2, 4, 8) else _lib.INVALID_INPUT), E
    assert L.redux_delta_check(0xFFFFFFFF) == _lib.INVALID_INPUT
    for params in ((8, 30, 32), (8, 14, 16), (4, 10, 16)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            plain_e = L.redux_encode_workspace_bytes(C.byref(p), n, B)
            plain_d = L.redux_decode_workspace_bytes(C.byref(p), L.redux_block_count(n, B), B)
            for E in (1, 2, 4, 8):  # E = 1 too: the filter changes the bytes, so the coder needs the transformed copy
                we = L.redux_encode_delta_workspace_bytes(C.byref(p), n, B, E)
                wd = L.redux_decode_delta_workspace_bytes(C.byref(p), n, B, E)
                assert we >= plain_e + n + 16 and wd >= plain_d + n, (params, n, B, E)
                assert we % 256 == plain_e % 256
                assert we == L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, 2)
                assert wd == L.redux_decode_planes_workspace_bytes(C.byref(p), n, B, E)
            assert L.redux_encode_delta_workspace_bytes(C.byref(p), n, B, 1) > L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, 1)
            for bad in (0, 3, 16):
                assert L.redux_encode_delta_workspace_bytes(C.byref(p), n, B, bad) == 0
                assert L.redux_decode_delta_workspace_bytes(C.byref(p), n, B, bad) == 0
    p = _lib.Params(8, 9, 16)  # invalid triple
    assert L.redux_encode_delta_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    assert L.redux_decode_delta_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    # argument checks of the device calls come before any device work
    ok = _lib.Params(8, 30, 32)
    assert L.redux_delta_planes_dev(None, None, 16, 4, 3, 0, None) == _lib.INVALID_INPUT
    assert L.redux_delta_planes_dev(None, None, 16, 0, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_delta_planes_dev(None, None, 16, 4, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_delta_planes_dev(None, None, 0, 4, 2, 0, None) == _lib.OK
    assert L.redux_delta_planes_dev(C.c_void_p(4096), C.c_void_p(4096 + 8), 16, 4, 2, 0, None) == _lib.INVALID_INPUT  # overlap
    assert L.redux_encode_blocks_delta(C.byref(ok), None, 4, 4, 3, None, 0, None, None, None) == _lib.INVALID_INPUT
    assert L.redux_decode_blocks_delta(C.byref(ok), None, None, 4, 4, 3, None, None, None, None) == _lib.INVALID_INPUT
