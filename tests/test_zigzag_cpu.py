"""Zigzag-folded delta filter for signed series (include/redux_hip.h, "zigzag-folded delta filter"): the numpy restatement
of the rule against hand-written expectations, the value claim on the CPU oracle, container version 11, the CLI flag, the
Python argument checks, the host-only ABI helpers and the range reader.  No GPU call.

The value claim rests on GENERATED series, a random walk and timestamps: nothing in the corpus fixtures is a signed series."""
import ctypes as C
import io

import numpy as np
import pytest

from test_delta_cpu import delta_ref
from test_planes_cpu import lengths, oracle_bytes, planes_ref


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def zigzag_ref(x, E, B, inverse=False):
    """The rule: the delta filter's frames and differences d, then z = (d << 1) ^ (0 - (d >> (8E-1))) mod 2^(8E) for every
    element of a frame, the first included; the trailing bytes of a frame unchanged.  inverse=True unfolds with
    d = (z >> 1) ^ (0 - (z & 1)) and takes delta_ref's running sum.  (The byte-plane layout is planes_ref's, behind this.)"""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    dt = np.dtype("<u%d" % E)
    one = dt.type(1)

    def elementwise(y, f):
        out = y.copy()
        for f0 in range(0, len(y), E * B):
            N = len(y[f0: f0 + E * B]) // E
            if N:
                out[f0: f0 + N * E] = f(y[f0: f0 + N * E].copy().view(dt)).view(np.uint8)
        return out
    if inverse:
        return delta_ref(elementwise(x, lambda z: (z >> one) ^ (dt.type(0) - (z & one))), E, B, inverse=True)
    return elementwise(delta_ref(x, E, B), lambda d: (d << one) ^ (dt.type(0) - (d >> dt.type(8 * E - 1))))


def zigzag_planes_ref(x, E, B, inverse=False):
    """what redux_zigzag_planes_dev computes: the filter, then the layout; the inverse the other way round"""
    if inverse:
        return zigzag_ref(planes_ref(x, E, B, inverse=True), E, B, inverse=True)
    return planes_ref(zigzag_ref(x, E, B), E, B)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_fold_matches_hand_written_expectations(E):
    dt = np.dtype("<u%d" % E)
    top, half = (1 << 8 * E) - 1, 1 << (8 * E - 1)
    v = np.array([0, 1, 0, top, half, 0], dtype=dt)
    x = np.concatenate([v.view(np.uint8), np.array([0xEE] * (E > 1), dtype=np.uint8)])  # + a trailing odd byte
    # d = 0, +1, -1, -1, half + 1 (= -(half - 1)), half (= -half, the most negative);  d >= 0 -> 2 d, d < 0 -> -2 d - 1
    want = [0, 2, 1, 1, 2 * (half - 1) - 1, top]
    z = zigzag_ref(x, E, 16)
    assert z[: 6 * E].view(dt).tolist() == want and z[6 * E:].tolist() == x[6 * E:].tolist()
    assert zigzag_ref(z, E, 16, inverse=True).tolist() == x.tolist()
    # a frame start: with B = 4 element 4 begins the second frame and is folded as it stands (half -> top, 0 - half -> top)
    z4 = zigzag_ref(x, E, 4)
    assert z4[: 6 * E].view(dt).tolist() == [0, 2, 1, 1, top, top] and z4[6 * E:].tolist() == x[6 * E:].tolist()
    assert zigzag_ref(z4, E, 4, inverse=True).tolist() == x.tolist()
    # the first element of a frame is folded too: top = -1 -> 1
    assert zigzag_ref(np.array([top], dtype=dt).view(np.uint8), E, 16).view(dt).tolist() == [1]
    if E > 1:  # the upper bytes of small differences of either sign are zero: what the fold is for
        walk = np.array([1000, 997, 1001, 990, 1003], dtype=dt).view(np.uint8)
        assert zigzag_ref(walk, E, 16).view(dt).tolist() == [2000, 5, 8, 21, 26]


@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("B", [4, 100, 4096])
def test_inverse_of_forward_is_identity(E, B):
    rng = np.random.default_rng(E * 10000 + B)
    for L in lengths(E, B):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        y = zigzag_planes_ref(x, E, B)
        assert len(y) == L
        assert np.array_equal(zigzag_planes_ref(y, E, B, inverse=True), x), (E, B, L)
        assert np.array_equal(zigzag_ref(zigzag_ref(x, E, B), E, B, inverse=True), x), (E, B, L)
        # the fold is a bijection on the elements, so the bytes taken as FOLDED values round-trip as well
        assert np.array_equal(zigzag_ref(zigzag_ref(x, E, B, inverse=True), E, B), x), (E, B, L)


# ---- the value claim, on the CPU oracle --------------------------------------------------------------------------------
# B = 4096, three frames + 100 elements, params (8, 30, 32).  The bounds are the issue's, from its measurements 0.896 / 0.752 /
# 0.599 with room for another generator; measured with this one: 0.897 / 0.752 / 0.598, and the timestamps within 1 byte.
def walk_and_stamps(E, B=4096):
    rng = np.random.default_rng(1)
    n = 3 * B + 100
    walk = np.cumsum(np.round(rng.normal(0, 50, n))).astype(np.int64).astype("<i%d" % E).view(np.uint8)
    stamps = np.cumsum(rng.integers(990, 1010, n)).astype(np.int64).astype("<u%d" % E).view(np.uint8)
    return walk, stamps


@pytest.mark.parametrize("E,bound", [(2, 0.92), (4, 0.80), (8, 0.65)])
def test_fold_pays_on_a_random_walk_and_costs_nothing_on_timestamps(E, bound):
    B = 4096
    walk, stamps = walk_and_stamps(E)
    delta = oracle_bytes(planes_ref(delta_ref(walk, E, B), E, B), B)
    zigzag = oracle_bytes(zigzag_planes_ref(walk, E, B), B)
    print("random walk, E = %d: delta %d, zigzag %d, %.3f x" % (E, delta, zigzag, zigzag / delta))
    assert zigzag <= bound * delta, (E, delta, zigzag)
    delta = oracle_bytes(planes_ref(delta_ref(stamps, E, B), E, B), B)
    zigzag = oracle_bytes(zigzag_planes_ref(stamps, E, B), B)
    print("timestamps, E = %d: delta %d, zigzag %d" % (E, delta, zigzag))
    assert abs(zigzag - delta) <= 8, (E, delta, zigzag)


# ---- container version 11 -----------------------------------------------------------------------------------------------
def test_container_v11_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    crc = np.array([1, 2, 3], dtype=np.uint32)
    v1 = container.pack(streams, offs, (8, 30, 32), 65536, total)
    assert container.pack(streams, offs, (8, 30, 32), 65536, total, filter=None) == v1 and v1[4] == 1
    for E in (1, 2, 4, 8):
        v6 = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, filter="delta")
        assert v6[4] == 6 and int.from_bytes(v6[12:16], "little") == 0x60000000 | E   # today's bytes
        v11 = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, filter="zigzag")
        assert v11[4] == 11 and int.from_bytes(v11[12:16], "little") == 0xB0000000 | E
        assert v11[:4] + v11[5:12] + v11[16:] == v6[:4] + v6[5:12] + v6[16:]  # version 6's bytes but the version and the word
        c = container._parse(v11)
        assert c.params.triple() == (8, 30, 32) and c.block_size == 65536 and c.total == total and c.element_size == E
        assert c.filter == "zigzag" and c.static is None and c.crcs is None and c.stored is None and c.base is None
        assert c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == streams.tobytes()
        assert container.filter(v11) == "zigzag" and container.element_size(v11) == E and container.header_is_wellformed(v11)
        v16 = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, block_crc=crc, filter="delta")
        v1b = container.pack(streams, offs, (8, 30, 32), 65536, total, element_size=E, block_crc=crc, filter="zigzag")
        assert v16[4] == 0x16 and v1b[4] == 0x1B and v1b[:4] + v1b[5:12] + v1b[16:] == v16[:4] + v16[5:12] + v16[16:]
        assert container.filter(v1b) == "zigzag" and container.block_crcs(v1b).tolist() == [1, 2, 3]
        assert container._parse(v1b).payload.tobytes() == streams.tobytes()
        for cut in (len(v1b) - 1, len(v1b) - 11, 32 + 12 + 11, 32 + 11, 33):  # payload, CRC table, size table
            with pytest.raises(rx.Eof):
                container._parse(v1b[:cut])
        for nb in (1, 3, 1000):
            for checksum in (False, True):
                assert container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="zigzag") == \
                    container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="delta")
        assert len(v11) - len(streams) == container.overhead_bytes("adaptive", 3, E, filter="zigzag")


def test_container_v11_takes_its_word_alone_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=2, filter="zigzag")
    for word in (0, 2, 0x60000002, 0xA0000000, 0xB0000000, 0xB0000003, 0xB0000010, 0xB0000102, 0xC0000002):
        bad = bytearray(good)
        bad[12:16] = word.to_bytes(4, "little")
        assert not container.header_is_wellformed(bytes(bad)), hex(word)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
        with pytest.raises(rx.InvalidInput):
            container.filter(bytes(bad))
    for E in (1, 2, 4, 8):
        for ver in range(256):  # no other version byte takes version 11's word
            if ver in (11, 0x1B):
                continue
            bad = bytearray(container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=E, filter="zigzag"))
            bad[4] = ver
            assert not container.header_is_wellformed(bytes(bad)), (E, hex(ver))
            with pytest.raises(rx.InvalidInput):
                container._parse(bytes(bad))
    flags = np.zeros(1, np.uint8)
    static = rx.StaticModel((8, 30, 32), np.arange(258))
    for kw in ({"element_size": 3}, {"stored": flags}, {"base": (0, 0)}, {"constant": flags},
               {"unit_layouts": np.zeros(1, np.uint8)}, {"params": static}):
        kw = dict(kw)
        params = kw.pop("params", (8, 30, 32))
        for f in ("delta", "zigzag"):  # whatever is refused for delta is refused for zigzag
            with pytest.raises(rx.InvalidInput):
                container.pack(streams, offs, params, 65536, 10, filter=f, **kw)
    for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
               {"model": "context-static"}, {"model": "auto"}, {"stored": True}, {"base": b"abcd"}, {"skip_constant": True},
               {"layout": "auto"}, {"layout": "mixed"}):
        for f in ("delta", "zigzag"):
            with pytest.raises(rx.InvalidInput):
                container.compress_bytes(b"abcd" * 4, 16, filter=f, **kw)
    for f in ("xor", "Zigzag", True):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(b"abcd" * 4, 16, filter=f)


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_filter_flag(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "zigzag"]) == {**base, "filter": "zigzag"}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "delta"]) == {**base, "filter": "delta"}
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "zigzag"]) == \
            {**base, "block_size": 4096, "element_size": int(E), "filter": "zigzag"}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "zigzag", "--model", "adaptive", "--checksum"]) == \
        {**base, "filter": "zigzag", "model": "adaptive", "checksum": True}
    some = ["-c", "--block-size", "65536", "--filter", "zigzag"]
    for bad in (["-c", "--filter", "zigzag"], ["-c", "--block-size", "0", "--filter", "zigzag"], some + ["--stored"],
                some + ["--base", "f"], some + ["--skip-constant"], some + ["--layout", "auto"], some + ["--layout", "mixed"],
                some + ["--model", "static"], some + ["--element-size", "2", "--model", "plane-static"],
                some + ["--model", "segment-static"], some + ["--model", "context-static"], some + ["--model", "auto"],
                ["-c", "--block-size", "65536", "--filter", "Zigzag"], ["-c", "--block-size", "65536", "--filter"]):
        assert cli.parse(bad) is None, bad
        assert cli.parse([a if a != "zigzag" else "delta" for a in bad]) is None, bad   # delta's rules
    assert cli.main(["-c", "--filter", "zigzag"]) == 1
    assert cli.main(some + ["--stored"]) == 1
    assert "delta|zigzag" in cli.USAGE and "--filter zigzag" in cli.__doc__ and "version 11" in cli.__doc__


# ---- Python argument checks ----------------------------------------------------------------------------------------------
def test_python_api_refuses_the_filter_wherever_it_refuses_delta_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api
    static = rx.StaticModel((8, 30, 32), np.arange(258))
    context = rx.ContextStaticModel((8, 30, 32), np.tile(np.arange(258), (256, 1)))
    plane = rx.PlaneStaticModel((8, 30, 32), np.tile(np.arange(258), (2, 1)))
    segment = rx.SegmentStaticModel.template((8, 30, 32), 2)
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    adaptive = rx.AdaptiveTreeModel.new(rx.Parameters(8, 30, 32))

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)

    def calls(f):
        c = [lambda m=m: rx.compress_blocks(b"abcd", 4, m, filter=f) for m in (static, context, plane, segment)]
        c += [lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, filter=f) for m in (static, context, plane, segment)]
        c += [lambda: rx.compress_blocks(b"abcd", 4, stored=flags, filter=f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, stored=flags, filter=f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, filter=f),                     # the filter needs the length
              lambda: rx.compress_blocks(b"abcd", 4, base=b"abcd", filter=f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, base=b"abcd", filter=f),
              lambda: rx.compress_blocks(b"abcd", 4, constant=True, filter=f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, constant=flags, filter=f),
              lambda: rx.compress_blocks(b"abcd", 4, unit_layouts=True, filter=f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, unit_layouts=flags, filter=f),
              lambda: rx.compress_blocks_v([b"abcd"], 4, filter=f),
              lambda: rx.decompress_blocks_v(b"\0", offs, [4], 4, filter=f),
              lambda: rx.compress(io.BytesIO(b"abcd"), io.BytesIO(), adaptive, filter=f),
              lambda: rx.decompress(io.BytesIO(b"\0"), io.BytesIO(), adaptive, filter=f),
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter=f, base=flags),
              lambda: rx.DeviceDecoder((8, 30, 32), 4096, 1, filter=f, base=flags),
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter=f, constant=True),
              lambda: rx.DeviceDecoder((8, 30, 32), 4096, 1, filter=f, constant=True),
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter=f, mixed=True),
              lambda: rx.DeviceDecoder((8, 30, 32), 4096, 1, filter=f, mixed=True)]
        return c
    for f in ("delta", "zigzag"):
        for i, call in enumerate(calls(f)):
            with pytest.raises(rx.InvalidInput):
                call()
    for f in ("xor", "Zigzag", "zigzag ", 2, True):
        with pytest.raises(rx.InvalidInput):
            rx.compress_blocks(b"abcd", 4, filter=f)
        with pytest.raises(rx.InvalidInput):
            rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter=f)
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(None, filter=f)
    front = lambda f: api._resolve_front(None, filter=f).front.infix
    assert front(None) == "planes" and front("delta") == "delta"
    assert front("zigzag") == "zigzag" and front("zigzag") != front("delta")
    with pytest.raises(rx.InvalidInput):
        api._resolve_front(None, filter="zigzag", stored=flags)


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_zigzag_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        assert L.redux_zigzag_check(E) == (_lib.OK if E in (1, 2, 4, 8) else _lib.INVALID_INPUT), E
    assert L.redux_zigzag_check(0xFFFFFFFF) == _lib.INVALID_INPUT
    for params in ((8, 30, 32), (8, 14, 16), (4, 10, 16)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            for E in (1, 2, 4, 8):
                we = L.redux_encode_zigzag_workspace_bytes(C.byref(p), n, B, E)
                wd = L.redux_decode_zigzag_workspace_bytes(C.byref(p), n, B, E)
                assert we > 0 and wd > 0
                assert we >= L.redux_encode_delta_workspace_bytes(C.byref(p), n, B, E), (params, n, B, E)
                assert wd >= L.redux_decode_delta_workspace_bytes(C.byref(p), n, B, E), (params, n, B, E)
            for bad in (0, 3, 16):
                assert L.redux_encode_zigzag_workspace_bytes(C.byref(p), n, B, bad) == 0
                assert L.redux_decode_zigzag_workspace_bytes(C.byref(p), n, B, bad) == 0
    p = _lib.Params(8, 9, 16)  # invalid triple
    assert L.redux_encode_zigzag_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    assert L.redux_decode_zigzag_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    # argument checks of the device calls come before any device work
    ok = _lib.Params(8, 30, 32)
    assert L.redux_zigzag_planes_dev(None, None, 16, 4, 3, 0, None) == _lib.INVALID_INPUT
    assert L.redux_zigzag_planes_dev(None, None, 16, 0, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_zigzag_planes_dev(None, None, 16, 4, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_zigzag_planes_dev(None, None, 0, 4, 2, 0, None) == _lib.OK
    assert L.redux_zigzag_planes_dev(C.c_void_p(4096), C.c_void_p(4096 + 8), 16, 4, 2, 0, None) == _lib.INVALID_INPUT  # overlap
    assert L.redux_encode_blocks_zigzag(C.byref(ok), None, 4, 4, 3, None, 0, None, None, None) == _lib.INVALID_INPUT
    assert L.redux_decode_blocks_zigzag(C.byref(ok), None, None, 4, 4, 3, None, None, None, None) == _lib.INVALID_INPUT


# ---- range reads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_reader_reports_the_filter_and_a_granule_of_a_frame(rx, E):
    from redux_amd import container
    nb, B = 19, 4096
    streams = np.arange(3 * nb, dtype=np.uint8)
    offs = np.arange(0, 3 * nb + 1, 3).astype(np.uint64)
    total = nb * B - 7
    for crc in (None, np.arange(nb, dtype=np.uint32)):
        buf = container.pack(streams, offs, (8, 30, 32), B, total, element_size=E, block_crc=crc, filter="zigzag")
        r = container.Reader(buf)
        assert r.filter == "zigzag" and r.granule_blocks == E and r.version == (11 if crc is None else 0x1B)
        assert r.total == total and r.block_size == B and r.nblocks == nb
        assert r.payload_offset == len(buf) - len(streams) and r.bytes_read == r.payload_offset
        assert r.read(5, 0) == b"" and r.bytes_read == r.payload_offset      # no bytes asked for: no coder call
        d = container.Reader(container.pack(streams, offs, (8, 30, 32), B, total, element_size=E, block_crc=crc, filter="delta"))
        assert d.filter == "delta" and d.granule_blocks == E and d.payload_offset == r.payload_offset
    assert container.Reader(container.pack(streams, offs, (8, 30, 32), B, total, element_size=E)).filter is None


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_zigzag_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "zigzag_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "zigzag_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_mirror_refuses_bad_arguments_before_any_device_call(tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_zigzag_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "zigzag mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
