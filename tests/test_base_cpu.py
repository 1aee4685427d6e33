"""XOR-against-base filter for series of snapshots (include/redux_hip.h, "XOR-against-base filter"): the numpy restatement
of the rule, container version 8 and its damaged forms, the base checks of decompress_bytes and the argument checks of the
Python API before the library is touched, the CLI flag, and the host-only ABI helpers.  No GPU call."""
import ctypes as C
import zlib

import numpy as np
import pytest

from test_planes_cpu import planes_ref


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def pad(y, n):
    """y' of the rule: the base cut or zero-padded to n bytes"""
    y = np.frombuffer(bytes(y), dtype=np.uint8) if not isinstance(y, np.ndarray) else np.ascontiguousarray(y, np.uint8)
    out = np.zeros(n, dtype=np.uint8)
    k = min(n, len(y))
    out[:k] = y[:k]
    return out


def base_planes_ref(x, y, E, B, inverse=False):
    """what redux_base_planes_dev computes: planes_ref(x ^ pad(y)); the inverse undoes the layout and XORs again"""
    x = np.ascontiguousarray(x, np.uint8)
    if inverse:
        return planes_ref(x, E, B, inverse=True) ^ pad(y, len(x))
    return planes_ref(x ^ pad(y, len(x)), E, B)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_restatement_of_the_rule(rx, E):
    """base_planes_ref, which the GPU tests hold api.base_planes against, on the rule's own properties"""
    assert callable(rx.base_planes)
    B = 4
    rng = np.random.default_rng(E)
    for L in (0, 1, E * B - 1, E * B, 3 * E * B + 5):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for yl in (0, 1, max(L - 1, 0), L, L + 17):
            y = rng.integers(0, 256, yl, dtype=np.uint8)
            d = base_planes_ref(x, y, E, B)
            assert np.array_equal(base_planes_ref(d, y, E, B, inverse=True), x), (E, L, yl)
            k = min(L, yl)
            assert np.array_equal(planes_ref(d, E, B, inverse=True)[k:], x[k:])    # past the base: x as it is
        assert not base_planes_ref(x, x, E, B).any()                                # x == y: all-zero coder input
        assert np.array_equal(base_planes_ref(x, b"", E, B), planes_ref(x, E, B))   # no base: the layout alone


# ---- container version 8 ------------------------------------------------------------------------------------------------
STREAMS = np.arange(10, dtype=np.uint8)
OFFS = np.array([0, 3, 3, 10], dtype=np.uint64)
TOTAL = 3 * 65536 - 5


def test_container_v8_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    v1 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL)
    assert container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, base=None) == v1   # no base: today's bytes
    assert container.base(v1) is None
    crc = np.array([1, 2, 3], dtype=np.uint32)
    record = (12345, 0xDEADBEEF)
    for E in (1, 2, 4, 8):
        plain = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=E)
        assert container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=E, base=None) == plain
        assert container.base(plain) is None
        assert container.base(container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=E, filter="delta")) is None
        v8 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=E, base=record)
        assert v8[4] == 8 and int.from_bytes(v8[12:16], "little") == 0x80000000 | E
        assert v8[32:44] == (12345).to_bytes(8, "little") + (0xDEADBEEF).to_bytes(4, "little")
        assert v8[:4] + v8[5:12] + v8[16:32] + v8[44:] == v1[:4] + v1[5:12] + v1[16:]  # version 2's sections
        c = container._parse(v8)
        assert c.params.triple() == (8, 30, 32) and c.block_size == 65536 and c.total == TOTAL and c.element_size == E
        assert c.base == record and c.filter is None and c.static is None and c.crcs is None and c.stored is None
        assert c.offsets.tolist() == OFFS.tolist() and c.payload.tobytes() == STREAMS.tobytes()
        assert container.base(v8) == record and container.element_size(v8) == E and container.header_is_wellformed(v8)
        assert container.filter(v8) is None
        v18 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=E, block_crc=crc, base=record)
        assert v18[4] == 0x18 and container.base(v18) == record and container.block_crcs(v18).tolist() == [1, 2, 3]
        assert container._parse(v18).payload.tobytes() == STREAMS.tobytes()
        assert v18[:44] == v8[:4] + b"\x18" + v8[5:44] and v18[44 + 12 + 12:] == v8[44 + 12:]
    assert container.base(container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, base=(0, 0))) == (0, 0)
    assert container.base(container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, base=(TOTAL, 7))) == (TOTAL, 7)


def test_container_v8_truncated_is_eof(rx):
    from redux_amd import container
    crc = np.array([1, 2, 3], dtype=np.uint32)
    v18 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=2, block_crc=crc, base=(9, 9))
    assert len(v18) == 32 + 12 + 12 + 12 + 10
    # inside the header, the record, the size table, the CRC table, the payload; and each section missing whole
    for cut in (31, 32, 33, 43, 44, 45, 55, 56, 57, 67, 68, 69, len(v18) - 1):
        with pytest.raises(rx.Eof):
            container._parse(v18[:cut])
        with pytest.raises(rx.Eof):
            container.base(v18[:cut])
    container._parse(v18)


def test_container_v8_requires_its_marker_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=2, base=(10, 1))
    assert container.header_is_wellformed(good)
    for word in (0, 0x80000000, 0x80000003, 0x80000010, 0x60000002, 0x70000000, 2, 0x80000102, 0x90000002):
        bad = bytearray(good)
        bad[12:16] = word.to_bytes(4, "little")
        assert not container.header_is_wellformed(bytes(bad)), hex(word)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
        with pytest.raises(rx.InvalidInput):
            container.base(bytes(bad))
    for ver in (0x48, 0x58, 0x28, 0x88):
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), hex(ver)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    for ver in (1, 2, 3, 4, 5, 6, 7, 0x11, 0x12, 0x16):  # no other version takes version 8's word
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), ver
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    for word in (0x60000002, 2, 0x00020002, 0x50000012, 0x70000000):  # nor does version 8 take another version's
        bad = bytearray(good)
        bad[12:16] = word.to_bytes(4, "little")
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    over = bytearray(good)
    over[32:40] = (11).to_bytes(8, "little")  # more of the base than there is data
    with pytest.raises(rx.InvalidInput):
        container._parse(bytes(over))
    flags = np.zeros(1, np.uint8)
    for kw in ({"element_size": 3}, {"stored": flags}, {"filter": "delta"}, {"filter": "xor"}, {"base": (11, 1)}, {"base": (1, 1 << 32)},
               {"base": (-1, 1)}, {"base": 5}, {"base": (1, 2, 3)}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, (8, 30, 32), 65536, 10, **{"base": (10, 1), **kw})
    for model in (rx.StaticModel((8, 30, 32), np.arange(258)), rx.PlaneStaticModel((8, 30, 32), np.tile(np.arange(258), (2, 1))),
                  rx.SegmentStaticModel.template((8, 30, 32), 2)):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, model, 65536, 10, base=(10, 1))


def no_library(monkeypatch):
    from redux_amd import _lib

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)


def header_parse_only(monkeypatch):
    """The library behind a guard that lets one symbol through: redux_params_check, the host-only check of a (symbol,
    frequency, code) triple that reading ANY container header makes (api.Parameters).  Every other symbol -- every coder, every
    device call -- raises."""
    from redux_amd import _lib
    real = _lib.lib()

    class Guard:
        def __getattr__(self, name):
            if name == "redux_params_check":
                return real.redux_params_check
            raise AssertionError("the library was loaded before the arguments were checked: " + name)
    monkeypatch.setattr(_lib, "lib", lambda: Guard())


def test_decompress_bytes_checks_the_base_before_any_library_call(rx, monkeypatch):
    """(Before any call but the header's parameter check, which _parse makes for every version: header_parse_only.)"""
    from redux_amd import container
    y = bytes(range(200)) * 3
    v8 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=2, base=(500, zlib.crc32(y[:500])))
    v2 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=2)
    v1 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL)
    v6 = container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, filter="delta")
    wrong = bytearray(y)
    wrong[499] ^= 1
    header_parse_only(monkeypatch)
    for bad in (None, y[:499], b"", bytes(wrong), np.frombuffer(bytes(wrong), np.uint8)):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(v8, base=bad)
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(v8, bad)
    for other in (v1, v2, v6):  # a base given for another version
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(other, base=y)
    # the right base, and a longer one whose first 500 bytes are right, pass the check (the decode is then attempted)
    wrong[499] ^= 1
    for ok in (y[:500], y, bytes(wrong) + b"tail"):
        with pytest.raises(AssertionError, match="the library was loaded"):
            container.decompress_bytes(v8, base=ok)


def test_python_api_refuses_the_base_where_it_is_not_available_before_any_library_call(rx, monkeypatch):
    from redux_amd import api, container
    static = rx.StaticModel((8, 30, 32), np.arange(258))
    plane = rx.PlaneStaticModel((8, 30, 32), np.tile(np.arange(258), (2, 1)))
    segment = rx.SegmentStaticModel.template((8, 30, 32), 2)
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    no_library(monkeypatch)
    y = b"abcd"
    calls = [lambda m=m: rx.compress_blocks(b"abcd", 4, m, base=y) for m in (static, plane, segment)]
    calls += [lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, base=y) for m in (static, plane, segment)]
    calls += [lambda: rx.compress_blocks(b"abcd", 4, stored=flags, base=y),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, stored=flags, base=y),
              lambda: rx.compress_blocks(b"abcd", 4, filter="delta", base=y),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, filter="delta", base=y),
              lambda: rx.compress_blocks(b"abcd", 4, filter="xor", base=y),
              lambda: rx.decompress_blocks(b"\0", offs, 4, base=y),                          # the base needs the length
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter="delta", base=y),
              lambda: rx.DeviceDecoder((8, 30, 32), 4096, 1, filter="delta", base=y),
              lambda: rx.DeviceEncoder((8, 30, 32), 4096, 4096, filter="xor", base=y),
              lambda: container.compress_bytes(b"abcd" * 4, 16, filter="delta", base=y),
              lambda: container.compress_bytes(b"abcd" * 4, 16, stored=True, base=y),
              lambda: container.compress_bytes(b"abcd" * 4, 16, model="auto", base=y)]
    calls += [lambda kw=kw: container.compress_bytes(b"abcd" * 4, 16, base=y, **kw)
              for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
                         {"model": "context-static"})]
    for i, call in enumerate(calls):
        with pytest.raises(rx.InvalidInput):
            call()
    flags = np.zeros(1, np.uint8)
    assert api._resolve_front(None).front.takes_base is False and api._resolve_front(None, base=b"").front.takes_base is True \
        and api._resolve_front(None, stored=flags).front.takes_base is False
    with pytest.raises(rx.InvalidInput):
        api._resolve_front(None, base=b"", stored=flags)


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_base_flag(rx, tmp_path, capsys):
    from redux_amd import cli
    want = {"compress": True, "input": None, "output": None, "block_size": 65536, "base": "prev.bin"}
    assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin"]) == want
    assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin", "--model", "adaptive"]) == {**want, "model": "adaptive"}
    assert cli.parse(["-c", "--block-size", "65536", "--base", "prev.bin", "--checksum"]) == {**want, "checksum": True}
    for E in ("1", "2", "4", "8"):
        got = cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--base", "b", "--checksum"])
        assert got["element_size"] == int(E) and got["base"] == "b" and got["checksum"]
    assert cli.parse(["-d", "--base", "prev.bin"]) == {"compress": False, "input": None, "output": None, "block_size": 0,
                                                       "base": "prev.bin"}
    assert cli.parse(["-d", "-i", "a", "-o", "b", "--base", "c"])["base"] == "c"
    bads = [["-c", "--base", "b"], ["-c", "--block-size", "0", "--base", "b"],
            ["-c", "--block-size", "65536", "--base", "b", "--stored"],
            ["-c", "--block-size", "65536", "--base", "b", "--filter", "delta"],
            ["-c", "--block-size", "65536", "--base", "b", "--filter", "xor"],
            ["-c", "--block-size", "65536", "--base", "b", "--model", "static"],
            ["-c", "--block-size", "65536", "--element-size", "2", "--base", "b", "--model", "plane-static"],
            ["-c", "--block-size", "65536", "--base", "b", "--model", "segment-static"],
            ["-c", "--block-size", "65536", "--base", "b", "--model", "context-static"],
            ["-c", "--block-size", "65536", "--base", "b", "--model", "auto"],
            ["-c", "--block-size", "65536", "--base"], ["--base", "b"]]
    for bad in bads:
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
    assert "--base" in cli.USAGE and "--base FILE" in cli.__doc__ and "version 8" in cli.__doc__
    # a base file that cannot be opened: exit 2, in the input file's message form, for -c and -d
    src = tmp_path / "in.bin"
    src.write_bytes(b"abcd" * 64)
    missing = str(tmp_path / "no" / "such.bin")
    capsys.readouterr()
    for argv in (["-c", "-i", str(src), "-o", str(tmp_path / "o"), "--block-size", "64", "--base", missing],
                 ["-d", "-i", str(src), "-o", str(tmp_path / "o"), "--base", missing]):
        assert cli.main(argv) == 2
        err = capsys.readouterr().err
        assert err.startswith("Error while opening base file " + missing + ": "), err
    assert not (tmp_path / "o").exists()
    # existing flags are untouched: the xor spelling stays a usage error
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "xor"]) is None


def test_cli_decode_exits_3_on_a_missing_wrong_or_misplaced_base(rx, tmp_path, capsys):
    from redux_amd import cli, container
    y = tmp_path / "y.bin"
    y.write_bytes(bytes(600))
    v2 = tmp_path / "v2.rdxb"
    v2.write_bytes(container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=2))
    v8 = tmp_path / "v8.rdxb"
    v8.write_bytes(container.pack(STREAMS, OFFS, (8, 30, 32), 65536, TOTAL, element_size=2, base=(600, zlib.crc32(bytes(600)) ^ 1)))
    short = tmp_path / "short.bin"
    short.write_bytes(bytes(599))
    capsys.readouterr()
    for argv in (["-d", "-i", str(v2), "-o", str(tmp_path / "o"), "--base", str(y)],        # not version 8
                 ["-d", "-i", str(v8), "-o", str(tmp_path / "o")],                          # no base
                 ["-d", "-i", str(v8), "-o", str(tmp_path / "o"), "--base", str(short)],    # too short
                 ["-d", "-i", str(v8), "-o", str(tmp_path / "o"), "--base", str(y)]):       # another CRC
        assert cli.main(argv) == 3, argv
        assert capsys.readouterr().err.startswith("Decompression error"), argv


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_base_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        assert L.redux_base_check(E) == (_lib.OK if E in (1, 2, 4, 8) else _lib.INVALID_INPUT), E
    assert L.redux_base_check(0xFFFFFFFF) == _lib.INVALID_INPUT
    for params in ((8, 30, 32), (8, 14, 16), (4, 10, 16)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            plain_e = L.redux_encode_workspace_bytes(C.byref(p), n, B)
            plain_d = L.redux_decode_workspace_bytes(C.byref(p), L.redux_block_count(n, B), B)
            for E in (1, 2, 4, 8):  # E = 1 too: the filter changes the bytes, so the coder needs the transformed copy
                we = L.redux_encode_base_workspace_bytes(C.byref(p), n, B, E)
                wd = L.redux_decode_base_workspace_bytes(C.byref(p), n, B, E)
                assert we >= plain_e + n + 16 and wd >= plain_d + n, (params, n, B, E)
                assert we % 256 == plain_e % 256
                assert we == L.redux_encode_delta_workspace_bytes(C.byref(p), n, B, E)
                assert wd == L.redux_decode_planes_workspace_bytes(C.byref(p), n, B, E)
            assert L.redux_encode_base_workspace_bytes(C.byref(p), n, B, 1) > L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, 1)
            for bad in (0, 3, 16):
                assert L.redux_encode_base_workspace_bytes(C.byref(p), n, B, bad) == 0
                assert L.redux_decode_base_workspace_bytes(C.byref(p), n, B, bad) == 0
    p = _lib.Params(8, 9, 16)  # invalid triple
    assert L.redux_encode_base_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    assert L.redux_decode_base_workspace_bytes(C.byref(p), 100, 64, 2) == 0


def test_argument_checks_come_before_any_device_work(rx):
    from redux_amd import _lib
    L = _lib.lib()
    ok = _lib.Params(8, 30, 32)
    V = C.c_void_p
    src, base, dst = V(1 << 20), V(2 << 20), V(3 << 20)
    dev = L.redux_base_planes_dev
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
    enc, dec = L.redux_encode_blocks_base, L.redux_decode_blocks_base
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


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_base_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "base_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "base_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_base_mirror_compiles_and_refuses(rx, tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_base_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "base mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
