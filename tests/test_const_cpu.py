"""Constant blocks (include/redux_hip.h, "constant blocks"): the numpy restatement of the rule, container version 9 and its
damaged forms, the argument checks of the Python API before the library is touched, the CLI flag, and the argument checks of
the C ABI that are decided before any device work.  No GPU call."""
import ctypes as C
import zlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def const_ref(xp, B):
    """the rule: flags uint8[nblocks] of the coder input xp cut into blocks of B bytes: 1 where the block has at least one
    byte and all its bytes are equal.  nblocks = max(1, ceil(len / B)): the empty input's one empty block is not constant."""
    xp = np.frombuffer(bytes(xp), np.uint8) if not isinstance(xp, np.ndarray) else np.ascontiguousarray(xp, np.uint8)
    nb = max(1, -(-len(xp) // B))
    flags = np.zeros(nb, dtype=np.uint8)
    for b in range(nb):
        blk = xp[b * B: (b + 1) * B]
        flags[b] = 1 if len(blk) >= 1 and bool((blk == blk[0]).all()) else 0
    return flags


def test_restatement_of_the_rule(rx):
    assert callable(rx.api.constant_blocks)
    assert const_ref(b"", 4).tolist() == [0]                       # the empty input's one empty block is not constant
    assert const_ref(b"a", 4).tolist() == [1]                      # a 1-byte block is
    assert const_ref(b"aaaab", 4).tolist() == [1, 1]
    assert const_ref(b"aaaabbbbabbb", 4).tolist() == [1, 1, 0]     # neighbours with different values; one byte off
    assert const_ref(b"aaabaaaa", 4).tolist() == [0, 1]
    assert const_ref(bytes(7), 1).tolist() == [1] * 7
    x = np.zeros(100, np.uint8)
    x[15] = 1
    assert const_ref(x, 16).tolist() == [0, 1, 1, 1, 1, 1, 1] and const_ref(x, 100).tolist() == [0]


# ---- container version 9 ------------------------------------------------------------------------------------------------
STREAMS = np.arange(10, dtype=np.uint8)
OFFS = np.array([0, 3, 4, 10], dtype=np.uint64)  # block 1: one byte
FLAGS = np.array([0, 1, 0], dtype=np.uint8)
TOTAL = 3 * 65536 - 5
P = (8, 30, 32)


def test_container_v9_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    crc = np.array([1, 2, 3], dtype=np.uint32)
    record = (12345, 0xDEADBEEF)
    for E in (1, 2, 4, 8):
        plain = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E)
        assert container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, constant=None) == plain  # without: today's bytes
        assert container.constant(plain) is None
        v8 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, base=record)
        assert container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, base=record, constant=None) == v8
        assert container.constant(v8) is None
        v18 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, base=record, block_crc=crc)
        for F, rec, ref in ((0, None, plain), (1, record, v8)):
            v9 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, base=rec, constant=FLAGS)
            assert v9[4] == 9 and int.from_bytes(v9[12:16], "little") == 0x90000000 | F << 4 | E
            h = 32 + 12 * F
            assert v9[5:12] == ref[5:12] and v9[16:h + 12] == ref[16:h + 12]   # the same header size, record and size table
            assert v9[h + 12] == 0b010 and v9[h + 13:] == STREAMS.tobytes()    # the bitmap, LSB first, then the payloads
            assert len(v9) == len(ref) + 1
            c = container._parse(v9)
            assert c.params.triple() == P and c.block_size == 65536 and c.total == TOTAL and c.element_size == E
            assert c.base == rec and c.constant.tolist() == [0, 1, 0] and c.constant.dtype == np.uint8
            assert c.filter is None and c.static is None and c.crcs is None and c.stored is None
            assert c.offsets.tolist() == OFFS.tolist() and c.payload.tobytes() == STREAMS.tobytes()
            assert container.constant(v9).tolist() == [0, 1, 0] and container.base(v9) == rec
            assert container.element_size(v9) == E and container.header_is_wellformed(v9)
            v19 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=E, base=rec, constant=FLAGS, block_crc=crc)
            assert v19[4] == 0x19 and container.block_crcs(v19).tolist() == [1, 2, 3] and container.constant(v19).tolist() == [0, 1, 0]
            assert v19[:h + 12] == v9[:4] + b"\x19" + v9[5:h + 12] and v19[h + 24:] == v9[h + 12:]   # CRCs, then the bitmap
            assert container._parse(v19).payload.tobytes() == STREAMS.tobytes() and container.base(v19) == rec
        assert v18[4] == 0x18
    # nine blocks: two bitmap bytes, padding bits zero
    offs9 = np.arange(10, dtype=np.uint64)
    f9 = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8)
    offs9 = np.concatenate([[0], np.cumsum(np.where(f9 == 1, 1, 2))]).astype(np.uint64)
    v9 = container.pack(np.zeros(int(offs9[-1]), np.uint8), offs9, P, 16, 9 * 16, constant=f9)
    assert v9[32 + 36: 32 + 38] == bytes([0x01, 0x01]) and container.constant(v9).tolist() == f9.tolist()


def test_container_v9_failures(rx):
    from redux_amd import container
    crc = np.array([1, 2, 3], dtype=np.uint32)
    good = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=2, constant=FLAGS)
    with_base = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=2, constant=FLAGS, base=(9, 9), block_crc=crc)
    assert len(with_base) == 32 + 12 + 12 + 12 + 1 + 10
    # truncated: inside and at the end of the header, the record, the size table, the CRC table, the bitmap, the payload
    for cut in (31, 32, 43, 44, 45, 55, 56, 57, 67, 68, 69, len(with_base) - 1):
        with pytest.raises(rx.Eof):
            container._parse(with_base[:cut])
        with pytest.raises(rx.Eof):
            container.constant(with_base[:cut])
    container._parse(with_base)
    with pytest.raises(rx.Eof):
        container._parse(good[:32 + 12])   # the bitmap missing whole
    # a constant block's size entry other than 1
    for size in (0, 2, 65536):
        bad = bytearray(good)
        bad[32 + 4: 32 + 8] = size.to_bytes(4, "little")
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad) + bytes(70000))
    # set padding bits
    for bit in range(3, 8):
        bad = bytearray(good)
        bad[32 + 12] |= 1 << bit
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    # no stored blocks, no other high bits
    for ver in (0x49, 0x59, 0x29, 0x89, 0x39, 0xC9):
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), hex(ver)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    # the marker nibble 9 is required, F is one bit, E one of 1, 2, 4, 8
    for word in (0, 2, 0x90000000, 0x90000003, 0x90000022, 0x90000102, 0x80000002, 0x60000002, 0x70000000, 0x00020002, 0x50000012):
        bad = bytearray(good)
        bad[12:16] = word.to_bytes(4, "little")
        assert not container.header_is_wellformed(bytes(bad)), hex(word)
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    for ver in (1, 2, 3, 4, 5, 6, 7, 8, 0x11, 0x12, 0x16, 0x18):  # no other version takes version 9's word
        bad = bytearray(good)
        bad[4] = ver
        assert not container.header_is_wellformed(bytes(bad)), ver
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    over = bytearray(with_base)
    over[32:40] = (TOTAL + 1).to_bytes(8, "little")   # version 8's record check applies when F = 1
    with pytest.raises(rx.InvalidInput):
        container._parse(bytes(over))
    # pack refuses what parse would
    for kw in ({"constant": np.array([0, 2, 0], np.uint8)}, {"constant": np.array([1, 1, 0], np.uint8)}, {"constant": FLAGS[:2]},
               {"stored": np.zeros(3, np.uint8)}, {"filter": "delta"}, {"element_size": 3}):
        with pytest.raises(rx.InvalidInput):
            container.pack(STREAMS, OFFS, P, 65536, TOTAL, **{"constant": FLAGS, **kw})
    with pytest.raises(rx.InvalidInput):   # a constant flag on the empty input's block
        container.pack(np.zeros(1, np.uint8), np.array([0, 1], np.uint64), P, 65536, 0, constant=np.ones(1, np.uint8))
    for model in (rx.StaticModel(P, np.arange(258)), rx.PlaneStaticModel(P, np.tile(np.arange(258), (2, 1))),
                  rx.SegmentStaticModel.template(P, 2)):
        with pytest.raises(rx.InvalidInput):
            container.pack(STREAMS, OFFS, model, 65536, TOTAL, constant=FLAGS)


def no_library(monkeypatch):
    from redux_amd import _lib

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)


def test_decompress_bytes_applies_version_8s_base_checks(rx, monkeypatch):
    from redux_amd import _lib, container
    y = bytes(range(200)) * 3
    f1 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=2, constant=FLAGS, base=(500, zlib.crc32(y[:500])))
    f0 = container.pack(STREAMS, OFFS, P, 65536, TOTAL, element_size=2, constant=FLAGS)
    real = _lib.lib()

    class Guard:  # (reading any header checks its parameter triple on the host: every other symbol raises)
        def __getattr__(self, name):
            if name == "redux_params_check":
                return real.redux_params_check
            raise AssertionError("the library was loaded before the arguments were checked: " + name)
    monkeypatch.setattr(_lib, "lib", lambda: Guard())
    wrong = bytearray(y)
    wrong[499] ^= 1
    for bad in (None, y[:499], b"", bytes(wrong)):
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(f1, base=bad)
    with pytest.raises(rx.InvalidInput):
        container.decompress_bytes(f0, base=y)   # a base given for F = 0
    for buf, base in ((f1, y), (f1, y[:500]), (f0, None)):   # these pass the checks: the decode is then attempted
        with pytest.raises(AssertionError, match="the library was loaded"):
            container.decompress_bytes(buf, base=base)


def test_python_api_refuses_the_option_where_it_is_not_available_before_any_library_call(rx, monkeypatch):
    from redux_amd import api, container
    static = rx.StaticModel(P, np.arange(258))
    plane = rx.PlaneStaticModel(P, np.tile(np.arange(258), (2, 1)))
    segment = rx.SegmentStaticModel.template(P, 2)
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    no_library(monkeypatch)
    calls = []
    for c in (True, flags):
        calls += [lambda m=m, c=c: rx.compress_blocks(b"abcd", 4, m, constant=c) for m in (static, plane, segment)]
        calls += [lambda c=c: rx.compress_blocks(b"abcd", 4, stored=flags, constant=c),
                  lambda c=c: rx.compress_blocks(b"abcd", 4, filter="delta", constant=c),
                  lambda c=c: rx.compress_blocks(b"abcd", 4, filter="delta", base=b"ab", constant=c),
                  lambda c=c: rx.compress_blocks_v([b"abcd"], 4, constant=c),
                  lambda c=c: rx.decompress_blocks_v(b"\0", offs, [4], 4, constant=c)]
    calls += [lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, constant=flags) for m in (static, plane, segment)]
    calls += [lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, stored=flags, constant=flags),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, filter="delta", constant=flags),
              lambda: rx.decompress_blocks(b"\0", offs, 4, constant=flags),                     # the option needs the length
              lambda: rx.DeviceEncoder(P, 4096, 4096, filter="delta", constant=True),
              lambda: rx.DeviceDecoder(P, 4096, 1, filter="delta", constant=True),
              lambda: rx.DeviceEncoder(static, 4096, 4096, constant=True),
              lambda: rx.DeviceDecoder(static, 4096, 1, constant=True),
              lambda: container.compress_bytes(b"abcd" * 4, 16, filter="delta", skip_constant=True),
              lambda: container.compress_bytes(b"abcd" * 4, 16, stored=True, skip_constant=True),
              lambda: container.compress_bytes(b"abcd" * 4, 16, model="auto", skip_constant=True)]
    calls += [lambda kw=kw: container.compress_bytes(b"abcd" * 4, 16, skip_constant=True, **kw)
              for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
                         {"model": "context-static"})]
    for i, call in enumerate(calls):
        with pytest.raises(rx.InvalidInput):
            call()
    const = lambda constant, **kw: api._resolve_front(None, constant=constant, **kw).constant
    assert const(None) is False and const(False) is False and const(None, stored=flags) is False
    assert const(True) is True and const(flags) is True
    with pytest.raises(rx.InvalidInput):
        const(True, stored=flags)


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_skip_constant_flag(rx):
    from redux_amd import cli
    want = {"compress": True, "input": None, "output": None, "block_size": 65536, "skip_constant": True}
    assert cli.parse(["-c", "--block-size", "65536", "--skip-constant"]) == want
    assert cli.parse(["-c", "--skip-constant", "--block-size", "65536", "--model", "adaptive"]) == {**want, "model": "adaptive"}
    assert cli.parse(["-c", "--block-size", "65536", "--skip-constant", "--checksum"]) == {**want, "checksum": True}
    assert cli.parse(["-c", "--block-size", "65536", "--skip-constant", "--base", "b"]) == {**want, "base": "b"}
    for E in ("1", "2", "4", "8"):
        got = cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--base", "b", "--checksum", "--skip-constant"])
        assert got["element_size"] == int(E) and got["base"] == "b" and got["checksum"] and got["skip_constant"]
    bads = [["-c", "--skip-constant"], ["-c", "--block-size", "0", "--skip-constant"],
            ["-c", "--block-size", "65536", "--skip-constant", "--stored"],
            ["-c", "--block-size", "65536", "--skip-constant", "--filter", "delta"],
            ["-c", "--block-size", "65536", "--skip-constant", "--model", "static"],
            ["-c", "--block-size", "65536", "--element-size", "2", "--skip-constant", "--model", "plane-static"],
            ["-c", "--block-size", "65536", "--skip-constant", "--model", "segment-static"],
            ["-c", "--block-size", "65536", "--skip-constant", "--model", "context-static"],
            ["-c", "--block-size", "65536", "--skip-constant", "--model", "auto"],
            ["-d", "--skip-constant"], ["--skip-constant"]]
    for bad in bads:
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
    assert "--skip-constant" in cli.USAGE and "--skip-constant" in cli.__doc__ and "version 9" in cli.__doc__
    # existing flags are untouched
    assert cli.parse(["-c", "--block-size", "65536"]) == {"compress": True, "input": None, "output": None, "block_size": 65536}


# ---- C ABI: what is decided before any device work ------------------------------------------------------------------------
def test_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for params in ((8, 30, 32), (8, 14, 16), (8, 22, 24)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 48)):
            nb = L.redux_block_count(n, B)
            for E in (1, 2, 4, 8):  # E = 1 too: room for the XOR against a base
                we = L.redux_encode_const_workspace_bytes(C.byref(p), n, B, E)
                wd = L.redux_decode_const_workspace_bytes(C.byref(p), n, B, E)
                assert we >= L.redux_encode_workspace_bytes(C.byref(p), n, B) + n + 16 * nb, (params, n, B, E)
                assert wd >= L.redux_decode_workspace_bytes(C.byref(p), nb, B) + n + 16 * nb, (params, n, B, E)
            for bad in (0, 3, 16):
                assert L.redux_encode_const_workspace_bytes(C.byref(p), n, B, bad) == 0
                assert L.redux_decode_const_workspace_bytes(C.byref(p), n, B, bad) == 0
            assert L.redux_encode_const_workspace_bytes(C.byref(p), n, 0, 1) == 0
    for params in ((4, 10, 16), (12, 20, 32), (8, 30, 48), (8, 9, 16)):   # coders without the table form; an invalid triple
        p = _lib.Params(*params)
        assert L.redux_encode_const_workspace_bytes(C.byref(p), 100, 64, 2) == 0
        assert L.redux_decode_const_workspace_bytes(C.byref(p), 100, 64, 2) == 0


def test_argument_checks_come_before_any_device_work(rx):
    from redux_amd import _lib
    L = _lib.lib()
    ok = _lib.Params(8, 30, 32)
    V = C.c_void_p
    a, b, c, d = V(1 << 20), V(2 << 20), V(3 << 20), V(4 << 20)
    det = L.redux_const_blocks_dev
    assert det(a, 16, 0, b, None) == _lib.INVALID_INPUT          # block size 0
    assert det(None, 16, 4, b, None) == _lib.INVALID_INPUT       # null input with a length
    assert det(a, 16, 4, None, None) == _lib.INVALID_INPUT       # null flags
    enc, dec = L.redux_encode_const_dev, L.redux_decode_const_dev
    ws = 1 << 30

    def e(p=ok, d_in=a, n=16, base=None, bl=0, B=4, E=2, out=b, offs=c, fl=d, st=d, w=V(8 << 20), wb=ws):
        return enc(C.byref(p), d_in, n, base, bl, B, E, out, 1 << 20, offs, fl, st, None, w, wb, None)
    assert e(E=3) == _lib.INVALID_INPUT and e(B=0) == _lib.INVALID_INPUT
    assert e(d_in=None) == _lib.INVALID_INPUT and e(bl=4) == _lib.INVALID_INPUT      # null base with a length
    assert e(out=None) == _lib.INVALID_INPUT and e(offs=None) == _lib.INVALID_INPUT
    assert e(fl=None) == _lib.INVALID_INPUT and e(st=None) == _lib.INVALID_INPUT and e(w=None) == _lib.INVALID_INPUT
    assert e(w=V((8 << 20) + 8)) == _lib.INVALID_INPUT                                # workspace off a 256-byte boundary
    assert e(wb=16) == _lib.OUTPUT_TOO_SMALL
    assert e(n=1 << 32, wb=1 << 40) == _lib.UNSUPPORTED                               # the table encoder's limit
    assert e(p=_lib.Params(4, 10, 16)) == _lib.UNSUPPORTED and e(p=_lib.Params(12, 20, 32)) == _lib.UNSUPPORTED
    assert e(p=_lib.Params(8, 9, 16)) == _lib.INVALID_INPUT

    def dd(p=ok, d_in=a, offs=c, fl=d, base=None, bl=0, n=16, B=4, E=2, out=b, sz=d, st=d, w=V(8 << 20), wb=ws):
        return dec(C.byref(p), d_in, offs, fl, base, bl, n, B, E, out, sz, st, None, w, wb, None)
    assert dd(E=3) == _lib.INVALID_INPUT and dd(B=0) == _lib.INVALID_INPUT
    assert dd(offs=None) == _lib.INVALID_INPUT and dd(fl=None) == _lib.INVALID_INPUT and dd(bl=4) == _lib.INVALID_INPUT
    assert dd(out=None) == _lib.INVALID_INPUT and dd(sz=None) == _lib.INVALID_INPUT and dd(st=None) == _lib.INVALID_INPUT
    assert dd(w=None) == _lib.INVALID_INPUT and dd(w=V((8 << 20) + 8)) == _lib.INVALID_INPUT
    assert dd(wb=16) == _lib.OUTPUT_TOO_SMALL
    assert dd(p=_lib.Params(4, 10, 16)) == _lib.UNSUPPORTED and dd(p=_lib.Params(8, 9, 16)) == _lib.INVALID_INPUT
    # host-pointer forms
    henc, hdec = L.redux_encode_blocks_const, L.redux_decode_blocks_const
    x = np.zeros(16, np.uint8)
    out = np.zeros(64, np.uint8)
    offs = np.zeros(5, np.uint64)
    sizes = np.zeros(4, np.uint32)
    fl = np.zeros(4, np.uint8)
    px, po, pf, ps, pc = x.ctypes.data, out.ctypes.data, offs.ctypes.data, sizes.ctypes.data, fl.ctypes.data
    assert henc(C.byref(ok), px, 16, None, 0, 4, 3, po, 64, pf, pc, None, None) == _lib.INVALID_INPUT      # bad E
    assert henc(C.byref(ok), px, 16, None, 0, 0, 2, po, 64, pf, pc, None, None) == _lib.INVALID_INPUT      # block size 0
    assert henc(C.byref(ok), None, 16, None, 0, 4, 2, po, 64, pf, pc, None, None) == _lib.INVALID_INPUT    # null input
    assert henc(C.byref(ok), px, 16, None, 16, 4, 2, po, 64, pf, pc, None, None) == _lib.INVALID_INPUT     # null base with a length
    assert henc(C.byref(ok), px, 16, None, 0, 4, 2, None, 64, pf, pc, None, None) == _lib.INVALID_INPUT
    assert henc(C.byref(ok), px, 16, None, 0, 4, 2, po, 64, None, pc, None, None) == _lib.INVALID_INPUT
    assert henc(C.byref(ok), px, 16, None, 0, 4, 2, po, 64, pf, None, None, None) == _lib.INVALID_INPUT    # null flags
    assert henc(C.byref(_lib.Params(8, 9, 16)), px, 16, None, 0, 4, 2, po, 64, pf, pc, None, None) == _lib.INVALID_INPUT
    assert henc(C.byref(_lib.Params(4, 10, 16)), px, 16, None, 0, 4, 2, po, 64, pf, pc, None, None) == _lib.UNSUPPORTED
    assert hdec(C.byref(ok), po, pf, pc, None, 0, 16, 4, 3, px, ps, None, None) == _lib.INVALID_INPUT      # bad E
    assert hdec(C.byref(ok), po, pf, pc, None, 0, 16, 0, 2, px, ps, None, None) == _lib.INVALID_INPUT      # block size 0
    assert hdec(C.byref(ok), po, pf, None, None, 0, 16, 4, 2, px, ps, None, None) == _lib.INVALID_INPUT    # null flags
    assert hdec(C.byref(ok), po, pf, pc, None, 16, 16, 4, 2, px, ps, None, None) == _lib.INVALID_INPUT     # null base with a length
    assert hdec(C.byref(ok), po, None, pc, None, 0, 16, 4, 2, px, ps, None, None) == _lib.INVALID_INPUT
    assert hdec(C.byref(ok), po, pf, pc, None, 0, 16, 4, 2, None, ps, None, None) == _lib.INVALID_INPUT
    assert hdec(C.byref(ok), po, pf, pc, None, 0, 16, 4, 2, px, None, None, None) == _lib.INVALID_INPUT
    assert hdec(C.byref(_lib.Params(4, 10, 16)), po, pf, pc, None, 0, 16, 4, 2, px, ps, None, None) == _lib.UNSUPPORTED


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_const_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "const_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "const_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_const_mirror_compiles_and_refuses(rx, tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_const_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "const mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
