"""Snapshot-stride filter (include/redux_hip.h, "snapshot-stride filter"): the numpy restatement against hand-written
expectations, the value claim on the CPU oracle, container version 15 kind 2, the refusals of the Python layer and the CLI,
the range paths that do not exist for it, the host-only ABI, and the host-side arithmetic under sanitizers.  No GPU call."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import cbind as ox
from test_base_cpu import OFFS, STREAMS, TOTAL, header_parse_only, no_library
from test_planes_cpu import lengths, planes_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = (8, 30, 32)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def stride_ref(x, E, S, inverse=False):
    """The filter alone, over the n = len // E whole little-endian elements of the WHOLE buffer: z[i] = x[i] for i < S,
    z[i] = fold(x[i] - x[i - S] mod 2^(8E)) from S on, fold(d) = (d << 1) ^ (0 - (d >> (8E - 1))); trailing bytes unchanged.
    inverse=True: x[i] = unfold(z[i]) + x[i - S] for i from S upward, a snapshot at a time."""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    n = len(x) // E
    out = x.copy()
    if S >= n:
        return out
    dt = np.dtype("<u%d" % E)
    v = x[: n * E].view(dt).copy()
    one, top = dt.type(1), dt.type(8 * E - 1)
    with np.errstate(over="ignore"):
        if not inverse:
            d = v[S:] - v[:-S]
            v[S:] = (d << one) ^ (dt.type(0) - (d >> top))
        else:
            for t in range(S, n, S):  # snapshot t // S from the one before it, which is final
                z = v[t: t + S]
                v[t: t + S] = ((z >> one) ^ (dt.type(0) - (z & one))) + v[t - S: t - S + len(z)]
    out[: n * E] = v.view(np.uint8)
    return out


def stride_planes_ref(x, E, S, B, inverse=False):
    """What redux_stride_planes_dev computes: the byte-plane layout of the filter's output, or the inverse of both"""
    if inverse:
        return stride_ref(planes_ref(x, E, B, inverse=True), E, S, inverse=True)
    return planes_ref(stride_ref(x, E, S), E, B)


def words(values, E):
    return np.array(values, dtype=np.dtype("<u%d" % E)).view(np.uint8)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_restatement_against_hand_written_expectations(E):
    top = (1 << 8 * E) - 1
    tail = np.array([0x5A] if E > 1 else [], dtype=np.uint8)  # (a trailing byte; at E = 1 it would be a ninth element)
    x = np.concatenate([words([10, 100, 12, 97, 11, 100, 0, top], E), tail])
    # S = 1: differences to the element before: +90, -88, +85, -86, +89, -100, -1 -> folds 180, 175, 170, 171, 178, 199, 1
    assert np.array_equal(stride_ref(x, E, 1), np.concatenate([words([10, 180, 175, 170, 171, 178, 199, 1], E), tail]))
    # S = 3: 97 - 10 = +87, 11 - 100 = -89, 100 - 12 = +88, 0 - 97 = -97, top - 11 = -12 mod 2^(8E)
    assert np.array_equal(stride_ref(x, E, 3), np.concatenate([words([10, 100, 12, 174, 177, 176, 193, 23], E), tail]))
    # S = 8 = n: nothing has a predecessor
    assert np.array_equal(stride_ref(x, E, 8), x) and np.array_equal(stride_ref(x, E, 8, inverse=True), x)
    for S in (1, 3, 8, 9, 1 << 40):
        assert np.array_equal(stride_ref(stride_ref(x, E, S), E, S, inverse=True), x)
    # the extremes of the fold: -2^(8E-1) folds to all ones, and all ones unfolds to it
    half = 1 << (8 * E - 1)
    assert np.array_equal(stride_ref(words([half, 0], E), E, 1), words([half, top], E))
    assert np.array_equal(stride_ref(words([half, top], E), E, 1, inverse=True), words([half, 0], E))


@pytest.mark.parametrize("B", [4, 16])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_restatement_round_trips(E, B):
    rng = np.random.default_rng(E * 1000 + B)
    for L in lengths(E, B):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        n = L // E
        for S in sorted({1, 2, 3, 5, max(n - 1, 1), max(n, 1), n + 7}):
            z = stride_ref(x, E, S)
            assert np.array_equal(z[n * E:], x[n * E:]) and np.array_equal(z[: min(S, n) * E], x[: min(S, n) * E])
            assert np.array_equal(stride_ref(z, E, S, inverse=True), x), (E, B, L, S)
            p = stride_planes_ref(x, E, S, B)
            assert np.array_equal(p, planes_ref(z, E, B))
            assert np.array_equal(stride_planes_ref(p, E, S, B, inverse=True), x), (E, B, L, S)
            if S >= n:
                assert np.array_equal(p, planes_ref(x, E, B))


# ---- the value claim, on the CPU oracle ------------------------------------------------------------------------------------
def series():
    """-> {name: (bytes, E, S)}, drawn from one generator in this order"""
    rng = np.random.default_rng(29)
    base = rng.uniform(0, 80, (10000, 3))
    traj = (base[None] + np.cumsum(rng.normal(0, .02, (12, 10000, 3)), axis=0)).astype(np.float32)
    scene = rng.integers(2000, 9000, (128, 160)).astype(np.float64)
    t = np.arange(6, dtype=np.float64)[:, None, None]
    frames = np.clip(scene[None] + 30 * np.sin(t / 5) + rng.normal(0, 6, (6, 128, 160)), 0, 65535).astype(np.uint16)
    noise = rng.normal(0, .02, (6, 50000)).astype(np.float32)
    return {"trajectory": (traj.tobytes(), 4, 30000), "frames": (frames.tobytes(), 2, 20480), "unrelated": (noise.tobytes(), 4, 50000)}


def oracle_total(data, B):
    data = bytes(data)
    return sum(len(s) for s in ox.compress_blocks(data, B, PARAMS)[0])


def best_existing(data, E, B):
    """the smallest of plain, the byte-plane layout, the zigzag filter and the lag filter at lag 3"""
    from test_lag_cpu import lag_planes_ref
    from test_zigzag_cpu import zigzag_planes_ref
    x = np.frombuffer(data, dtype=np.uint8)
    return min(oracle_total(x, B), oracle_total(planes_ref(x, E, B), B), oracle_total(zigzag_planes_ref(x, E, B), B),
               oracle_total(lag_planes_ref(x, E, B, 3), B))


def test_stride_difference_pays_on_related_snapshots_and_costs_on_unrelated_ones():
    """Measured with this generator: trajectory 783,044 against 1,166,138 (0.671), frames 107,717 against 202,942 (0.531),
    unrelated 1,040,513 against 1,023,366 (1.017)"""
    B, ratio = 4096, {}
    for name, (data, E, S) in series().items():
        got = oracle_total(stride_planes_ref(np.frombuffer(data, dtype=np.uint8), E, S, B), B)
        best = best_existing(data, E, B)
        ratio[name] = got / best
        print(f"{name}: stride {got} against best existing {best}, ratio {ratio[name]:.3f}")
    assert ratio["trajectory"] <= 0.75
    assert ratio["frames"] <= 0.60
    assert ratio["unrelated"] >= 1.0


# ---- container version 15, kind 2 ------------------------------------------------------------------------------------------
def oracle_container(E, S, B=4096, checksum=False, n=3 * 4096 * 8 + 29):
    """-> (x, the container of the oracle's streams behind the restatement, the streams' bytes)"""
    import zlib
    from redux_amd import container
    x = np.cumsum(np.random.default_rng(E * 7 + S).integers(-2, 3, n), dtype=np.int64).astype(np.uint8)
    streams, _ = ox.compress_blocks(stride_planes_ref(x, E, S, B).tobytes(), B, PARAMS)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.uint64)
    payload = np.frombuffer(b"".join(streams), dtype=np.uint8)
    crc = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(len(streams))], dtype=np.uint32) if checksum else None
    return x, container.pack(payload, offs, PARAMS, B, n, element_size=E, block_crc=crc, filter="stride", stride=S), payload, offs, crc


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_container_kind_2_roundtrip_with_oracle_streams(rx, E):
    from redux_amd import container
    for S, checksum in ((1, False), (5000, True), (1 << 40, False)):
        x, buf, payload, offs, crc = oracle_container(E, S, checksum=checksum)
        nb = len(offs) - 1
        assert buf[4] == (0x1F if checksum else 0x0F)
        assert int.from_bytes(buf[12:16], "little") == 0xF0000000 | 2 << 24 | E          # the exact word: nothing else in it
        assert struct.unpack_from("<Q", buf, 32)[0] == S                                 # the record, behind the header
        c = container._parse(buf)
        assert c.params.triple() == PARAMS and c.block_size == 4096 and c.total == len(x) and c.element_size == E
        assert c.filter == "stride" and c.stride == S and c.record is None and c.lag is None and c.order is None and c.base is None
        assert c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == payload.tobytes()
        assert (c.crcs is None) if crc is None else c.crcs.tolist() == crc.tolist()
        assert container.stride(buf) == (E, S) and container.record(buf) is None and container.filter(buf) == "stride"
        assert container.element_size(buf) == E and container.header_is_wellformed(buf) and container.lag(buf) is None
        assert len(buf) - len(payload) == container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="stride")
        # version 2's sections behind the record: the same bytes but for the version, the word and the 8 bytes of S
        v2 = container.pack(payload, offs, PARAMS, 4096, len(x), element_size=E, block_crc=crc)
        if E > 1:
            assert buf[:4] + buf[5:12] + buf[16:32] + buf[40:] == v2[:4] + v2[5:12] + v2[16:]
    assert container.stride(container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL)) is None
    assert container.stride(container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, record_size=12)) is None


def test_container_kind_2_refuses_every_malformed_word_and_record(rx):
    from redux_amd import container
    good = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=4, filter="stride", stride=30000)
    assert container.header_is_wellformed(good) and container.stride(good) == (4, 30000)

    def with_word(word, ver=15):
        bad = bytearray(good)
        bad[4] = ver
        bad[12:16] = word.to_bytes(4, "little")
        return bytes(bad)
    # 0xF2000017 and its like: any bit beside the kind and E, an E outside the set, other kinds
    words = [0xF2000017, 0xF3000017, 0xFF000017, 0xF2000000, 0xF2000003, 0xF2000005, 0xF2000006, 0xF2000007, 0xF2000009, 0xF200000C,
             0xF200000F, 0xF2000014, 0xF2000104, 0xF2001004, 0xF2010004, 0xF2100004, 0xF2800004, 0xF3000004, 0xF4000004, 0xF0000004,
             0xFA000004, 0x02000004, 0xE2000004, 0xD2000004]
    words += [0xF2000004 | 1 << bit for bit in range(4, 24)]
    for word in words:
        for ver in (15, 0x1F):
            assert not container.header_is_wellformed(with_word(word, ver)), hex(word)
            with pytest.raises(rx.InvalidInput):
                container._parse(with_word(word, ver))
    for E in (1, 2, 4, 8):
        assert container.header_is_wellformed(with_word(0xF2000000 | E)) and container.stride(with_word(0xF2000000 | E)) == (E, 30000)
    # no other version byte takes the word, and the kind has no stored blocks
    for ver in list(range(1, 15)) + [0x10 | v for v in range(1, 15)] + [0x4F, 0x5F, 0x2F, 0x8F]:
        assert not container.header_is_wellformed(with_word(0xF2000004, ver)), hex(ver)
        with pytest.raises(rx.InvalidInput):
            container._parse(with_word(0xF2000004, ver))
    # S = 0 is malformed; a record or anything behind it cut short is Eof
    zero = bytearray(good)
    zero[32:40] = bytes(8)
    with pytest.raises(rx.InvalidInput):
        container._parse(bytes(zero))
    assert len(good) == 32 + 8 + 12 + 10
    for cut in (31, 32, 33, 39, 40, 41, 51, 52, len(good) - 1):
        with pytest.raises(rx.Eof):
            container._parse(good[:cut])
        with pytest.raises(rx.Eof):
            container.stride(good[:cut])
    big = bytearray(good)
    big[32:40] = (2 ** 64 - 1).to_bytes(8, "little")  # any S from 1 up is the layout alone past n: well-formed
    assert container.stride(bytes(big)) == (4, 2 ** 64 - 1)


def test_writers_without_the_filter_emit_the_bytes_they_emitted_before(rx):
    from redux_amd import container
    pk = lambda **kw: container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, **kw)
    crc = np.array([1, 2, 3], dtype=np.uint32)
    assert pk(stride=None) == pk() and pk()[4] == 1 and len(pk()) == 32 + 12 + 10
    for kw in ({"element_size": 4}, {"filter": "zigzag", "element_size": 2}, {"filter": "lag", "lag": 3}, {"record_size": 12},
               {"base": (5, 6)}, {"block_crc": crc}):
        assert pk(stride=None, **kw) == pk(**kw)
    assert pk(record_size=12)[4] == 15 and int.from_bytes(pk(record_size=12)[12:16], "little") == 0xF100000C
    assert pk(element_size=4)[4] == 2 and pk(filter="lag", lag=3)[4] == 13
    assert container.overhead_bytes("adaptive", 3, 4, filter="stride") == container.overhead_bytes("adaptive", 3, 4) + 8
    for kw in ({"stored": True}, {"mixed": True}, {"base": True}, {"record_size": 12}):
        with pytest.raises(rx.InvalidInput):
            container.overhead_bytes("adaptive", 3, 4, filter="stride", **kw)
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("static", 3, filter="stride")


# ---- refusals before the library is touched ---------------------------------------------------------------------------------

def test_python_api_refuses_before_any_library_call(rx, monkeypatch):
    import inspect
    from redux_amd import api, container
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)
    static = rx.StaticModel(PARAMS, np.arange(258))
    models = [static, rx.PlaneStaticModel(PARAMS, np.tile(np.arange(258), (2, 1))), rx.SegmentStaticModel.template(PARAMS, 2)]
    no_library(monkeypatch)
    calls = []
    # a stride without the filter, the filter without a stride, and strides that are none
    for kw in ({"stride": 3}, {"filter": "stride"}, {"filter": "zigzag", "stride": 3}, {"filter": "lag", "lag": 2, "stride": 3},
               {"filter": "stride", "stride": 0}, {"filter": "stride", "stride": -1}, {"filter": "stride", "stride": True},
               {"filter": "stride", "stride": 3.0}, {"filter": "stride", "stride": "3"}, {"filter": "stride", "stride": 1 << 64},
               # and everything the filter does not go with
               {"filter": "stride", "stride": 3, "stored": flags}, {"filter": "stride", "stride": 3, "base": b"abcd"},
               {"filter": "stride", "stride": 3, "constant": flags}, {"filter": "stride", "stride": 3, "constant": True},
               {"filter": "stride", "stride": 3, "unit_layouts": True}, {"filter": "stride", "stride": 3, "record_size": 4},
               {"filter": "stride", "stride": 3, "lag": 2}, {"filter": "stride", "stride": 3, "order": 1}):
        calls += [lambda kw=kw: rx.compress_blocks(b"abcd", 4, **kw),
                  lambda kw=kw: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                  lambda kw=kw: container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, **kw)]
        if "unit_layouts" not in kw:
            dev = {("constant" if k == "constant" else k): (True if k == "constant" else v) for k, v in kw.items() if k != "stored"}
            if dev != {"filter": "stride", "stride": 3}:
                calls += [lambda dev=dev: rx.DeviceEncoder(PARAMS, 4096, 4096, **dev), lambda dev=dev: rx.DeviceDecoder(PARAMS, 4096, 1, **dev)]
    calls += [lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, filter="stride", stride=3, mixed=True),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, filter="stride", stride=3, mixed=True),
              lambda: rx.decompress_blocks(b"\0", offs, 4, filter="stride", stride=3),          # the length is required
              lambda: rx.stride_planes(None, 4, 4096, 0), lambda: rx.stride_planes(None, 4, 4096, None),
              lambda: container.compress_bytes(b"abcd" * 4, 16, stride=3), lambda: container.compress_bytes(b"abcd" * 4, 16, filter="stride"),
              lambda: container.compress_bytes(b"abcd" * 4, 16, filter="stride", stride=0)]
    for kw in ({"model": "static"}, {"model": "auto"}, {"stored": True}, {"segment_blocks": 64}, {"base": b"abcd"}, {"skip_constant": True},
               {"layout": "auto"}, {"layout": "mixed"}, {"record_size": 4}, {"record_size": "auto"}, {"lag": 2}, {"lag": "auto"}, {"order": 2},
               {"order": "auto"}, {"base_op": "sub"}, {"block_size": 0}):
        calls += [lambda kw=kw: container.compress_bytes(b"abcd" * 4, **{"block_size": 16, "filter": "stride", "stride": 3, **kw})]
    for m in models:  # a static model
        calls += [lambda m=m: rx.compress_blocks(b"abcd", 4, m, filter="stride", stride=3),
                  lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, filter="stride", stride=3),
                  lambda m=m: rx.DeviceEncoder(m, 4096, 4096, filter="stride", stride=3),
                  lambda m=m: rx.DeviceDecoder(m, 4096, 1, filter="stride", stride=3),
                  lambda m=m: container.pack(STREAMS, OFFS, m, 65536, TOTAL, filter="stride", stride=3)]
    for i, call in enumerate(calls):
        with pytest.raises(rx.InvalidInput):
            call()
    r = api._resolve_front(None, 4, "stride", stride=np.int64(30000))
    assert r.front.infix == "stride" and r.front.stride == 30000 and type(r.front.stride) is int and not r.constant and not r.mixed
    assert api._elem_args(r.front, 4) == (4, 30000)
    # stride= stands directly before record_size= wherever both are taken
    for f in (rx.compress_blocks, rx.decompress_blocks, rx.DeviceEncoder.__init__, rx.DeviceDecoder.__init__, container.compress_bytes,
              container.pack):
        names = list(inspect.signature(f).parameters)
        assert names[names.index("record_size") - 1] == "stride" and inspect.signature(f).parameters["stride"].default is None, f


def test_range_reads_of_kind_2_are_unsupported(rx, monkeypatch):
    from redux_amd import container
    buf = container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=4, filter="stride", stride=30000)
    header_parse_only(monkeypatch)
    reader = container.Reader(buf)
    assert reader.stride == 30000 and reader.filter == "stride" and reader.record is None
    with pytest.raises(rx.Unsupported):
        reader.read(0, 16)
    with pytest.raises(rx.Unsupported):
        reader.read_many([(0, 1), (70000, 5)])
    with pytest.raises(rx.Unsupported):
        container.decompress_range(buf, 0, 0)


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_stride_flags(rx, tmp_path, capsys):
    from redux_amd import cli, container
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "stride", "--stride", "30000", "--element-size", "4"]) == \
        {**base, "filter": "stride", "stride": 30000, "element_size": 4}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "stride", "--stride", str(2 ** 64 - 1), "--checksum"]) == \
        {**base, "filter": "stride", "stride": 2 ** 64 - 1, "checksum": True}
    ok = ["-c", "--block-size", "65536", "--filter", "stride", "--stride", "7"]
    assert cli.parse(ok) is not None
    for argv in (["-c", "--block-size", "65536", "--stride", "7"],                          # the stride without its filter
                 ["-c", "--block-size", "65536", "--filter", "zigzag", "--stride", "7"],
                 ["-c", "--block-size", "65536", "--filter", "stride"],                      # the filter without a stride
                 ["-c", "--block-size", "65536", "--filter", "stride", "--stride"],
                 ["-c", "--block-size", "0", "--filter", "stride", "--stride", "7"],
                 ["-c", "--filter", "stride", "--stride", "7"],
                 ["-d", "--filter", "stride", "--stride", "7", "--block-size", "65536"], ["-d", "--stride", "7"]):
        assert cli.parse(argv) is None and cli.main(argv) == 1, argv
    for bad in ("0", "-1", "auto", "1.5", "0x10", "", str(2 ** 64), "٣"):
        assert cli.parse(["-c", "--block-size", "65536", "--filter", "stride", "--stride", bad]) is None, bad
    for extra in (["--stored"], ["--model", "static"], ["--model", "auto"], ["--lag", "2"], ["--order", "2"], ["--order-auto"],
                  ["--record-size", "4"], ["--record-size", "auto"], ["--base", "b.bin"], ["--skip-constant"], ["--layout", "auto"],
                  ["--layout", "mixed"], ["--base-op", "sub"], ["--range", "0:4"]):
        assert cli.parse(ok + extra) is None, extra
    assert "--stride" in cli.USAGE and "stride" in cli.__doc__
    capsys.readouterr()
    # -d --range on a kind 2 container: a usage error with a message, known once the header is read
    packed = tmp_path / "t.rdxb"
    packed.write_bytes(container.pack(STREAMS, OFFS, PARAMS, 65536, TOTAL, element_size=4, filter="stride", stride=30000))
    assert cli.main(["-d", "-i", str(packed), "-o", str(tmp_path / "out"), "--range", "0:16"]) == 1
    err = capsys.readouterr().err
    assert "--range" in err and "stride" in err and "Usage" in err


# ---- the host-only ABI -----------------------------------------------------------------------------------------------------
def test_stride_check_workspace_sizes_and_kernel_names(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in (1, 2, 4, 8):
        for S in (1, 3, 30000, 2 ** 32, 2 ** 64 - 1):
            assert L.redux_stride_check(E, S) == _lib.OK
        assert L.redux_stride_check(E, 0) == _lib.INVALID_INPUT
    for E in (0, 3, 5, 16, 2 ** 32 - 1):
        assert L.redux_stride_check(E, 1) == _lib.INVALID_INPUT
    cp = _lib.Params(*PARAMS)
    n, B = 1 << 24, 65536
    for E in (1, 2, 4, 8):
        assert L.redux_encode_stride_workspace_bytes(C.byref(cp), n, B, E) == L.redux_encode_zigzag_workspace_bytes(C.byref(cp), n, B, E)
        planes = L.redux_decode_planes_workspace_bytes(C.byref(cp), n, B, E)
        # no segments where a snapshot fills the machine or S >= n; a bounded workspace where it does not
        for S in (n // E, n, 2 ** 40, (1 << 22) // E * 16):
            assert L.redux_stride_workspace_bytes(n, E, S) == 0
            assert L.redux_decode_stride_workspace_bytes(C.byref(cp), n, B, E, S) == (planes + 255) // 256 * 256
        for S in (1, 3, 64, 1024):
            ws = L.redux_stride_workspace_bytes(n, E, S)
            assert 0 < ws <= (1 << 18) * 16 + 512 and ws % 256 == 0
            assert L.redux_decode_stride_workspace_bytes(C.byref(cp), n, B, E, S) == (planes + 255) // 256 * 256 + ws
            assert L.redux_stride_workspace_bytes(2 * n, E, S) >= ws  # (never falls as the length grows)
        assert L.redux_decode_stride_workspace_bytes(C.byref(cp), n, B, E, 0) == 0
    assert L.redux_stride_workspace_bytes(n, 3, 1) == 0 and L.redux_decode_stride_workspace_bytes(C.byref(cp), n, B, 3, 1) == 0
    assert L.redux_encode_stride_workspace_bytes(C.byref(cp), n, B, 3) == 0
    name = rx.stride_kernel_name
    assert name(3 * 4 * 4096 + 5, 4096, 4, 1024) == "k_stride_planes + k_stride_planes_bytes"
    assert name(3 * 4 * 4096, 4096, 4, 1024) == "k_stride_planes" and name(3 * 4 * 4096, 100, 4, 1024) == "k_stride_planes_bytes"
    assert name(3 * 4 * 4096, 4096, 4, 1024, inverse=True) == "k_planes + k_stride_sum"
    assert name(3 * 4 * 4096 + 5, 4096, 4, 1025, inverse=True) == "k_planes + k_planes_bytes + k_stride_sum_bytes"
    assert name(3 * 4 * 4096 + 8, 4096, 4, 1024, inverse=True) == "k_planes + k_planes_bytes + k_stride_sum + k_stride_sum_tail"
    assert name(1 << 24, 4096, 4, 64, inverse=True) == "k_planes + k_stride_totals + k_stride_scan + k_stride_sum"
    assert name(400012, 4096, 4, 3, inverse=True) == "k_planes + k_planes_bytes + k_stride_totals_bytes + k_stride_scan_bytes + k_stride_sum_bytes"
    assert name(1 << 20, 4096, 1, 4096, inverse=True) == "copy + k_stride_totals + k_stride_scan + k_stride_sum"  # (256 columns)
    assert name(1 << 20, 4096, 1, 1 << 18, inverse=True) == "copy + k_stride_sum"
    assert name(1 << 20, 4096, 4, 1 << 18, inverse=True) == "k_planes" and name(1 << 20, 4096, 4, 2 ** 64 - 1) == "k_stride_planes"
    for bad in ((0, 4096, 4, 3), (4096, 0, 4, 3), (4096, 4096, 3, 3), (4096, 4096, 4, 0)):
        assert name(*bad) == "" and name(*bad, inverse=True) == ""
    for entry in ("stride_planes", "stride_kernel_name"):
        assert getattr(rx, entry) is getattr(rx.api, entry)


# ---- the host-side arithmetic under sanitizers -----------------------------------------------------------------------------
def test_check_plan_and_record_under_address_and_undefined_sanitizers(tmp_path):
    """redux_stride_check, the segment-count and workspace arithmetic and the container record are split from the launches
    (redux_stride_host.hpp): a stand-alone program runs them at their extremes"""
    exe = str(tmp_path / "stride_plan_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "stride_plan_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout, run.stderr)
