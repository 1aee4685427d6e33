"""Lagged delta filter for interleaved channels and fixed-width records (include/redux_hip.h, "lagged delta filter"): the
numpy restatement of the rule against hand-written expectations and against the zigzag filter's restatement at lag 1, the
value claim on the CPU oracle, container version 13, the Python argument checks, the CLI flags, the range reader, the
host-only ABI helpers and the C++ mirror's refusals.  No GPU call.

The value claim rests on GENERATED data, interleaved random walks and four-column records: nothing in the corpus fixtures
interleaves series."""
import ctypes as C
import io

import numpy as np
import pytest

from test_delta_cpu import delta_ref
from test_planes_cpu import lengths, oracle_bytes, planes_ref
from test_zigzag_cpu import zigzag_planes_ref, zigzag_ref

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def lag_ref(x, E, B, S, inverse=False):
    """The rule: frames of E*B bytes; in a frame of N whole elements d[i] = x[i] for i < S and x[i] - x[i-S] mod 2^(8E) for
    i >= S, then z = (d << 1) ^ (0 - (d >> (8E-1))) for every element; the trailing bytes of a frame unchanged.  inverse=True
    unfolds with d = (z >> 1) ^ (0 - (z & 1)) and takes the S running sums of the frame.  (The byte-plane layout is
    planes_ref's, behind this.)"""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    assert 1 <= S <= 256
    dt = np.dtype("<u%d" % E)
    one, zero, top = dt.type(1), dt.type(0), dt.type(8 * E - 1)
    out = x.copy()
    for f0 in range(0, len(x), E * B):
        N = len(x[f0: f0 + E * B]) // E
        if N == 0:
            continue
        v = x[f0: f0 + N * E].copy().view(dt)
        if inverse:
            r = (v >> one) ^ (zero - (v & one))
            for c in range(min(S, N)):  # chain c: elements c, c + S, ...
                r[c::S] = np.cumsum(r[c::S], dtype=dt)
        else:
            d = v.copy()
            d[S:] = v[S:] - v[:-S] if N > S else d[S:]
            r = (d << one) ^ (zero - (d >> top))
        out[f0: f0 + N * E] = r.view(np.uint8)
    return out


def lag_planes_ref(x, E, B, S, inverse=False):
    """what redux_lag_planes_dev computes: the filter, then the layout; the inverse the other way round"""
    if inverse:
        return lag_ref(planes_ref(x, E, B, inverse=True), E, B, S, inverse=True)
    return planes_ref(lag_ref(x, E, B, S), E, B)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_rule_matches_hand_written_expectations(E):
    dt = np.dtype("<u%d" % E)
    top = (1 << 8 * E) - 1
    v = np.array([10, 100, 12, 97, 11, 100, 0, top], dtype=dt)
    x = np.concatenate([v.view(np.uint8), np.array([0xEE] * (E > 1), dtype=np.uint8)])  # + a trailing odd byte
    fold = lambda d: 2 * d if d >= 0 else -2 * d - 1
    # one frame, S = 2: the first two as they stand, then +2, -3, -1, +3, -11, and top - 100 = -101 mod 2^(8E)
    want2 = [20, 200, fold(2), fold(-3), fold(-1), fold(3), fold(-11), fold(-101)]
    z = lag_ref(x, E, 16, 2)
    assert z[: 8 * E].view(dt).tolist() == want2 and z[8 * E:].tolist() == x[8 * E:].tolist()
    assert lag_ref(z, E, 16, 2, inverse=True).tolist() == x.tolist()
    # S = 3: three as they stand, then 97 - 10, 11 - 100, 100 - 12, 0 - 97, top - 11 = -12
    want3 = [20, 200, 24, fold(87), fold(-89), fold(88), fold(-97), fold(-12)]
    z = lag_ref(x, E, 16, 3)
    assert z[: 8 * E].view(dt).tolist() == want3 and z[8 * E:].tolist() == x[8 * E:].tolist()
    assert lag_ref(z, E, 16, 3, inverse=True).tolist() == x.tolist()
    # a second frame starts afresh: B = 4, S = 2: elements 4 and 5 are folded as they stand, 6 and 7 are differences in it
    z4 = lag_ref(x, E, 4, 2)
    assert z4[: 8 * E].view(dt).tolist() == [20, 200, fold(2), fold(-3), 22, 200, fold(-11), fold(-101)]
    assert z4[8 * E:].tolist() == x[8 * E:].tolist() and lag_ref(z4, E, 4, 2, inverse=True).tolist() == x.tolist()
    # S >= N folds every element and subtracts nothing (the two's complement reading: top = -1 -> 1)
    for S in (8, 9, 256):
        zs = lag_ref(x, E, 16, S)
        assert zs[: 8 * E].view(dt).tolist() == [20, 200, 24, 194, 22, 200, 0, 1]
        assert lag_ref(zs, E, 16, S, inverse=True).tolist() == x.tolist()
    if E == 1:  # (97 and 100 are non-negative as int8, 200 is not: the fold of a byte that stands for itself)
        assert lag_ref(np.array([100, 200], np.uint8), 1, 16, 8).tolist() == [200, 2 * 56 - 1]


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_lag_one_is_the_zigzag_filter(E):
    rng = np.random.default_rng(E)
    for Bk in (4, 100, 4096):
        for L in lengths(E, Bk):
            x = rng.integers(0, 256, L, dtype=np.uint8)
            assert np.array_equal(lag_ref(x, E, Bk, 1), zigzag_ref(x, E, Bk)), (E, Bk, L)
            assert np.array_equal(lag_ref(x, E, Bk, 1, inverse=True), zigzag_ref(x, E, Bk, inverse=True)), (E, Bk, L)
            assert np.array_equal(lag_planes_ref(x, E, Bk, 1), zigzag_planes_ref(x, E, Bk)), (E, Bk, L)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("Bk", [4, 100, 4096])
def test_inverse_of_forward_is_identity(E, Bk):
    rng = np.random.default_rng(E * 10000 + Bk)
    for S in (1, 2, 3, 7, 16, 255, 256):
        for L in lengths(E, Bk):
            x = rng.integers(0, 256, L, dtype=np.uint8)
            y = lag_planes_ref(x, E, Bk, S)
            assert len(y) == L
            assert np.array_equal(lag_planes_ref(y, E, Bk, S, inverse=True), x), (E, Bk, S, L)
            assert np.array_equal(lag_ref(lag_ref(x, E, Bk, S), E, Bk, S, inverse=True), x), (E, Bk, S, L)
            assert np.array_equal(lag_ref(lag_ref(x, E, Bk, S, inverse=True), E, Bk, S), x), (E, Bk, S, L)


# ---- the value claim, on the CPU oracle --------------------------------------------------------------------------------
def channels(C_, E, seed):
    rng = np.random.default_rng(seed)
    n = 3 * B + 100
    w = np.stack([np.cumsum(np.round(rng.normal(0, 50, n))) + 5000 * c * (-1) ** c for c in range(C_)], 1)
    return w.reshape(-1).astype(np.int64).astype("<i%d" % E).view(np.uint8)


def records(seed):
    rng = np.random.default_rng(seed)
    m = 3 * B + 100
    cols = [np.cumsum(rng.integers(990, 1010, m)), np.arange(m) * 3 + 7,
            np.cumsum(np.round(rng.normal(0, 20, m))), rng.integers(0, 2, m)]
    return np.stack(cols, 1).reshape(-1).astype(np.int64).astype("<i4").view(np.uint8)


def best_existing(x, E):
    """the smallest oracle total over the fronts that exist without the lag: plain bytes, planes, delta and zigzag"""
    return min(oracle_bytes(x, B), oracle_bytes(planes_ref(x, E, B), B), oracle_bytes(planes_ref(delta_ref(x, E, B), E, B), B),
               oracle_bytes(zigzag_planes_ref(x, E, B), B))


@pytest.mark.parametrize("C_", [2, 3, 6])
@pytest.mark.parametrize("E", [2, 4])
def test_lag_pays_on_interleaved_channels(C_, E):
    x = channels(C_, E, 100 + 10 * C_ + E)
    best = best_existing(x, E)
    lag = oracle_bytes(lag_planes_ref(x, E, B, C_), B)
    print("%d channels, E = %d: best existing %d, lag %d: %d, %.3f x" % (C_, E, best, C_, lag, lag / best))
    assert lag <= 0.75 * best, (C_, E, best, lag)


def test_lag_pays_on_records_of_four_columns():
    x = records(1)
    best = best_existing(x, 4)
    lag = oracle_bytes(lag_planes_ref(x, 4, B, 4), B)
    print("records of 4 int32 columns: best existing %d, lag 4: %d, %.3f x" % (best, lag, lag / best))
    assert lag <= 0.60 * best, (best, lag)


def test_a_wrong_lag_costs_bytes():
    """why the filter is opt-in and nothing chooses the lag"""
    x = channels(3, 2, 132)
    best = best_existing(x, 2)
    wrong = oracle_bytes(lag_planes_ref(x, 2, B, 4), B)
    print("3 channels, E = 2, lag 4: best existing %d, lag 4: %d, %.3f x" % (best, wrong, wrong / best))
    assert wrong > best, (best, wrong)


# ---- container version 13 -----------------------------------------------------------------------------------------------
def test_container_v13_roundtrip_and_others_unchanged(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    crc = np.array([1, 2, 3], dtype=np.uint32)
    for E in (1, 2, 4, 8):
        v11 = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="zigzag")
        v1b = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, block_crc=crc, filter="zigzag")
        assert v11[4] == 11 and int.from_bytes(v11[12:16], "little") == 0xB0000000 | E and container.lag(v11) is None
        assert container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="zigzag", lag=None) == v11
        for S in (1, 3, 256):
            v13 = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="lag", lag=S)
            assert v13[4] == 13 and int.from_bytes(v13[12:16], "little") == 0xD0000000 | S << 4 | E
            assert v13[:4] + v13[5:12] + v13[16:] == v11[:4] + v11[5:12] + v11[16:]  # version 11's bytes but the version and the word
            c = container._parse(v13)
            assert c.params.triple() == PARAMS and c.block_size == 65536 and c.total == total and c.element_size == E
            assert c.filter == "lag" and c.lag == S and c.static is None and c.crcs is None and c.stored is None and c.base is None
            assert c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == streams.tobytes()
            assert container.filter(v13) == "lag" and container.lag(v13) == S and container.element_size(v13) == E
            assert container.header_is_wellformed(v13)
            v1d = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, block_crc=crc, filter="lag", lag=S)
            assert v1d[4] == 0x1D and v1d[:4] + v1d[5:12] + v1d[16:] == v1b[:4] + v1b[5:12] + v1b[16:]
            assert container.filter(v1d) == "lag" and container.lag(v1d) == S and container.block_crcs(v1d).tolist() == [1, 2, 3]
            assert container._parse(v1d).payload.tobytes() == streams.tobytes()
            for cut in (len(v1d) - 1, len(v1d) - 11, 32 + 12 + 11, 32 + 11, 33, 31):  # payload, CRC table, size table, header
                with pytest.raises(rx.Eof):
                    container._parse(v1d[:cut])
            assert len(v13) - len(streams) == container.overhead_bytes("adaptive", 3, E, filter="lag")
        for nb in (1, 3, 1000):
            for checksum in (False, True):
                assert container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="lag") == \
                    container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="zigzag")


def test_container_lag_is_none_for_the_other_versions_and_their_bytes_are_todays(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    size_table = np.diff(offs.astype(np.int64)).astype("<u4").tobytes()
    for ver, word, kw in ((1, 0, {}), (2, 4, {"element_size": 4}), (6, 0x60000004, {"element_size": 4, "filter": "delta"}),
                          (11, 0xB0000004, {"element_size": 4, "filter": "zigzag"})):
        buf = container.pack(streams, offs, PARAMS, 65536, total, **kw)
        # the bytes written before the version existed: header, size table, payload
        assert buf == container.HEADER.pack(b"RDXB", ver, 8, 30, 32, 65536, word, 3, total) + size_table + streams.tobytes()
        assert container.lag(buf) is None and container._parse(buf).lag is None


def test_container_v13_takes_its_word_alone_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, PARAMS, 65536, 10, element_size=2, filter="lag", lag=3)
    assert good[4] == 13 and int.from_bytes(good[12:16], "little") == 0xD0000032
    # S = 0, S = 257, E = 3, another version's nibble with a lag, and the other versions' words
    for word in (0xD0000002, 0xD0000000 | 257 << 4 | 2, 0xD0000033, 0xD0000030, 0xB0000032, 0xC0000032, 0x60000032, 0,
                 2, 0x60000002, 0xA0000000, 0xB0000002, 0xC0000002, 0xD0000000 | 1 << 20 | 2, 0xDFFFFFF2):
        for ver in (13, 0x1D):
            bad = bytearray(good)
            bad[4] = ver
            bad[12:16] = word.to_bytes(4, "little")
            assert not container.header_is_wellformed(bytes(bad)), hex(word)
            with pytest.raises(rx.InvalidInput):
                container._parse(bytes(bad))
            with pytest.raises(rx.InvalidInput):
                container.lag(bytes(bad))
    for E in (1, 2, 4, 8):
        for S in (1, 256):
            for ver in range(256):  # no other version byte takes version 13's word, and it has no stored blocks (0x4D / 0x5D)
                if ver in (13, 0x1D):
                    continue
                bad = bytearray(container.pack(streams, offs, PARAMS, 65536, 10, element_size=E, filter="lag", lag=S))
                bad[4] = ver
                assert not container.header_is_wellformed(bytes(bad)), (E, S, hex(ver))
                with pytest.raises(rx.InvalidInput):
                    container._parse(bytes(bad))
    flags = np.zeros(1, np.uint8)
    static = rx.StaticModel(PARAMS, np.arange(258))
    for kw in ({"element_size": 3}, {"stored": flags}, {"base": (0, 0)}, {"constant": flags},
               {"unit_layouts": np.zeros(1, np.uint8)}, {"params": static}):
        kw = dict(kw)
        params = kw.pop("params", PARAMS)
        with pytest.raises(rx.InvalidInput):  # whatever is refused for zigzag is refused for lag
            container.pack(streams, offs, params, 65536, 10, filter="zigzag", **kw)
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, params, 65536, 10, filter="lag", lag=3, **kw)
    for kw in ({"filter": "lag"}, {"lag": 3}, {"filter": "zigzag", "lag": 3}, {"filter": "delta", "lag": 1},
               {"filter": "lag", "lag": 0}, {"filter": "lag", "lag": 257}, {"filter": "lag", "lag": 2.0},
               {"filter": "lag", "lag": True}, {"filter": "lag", "lag": "3"}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, PARAMS, 65536, 10, element_size=2, **kw)


# ---- Python argument checks ----------------------------------------------------------------------------------------------
def test_python_api_checks_the_lag_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api, container
    static = rx.StaticModel(PARAMS, np.arange(258))
    context = rx.ContextStaticModel(PARAMS, np.tile(np.arange(258), (256, 1)))
    plane = rx.PlaneStaticModel(PARAMS, np.tile(np.arange(258), (2, 1)))
    segment = rx.SegmentStaticModel.template(PARAMS, 2)
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)

    def five(**kw):
        """the five calls that take the filter, with these options"""
        return [lambda: rx.compress_blocks(b"abcd", 4, **kw),
                lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, **kw),
                lambda: rx.DeviceDecoder(PARAMS, 4096, 1, **kw),
                lambda: container.compress_bytes(b"abcd" * 4, 16, **kw)]
    bad = [{"filter": "lag"},                                      # the filter without a lag
           {"lag": 3}, {"filter": "zigzag", "lag": 3}, {"filter": "delta", "lag": 1},   # a lag with another filter, or none
           {"filter": "lag", "lag": 0}, {"filter": "lag", "lag": 257}, {"filter": "lag", "lag": -1},
           {"filter": "lag", "lag": 3.0}, {"filter": "lag", "lag": "3"}, {"filter": "lag", "lag": True},
           {"filter": "lag", "lag": (3,)}, {"filter": "Lag", "lag": 3}]
    for kw in bad:
        for i, call in enumerate(five(**kw)):
            with pytest.raises(rx.InvalidInput):
                call()
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(None, **kw)
    with pytest.raises(rx.InvalidInput):
        api.lag_planes(None, 2, 4096, 0)
    with pytest.raises(rx.InvalidInput):
        api.lag_planes(None, 2, 4096, 257)
    # everything refused for zigzag is refused for lag
    for f in ({"filter": "zigzag"}, {"filter": "lag", "lag": 3}):
        c = [lambda m=m: rx.compress_blocks(b"abcd", 4, m, **f) for m in (static, context, plane, segment)]
        c += [lambda m=m: rx.decompress_blocks(b"\0", offs, 4, m, length=4, **f) for m in (static, context, plane, segment)]
        c += [lambda: rx.compress_blocks(b"abcd", 4, stored=flags, **f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, stored=flags, **f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, **f),                     # the filter needs the length
              lambda: rx.compress_blocks(b"abcd", 4, base=b"abcd", **f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, base=b"abcd", **f),
              lambda: rx.compress_blocks(b"abcd", 4, constant=True, **f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, constant=flags, **f),
              lambda: rx.compress_blocks(b"abcd", 4, unit_layouts=True, **f),
              lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, unit_layouts=flags, **f),
              lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, base=flags, **f),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, base=flags, **f),
              lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, constant=True, **f),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, constant=True, **f),
              lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, mixed=True, **f),
              lambda: rx.DeviceDecoder(PARAMS, 4096, 1, mixed=True, **f)]
        for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
                   {"model": "context-static"}, {"model": "auto"}, {"stored": True}, {"base": b"abcd"}, {"skip_constant": True},
                   {"layout": "auto"}, {"layout": "mixed"}):
            c.append(lambda kw=kw: container.compress_bytes(b"abcd" * 4, 16, **f, **kw))
        for call in c:
            with pytest.raises(rx.InvalidInput):
                call()
    r = api._resolve_front(None, filter="lag", lag=3)
    assert r.front.infix == "lag" and r.front.lag == 3 and r.front.needs_length and not r.front.takes_base
    assert api._resolve_front(None, filter="lag", lag=np.int64(256)).front.lag == 256
    assert api._resolve_front(None, filter="zigzag").front.lag is None and api._resolve_front(None).front.lag is None
    assert set(api._FILTERS) == {"delta", "zigzag", "lag"} and api.LAG_MAX == 256
    assert len(api.LAYOUTS) == 8 and all(f in (None, "delta") for _, f in api.LAYOUTS)  # the layouts a choice is made among


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_lag_flags(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    some = ["-c", "--block-size", "65536", "--filter", "lag", "--lag", "3"]
    assert cli.parse(some) == {**base, "filter": "lag", "lag": 3}
    assert cli.parse(["-c", "--lag", "256", "--filter", "lag", "--block-size", "65536"]) == {**base, "filter": "lag", "lag": 256}
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "lag", "--lag", "1"]) == \
            {**base, "block_size": 4096, "element_size": int(E), "filter": "lag", "lag": 1}
    assert cli.parse(some + ["--model", "adaptive", "--checksum"]) == {**base, "filter": "lag", "lag": 3, "model": "adaptive", "checksum": True}
    # calls that do not use it get the dicts they got
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "zigzag"]) == {**base, "filter": "zigzag"}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "delta"]) == {**base, "filter": "delta"}
    assert cli.parse(["-c"]) == {**base, "block_size": 0}
    assert cli.parse(["-d", "-i", "a", "-o", "b"]) == {"compress": False, "input": "a", "output": "b", "block_size": 0}
    assert cli.parse(["-d", "--range", "3:4"]) == {"compress": False, "input": None, "output": None, "block_size": 0, "range": (3, 4)}
    head = ["-c", "--block-size", "65536"]
    for bad in (head + ["--filter", "lag"], head + ["--lag", "3"], head + ["--filter", "zigzag", "--lag", "3"],
                head + ["--filter", "delta", "--lag", "1"], head + ["--filter", "lag", "--lag", "0"],
                head + ["--filter", "lag", "--lag", "257"], head + ["--filter", "lag", "--lag", "-1"],
                head + ["--filter", "lag", "--lag", "3.0"], head + ["--filter", "lag", "--lag", "x"],
                head + ["--filter", "lag", "--lag", ""], head + ["--filter", "lag", "--lag"],
                ["-c", "--filter", "lag", "--lag", "3"], ["-c", "--block-size", "0", "--filter", "lag", "--lag", "3"],
                some + ["--stored"], some + ["--base", "f"], some + ["--skip-constant"], some + ["--layout", "auto"],
                some + ["--layout", "mixed"], some + ["--model", "static"], some + ["--element-size", "2", "--model", "plane-static"],
                some + ["--model", "segment-static"], some + ["--model", "context-static"], some + ["--model", "auto"]):
        assert cli.parse(bad) is None, bad
    for bad in (head + ["--filter", "lag"], head + ["--lag", "3"], head + ["--filter", "lag", "--lag", "257"], some + ["--stored"]):
        assert cli.main(bad) == 1, bad
    assert "delta|zigzag" in cli.USAGE and "delta|zigzag|lag" in cli.USAGE and "--lag" in cli.USAGE
    assert "--filter lag --lag S" in cli.__doc__ and "version 13" in cli.__doc__


# ---- range reads ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_reader_reports_the_filter_the_lag_and_a_granule_of_a_frame(rx, E):
    from redux_amd import container
    nb, Bk = 19, 4096
    streams = np.arange(3 * nb, dtype=np.uint8)
    offs = np.arange(0, 3 * nb + 1, 3).astype(np.uint64)
    total = nb * Bk - 7
    for crc in (None, np.arange(nb, dtype=np.uint32)):
        for S in (1, 5, 256):
            buf = container.pack(streams, offs, PARAMS, Bk, total, element_size=E, block_crc=crc, filter="lag", lag=S)
            r = container.Reader(buf)
            assert r.filter == "lag" and r.lag == S and r.granule_blocks == E and r.version == (13 if crc is None else 0x1D)
            assert r.total == total and r.block_size == Bk and r.nblocks == nb and r.base_op is None
            assert r.payload_offset == len(buf) - len(streams) and r.bytes_read == r.payload_offset
            assert r.read(5, 0) == b"" and r.bytes_read == r.payload_offset      # no bytes asked for: no coder call
        z = container.Reader(container.pack(streams, offs, PARAMS, Bk, total, element_size=E, block_crc=crc, filter="zigzag"))
        assert z.filter == "zigzag" and z.lag is None and z.granule_blocks == E and z.payload_offset == r.payload_offset
    assert container.Reader(container.pack(streams, offs, PARAMS, Bk, total, element_size=E)).lag is None


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_lag_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        for S in (0, 1, 2, 3, 255, 256, 257, 1 << 16, 0xFFFFFFFF):
            want = _lib.OK if E in (1, 2, 4, 8) and 1 <= S <= 256 else _lib.INVALID_INPUT
            assert L.redux_lag_check(E, S) == want, (E, S)
    assert L.redux_lag_check(0xFFFFFFFF, 1) == _lib.INVALID_INPUT
    for params in (PARAMS, (8, 14, 16), (4, 10, 16)):
        p = _lib.Params(*params)
        for n, Bk in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            for E in (1, 2, 4, 8, 0, 3, 16):
                assert L.redux_encode_lag_workspace_bytes(C.byref(p), n, Bk, E) == \
                    L.redux_encode_zigzag_workspace_bytes(C.byref(p), n, Bk, E), (params, n, Bk, E)
                assert L.redux_decode_lag_workspace_bytes(C.byref(p), n, Bk, E) == \
                    L.redux_decode_zigzag_workspace_bytes(C.byref(p), n, Bk, E), (params, n, Bk, E)
            assert L.redux_encode_lag_workspace_bytes(C.byref(p), n, Bk, 2) > 0
    # argument checks of the device calls come before any device work
    ok = _lib.Params(*PARAMS)
    assert L.redux_lag_planes_dev(None, None, 16, 4, 3, 1, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(None, None, 16, 0, 2, 1, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(None, None, 16, 4, 2, 1, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(None, None, 0, 4, 2, 1, 0, None) == _lib.OK
    assert L.redux_lag_planes_dev(None, None, 0, 4, 2, 0, 0, None) == _lib.INVALID_INPUT     # the lag, for an empty input too
    assert L.redux_lag_planes_dev(None, None, 0, 4, 2, 257, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_planes_dev(C.c_void_p(4096), C.c_void_p(4096 + 8), 16, 4, 2, 1, 0, None) == _lib.INVALID_INPUT  # overlap
    assert L.redux_encode_blocks_lag(C.byref(ok), None, 4, 4, 3, 1, None, 0, None, None, None) == _lib.INVALID_INPUT
    assert L.redux_decode_blocks_lag(C.byref(ok), None, None, 4, 4, 3, 1, None, None, None, None) == _lib.INVALID_INPUT
    x = np.zeros(8, np.uint8)
    out, offs = np.zeros(64, np.uint8), np.zeros(3, np.uint64)
    for S in (0, 257):
        assert L.redux_encode_blocks_lag(C.byref(ok), x.ctypes.data, 8, 4, 2, S, out.ctypes.data, 64, offs.ctypes.data, None,
                                         None) == _lib.INVALID_INPUT
        assert L.redux_encode_lag_dev(C.byref(ok), C.c_void_p(4096), 8, 4, 2, S, C.c_void_p(8192), 64, None, None, None,
                                      C.c_void_p(16384), 1 << 20, None) == _lib.INVALID_INPUT
        assert L.redux_decode_lag_dev(C.byref(ok), C.c_void_p(4096), C.c_void_p(4096), 8, 4, 2, S, C.c_void_p(8192), C.c_void_p(8192),
                                      C.c_void_p(8192), None, C.c_void_p(16384), 1 << 20, None) == _lib.INVALID_INPUT


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_lag_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "lag_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "lag_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_mirror_refuses_bad_arguments_before_any_device_call(tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_lag_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "lag mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
