"""Higher-order lagged differences (include/redux_hip.h, "higher-order lagged differences"): the numpy restatement of the rule
against hand-written expectations and against the lagged delta filter's restatement at order 1, the value claim on the CPU
oracle, container version 14, the Python argument checks, the CLI flag, the host-only ABI helper and the C++ mirror's
refusals.  No GPU call.

The value claim rests on GENERATED data -- sums of three sinusoids with white noise, and interleaved random walks: no recorded
PCM or sensor log is among the fixtures."""
import ctypes as C

import numpy as np
import pytest

from test_lag_cpu import channels, lag_planes_ref, lag_ref
from test_planes_cpu import lengths, oracle_bytes, planes_ref

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def lag_order_ref(x, E, B, S, K, inverse=False):
    """The rule: frames of E*B bytes; in a frame of N whole elements the lag-S difference (d[i] = x[i] for i < S and
    x[i] - x[i-S] mod 2^(8E) for i >= S) is applied K times, then z = (d << 1) ^ (0 - (d >> (8E-1))) for every element; the
    trailing bytes of a frame unchanged.  inverse=True unfolds with d = (z >> 1) ^ (0 - (z & 1)) and takes the S running sums
    of the frame K times.  (The byte-plane layout is planes_ref's, behind this.)"""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    assert 1 <= S <= 256 and 1 <= K <= 3
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
            for _ in range(K):
                for c in range(min(S, N)):  # chain c: elements c, c + S, ...
                    r[c::S] = np.cumsum(r[c::S], dtype=dt)
        else:
            d = v.copy()
            for _ in range(K):
                if N > S:
                    d[S:] = d[S:] - d[:-S]
            r = (d << one) ^ (zero - (d >> top))
        out[f0: f0 + N * E] = r.view(np.uint8)
    return out


def lag_order_planes_ref(x, E, B, S, K, inverse=False):
    """what redux_lag_order_planes_dev computes: the filter, then the layout; the inverse the other way round"""
    if inverse:
        return lag_order_ref(planes_ref(x, E, B, inverse=True), E, B, S, K, inverse=True)
    return planes_ref(lag_order_ref(x, E, B, S, K), E, B)


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_rule_matches_hand_written_expectations(E):
    dt = np.dtype("<u%d" % E)
    mod = 1 << 8 * E
    top = mod - 1
    v = np.array([10, 100, 12, 97, 11, 100, 0, top], dtype=dt)  # (top reads as -1)
    x = np.concatenate([v.view(np.uint8), np.array([0xEE] * (E > 1), dtype=np.uint8)])  # + a trailing odd byte

    def fold(d):  # of the difference as the element holds it: mod 2^(8E), read as two's complement
        d = (d + mod // 2) % mod - mod // 2
        return 2 * d if d >= 0 else -2 * d - 1

    def check(Bk, S, K, want):
        z = lag_order_ref(x, E, Bk, S, K)
        assert z[: 8 * E].view(dt).tolist() == [fold(d) for d in want], (Bk, S, K)
        assert z[8 * E:].tolist() == x[8 * E:].tolist()
        assert lag_order_ref(z, E, Bk, S, K, inverse=True).tolist() == x.tolist()
    # one frame, S = 2.  Order 1: 10, 100, +2, -3, -1, +3, -11, -101.  Order 2, x[i] - 2 x[i-2] + x[i-4] with zeros before the
    # frame: 12 - 20, 97 - 200, 11 - 24 + 10, 100 - 194 + 100, 0 - 22 + 12, -1 - 200 + 97
    check(16, 2, 2, [10, 100, -8, -103, -3, 6, -10, -104])
    # order 3, x[i] - 3 x[i-2] + 3 x[i-4] - x[i-6]: 12 - 30, 97 - 300, 11 - 36 + 30, 100 - 291 + 300, 0 - 33 + 36 - 10,
    # -1 - 300 + 291 - 100
    check(16, 2, 3, [10, 100, -18, -203, 5, 109, -7, -110])
    # a second frame starts afresh: B = 4, S = 2: elements 4 and 5 stand as they are, 6 and 7 see only their own frame
    check(4, 2, 2, [10, 100, -8, -103, 11, 100, 0 - 22, -1 - 200])
    check(4, 2, 3, [10, 100, -18, -203, 11, 100, 0 - 33, -1 - 300])
    # 2S <= N < 3S at order 3 (S = 3, N = 8): the term 3S back never exists, the one 2S back for elements 6 and 7 only
    check(16, 3, 3, [10, 100, 12, 97 - 30, 11 - 300, 100 - 36, 0 - 291 + 30, -1 - 33 + 300])
    check(16, 3, 2, [10, 100, 12, 97 - 20, 11 - 200, 100 - 24, 0 - 194 + 10, -1 - 22 + 100])
    # S >= N folds every element and subtracts nothing, at any order
    for S in (8, 9, 256):
        for K in (1, 2, 3):
            check(16, S, K, [10, 100, 12, 97, 11, 100, 0, -1])


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_order_one_is_the_lag_filter(E):
    rng = np.random.default_rng(E)
    for Bk in (4, 100, 4096):
        for L in lengths(E, Bk):
            x = rng.integers(0, 256, L, dtype=np.uint8)
            for S in (1, 3, 256):
                assert np.array_equal(lag_order_ref(x, E, Bk, S, 1), lag_ref(x, E, Bk, S)), (E, Bk, L, S)
                assert np.array_equal(lag_order_ref(x, E, Bk, S, 1, inverse=True), lag_ref(x, E, Bk, S, inverse=True)), (E, Bk, L, S)
                assert np.array_equal(lag_order_planes_ref(x, E, Bk, S, 1), lag_planes_ref(x, E, Bk, S)), (E, Bk, L, S)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_the_rule_is_the_binomial_sum(E):
    """the K-fold application against the closed form d[i] = sum (-1)^j C(K, j) x[i - jS] with zeros before the frame"""
    rng = np.random.default_rng(50 + E)
    dt = np.dtype("<u%d" % E)
    N = 40
    v = rng.integers(0, 256, N * E, dtype=np.uint8)
    xs = [int(a) for a in v.view(dt)]
    for S in (1, 3, 13, 14, 20, 40):
        for K, coef in ((2, (1, -2, 1)), (3, (1, -3, 3, -1))):
            d = [sum(c * (xs[i - j * S] if i >= j * S else 0) for j, c in enumerate(coef)) % (1 << 8 * E) for i in range(N)]
            want = lag_ref(np.array(d, dtype=dt).view(np.uint8), E, N, 256)  # (S >= N: the fold alone)
            assert np.array_equal(lag_order_ref(v, E, N, S, K), want), (S, K)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
@pytest.mark.parametrize("Bk", [4, 100, 4096])
def test_inverse_of_forward_is_identity(E, Bk):
    rng = np.random.default_rng(E * 10000 + Bk)
    for K in (2, 3):
        for S in (1, 2, 3, 7, 16, 255, 256):
            for L in lengths(E, Bk):
                x = rng.integers(0, 256, L, dtype=np.uint8)
                y = lag_order_planes_ref(x, E, Bk, S, K)
                assert len(y) == L
                assert np.array_equal(lag_order_planes_ref(y, E, Bk, S, K, inverse=True), x), (E, Bk, S, K, L)
                assert np.array_equal(lag_order_ref(lag_order_ref(x, E, Bk, S, K, inverse=True), E, Bk, S, K), x), (E, Bk, S, K, L)


# ---- the value claim, on the CPU oracle --------------------------------------------------------------------------------
CASES = [(1, 2), (2, 2), (3, 4), (2, 8)]  # (channels, element size); the lag is the number of channels


def tones(C_, E, seed):
    """C_ interleaved channels, each three sinusoids and white noise of standard deviation 4"""
    rng = np.random.default_rng(seed)
    n = 3 * B + 100
    t = np.arange(n)
    cols = []
    for c in range(C_):
        ph = rng.uniform(0, 6.28, 3)
        s = sum(a * np.sin(2 * np.pi * f * t + p) for a, f, p in zip((6000, 2500, 900), (0.003 * (c + 1), 0.011, 0.031), ph))
        cols.append(np.round(s + rng.normal(0, 4, n)))
    return np.stack(cols, 1).reshape(-1).astype(np.int64).astype("<i%d" % E).view(np.uint8)


def order_bytes(x, E, S):
    """the oracle's total behind orders 1, 2 and 3 at lag S"""
    return [oracle_bytes(lag_order_planes_ref(x, E, B, S, K), B) for K in (1, 2, 3)]


@pytest.mark.parametrize("C_,E", CASES)
def test_higher_orders_pay_on_tones(C_, E):
    k1, k2, k3 = order_bytes(tones(C_, E, 7), E, C_)
    print("tones, %d channels, E = %d: order 1 %d, order 2 %d (%.3f), order 3 %d (%.3f)" % (C_, E, k1, k2, k2 / k1, k3, k3 / k1))
    assert k2 <= 0.80 * k1, (k1, k2)
    assert k3 <= 0.75 * k1 and k3 < k2, (k1, k2, k3)


@pytest.mark.parametrize("C_,E", CASES)
def test_a_higher_order_costs_bytes_on_walks(C_, E):
    """why the order is opt-in: for a random walk the first difference is white, and differencing it again adds noise"""
    k1, k2, k3 = order_bytes(channels(C_, E, 7), E, C_)
    print("walks, %d channels, E = %d: order 1 %d, order 2 %d (%.3f), order 3 %d (%.3f)" % (C_, E, k1, k2, k2 / k1, k3, k3 / k1))
    assert k2 >= 1.03 * k1, (k1, k2)


# ---- container version 14 -----------------------------------------------------------------------------------------------
def test_container_v14_roundtrip_and_order_one_is_v13(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    crc = np.array([1, 2, 3], dtype=np.uint32)
    assert container.VERSION_LAG_ORDER == 14 and container.LAG_ORDER_MAX == 3
    for E in (1, 2, 4, 8):
        for S in (1, 3, 256):
            v13 = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="lag", lag=S)
            v1d = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, block_crc=crc, filter="lag", lag=S)
            # order 1 and no order: version 13, byte for byte
            assert container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="lag", lag=S, order=1) == v13
            assert container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="lag", lag=S, order=None) == v13
            assert v13[4] == 13 and container.order(v13) == 1 and container.order(v1d) == 1 and container._parse(v13).order is None
            for K in (2, 3):
                v14 = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, filter="lag", lag=S, order=K)
                assert v14[4] == 14 and int.from_bytes(v14[12:16], "little") == 0xE0000000 | K << 16 | S << 4 | E
                assert v14[:4] + v14[5:12] + v14[16:] == v13[:4] + v13[5:12] + v13[16:]  # version 13's bytes but the version and the word
                c = container._parse(v14)
                assert c.params.triple() == PARAMS and c.block_size == 65536 and c.total == total and c.element_size == E
                assert c.filter == "lag" and c.lag == S and c.order == K and c.static is None and c.crcs is None and c.stored is None
                assert c.base is None and c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == streams.tobytes()
                assert container.filter(v14) == "lag" and container.lag(v14) == S and container.order(v14) == K
                assert container.element_size(v14) == E and container.header_is_wellformed(v14)
                v1e = container.pack(streams, offs, PARAMS, 65536, total, element_size=E, block_crc=crc, filter="lag", lag=S, order=K)
                assert v1e[4] == 0x1E and v1e[:4] + v1e[5:12] + v1e[16:] == v1d[:4] + v1d[5:12] + v1d[16:]
                assert container.order(v1e) == K and container.lag(v1e) == S and container.block_crcs(v1e).tolist() == [1, 2, 3]
                assert container._parse(v1e).payload.tobytes() == streams.tobytes()
                for cut in (len(v1e) - 1, len(v1e) - 11, 32 + 12 + 11, 32 + 11, 33, 31):  # payload, CRC table, size table, header
                    with pytest.raises(rx.Eof):
                        container._parse(v1e[:cut])
                assert len(v14) - len(streams) == container.overhead_bytes("adaptive", 3, E, filter="lag")
                r = container.Reader(v1e)
                assert r.filter == "lag" and r.lag == S and r.order == K and r.granule_blocks == E and r.version == 0x1E
                assert r.read(5, 0) == b""
            assert container.Reader(v13).order is None and container.Reader(v13).lag == S
    for kw in ({}, {"element_size": 4}, {"element_size": 4, "filter": "delta"}, {"element_size": 4, "filter": "zigzag"}):
        assert container.order(container.pack(streams, offs, PARAMS, 65536, total, **kw)) is None


def test_container_v14_takes_its_word_alone_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, PARAMS, 65536, 10, element_size=2, filter="lag", lag=3, order=2)
    assert good[4] == 14 and int.from_bytes(good[12:16], "little") == 0xE0020032

    def word(K, S, E=2, mark=0xE0000000):
        return mark | K << 16 | S << 4 | E
    # K = 0, 1, 4; S = 0, 257; a wrong marker; E = 3; bits between the fields and above the order; the other versions' words
    for w in (word(0, 3), word(1, 3), word(4, 3), word(2, 0), word(2, 257), word(2, 3, mark=0xD0000000), word(2, 3, mark=0xB0000000),
              word(2, 3, mark=0), word(2, 3, E=3), word(2, 3, E=0), word(2, 3) | 1 << 13, word(2, 3) | 1 << 15, word(2, 3) | 1 << 18,
              word(2, 3) | 1 << 27, 0xD0000032, 0xB0000002, 0, 2, 0xEFFFFFF2):
        for ver in (14, 0x1E):
            bad = bytearray(good)
            bad[4] = ver
            bad[12:16] = w.to_bytes(4, "little")
            assert not container.header_is_wellformed(bytes(bad)), hex(w)
            for call in (container._parse, container.order, container.lag):
                with pytest.raises(rx.InvalidInput):
                    call(bytes(bad))
    for E in (1, 2, 4, 8):
        for S, K in ((1, 2), (256, 3)):
            for ver in range(256):  # no other version byte takes version 14's word, and it has no stored blocks (0x4E / 0x5E)
                if ver in (14, 0x1E):
                    continue
                bad = bytearray(container.pack(streams, offs, PARAMS, 65536, 10, element_size=E, filter="lag", lag=S, order=K))
                bad[4] = ver
                assert not container.header_is_wellformed(bytes(bad)), (E, S, K, hex(ver))
                with pytest.raises(rx.InvalidInput):
                    container._parse(bytes(bad))
    flags = np.zeros(1, np.uint8)
    static = rx.StaticModel(PARAMS, np.arange(258))
    for kw in ({"element_size": 3}, {"stored": flags}, {"base": (0, 0)}, {"constant": flags},
               {"unit_layouts": np.zeros(1, np.uint8)}, {"params": static}):
        kw = dict(kw)
        params = kw.pop("params", PARAMS)
        with pytest.raises(rx.InvalidInput):  # whatever is refused for the lag filter is refused at a higher order
            container.pack(streams, offs, params, 65536, 10, filter="lag", lag=3, order=2, **kw)
    for kw in ({"order": 2}, {"filter": "lag", "order": 2}, {"filter": "zigzag", "order": 2}, {"filter": "delta", "order": 1},
               {"filter": "lag", "lag": 3, "order": 0}, {"filter": "lag", "lag": 3, "order": 4}, {"filter": "lag", "lag": 3, "order": 2.0},
               {"filter": "lag", "lag": 3, "order": True}, {"filter": "lag", "lag": 3, "order": "2"}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, PARAMS, 65536, 10, element_size=2, **kw)


# ---- Python argument checks ----------------------------------------------------------------------------------------------
def test_python_api_checks_the_order_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api, container
    offs = np.array([0, 1], np.uint64)
    flags = np.zeros(1, np.uint8)
    static = rx.StaticModel(PARAMS, np.arange(258))

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)

    def five(**kw):
        """the five calls that take the order, with these options"""
        return [lambda: rx.compress_blocks(b"abcd", 4, **kw),
                lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, **kw),
                lambda: rx.DeviceDecoder(PARAMS, 4096, 1, **kw),
                lambda: container.compress_bytes(b"abcd" * 4, 16, **kw)]
    lag3 = {"filter": "lag", "lag": 3}
    bad = [{"order": 2}, {"order": 1},                                               # an order without the filter
           {"filter": "lag", "order": 2},                                            # or without a lag
           {"filter": "zigzag", "order": 2}, {"filter": "delta", "order": 1},        # or with another filter
           {**lag3, "order": 0}, {**lag3, "order": 4}, {**lag3, "order": -1}, {**lag3, "order": 2.0}, {**lag3, "order": "2"},
           {**lag3, "order": True}, {**lag3, "order": (2,)}, {**lag3, "order": np.float64(2)}]
    for kw in bad:
        for call in five(**kw):
            with pytest.raises(rx.InvalidInput):
                call()
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(None, **kw)
    for K in (2, 3):  # the lag estimates count order 1 only
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(b"abcd" * 4, 16, filter="lag", lag="auto", order=K)
    for args in ((0, 2), (257, 2), (3, 0), (3, 4), (3, True), (3, 2.0), (3, None)):
        with pytest.raises(rx.InvalidInput):
            api.lag_order_planes(None, 2, 4096, *args)
    # everything refused for the lag filter is refused at a higher order
    f = {**lag3, "order": 2}
    c = [lambda: rx.compress_blocks(b"abcd", 4, static, **f), lambda: rx.decompress_blocks(b"\0", offs, 4, static, length=4, **f),
         lambda: rx.compress_blocks(b"abcd", 4, stored=flags, **f), lambda: rx.decompress_blocks(b"\0", offs, 4, **f),
         lambda: rx.compress_blocks(b"abcd", 4, base=b"abcd", **f), lambda: rx.compress_blocks(b"abcd", 4, constant=True, **f),
         lambda: rx.compress_blocks(b"abcd", 4, unit_layouts=True, **f),
         lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, base=flags, **f), lambda: rx.DeviceDecoder(PARAMS, 4096, 1, constant=True, **f),
         lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, mixed=True, **f)]
    for kw in ({"model": "static"}, {"model": "auto"}, {"stored": True}, {"base": b"abcd"}, {"skip_constant": True},
               {"layout": "auto"}, {"layout": "mixed"}):
        c.append(lambda kw=kw: container.compress_bytes(b"abcd" * 4, 16, **f, **kw))
    for call in c:
        with pytest.raises(rx.InvalidInput):
            call()
    # what the resolver makes of an order
    lag = api._resolve_front(None, **lag3).front
    assert api._resolve_front(None, **lag3, order=None).front == lag and api._resolve_front(None, **lag3, order=1).front == lag
    assert lag.infix == "lag" and lag.order is None and api._lag_arg(lag) == (3,)
    for K in (2, 3, np.int64(3)):
        r = api._resolve_front(None, **lag3, order=K).front
        assert r.infix == "lag_order" and r.lag == 3 and r.order == int(K) and r.needs_length and not r.takes_base
        assert api._lag_arg(r) == (3, int(K))
    assert api._resolve_front(None, filter="zigzag").front.order is None and api._lag_arg(api._resolve_front(None).front) == ()
    assert set(api._FILTERS) == {"delta", "zigzag", "lag"} and api.LAG_ORDER_MAX == 3
    for name in ("check", "planes_dev"):
        assert "redux_lag_order_%s" % name in _lib.SIGNATURES
    for d in ("encode", "decode"):
        for name in ("redux_%s_lag_order_workspace_bytes", "redux_%s_lag_order_dev", "redux_%s_blocks_lag_order"):
            assert name % d in _lib.SIGNATURES
            lag_sig, sig = _lib.SIGNATURES[(name % d).replace("lag_order", "lag")], _lib.SIGNATURES[name % d]
            assert sig[0] == lag_sig[0] and len(sig[1]) == len(lag_sig[1]) + ("workspace" not in name)


def test_order_stands_directly_before_base_op():
    import inspect
    import redux_amd as rx
    from redux_amd import api, container
    for f in (rx.compress_blocks, rx.decompress_blocks, rx.DeviceEncoder.__init__, rx.DeviceDecoder.__init__, container.compress_bytes,
              container.pack):
        names = list(inspect.signature(f).parameters)
        assert names[-3:] == ["lag", "order", "base_op"], (f, names)
    assert list(inspect.signature(api._resolve_front).parameters)[-1] == "order"
    assert list(inspect.signature(api.lag_order_planes).parameters) == ["d_src", "element_size", "block_size", "lag", "order", "inverse", "out"]


# ---- CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_order_flag(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    some = ["-c", "--block-size", "65536", "--filter", "lag", "--lag", "3"]
    for K in ("1", "2", "3"):
        assert cli.parse(some + ["--order", K]) == {**base, "filter": "lag", "lag": 3, "order": int(K)}
        assert cli.parse(["-c", "--order", K, "--lag", "256", "--filter", "lag", "--block-size", "65536"]) == \
            {**base, "filter": "lag", "lag": 256, "order": int(K)}
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "lag", "--lag", "1", "--order", "2"]) == \
            {**base, "block_size": 4096, "element_size": int(E), "filter": "lag", "lag": 1, "order": 2}
    assert cli.parse(some + ["--order", "3", "--checksum"]) == {**base, "filter": "lag", "lag": 3, "order": 3, "checksum": True}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "lag", "--lag", "auto", "--order", "1"]) == \
        {**base, "filter": "lag", "lag": "auto", "order": 1}
    # calls that do not use it get the dicts they got
    assert cli.parse(some) == {**base, "filter": "lag", "lag": 3}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "lag", "--lag", "auto"]) == {**base, "filter": "lag", "lag": "auto"}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "zigzag"]) == {**base, "filter": "zigzag"}
    assert cli.parse(["-d", "--range", "3:4"]) == {"compress": False, "input": None, "output": None, "block_size": 0, "range": (3, 4)}
    head = ["-c", "--block-size", "65536"]
    auto = head + ["--filter", "lag", "--lag", "auto"]
    for bad in (head + ["--order", "2"], head + ["--order", "1"], head + ["--filter", "zigzag", "--order", "2"],
                head + ["--filter", "delta", "--order", "1"], head + ["--filter", "lag", "--order", "2"],
                some + ["--order", "0"], some + ["--order", "4"], some + ["--order", "-1"], some + ["--order", "2.0"],
                some + ["--order", "02"], some + ["--order", " 2"], some + ["--order", "x"], some + ["--order", ""], some + ["--order"],
                some + ["--order", "auto"], auto + ["--order", "2"], auto + ["--order", "3"],
                ["-c", "--filter", "lag", "--lag", "3", "--order", "2"], some + ["--order", "2", "--stored"],
                some + ["--order", "2", "--base", "f"], some + ["--order", "2", "--skip-constant"], some + ["--order", "2", "--layout", "auto"],
                some + ["--order", "2", "--model", "static"], some + ["--order", "2", "--model", "auto"],
                ["-d", "--order", "2"]):
        assert cli.parse(bad) is None, bad
    for bad in (head + ["--order", "2"], some + ["--order", "4"], auto + ["--order", "2"]):
        assert cli.main(bad) == 1, bad
    assert "delta|zigzag|lag" in cli.USAGE and "--lag" in cli.USAGE and "--order <1|2|3>" in cli.USAGE
    assert "--order K" in cli.__doc__ and "version 14" in cli.__doc__ and "generated" in cli.__doc__


# ---- host-only ABI helpers -----------------------------------------------------------------------------------------------
def test_lag_order_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 12):
        for S in (0, 1, 2, 255, 256, 257, 0xFFFFFFFF):
            for K in (0, 1, 2, 3, 4, 255, 1 << 16, 0xFFFFFFFF):
                want = _lib.OK if E in (1, 2, 4, 8) and 1 <= S <= 256 and 1 <= K <= 3 else _lib.INVALID_INPUT
                assert L.redux_lag_order_check(E, S, K) == want, (E, S, K)
    for params in (PARAMS, (8, 14, 16)):
        p = _lib.Params(*params)
        for n, Bk in ((0, 65536), (3 * 65536 + 7, 65536), (1000, 4)):
            for E in (1, 2, 4, 8, 0, 3):
                assert L.redux_encode_lag_order_workspace_bytes(C.byref(p), n, Bk, E) == \
                    L.redux_encode_zigzag_workspace_bytes(C.byref(p), n, Bk, E), (params, n, Bk, E)
                assert L.redux_decode_lag_order_workspace_bytes(C.byref(p), n, Bk, E) == \
                    L.redux_decode_zigzag_workspace_bytes(C.byref(p), n, Bk, E), (params, n, Bk, E)
    # argument checks of the device calls come before any device work
    ok = _lib.Params(*PARAMS)
    assert L.redux_lag_order_planes_dev(None, None, 16, 4, 3, 1, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(None, None, 16, 0, 2, 1, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(None, None, 16, 4, 2, 1, 2, 0, None) == _lib.INVALID_INPUT
    for K in (1, 2, 3):
        assert L.redux_lag_order_planes_dev(None, None, 0, 4, 2, 1, K, 0, None) == _lib.OK
    for S, K in ((0, 2), (257, 2), (1, 0), (1, 4)):  # the lag and the order, for an empty input too
        assert L.redux_lag_order_planes_dev(None, None, 0, 4, 2, S, K, 0, None) == _lib.INVALID_INPUT
    assert L.redux_lag_order_planes_dev(C.c_void_p(4096), C.c_void_p(4096 + 8), 16, 4, 2, 1, 2, 0, None) == _lib.INVALID_INPUT  # overlap
    x = np.zeros(8, np.uint8)
    out, offs = np.full(64, 0xAB, np.uint8), np.full(3, 0xAB, np.uint64)
    sizes = np.full(2, 0xAB, np.uint32)
    for S, K in ((3, 0), (3, 4), (0, 2), (257, 2)):
        assert L.redux_encode_blocks_lag_order(C.byref(ok), x.ctypes.data, 8, 4, 2, S, K, out.ctypes.data, 64, offs.ctypes.data, None,
                                               None) == _lib.INVALID_INPUT
        assert L.redux_decode_blocks_lag_order(C.byref(ok), x.ctypes.data, offs.ctypes.data, 8, 4, 2, S, K, out.ctypes.data,
                                               sizes.ctypes.data, None, None) == _lib.INVALID_INPUT
        assert L.redux_encode_lag_order_dev(C.byref(ok), C.c_void_p(4096), 8, 4, 2, S, K, C.c_void_p(8192), 64, None, None, None,
                                            C.c_void_p(16384), 1 << 20, None) == _lib.INVALID_INPUT
        assert L.redux_decode_lag_order_dev(C.byref(ok), C.c_void_p(4096), C.c_void_p(4096), 8, 4, 2, S, K, C.c_void_p(8192),
                                            C.c_void_p(8192), C.c_void_p(8192), None, C.c_void_p(16384), 1 << 20, None) == _lib.INVALID_INPUT
    assert (out == 0xAB).all() and (offs == 0xAB).all() and (sizes == 0xAB).all()  # nothing was written


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------
def build_lag_order_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "lag_order_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "lag_order_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_mirror_refuses_bad_arguments_before_any_device_call(tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_lag_order_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "lag order mirror host-side checks ok" in out.stdout, out.stdout + out.stderr
