"""Record layout for fixed-width structs (include/redux_hip.h, "record layout"): the numpy restatement of the rule against
hand-written expectations and against the byte-plane layout's restatement, the value claim on the CPU oracle, the Python
argument checks, container version 15, the CLI flags, the range reader, the host-only ABI helpers, the chunk rounding of the host
pipeline and the C++ mirror's refusals.  No GPU call.

The value claim rests on GENERATED data, two tables of packed structs (imu23, ticks20): nothing in the corpus fixtures
consists of fixed-width records."""
from collections import namedtuple

import numpy as np
import pytest

from test_lag_cpu import lag_planes_ref
from test_planes_cpu import lengths, oracle_bytes, planes_ref

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def record_ref(x, R, B, delta=False, inverse=False):
    """The rule: frames of R*B bytes (the last may be shorter); in a frame of L bytes with N = L // R records, with the
    delta d[i][p] = x[i][p] - x[i-1][p] mod 256 for i >= 1 and d[0][p] = x[0][p], else d = x; byte p of record i moves to
    frame offset p*N + i; the L - N*R trailing bytes stay where they are.  inverse=True undoes the layout, then takes the R
    running sums mod 256 of the frame."""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    assert 2 <= R <= 256
    out = x.copy()
    for f0 in range(0, len(x), R * B):
        N = len(x[f0: f0 + R * B]) // R
        if N == 0:
            continue
        fr = x[f0: f0 + N * R]
        if inverse:
            d = fr.reshape(R, N).T
            r = np.cumsum(d, axis=0, dtype=np.uint8) if delta else d
        else:
            v = fr.reshape(N, R)
            d = v.copy()
            if delta:
                d[1:] = v[1:] - v[:-1]
            r = d.T
        out[f0: f0 + N * R] = np.ascontiguousarray(r).reshape(-1)
    return out


def test_rule_matches_hand_written_expectations():
    """R = 3, B = 4: a full frame of 12 bytes, then a short one of 2 records and 2 trailing bytes"""
    x = np.array([10, 20, 30, 11, 22, 33, 13, 26, 39, 16, 32, 48,      # records (10,20,30) (11,22,33) (13,26,39) (16,32,48)
                  200, 5, 7, 100, 10, 9, 77, 78], dtype=np.uint8)     # records (200,5,7) (100,10,9), trailing 77 78
    plain = [10, 11, 13, 16, 20, 22, 26, 32, 30, 33, 39, 48, 200, 100, 5, 10, 7, 9, 77, 78]
    delta = [10, 1, 2, 3, 20, 2, 4, 6, 30, 3, 6, 9, 200, 156, 5, 5, 7, 2, 77, 78]
    assert record_ref(x, 3, 4).tolist() == plain
    assert record_ref(x, 3, 4, delta=True).tolist() == delta
    assert record_ref(np.array(plain, np.uint8), 3, 4, inverse=True).tolist() == x.tolist()
    assert record_ref(np.array(delta, np.uint8), 3, 4, delta=True, inverse=True).tolist() == x.tolist()
    for L in (0, 1, 2):  # less than a record: trailing bytes only
        assert record_ref(x[:L], 3, 4, delta=True).tolist() == x[:L].tolist()


@pytest.mark.parametrize("R", [2, 3, 4, 7, 8, 23, 256])
def test_without_the_filter_it_is_the_byte_plane_rule(R):
    rng = np.random.default_rng(R)
    for Bs in (4, 100):
        for L in lengths(R, Bs):
            x = rng.integers(0, 256, L, dtype=np.uint8)
            assert np.array_equal(record_ref(x, R, Bs), planes_ref(x, R, Bs)), (R, Bs, L)
            assert np.array_equal(record_ref(x, R, Bs, inverse=True), planes_ref(x, R, Bs, inverse=True)), (R, Bs, L)


@pytest.mark.parametrize("R", [2, 3, 7, 16, 23, 255, 256])
@pytest.mark.parametrize("Bs", [4, 100, 4096])
def test_inverse_of_forward_is_identity(R, Bs):
    rng = np.random.default_rng(R * 10000 + Bs)
    for L in lengths(R, Bs):
        x = rng.integers(0, 256, L, dtype=np.uint8)
        for delta in (False, True):
            y = record_ref(x, R, Bs, delta)
            assert np.array_equal(record_ref(y, R, Bs, delta, inverse=True), x), (R, Bs, L, delta)
        if L >= R * Bs:  # a full frame is R blocks, block p = byte column p of B records
            y = record_ref(x, R, Bs)
            for p in (0, R - 1):
                assert np.array_equal(y[p * Bs: (p + 1) * Bs], x[: R * Bs].reshape(Bs, R)[:, p])


# ---- the value claim -------------------------------------------------------------------------------------------------
def generated_tables(n=40000):
    """imu23 and ticks20: n records each of two packed structs, GENERATED -> {name: (bytes as uint8, record size)}"""
    rng = np.random.default_rng(5)
    t = np.arange(n)
    imu = np.zeros(n, dtype=[("ts", "<i8"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("flags", "<u2"), ("st", "u1")])
    imu["ts"] = 1700000000000000 + np.cumsum(rng.integers(900, 1100, n))
    imu["x"] = np.sin(t / 300) + rng.normal(0, .01, n)
    imu["y"] = 9.8 + rng.normal(0, .02, n)
    imu["z"] = np.cumsum(rng.normal(0, .01, n))
    imu["flags"] = rng.choice([0, 1, 4, 0x8000], n, p=[.9, .05, .04, .01])
    imu["st"] = rng.integers(0, 3, n)
    tk = np.zeros(n, dtype=[("id", "<u4"), ("px", "<i4"), ("qty", "<u2"), ("side", "u1"), ("pad", "u1"), ("ts", "<u8")])
    tk["id"] = np.arange(n) + rng.integers(0, 3, n)
    tk["px"] = 100000 + np.cumsum(rng.integers(-5, 6, n))
    tk["qty"] = rng.geometric(.05, n)
    tk["side"] = rng.integers(0, 2, n)
    tk["pad"] = 0
    tk["ts"] = 1700000000000 + np.cumsum(rng.integers(0, 50, n))
    assert imu.dtype.itemsize == 23 and tk.dtype.itemsize == 20
    return {"imu23": (imu.view(np.uint8).reshape(-1).copy(), 23), "ticks20": (tk.view(np.uint8).reshape(-1).copy(), 20)}


@pytest.mark.parametrize("name", ["imu23", "ticks20"])
def test_record_layout_with_delta_pays_on_generated_tables(name):
    """The record layout with the byte delta codes to at most 0.85 of the smallest of plain, lag (E = 1, S = R) and, for
    ticks20, planes and lag at E = 2 and 4 with S = R / E.  Measured with the oracle at B = 4096: imu23 378,060 against
    514,150 (0.735), ticks20 136,086 against 181,079 (0.752).  GENERATED data."""
    x, R = generated_tables()[name]
    others = {"plain": oracle_bytes(x, B), "lag E=1": oracle_bytes(lag_planes_ref(x, 1, B, R), B)}
    if name == "ticks20":
        for E in (2, 4):
            others["planes E=%d" % E] = oracle_bytes(planes_ref(x, E, B), B)
            others["lag E=%d" % E] = oracle_bytes(lag_planes_ref(x, E, B, R // E), B)
    alone = oracle_bytes(record_ref(x, R, B), B)
    both = oracle_bytes(record_ref(x, R, B, delta=True), B)
    print(name, others, "record", alone, "record + delta", both, "ratio %.3f" % (both / min(others.values())))
    assert both <= 0.85 * min(others.values()), (others, alone, both)


# ---- the Python argument checks --------------------------------------------------------------------------------------
def test_resolve_front_refusals(rx):
    """before any library or torch call: the record layout goes with the adaptive model, element size 1 and filter None or
    "delta" only"""
    from redux_amd import api
    r = api._resolve_front(PARAMS, record_size=23)
    assert r.front.infix == "record" and r.front.record == (23, 0) and not r.constant and not r.mixed
    assert api._resolve_front(PARAMS, filter="delta", record_size=np.int64(256)).front.record == (256, 1)
    assert api._resolve_front(PARAMS, record_size=2, device=True).front.record == (2, 0)
    assert api.RECORD_MAX == rx.RECORD_MAX == 256
    flags = np.zeros(1, np.uint8)
    bad = [dict(record_size=R) for R in (0, 1, 257, 1 << 20, -3, 2.0, "23", True)]
    bad += [dict(record_size=23, element_size=E) for E in (2, 4, 8, 3, 0)]
    bad += [dict(record_size=23, filter=f) for f in ("zigzag", "lag", "xor", 1)]
    bad += [dict(record_size=23, filter="lag", lag=23), dict(record_size=23, lag=1), dict(record_size=23, filter="lag", lag=2, order=2),
            dict(record_size=23, order=1), dict(record_size=23, base=b"abc"), dict(record_size=23, base=b"abc", base_op="sub"),
            dict(record_size=23, constant=True), dict(record_size=23, constant=flags), dict(record_size=23, stored=flags),
            dict(record_size=23, unit_layouts=True), dict(record_size=23, unit_layouts=flags)]
    for kw in bad:
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(PARAMS, **kw)
    static = api.StaticModel(api.Parameters(*PARAMS), np.arange(258, dtype=np.uint32))
    for device in (False, True):
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(static, record_size=23, device=device)
    # the callers refuse the same before they touch the library
    for call in (lambda **kw: rx.compress_blocks(b"x" * 100, 16, **kw),
                 lambda **kw: rx.decompress_blocks(b"", [0], 16, length=0, **kw)):
        for kw in (dict(record_size=1), dict(record_size=23, element_size=2), dict(record_size=23, filter="zigzag")):
            with pytest.raises(rx.InvalidInput):
                call(**kw)


# ---- the host-only ABI helpers ---------------------------------------------------------------------------------------
def test_record_check_and_kernel_names(rx):
    from redux_amd import _lib, api
    L = _lib.lib()
    for R in (2, 3, 23, 255, 256):
        for delta in (0, 1):
            assert L.redux_record_check(R, delta) == _lib.OK
    for R, delta in ((0, 0), (1, 0), (257, 0), (1 << 20, 1), (23, 2), (23, -1)):
        assert L.redux_record_check(R, delta) == _lib.INVALID_INPUT
    fast, byte = ("k_record_planes", "k_record_unplanes"), ("k_record_planes_bytes", "k_record_unplanes_bytes")
    for inv in (0, 1):
        for R in (3, 16, 256):
            for Bs in (64, 4096, 4112):
                assert api.record_kernel_name(2 * R * Bs, Bs, R, inv) == fast[inv]
                assert api.record_kernel_name(2 * R * Bs + 5, Bs, R, inv) == fast[inv] + " + " + byte[inv]
                assert api.record_kernel_name(R * Bs - 1, Bs, R, inv) == byte[inv]
            for Bs in (100, 4099):
                assert api.record_kernel_name(3 * R * Bs, Bs, R, inv) == byte[inv]
        assert L.redux_record_kernel_name_at(1, 0, 2 * 3 * 64, 64, 3, inv).decode() == byte[inv]  # an unaligned source
        assert L.redux_record_kernel_name_at(0, 17, 2 * 3 * 64, 64, 3, inv).decode() == byte[inv]  # an unaligned destination
        assert L.redux_record_kernel_name_at(256, 512, 2 * 3 * 64, 64, 3, inv).decode() == fast[inv]
        for R, Bs in ((1, 64), (257, 64), (3, 0)):
            assert api.record_kernel_name(4096, Bs, R, inv) == ""
    P = api.Parameters(*PARAMS)._c()
    import ctypes as C
    for R in (2, 23, 256):  # the workspaces are the lag family's at element size 1
        assert L.redux_encode_record_workspace_bytes(C.byref(P), 1 << 20, 4096, R) == L.redux_encode_lag_workspace_bytes(C.byref(P), 1 << 20, 4096, 1)
        assert L.redux_decode_record_workspace_bytes(C.byref(P), 1 << 20, 4096, R) == L.redux_decode_lag_workspace_bytes(C.byref(P), 1 << 20, 4096, 1)
    for R in (0, 1, 257):
        assert L.redux_encode_record_workspace_bytes(C.byref(P), 1 << 20, 4096, R) == 0
        assert L.redux_decode_record_workspace_bytes(C.byref(P), 1 << 20, 4096, R) == 0


def test_record_calls_refuse_bad_arguments_before_the_device(rx):
    """null pointers, a zero block size, a bad record size and overlapping buffers are INVALID_INPUT on the host side"""
    import ctypes as C
    from redux_amd import _lib
    L = _lib.lib()
    buf = (C.c_uint8 * 4096)()
    a = C.addressof(buf)
    assert L.redux_record_planes_dev(None, a, 64, 16, 3, 0, 0, None) == _lib.INVALID_INPUT
    assert L.redux_record_planes_dev(a, None, 64, 16, 3, 0, 0, None) == _lib.INVALID_INPUT
    assert L.redux_record_planes_dev(a, a + 2048, 64, 0, 3, 0, 0, None) == _lib.INVALID_INPUT
    assert L.redux_record_planes_dev(a, a + 32, 64, 16, 3, 0, 0, None) == _lib.INVALID_INPUT  # overlap
    for R in (0, 1, 257, 1 << 20):
        assert L.redux_record_planes_dev(a, a + 2048, 64, 16, R, 0, 0, None) == _lib.INVALID_INPUT
    assert L.redux_record_planes_dev(a, a + 2048, 64, 16, 3, 2, 0, None) == _lib.INVALID_INPUT
    assert L.redux_record_planes_dev(None, None, 0, 16, 3, 1, 0, None) == _lib.OK  # nothing to do
    assert bytes(buf) == bytes(4096)


# ---- the chunk rounding of the host pipeline -------------------------------------------------------------------------
def test_chunks_are_whole_frames_and_existing_plans_are_unchanged(rx):
    from redux_amd import api
    shapes = [(1000, 4096), (100000, 4096), (1 << 20, 4096), (5000, 65536), (70, 1 << 20), (3, 100), (12345, 1000)]
    try:
        for lo, hi in ((0, 0), (1 << 16, 1 << 18)):
            api.host_set_chunk_bytes(lo, hi)
            for nb, Bs in shapes:
                for nctx in (1, 2, 3):
                    for decode in (False, True):
                        cb0, nc0 = api.host_chunk_plan(nb, Bs, nctx, decode)
                        assert cb0 == nb or cb0 % 64 == 0
                        for R in (23, 255, 2, 64):
                            cb, nc = api.host_chunk_plan(nb, Bs, nctx, decode, record_size=R)
                            assert cb == nb or cb % R == 0, (nb, Bs, R, cb)
                            assert cb0 <= cb < cb0 + R and nc == -(-nb // cb), (nb, Bs, R, cb0, cb)
                            if 64 % R == 0:  # frames that divide a wave: the plan every layout has had
                                assert (cb, nc) == (cb0, nc0)
    finally:
        api.host_set_chunk_bytes(0, 0)
    with pytest.raises(rx.InvalidInput):
        api.host_chunk_plan(100, 4096, record_size=1)



# ---- container version 15 --------------------------------------------------------------------------------------------
def word(R, F=0, kind=1):
    return 0xF0000000 | kind << 24 | F << 12 | R


def test_container_v15_roundtrip_with_oracle_streams(rx):
    from oracle import cbind as ox
    from redux_amd import container
    Bk, R = 256, 23
    x = generated_tables(100)["imu23"][0][: 2 * R * Bk + 30 * R + 7]
    nb = -(-len(x) // Bk)
    for delta in (False, True):
        streams, status = ox.compress_blocks(record_ref(x, R, Bk, delta), Bk, PARAMS)
        assert not status.any() and len(streams) == nb
        offs = np.zeros(nb + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s) for s in streams])
        dense = np.frombuffer(b"".join(streams), dtype=np.uint8)
        f = "delta" if delta else None
        crc = np.arange(nb, dtype=np.uint32)
        v15 = container.pack(dense, offs, PARAMS, Bk, len(x), filter=f, record_size=R)
        v1f = container.pack(dense, offs, PARAMS, Bk, len(x), filter=f, record_size=R, block_crc=crc)
        assert v15[4] == 15 and v1f[4] == 0x1F and int.from_bytes(v15[12:16], "little") == word(R, int(delta)) == int.from_bytes(v1f[12:16], "little")
        v1 = container.pack(dense, offs, PARAMS, Bk, len(x))
        assert v15[:4] + v15[5:12] + v15[16:] == v1[:4] + v1[5:12] + v1[16:]  # version 1's sections (version 2's: no element size)
        for buf, crcs in ((v15, None), (v1f, crc)):
            c = container._parse(buf)
            assert c.params.triple() == PARAMS and c.block_size == Bk and c.total == len(x) and c.element_size == 1
            assert c.record == (R, delta) and c.filter is None and c.lag is None and c.order is None and c.static is None
            assert c.stored is None and c.base is None and c.constant is None and c.unit_layouts is None
            assert c.offsets.tolist() == offs.tolist() and c.payload.tobytes() == dense.tobytes()
            assert (c.crcs is None) if crcs is None else c.crcs.tolist() == crcs.tolist()
            assert container.record(buf) == (R, delta) and container.filter(buf) is None and container.element_size(buf) == 1
            assert container.header_is_wellformed(buf)
            # the streams decode, on the CPU, to the transformed bytes, whose inverse is the input
            back = np.concatenate([np.frombuffer(ox.decompress(s, PARAMS)[0], dtype=np.uint8) for s in split_streams(c)])
            assert np.array_equal(record_ref(back, R, Bk, delta, inverse=True), x)
        for cut in (len(v1f) - 1, len(v1f) - len(dense) - 1, 32 + 4 * nb + 3, 32 + 3, 33, 31):  # payload, CRC table, size table, header
            with pytest.raises(rx.Eof):
                container._parse(v1f[:cut])
        assert len(v15) - len(dense) == container.overhead_bytes("adaptive", nb, filter=f, record_size=R) == \
            container.overhead_bytes("adaptive", nb)
        assert len(v1f) - len(dense) == container.overhead_bytes("adaptive", nb, checksum=True, filter=f, record_size=R)
    assert "one version number" not in container.__doc__.lower() and "kinds 2 .. 15" in container.__doc__


def split_streams(c):
    return [c.payload[int(c.offsets[b]): int(c.offsets[b + 1])].tobytes() for b in range(len(c.offsets) - 1)]


def test_container_without_a_record_size_writes_todays_bytes(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    total = 3 * 65536 - 5
    size_table = np.diff(offs.astype(np.int64)).astype("<u4").tobytes()
    for ver, w, kw in ((1, 0, {}), (2, 4, {"element_size": 4}), (6, 0x60000001, {"filter": "delta"}),
                       (13, 0xD0000171, {"filter": "lag", "lag": 23}), (14, 0xE0020171, {"filter": "lag", "lag": 23, "order": 2})):
        for extra in ({}, {"record_size": None}):
            buf = container.pack(streams, offs, PARAMS, 65536, total, **kw, **extra)
            assert buf == container.HEADER.pack(b"RDXB", ver, 8, 30, 32, 65536, w, 3, total) + size_table + streams.tobytes()
            assert container.record(buf) is None and container.Reader(buf).record is None


def test_container_v15_takes_its_word_alone_and_has_no_stored_blocks(rx):
    from redux_amd import container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    good = container.pack(streams, offs, PARAMS, 65536, 10, filter="delta", record_size=23)
    assert good[4] == 15 and int.from_bytes(good[12:16], "little") == 0xF1001017
    # every other kind, any other set bit, R outside 2 .. 256, and the other versions' words
    words = [word(23, kind=k) for k in (0, 2, 3, 15)] + [word(R) for R in (0, 1, 257, 300, 511)]
    words += [word(23) | 1 << b for b in (9, 10, 11, 13, 14, 15, 16, 20, 23)] + [word(23, 1) | 1 << 13]
    words += [0, 2, 0x60000001, 0xB0000001, 0xD0000171, 0xE0020171, 0xA0000000, 0x00000017, 0xFFFFFFFF, 0xF0000000, 0xF0000017]
    for w in words:
        for ver in (15, 0x1F):
            bad = bytearray(good)
            bad[4] = ver
            bad[12:16] = w.to_bytes(4, "little")
            assert not container.header_is_wellformed(bytes(bad)), hex(w)
            with pytest.raises(rx.InvalidInput):
                container._parse(bytes(bad))
            with pytest.raises(rx.InvalidInput):
                container.record(bytes(bad))
    for R in (2, 23, 256):
        for f in (None, "delta"):
            buf = container.pack(streams, offs, PARAMS, 65536, 10, filter=f, record_size=R)
            assert container.record(buf) == (R, f is not None)
            for ver in range(256):  # no other version byte takes version 15's word, and it has no stored blocks (0x4F / 0x5F)
                if ver in (15, 0x1F):
                    continue
                bad = bytearray(buf)
                bad[4] = ver
                assert not container.header_is_wellformed(bytes(bad)), (R, f, hex(ver))
                with pytest.raises(rx.InvalidInput):
                    container._parse(bytes(bad))
    flags = np.zeros(1, np.uint8)
    static = rx.StaticModel(PARAMS, np.arange(258))
    for kw in ({"element_size": 2}, {"stored": flags}, {"base": (0, 0)}, {"constant": flags}, {"unit_layouts": flags},
               {"params": static}, {"filter": "zigzag"}, {"filter": "lag", "lag": 23}, {"lag": 1}, {"order": 1}):
        kw = dict(kw)
        params = kw.pop("params", PARAMS)
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, params, 65536, 10, record_size=23, **kw)
    for R in (0, 1, 257, 2.0, "23", True):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, PARAMS, 65536, 10, record_size=R)
        with pytest.raises(rx.InvalidInput):
            container.overhead_bytes("adaptive", 3, record_size=R)
    for kw in ({"element_size": 2}, {"stored": True}, {"mixed": True}, {"base": True}, {"filter": "zigzag"}):
        with pytest.raises(rx.InvalidInput):
            container.overhead_bytes("adaptive", 3, record_size=23, **kw)
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("static", 3, record_size=23)


def test_python_callers_check_the_record_size_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api, container
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(api, "_torch", touched)

    def six(**kw):
        return [lambda: rx.compress_blocks(b"abcd", 4, **kw),
                lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, **kw),
                lambda: rx.DeviceDecoder(PARAMS, 4096, 1, **kw),
                lambda: container.compress_bytes(b"abcd" * 4, 16, **kw),
                lambda: api.record_planes(None, kw["record_size"], 16, delta=kw.get("filter") == "delta") if set(kw) <= {"record_size", "filter"}
                and kw.get("filter") in (None, "delta") else api._resolve_front(None, **kw)]
    bad = [{"record_size": R} for R in (0, 1, 257, 1 << 20, -1, 3.0, "3", True, (3,))]
    bad += [{"record_size": 23, "element_size": 2}, {"record_size": 23, "filter": "zigzag"}, {"record_size": 23, "filter": "lag", "lag": 23},
            {"record_size": 23, "lag": 23}, {"record_size": 23, "order": 1}, {"record_size": 23, "filter": "Delta"}]
    for kw in bad:
        for call in six(**kw):
            with pytest.raises(rx.InvalidInput):
                call()
    c = [lambda: rx.compress_blocks(b"abcd", 4, record_size=23, stored=flags),
         lambda: rx.compress_blocks(b"abcd", 4, record_size=23, base=b"abcd"),
         lambda: rx.compress_blocks(b"abcd", 4, record_size=23, constant=True),
         lambda: rx.compress_blocks(b"abcd", 4, record_size=23, unit_layouts=True),
         lambda: rx.decompress_blocks(b"\0", offs, 4, record_size=23),                 # the layout needs the length
         lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, record_size=23, base=flags),
         lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, record_size=23, constant=True),
         lambda: rx.DeviceDecoder(PARAMS, 4096, 1, record_size=23, mixed=True)]
    for kw in ({"model": "static"}, {"model": "segment-static"}, {"model": "context-static"}, {"model": "auto"}, {"stored": True},
               {"base": b"abcd"}, {"skip_constant": True}, {"layout": "auto"}, {"layout": "mixed"}, {"segment_blocks": 64},
               {"lag": "auto"}, {"order": "auto"}, {"element_size": 4}, {"base_op": "sub"}):
        c.append(lambda kw=kw: container.compress_bytes(b"abcd" * 4, 16, record_size=23, **kw))
    for call in c:
        with pytest.raises(rx.InvalidInput):
            call()


# ---- CLI -------------------------------------------------------------------------------------------------------------
def test_cli_record_flags(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    some = ["-c", "--block-size", "65536", "--record-size", "23"]
    assert cli.parse(some) == {**base, "record_size": 23}
    assert cli.parse(some + ["--filter", "delta"]) == {**base, "record_size": 23, "filter": "delta"}
    assert cli.parse(["-c", "--filter", "delta", "--record-size", "256", "--block-size", "4096", "--checksum", "--element-size", "1",
                      "--model", "adaptive"]) == {**base, "block_size": 4096, "record_size": 256, "filter": "delta", "checksum": True,
                                                  "element_size": 1, "model": "adaptive"}
    assert cli.parse(["-c", "--block-size", "65536", "--record-size", "2"]) == {**base, "record_size": 2}
    # calls that do not use it get the dicts they got
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "delta"]) == {**base, "filter": "delta"}
    assert cli.parse(["-c"]) == {**base, "block_size": 0}
    assert cli.parse(["-d", "--range", "3:4"]) == {"compress": False, "input": None, "output": None, "block_size": 0, "range": (3, 4)}
    head = ["-c", "--block-size", "65536"]
    for bad in (head + ["--record-size", v] for v in ("0", "1", "257", "-3", "3.0", "x", "")):
        assert cli.parse(bad) is None, bad
    for bad in (head + ["--record-size"], ["-c", "--record-size", "23"], ["-c", "--block-size", "0", "--record-size", "23"],
                ["-d", "--record-size", "23"], ["-d", "--block-size", "65536", "--record-size", "23"],
                some + ["--element-size", "2"], some + ["--element-size", "8"], some + ["--filter", "zigzag"],
                some + ["--filter", "lag", "--lag", "23"], some + ["--lag", "23"], some + ["--filter", "delta", "--order", "1"],
                some + ["--order-auto"], some + ["--stored"], some + ["--base", "f"], some + ["--skip-constant"],
                some + ["--layout", "auto"], some + ["--layout", "mixed"], some + ["--model", "static"],
                some + ["--model", "segment-static"], some + ["--model", "context-static"], some + ["--model", "auto"]):
        assert cli.parse(bad) is None, bad
    for bad in (head + ["--record-size", "1"], some + ["--stored"], some + ["--filter", "zigzag"], ["-d", "--record-size", "23"]):
        assert cli.main(bad) == 1, bad
    assert "--record-size <2..256>" in cli.USAGE and "--record-size R [--filter delta]" in cli.__doc__ and "version 15" in cli.__doc__


# ---- range reads -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 23, 256])
def test_reader_reports_the_record_and_a_granule_of_a_frame(rx, R):
    from redux_amd import api, container
    nb, Bk = 2 * R + 1, 4096  # two full frames and one block of a third
    streams = np.arange(3 * nb, dtype=np.uint32).astype(np.uint8)
    offs = np.arange(0, 3 * nb + 1, 3).astype(np.uint64)
    total = nb * Bk - 7
    for crc in (None, np.arange(nb, dtype=np.uint32)):
        for f in (None, "delta"):
            buf = container.pack(streams, offs, PARAMS, Bk, total, block_crc=crc, filter=f, record_size=R)
            r = container.Reader(buf)
            assert r.record == (R, f is not None) and r.granule_blocks == R and r.version == (15 if crc is None else 0x1F)
            assert r.filter is None and r.lag is None and r.order is None and r.base_op is None
            assert r.total == total and r.block_size == Bk and r.nblocks == nb
            assert r.payload_offset == len(buf) - len(streams) and r.bytes_read == r.payload_offset
            assert r.read(5, 0) == b"" and r.bytes_read == r.payload_offset      # no bytes asked for: no coder call
    F = R * Bk
    runs, virt_off, virt_len = api.range_plan(total, Bk, R, [(F + 100, 40), (2 * F - 7, 20)])  # redux_range_plan takes R as it is
    assert [tuple(r) for r in runs] == [(1, 2)] and virt_len == total - F and list(virt_off) == [100, F - 7]
    assert api.range_plan(total, Bk, R, [(5, 10)])[2] == F


# ---- C++ mirror ------------------------------------------------------------------------------------------------------
def build_record_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "record_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(root, "tests", "cpp", "record_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_mirror_refuses_bad_arguments_before_any_device_call(tmp_path):
    import subprocess
    from redux_amd import _lib
    _lib.lib()
    out = subprocess.run([build_record_mirror_test(tmp_path), "--no-gpu"], capture_output=True, text=True)
    assert out.returncode == 0 and "record mirror host-side checks ok" in out.stdout, out.stdout + out.stderr


# ---- the launch plan -------------------------------------------------------------------------------------------------
# redux_record_plan reports the shape launch_record launches with, from the function the launch takes it from.  The
# constants of redux_record.hpp, restated: the LDS tile's bytes, the inverse's work items (16 records of a column) a tile.
LDS_BYTES, ITEMS = 33792, 2048
LG_MAX = 12                       # record_lg_tile stops there: the largest tile is 4096 records (R up to 7)
PCS = (64, 80, 96, 112, 128)      # the widths of a column range, besides R itself


def tile_bytes(T, row):
    """the LDS tile of T records of `row` bytes: for an even row every group of 16 records is followed by 16 bytes"""
    return T * row + (T // 16) * (0 if row & 1 else 16)


def plan_of(nfull, R, B, inverse, cus, delta=False, tail=0):
    from redux_amd import api
    return api.record_plan(nfull * R * B + tail, B, R, delta, inverse, cus)


def max_tile(R, nfull, inverse, cus):
    """the tile the plan takes where the block size does not hold it down"""
    return 1 << plan_of(nfull, R, 1 << 16, inverse, cus).lgT


# The sweep of tests/test_record_gpu.py: id -> (R, block size, full frames, a short frame and trailing bytes behind them,
# what the row is there for).  A block size (d, k, a) is k * T + a for T the largest tile of the forward ("f") or the
# inverse ("i") launch at this R and frame count; full frames ("pc", n): the fewest at which the inverse runs with PC = n;
# ("cus", a, b): a * CUs + b.  The claims, checked against redux_record_plan by claims_hold: "lgT" / "ilgT" the forward /
# inverse tile, "PC", "last" the columns of the last range, "G" the groups of the (forward, inverse) frame's last tile,
# "tiles" the inverse's tiles a frame, "wrap": more frames than workgroups, "split": whether the columns are cut.
SWEEP = {}
GROUP_R = (3, 16, 23, 64, 255, 256)
GROUP_B = (16, 32, 48, 80, 112, 1008, ("f", 1, 48))   # 1, 2, 3, 5, 7 and 63 groups; a full tile and 3 groups
for _R in GROUP_R:
    for _B in GROUP_B:
        SWEEP["groups_r%d_b%s" % (_R, _B if isinstance(_B, int) else "T48")] = (_R, _B, 2, True, {})
SWEEP["groups_r3_b16"][4]["lgT"] = 4
SWEEP["groups_r3_b32"][4]["lgT"] = 5
SWEEP["groups_r3_b48"][4].update(lgT=6, G=(3, 3))
SWEEP["groups_r3_b112"][4].update(lgT=7, G=(7, 7))
SWEEP["groups_r23_b80"][4].update(lgT=7, G=(5, 5))
SWEEP["groups_r3_b1008"][4].update(lgT=10, G=(63, 63))
SWEEP["groups_r64_b1008"][4].update(lgT=9, G=(31, 31))
SWEEP["groups_r256_b1008"][4].update(lgT=7, G=(7, 31), split=True)        # forward: seven tiles of 128 records, then 7 groups
SWEEP["groups_r3_bT48"][4].update(lgT=12, G=(3, 3), tiles=2)
SWEEP["groups_r23_bT48"][4].update(lgT=10, G=(3, 3), tiles=2)
SWEEP["groups_r64_bT48"][4].update(lgT=9, ilgT=9, G=(3, 3), tiles=2, split=False)
SWEEP["groups_r255_bT48"][4].update(lgT=7, G=(3, 11), PC=64, last=63)
for _id, _row in {
    # the column ranges, one tile a frame and several with a ragged last one
    "pc64_r255": (255, 64, 3, False, dict(PC=64, last=63, split=True)),
    "pc64_r81": (81, 64, 3, False, dict(PC=64, last=17, split=True)),
    "pc64_r65": (65, 64, 3, False, dict(PC=64, last=1, split=True)),
    "pc0_r64": (64, 64, 3, False, dict(PC=64, split=False)),                      # R = 64 against 65 at the same frame count
    "pc80_r200": (200, 64, ("pc", 80), False, dict(PC=80, last=40)),
    "pc96_r256": (256, 64, ("pc", 96), False, dict(PC=96, last=64)),
    "pc112_r200": (200, 64, ("pc", 112), False, dict(PC=112, last=88)),
    "pc128_r256": (256, 64, ("pc", 128), False, dict(PC=128, last=128)),
    "pc128_r256_below_2cus": (256, 64, ("cus", 2, -1), False, dict(PC=128, split=True)),
    "pc0_r256_at_2cus": (256, 64, ("cus", 2, 0), False, dict(PC=256, split=False)),
    "pc64_r65_tiles": (65, ("i", 2, 48), 3, False, dict(PC=64, last=1, ilgT=9, tiles=3, G=(None, 3))),
    "pc64_r255_tiles": (255, ("i", 2, 48), 3, False, dict(PC=64, last=63, ilgT=9, tiles=3, G=(None, 3))),
    "pc80_r200_tiles": (200, ("i", 2, 48), ("pc", 80), False, dict(PC=80, last=40, ilgT=8, tiles=3, G=(None, 3))),
    "pc96_r256_tiles": (256, ("i", 2, 48), ("pc", 96), False, dict(PC=96, last=64, ilgT=8, tiles=3, G=(None, 3))),
    "pc112_r200_tiles": (200, ("i", 2, 48), ("pc", 112), False, dict(PC=112, last=88, ilgT=8, tiles=3, G=(None, 3))),
    "pc128_r256_tiles": (256, ("i", 2, 48), ("pc", 128), False, dict(PC=128, last=128, ilgT=8, tiles=3, G=(None, 3))),
    # one full frame of a very large block and a short one: a last tile of one group, i0 * R and p * B far from small
    "large_block_r17": (17, (1 << 22) + 16, 1, True, dict(lgT=10, ilgT=10, G=(1, 1), tiles=4097, split=False)),
    # R = 13: tiles of 2048 records
    "lg11_r13": (13, 4112, 2, True, dict(lgT=11, ilgT=11, G=(1, 1), tiles=3)),
}.items():
    SWEEP[_id] = _row
Case = namedtuple("Case", "id R B nfull tail claims")


def resolve(key, cus):
    """the row with its block size and frame count worked out for `cus` CUs; None where no frame count reaches its PC"""
    R, B, nfull, tail, claims = SWEEP[key]
    if isinstance(nfull, tuple) and nfull[0] == "pc":
        hits = [n for n in range(1, 2 * cus) if plan_of(n, R, 64, True, cus).PC == nfull[1]]
        if not hits:
            return None
        nfull = hits[0]
    elif isinstance(nfull, tuple):
        nfull = nfull[1] * cus + nfull[2]
    if isinstance(B, tuple):
        B = B[1] * max_tile(R, nfull, B[0] == "i", cus) + B[2]
    return Case(key, R, B, nfull, tail, claims)


def tail_bytes(c):
    """the short frame of B // 3 + 1 records and R - 1 trailing bytes behind the full frames of a row that has one"""
    return (c.B // 3 + 1) * c.R + c.R - 1 if c.tail else 0


def claims_hold(c, cus):
    """the row's launches, by redux_record_plan for `cus` CUs (0: the device's), are what the row is there for"""
    fwd = plan_of(c.nfull, c.R, c.B, False, cus, tail=tail_bytes(c))
    inv = plan_of(c.nfull, c.R, c.B, True, cus, tail=tail_bytes(c))
    assert fwd.grid_fast and inv.grid_fast and bool(fwd.grid_bytes) == bool(inv.grid_bytes) == c.tail, c
    got = {"lgT": fwd.lgT, "ilgT": inv.lgT, "PC": inv.PC, "last": c.R - (-(-c.R // inv.PC) - 1) * inv.PC, "split": inv.PC < c.R,
           "tiles": -(-c.B // (1 << inv.lgT))}
    for k, v in c.claims.items():
        if k == "G":
            for want, p in zip(v, (fwd, inv)):
                last = c.B % (1 << p.lgT) or min(c.B, 1 << p.lgT)
                assert want is None or last // 16 == want, (c, k, last // 16)
        else:
            assert got[k] == v, (c, k, got[k])
    assert fwd.PC == c.R and (inv.PC == c.R or (inv.PC % 16 == 0 and 64 <= inv.PC < c.R))
    return fwd, inv


@pytest.mark.parametrize("cus", [256, 8])
def test_the_sweep_reaches_what_it_claims(rx, cus):
    """Every row of SWEEP resolves for these CU counts and its claims hold; and the rows, compared with a list written out
    here, between them reach every PC, every tile size, both sides of R > 64 and of nfull < 2 * CUs, last ranges of 1, 17, 63
    and 88 columns, and last tiles of 3, 7 and 63 groups behind full ones."""
    want = ["groups_r%d_b%s" % (R, B) for R in (3, 16, 23, 64, 255, 256) for B in ("16", "32", "48", "80", "112", "1008", "T48")]
    want += ["pc64_r255", "pc64_r81", "pc64_r65", "pc0_r64", "pc80_r200", "pc96_r256", "pc112_r200", "pc128_r256",
             "pc128_r256_below_2cus", "pc0_r256_at_2cus", "pc64_r65_tiles", "pc64_r255_tiles", "pc80_r200_tiles", "pc96_r256_tiles",
             "pc112_r200_tiles", "pc128_r256_tiles", "large_block_r17", "lg11_r13"]
    assert sorted(SWEEP) == sorted(want) and len(SWEEP) == 42 + 18
    cases = {k: resolve(k, cus) for k in SWEEP}
    assert all(cases.values()), [k for k, c in cases.items() if c is None]
    plans = {k: claims_hold(c, cus) for k, c in cases.items()}
    claimed = lambda name: sorted(c.claims[name] for c in cases.values() if name in c.claims)  # noqa: E731
    # the claims are of rows of their own: one row less and a value is claimed once less
    assert claimed("PC") == [64] * 7 + [80, 80, 96, 96, 112, 112, 128, 128, 128, 256]
    assert sorted(set(claimed("lgT") + claimed("ilgT"))) == list(range(4, LG_MAX + 1))
    assert claimed("lgT") == [4, 5, 6, 7, 7, 7, 7, 9, 9, 10, 10, 10, 11, 12] and claimed("ilgT") == [8, 8, 8, 8, 9, 9, 9, 10, 11]
    assert claimed("last") == [1, 1, 17, 40, 40, 63, 63, 63, 64, 64, 88, 88, 128, 128]
    assert claimed("split") == [False] * 4 + [True] * 5
    assert sorted(g for G in claimed_groups(cases) for g in G) == [1] * 4 + [3] * 15 + [5, 5, 7, 7, 7, 11, 31, 31, 31, 63, 63]
    # the thresholds: R = 64 against 65 at one frame count; 2 * CUs - 1 frames against 2 * CUs at R = 256
    a, b = cases["pc0_r64"], cases["pc64_r65"]
    assert (a.R, b.R) == (64, 65) and a[2:5] == b[2:5] and plans["pc0_r64"][1].PC == 64 == a.R and plans["pc64_r65"][1].PC == 64 < b.R
    a, b = cases["pc128_r256_below_2cus"], cases["pc0_r256_at_2cus"]
    assert (a.nfull, b.nfull) == (2 * cus - 1, 2 * cus) and a.R == b.R == 256 and a.B == b.B
    assert plans["pc128_r256_below_2cus"][1].grid_fast == 2 * a.nfull and plans["pc0_r256_at_2cus"][1].grid_fast == b.nfull
    # a range's rows leave in pieces of 16: the ranges of the tile rows keep more than one tile a frame and a ragged last one
    for k, c in cases.items():
        if k.endswith("_tiles"):
            T = 1 << plans[k][1].lgT
            assert c.B == 2 * T + 48 and c.nfull < 2 * cus and c.R > 64
        assert c.B % 16 == 0 and c.nfull * c.R * c.B + tail_bytes(c) <= 110 << 20, c   # (the largest buffer: about 100 MB)


def claimed_groups(cases):
    return [[g for g in c.claims["G"] if g is not None] for c in cases.values() if "G" in c.claims]


def test_plan_budgets_for_every_record_size(rx):
    """For every R in 2 .. 256, block sizes either side of every tile size and frame counts on both sides of the CU counts:
    the tile fits the LDS array, the inverse's items fit their array, PC is R or a multiple of 16 of at least 64, a range
    never outnumbers the columns, and the grids are what the header promises."""
    from redux_amd import api
    for cus in (256, 8):
        for R in range(2, 257):
            for B in (16, 48, 64, 1008, 4096, 4112, 1 << 16, (1 << 22) + 16):
                for nfull in (1, 3, cus - 1, 2 * cus - 1, 2 * cus, 8 * cus + 37):
                    for delta in (False, True):
                        fwd = api.record_plan(nfull * R * B, B, R, delta, False, cus)
                        inv = api.record_plan(nfull * R * B, B, R, delta, True, cus)
                        at = (cus, R, B, nfull)
                        for p in (fwd, inv):
                            assert 4 <= p.lgT <= LG_MAX and (p.lgT == 4 or 1 << (p.lgT - 1) < B) and p.grid_bytes == 0, (at, p)
                        T = 1 << fwd.lgT
                        assert fwd.PC == R and tile_bytes(T, R) <= LDS_BYTES and fwd.grid_fast == min(nfull * -(-B // T), 8 * cus), (at, fwd)
                        assert fwd.lgT == LG_MAX or T >= B or tile_bytes(2 * T, R) > LDS_BYTES, (at, fwd)     # no tile smaller than need be
                        T, PC = 1 << inv.lgT, inv.PC
                        assert PC == R or (PC % 16 == 0 and 64 <= PC < R and R > 64 and nfull < 2 * cus), (at, inv)
                        nr = -(-R // PC)
                        assert inv.grid_fast == min(nfull, 8 * cus) * nr and (nr - 1) * PC < R, (at, inv)
                        assert tile_bytes(T, PC) <= LDS_BYTES and min(PC, R) * (T // 16) <= ITEMS, (at, inv)
                        if nfull >= 2 * cus or R <= 64:
                            assert PC == R, (at, inv)
                        elif PC > 64:  # no narrower than it takes to give every CU two workgroups' worth
                            assert nfull * -(-R // (PC - 16)) >= 2 * cus or -(-R // (PC - 16)) == nr, (at, inv)
    # the byte kernels: a thread a byte, at most 8192 workgroups; the delta inverse a thread per (frame, column)
    for R, B, L in ((4, 4100, 3 * 4 * 4100 + 5), (23, 4096, 23 * 4096 - 1), (4, 4100, 1 << 32), (256, 100, 7 * 25600 + 3)):
        nfr = -(-L // (R * B))
        for delta in (False, True):
            assert api.record_plan(L, B, R, delta, False, 256) == (4, R, 0, min(-(-L // 256), 8192))
            assert api.record_plan(L, B, R, delta, True, 256) == (4, R, 0, min(-(-(nfr * R if delta else L) // 256), 8192))
    p = api.record_plan(2 * 23 * 4096 + 100, 4096, 23, True, True, 256)     # full frames, then a short one
    assert p.grid_fast == 2 and p.grid_bytes == 1 and api.record_plan(2 * 23 * 4096 + 100, 4096, 23, False, True, 256).grid_bytes == 1
    assert api.record_plan(0, 4096, 23) == (4, 23, 0, 0)
    L = 3 * 255 * 4096   # cus = 0: the current device's CU count, whatever it is (256 without a device)
    assert api.record_plan(L, 4096, 255, inverse=True) in {api.record_plan(L, 4096, 255, inverse=True, cus=c) for c in range(1, 1025)}
    for kw in (dict(block_size=0, record_size=23), dict(block_size=64, record_size=1), dict(block_size=64, record_size=257)):
        with pytest.raises(rx.InvalidInput):
            api.record_plan(4096, **kw)


def test_record_div_is_exact_for_every_divisor_and_dividend_the_kernels_pass():
    """record_div(n, d, record_magic(d)) of redux_record.hpp, restated: m = 0xFFFFFFFF // d + 1 and n * m >> 32 (d = 1: n
    itself).  The kernels divide chunk indices c < Gn * R <= 256 * 256 by the row width and piece indices it < Tn * npc <= 4096 * 16
    by the pieces a row: every n below 2^16, every d in 1 .. 256."""
    n = np.arange(1 << 16, dtype=np.uint64)
    for d in range(1, 257):
        m = np.uint64(0xFFFFFFFF // d + 1)
        got = (n * m) >> np.uint64(32) if d > 1 else n
        assert np.array_equal(got, n // np.uint64(d)), d
        assert m < 1 << 32 or d == 1                    # the reciprocal is a 32-bit value (and unused for d = 1)
    assert 256 * 256 <= 1 << 16 and 4096 * 16 <= 1 << 16 and (LDS_BYTES // 16) * 16 == LDS_BYTES
