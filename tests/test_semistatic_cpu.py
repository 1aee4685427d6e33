"""Semi-static coding (include/redux_hip.h, "semi-static coding") without a GPU: a numpy restatement of the rule against
redux_static_table_from_counts, container version 3 and the CLI's --model flag."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def rule_ref(counts, total):
    """The rule in exact integers: f = 1 + floor(c R / N), the D = T - sum f bytes with the largest remainders c R mod N
    (lower index first on ties) get one more, EOF = 1; N = 0: all ones.  None where N R >= 2^64 or N itself does not fit
    in 64 bits."""
    c = [int(x) for x in counts]
    N, R = sum(c), total - 257
    if N >= 1 << 64 or N * R >= 1 << 64:
        return None
    if N == 0:
        f = [1] * 257
    else:
        f = [1 + x * R // N for x in c] + [1]
        r = [x * R % N for x in c]
        D = total - sum(f)
        assert 0 <= D <= 255
        for s in sorted(range(256), key=lambda s: (-r[s], s))[:D]:
            f[s] += 1
    return np.concatenate([[0], np.cumsum(f)]).astype(np.uint32)


def c_table(lib, counts, total, params=(8, 30, 32)):
    cp = lib.Params(*params)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    cum = np.zeros(258, dtype=np.uint32)
    st = lib.lib().redux_static_table_from_counts(C.byref(cp), c.ctypes.data, total, cum.ctypes.data)
    return st, cum


def count_cases():
    rng = np.random.default_rng(2026)
    one = np.zeros(256, np.uint64)
    one[97] = 12345
    ties = np.zeros(256, np.uint64)
    ties[::3] = 7  # 86 equal bins: equal remainders everywhere
    ties[1::3] = 1
    zipf = (1e6 / np.arange(1, 257) ** 1.2).astype(np.uint64)
    return {
        "random": rng.integers(0, 1 << 40, 256, dtype=np.uint64),
        "random_small": rng.integers(0, 50, 256, dtype=np.uint64),
        "sparse": np.where(rng.random(256) < 0.1, rng.integers(1, 1000, 256), 0).astype(np.uint64),
        "zeros": np.zeros(256, np.uint64),
        "one_bin": one,
        "equal": np.full(256, 4096, np.uint64),
        "ties": ties,
        "zipf": zipf,
    }


TOTALS = [257, 258, 1000, 1 << 16, (1 << 16) + 1, (1 << 30) - 1]


@pytest.mark.parametrize("name", sorted(count_cases()))
def test_rule_matches_restatement(lib, name):
    counts = count_cases()[name]
    for T in TOTALS:
        want = rule_ref(counts, T)
        st, cum = c_table(lib, counts, T)
        if want is None:
            assert st == lib.UNSUPPORTED, (name, T)
            continue
        assert st == lib.OK, (name, T)
        assert cum.tolist() == want.tolist(), (name, T)
        cp = lib.Params(8, 30, 32)
        assert lib.lib().redux_static_table_check(C.byref(cp), cum.ctypes.data_as(C.POINTER(C.c_uint32))) == lib.OK
        assert int(cum[-1]) == (257 if not counts.any() else T)
        assert int(cum[257] - cum[256]) == 1  # EOF


def test_rule_at_freq_max_of_other_widths(lib):
    counts = count_cases()["zipf"]
    for params in ((8, 16, 32), (8, 14, 16), (8, 20, 24)):
        fmax = (1 << params[1]) - 1
        st, cum = c_table(lib, counts, fmax, params)
        assert st == lib.OK and cum.tolist() == rule_ref(counts, fmax).tolist(), params
        assert c_table(lib, counts, fmax + 1, params)[0] == lib.INVALID_INPUT


def test_overflow_limit(lib):
    T = 1 << 16
    R = T - 257
    lim = ((1 << 64) - 1) // R  # the largest N with N R < 2^64
    counts = np.zeros(256, np.uint64)
    counts[0] = lim - 1000
    counts[200] = 1000
    st, cum = c_table(lib, counts, T)
    assert st == lib.OK and cum.tolist() == rule_ref(counts, T).tolist()
    counts[200] += 1  # N = lim + 1: N R >= 2^64
    assert rule_ref(counts, T) is None
    assert c_table(lib, counts, T)[0] == lib.UNSUPPORTED
    big = np.full(256, (1 << 64) - 1, np.uint64)  # N itself beyond 64 bits
    assert c_table(lib, big, T)[0] == lib.UNSUPPORTED
    assert c_table(lib, big, 257)[0] == lib.UNSUPPORTED  # (R = 0, but N does not fit)


def test_bad_arguments(lib):
    counts = np.ones(256, np.uint64)
    for T in (0, 1, 256, 1 << 30, 0xFFFFFFFF):
        assert c_table(lib, counts, T)[0] == lib.INVALID_INPUT, T
    good = rule_ref(counts, 1000)
    for params in ((4, 10, 16), (8, 30, 40), (8, 40, 48), (8, 9, 16), (12, 20, 32)):  # what redux_static_table_check says
        cp = lib.Params(*params)
        want = lib.lib().redux_static_table_check(C.byref(cp), good.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert want != lib.OK and c_table(lib, counts, 1000, params)[0] == want, params
    assert c_table(lib, counts, 1 << 16, (4, 10, 16))[0] == lib.UNSUPPORTED   # symbol_bits != 8
    cp = lib.Params(8, 30, 32)
    cum = np.zeros(258, np.uint32)
    assert lib.lib().redux_static_table_from_counts(C.byref(cp), None, 1 << 16, cum.ctypes.data) == lib.INVALID_INPUT
    assert lib.lib().redux_histogram_workspace_bytes(1 << 32) == 0


def test_python_wrappers(rx):
    counts = count_cases()["zipf"]
    assert rx.static_table_from_counts(counts).tolist() == rule_ref(counts, 1 << 16).tolist()  # default total 2^16
    assert rx.static_table_from_counts(counts, (8, 14, 16)).tolist() == rule_ref(counts, (1 << 14) - 1).tolist()
    m = rx.StaticModel((8, 30, 32), rule_ref(counts, 1000))
    assert m.parameters().triple() == (8, 30, 32) and m.total() == 1000
    for bad in (np.zeros(258), np.arange(257), np.arange(258)[::-1]):
        with pytest.raises(rx.InvalidInput):
            rx.StaticModel((8, 30, 32), bad)
    with pytest.raises(rx.InvalidInput):  # no byte-plane form of the static model
        rx.compress_blocks(b"abcd", 4, m, element_size=2)


# ---- container version 3 --------------------------------------------------------------------------------------------
def test_container_v3_roundtrip_and_v1_v2_unchanged(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    cum = rule_ref(count_cases()["zipf"], 1 << 16)
    m = rx.StaticModel((8, 30, 32), cum)
    v1 = container.pack(streams, offs, (8, 30, 32), 65536, 3 * 65536 - 5)
    v2 = container.pack(streams, offs, (8, 30, 32), 65536, 3 * 65536 - 5, element_size=2)
    v3 = container.pack(streams, offs, m, 65536, 3 * 65536 - 5)
    assert v3[4] == 3 and v3[12:16] == b"\0\0\0\0"
    H = container.HEADER.size  # 32
    assert v3[:4] + v3[5:H] == v1[:4] + v1[5:H]
    assert np.frombuffer(v3[H:H + 1032], "<u4").tolist() == cum.tolist()
    assert v3[H + 1032:] == v1[H:]  # sizes and payloads as in version 1
    P, bs, total, o3, payload = container.unpack(v3)
    assert P.triple() == (8, 30, 32) and bs == 65536 and total == 3 * 65536 - 5
    assert o3.tolist() == offs.tolist() and payload.tobytes() == streams.tobytes()
    assert container.static_table(v3).tolist() == cum.tolist()
    assert container.static_table(v1) is None and container.static_table(v2) is None
    assert container.element_size(v3) == 1 and container.header_is_wellformed(v3)
    # versions 1 and 2: the bytes this module wrote before version 3
    head = bytes.fromhex("52445842") + bytes([1, 8, 30, 32]) + (65536).to_bytes(4, "little") + bytes(4) + \
        (3).to_bytes(8, "little") + (3 * 65536 - 5).to_bytes(8, "little")
    assert v1 == head + np.array([3, 0, 7], "<u4").tobytes() + streams.tobytes()
    assert v2 == head[:4] + b"\x02" + head[5:12] + (2).to_bytes(4, "little") + head[16:] + v1[H:]
    with pytest.raises(rx.InvalidInput):
        container.pack(streams, offs, m, 65536, 3 * 65536 - 5, element_size=2)


def test_container_v3_rejects_damage(rx):
    from redux_amd import container
    cum = rule_ref(count_cases()["random_small"], 1 << 16)
    good = container.pack(np.zeros(4, np.uint8), np.array([0, 4], np.uint64), rx.StaticModel((8, 30, 32), cum), 65536, 10)
    H = container.HEADER.size
    for cut in (H, H + 1, H + 1031):  # a truncated table
        with pytest.raises(rx.Eof):
            container.unpack(good[:cut])
        with pytest.raises(rx.Eof):
            container.static_table(good[:cut])
    with pytest.raises(rx.Eof):  # truncated sizes / payload
        container.unpack(good[:-1])
    bad_tables = []
    t = bytearray(good); t[H:H + 4] = (1).to_bytes(4, "little"); bad_tables.append(t)            # cum[0] != 0
    t = bytearray(good); t[H + 4:H + 8] = (0).to_bytes(4, "little"); bad_tables.append(t)        # a zero frequency
    t = bytearray(good); t[H + 4 * 257: H + 4 * 258] = (1 << 31).to_bytes(4, "little"); bad_tables.append(t)  # > freq_max
    for t in bad_tables:
        with pytest.raises(rx.InvalidInput):
            container.unpack(bytes(t))
        with pytest.raises(rx.InvalidInput):
            container.static_table(bytes(t))
        with pytest.raises(rx.InvalidInput):
            container.decompress_bytes(bytes(t))
    t = bytearray(good)
    t[12] = 1  # version 3 keeps its reserved word zero
    assert not container.header_is_wellformed(bytes(t))
    with pytest.raises(rx.InvalidInput):
        container.unpack(bytes(t))
    t = bytearray(good)
    t[5:8] = bytes([4, 10, 16])  # parameters the static coder does not take
    with pytest.raises(rx.InvalidInput):
        container.unpack(bytes(t))
    t = bytearray(good)
    t[4] = 4  # no version 4
    assert not container.header_is_wellformed(bytes(t))
    with pytest.raises(rx.InvalidInput):
        container.unpack(bytes(t))


# ---- CLI ------------------------------------------------------------------------------------------------------------
def test_cli_model_flag(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    assert cli.parse(["-c", "--block-size", "65536", "--model", "static"]) == dict(base, model="static")
    assert cli.parse(["-c", "--block-size", "65536", "--model", "adaptive"]) == dict(base, model="adaptive")
    assert cli.parse(["-c", "--model", "adaptive"]) is not None  # the reference's model: the raw stream is fine
    assert cli.parse(["-d", "--model", "static"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--element-size", "1", "--model", "static"])["model"] == "static"
    for bad in (["-c", "--model", "static"], ["-c", "--block-size", "0", "--model", "static"],
                ["-c", "--block-size", "65536", "--element-size", "2", "--model", "static"],
                ["-c", "--block-size", "65536", "--model", "Static"], ["-c", "--block-size", "65536", "--model"]):
        assert cli.parse(bad) is None, bad
        assert cli.main(bad) == 1, bad
    assert "--model" in cli.USAGE and "static" in cli.USAGE


# ---- C++ mirror -----------------------------------------------------------------------------------------------------
def build_semistatic_mirror_test(tmpdir):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(tmpdir), "semistatic_mirror_test")
    libdir = os.path.join(root, "redux_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe,
                           os.path.join(root, "tests", "cpp", "semistatic_mirror_test.cpp"),
                           "-L" + libdir, "-lredux_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_semistatic_mirror_compiles(lib, tmp_path):
    import os
    lib.lib()
    assert os.access(build_semistatic_mirror_test(tmp_path), os.X_OK)
