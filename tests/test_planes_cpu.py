"""Byte-plane layout of typed data (include/redux_hip.h, "byte-plane layout"): the numpy restatement of the layout
against hand-written expectations, container version 2, the CLI flag, the host-only ABI helpers, and the value claim
on the CPU oracle.  No GPU call."""
import ctypes as C

import numpy as np
import pytest

from oracle import cbind as ox


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def planes_ref(x, E, B, inverse=False):
    """The layout: frames of E*B bytes (the last may be shorter); in a frame of L bytes with N = L // E elements, byte p
    of element i moves to frame offset p*N + i; the L - N*E trailing bytes stay at the end.  inverse=True undoes it."""
    x = np.frombuffer(bytes(x), dtype=np.uint8) if not isinstance(x, np.ndarray) else np.ascontiguousarray(x, np.uint8)
    out = x.copy()
    F = E * B
    for f0 in range(0, len(x), F):
        fr = x[f0: f0 + F]
        N = len(fr) // E
        if N:
            shape = (E, N) if inverse else (N, E)
            out[f0: f0 + N * E] = fr[: N * E].reshape(shape).T.reshape(-1)
    return out


def lengths(E, B):
    return [0, 1, E - 1, E * B - 1, E * B, E * B + 1, 3 * E * B + 5]


# x = bytes(range(L)); the layout by hand for B = 4
F2 = [0, 2, 4, 6, 1, 3, 5, 7]                                    # E = 2: one full frame of 8 bytes
F4 = [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]      # E = 4: one full frame of 16 bytes
HAND = {
    (2, 0): [], (2, 1): [0],
    (2, 7): [0, 2, 4, 1, 3, 5, 6],                               # N = 3 elements + 1 trailing byte
    (2, 8): F2, (2, 9): F2 + [8],
    (2, 29): F2 + [8 + v for v in F2] + [16 + v for v in F2] + [24, 26, 25, 27, 28],
    (4, 0): [], (4, 1): [0], (4, 3): [0, 1, 2],
    (4, 15): [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11, 12, 13, 14],  # N = 3 elements + 3 trailing bytes
    (4, 16): F4, (4, 17): F4 + [16],
    (4, 53): F4 + [16 + v for v in F4] + [32 + v for v in F4] + [48, 49, 50, 51, 52],  # last frame: 1 element + 1
}


@pytest.mark.parametrize("E", [2, 4])
def test_layout_matches_hand_written_expectations(E):
    B = 4
    for L in lengths(E, B):
        x = np.arange(L, dtype=np.uint8)
        got = planes_ref(x, E, B)
        assert got.tolist() == HAND[(E, L)], (E, L)
        assert planes_ref(got, E, B, inverse=True).tolist() == x.tolist(), (E, L)


@pytest.mark.parametrize("E", [2, 4, 8])
@pytest.mark.parametrize("B", [4, 16, 1000])
def test_inverse_of_forward_is_identity(E, B):
    rng = np.random.default_rng(E * 1000 + B)
    for L in lengths(E, B) + [7 * E * B + 3]:
        x = rng.integers(0, 256, L, dtype=np.uint8)
        y = planes_ref(x, E, B)
        assert np.array_equal(planes_ref(y, E, B, inverse=True), x)
        if L >= E * B:  # a full frame is E blocks, block j = byte j of each of B elements
            for j in range(E):
                assert np.array_equal(y[j * B: (j + 1) * B], x[: E * B].reshape(B, E)[:, j])


def test_element_size_one_is_the_identity():
    x = np.arange(100, dtype=np.uint8)
    assert np.array_equal(planes_ref(x, 1, 7), x)


# ---- container version 2 -----------------------------------------------------------------------------------------
def test_container_v2_roundtrip_and_v1_unchanged(rx):
    from redux_amd import container
    streams = np.arange(10, dtype=np.uint8)
    offs = np.array([0, 3, 3, 10], dtype=np.uint64)
    v1 = container.pack(streams, offs, (8, 30, 32), 65536, 3 * 65536 - 5)
    assert container.pack(streams, offs, (8, 30, 32), 65536, 3 * 65536 - 5, element_size=1) == v1
    assert v1[4] == 1 and v1[12:16] == b"\0\0\0\0" and container.element_size(v1) == 1
    for E in (2, 4, 8):
        v2 = container.pack(streams, offs, (8, 30, 32), 65536, 3 * 65536 - 5, element_size=E)
        assert v2[4] == 2 and int.from_bytes(v2[12:16], "little") == E
        assert v2[:4] + v2[5:12] + v2[16:] == v1[:4] + v1[5:12] + v1[16:]  # same layout otherwise
        P, bs, total, o2, payload = container.unpack(v2)
        assert P.triple() == (8, 30, 32) and bs == 65536 and total == 3 * 65536 - 5
        assert o2.tolist() == offs.tolist() and payload.tobytes() == streams.tobytes()
        assert container.element_size(v2) == E
        assert container.header_is_wellformed(v2) and container.header_is_wellformed(v1)


def test_container_v2_rejects_other_element_sizes(rx):
    from redux_amd import api, container
    streams = np.zeros(4, np.uint8)
    offs = np.array([0, 4], np.uint64)
    for E in (0, 3, 16):
        with pytest.raises(api.InvalidInput):
            container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=E)
    good = container.pack(streams, offs, (8, 30, 32), 65536, 10, element_size=2)
    for E in (0, 1, 3, 16):
        bad = bytearray(good)
        bad[12:16] = E.to_bytes(4, "little")
        assert not container.header_is_wellformed(bytes(bad))
        with pytest.raises(api.InvalidInput):
            container.unpack(bytes(bad))
        with pytest.raises(api.InvalidInput):
            container.element_size(bytes(bad))
    v1 = bytearray(container.pack(streams, offs, (8, 30, 32), 65536, 10))
    v1[12] = 2  # version 1 keeps its reserved field zero
    assert not container.header_is_wellformed(bytes(v1))
    v3 = bytearray(good)
    v3[4] = 3
    assert not container.header_is_wellformed(bytes(v3))
    with pytest.raises(api.InvalidInput):
        container.unpack(bytes(v3))


# ---- CLI ----------------------------------------------------------------------------------------------------------
def test_cli_element_size_flag(rx):
    from redux_amd import cli
    assert cli.parse(["-c", "--block-size", "65536", "--element-size", "2"]) == \
        {"compress": True, "input": None, "output": None, "block_size": 65536, "element_size": 2}
    assert cli.parse(["-c", "--block-size", "65536"]) == {"compress": True, "input": None, "output": None, "block_size": 65536}
    assert cli.parse(["-c", "--block-size", "4096", "--element-size", "1"])["element_size"] == 1
    assert cli.parse(["-c", "--element-size", "1"]) is not None  # no layout: the raw stream is fine
    for bad in (["-c", "--element-size", "2"], ["-c", "--block-size", "0", "--element-size", "8"],
                ["-c", "--block-size", "65536", "--element-size", "3"], ["-c", "--block-size", "65536", "--element-size", "16"],
                ["-c", "--block-size", "65536", "--element-size", "x"], ["-c", "--block-size", "65536", "--element-size"]):
        assert cli.parse(bad) is None, bad
    assert cli.main(["-c", "--element-size", "4"]) == 1
    assert cli.main(["-c", "--block-size", "0", "--element-size", "2"]) == 1


# ---- host-only ABI helpers ------------------------------------------------------------------------------------------
def test_planes_check_and_workspace_helpers(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in range(0, 20):
        assert L.redux_planes_check(E) == (_lib.OK if E in (1, 2, 4, 8) else _lib.INVALID_INPUT), E
    assert L.redux_planes_check(0xFFFFFFFF) == _lib.INVALID_INPUT
    for params in ((8, 30, 32), (8, 14, 16), (4, 10, 16)):
        p = _lib.Params(*params)
        for n, B in ((0, 65536), (1, 65536), (3 * 65536 + 7, 65536), (64 << 20, 65536), (1000, 4)):
            plain_e = L.redux_encode_workspace_bytes(C.byref(p), n, B)
            plain_d = L.redux_decode_workspace_bytes(C.byref(p), L.redux_block_count(n, B), B)
            assert L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, 1) == plain_e
            for E in (2, 4, 8):
                we = L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, E)
                wd = L.redux_decode_planes_workspace_bytes(C.byref(p), n, B, E)
                assert we > 0 and wd > 0
                assert we >= plain_e + n and wd >= plain_d + n, (params, n, B, E)
                assert we % 256 == plain_e % 256  # (the carved copy keeps what follows aligned)
            for bad in (0, 3, 16):
                assert L.redux_encode_planes_workspace_bytes(C.byref(p), n, B, bad) == 0
                assert L.redux_decode_planes_workspace_bytes(C.byref(p), n, B, bad) == 0
    p = _lib.Params(8, 9, 16)  # invalid triple
    assert L.redux_encode_planes_workspace_bytes(C.byref(p), 100, 64, 2) == 0
    assert L.redux_decode_planes_workspace_bytes(C.byref(p), 100, 64, 2) == 0


def test_python_api_rejects_bad_element_sizes_before_any_device_call(rx):
    for E in (0, 3, 16, -2, 2.0):
        with pytest.raises(rx.InvalidInput):
            rx.compress_blocks(b"abcd", 4, element_size=E)
    with pytest.raises(rx.InvalidInput):  # element_size > 1 needs the original length
        rx.decompress_blocks(b"\0", np.array([0, 1], np.uint64), 4, element_size=2)


# ---- the value claim, on the CPU oracle ------------------------------------------------------------------------------
def bf16_data(n_elems, seed=7):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal(n_elems) * 0.02).astype(np.float32)
    return (f.view(np.uint32) >> 16).astype(np.uint16).view(np.uint8)  # bf16 by truncation: the high half of fp32


def oracle_bytes(data, block):
    streams, status = ox.compress_blocks(data, block, (8, 30, 32))
    assert not status.any()
    return sum(len(s) for s in streams)


def test_layout_pays_on_bf16_and_only_across_blocks():
    B = 65536
    x = bf16_data(8 * B // 2)  # 8 blocks of bf16
    plain = oracle_bytes(x, B)
    planes = oracle_bytes(planes_ref(x, 2, B), B)
    assert planes <= 0.9 * plain, (plain, planes)
    # the same layout INSIDE each block (frames of one block): the adaptive model's cost of a block does not depend on the
    # order of its bytes, so this gains nothing
    inside = np.concatenate([planes_ref(x[o: o + B], 2, B // 2) for o in range(0, len(x), B)])
    assert sorted(inside[:B].tolist()) == sorted(x[:B].tolist())
    assert abs(oracle_bytes(inside, B) - plain) <= 0.002 * plain, (plain, oracle_bytes(inside, B))
