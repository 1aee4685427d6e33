"""Stored blocks without a GPU: the rule against the CPU oracle's stream sizes, the container's stored-block bitmap (versions
0x41 / 0x42 / 0x51 / 0x52) and every rejection of it, the unchanged flagless writers, the CLI's usage errors and the
host-side workspace functions."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import cbind as ox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 65536


def rule(status, s, L, t):
    """stored_b <=> status_b == OK and s_b * 65536 >= t * L_b (include/redux_hip.h, "stored blocks")"""
    s, L = np.asarray(s, dtype=np.uint64), np.asarray(L, dtype=np.uint64)
    return (np.asarray(status) == 0) & (s * np.uint64(65536) >= np.uint64(t) * L)


def oracle_sizes(x, block_size):
    _, sizes, status, _ = ox.compress_blocks_raw(x, block_size)
    n = len(x)
    L = [min(block_size, n - o) for o in range(0, n, block_size)] or [0]
    return sizes, status, np.array(L, dtype=np.uint64)


def test_rule_on_oracle_sizes():
    rng = np.random.default_rng(7)
    iid = rng.integers(0, 256, 4 * B, dtype=np.uint8)
    s, st, L = oracle_sizes(iid, B)
    assert rule(st, s, L, 65536).all() and (s >= L).all()  # uniform bytes expand
    const = np.full(B, 0x41, dtype=np.uint8)
    s, st, L = oracle_sizes(const, B)
    assert not rule(st, s, L, 65536).any() and rule(st, s, L, 0).all()
    # equality: s * 65536 == t * L is stored, one step above it is not
    assert rule(st, s, L, int(s[0])).all() and not rule(st, s, L, int(s[0]) + 1).any()
    s, st, L = oracle_sizes(np.zeros(0, dtype=np.uint8), B)
    assert list(L) == [0] and rule(st, s, L, 0).all() and rule(st, s, L, 65536).all()
    assert not rule([3], [100], [10], 0).any()  # a failing block is never stored


# ---- container ---------------------------------------------------------------------------------------------------------
def _fake(kind, nb=11, crc=False):
    """pack() of made-up payloads (no GPU): blocks 1, 4, 7, 8 and the ragged last one stored"""
    from redux_amd import container
    Bs = 100
    total = Bs * (nb - 1) + 37
    L = [min(Bs, total - b * Bs) for b in range(nb)]
    flags = np.zeros(nb, dtype=np.uint8)
    flags[[b for b in (1, 4, 7, 8, nb - 1) if b < nb]] = 1
    sizes = np.array([L[b] if flags[b] else 3 + b for b in range(nb)], dtype=np.uint64)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    streams = (np.arange(int(offs[-1])) * 7).astype(np.uint8)
    E = 4 if kind == "planes" else 1
    c = (np.arange(nb, dtype=np.uint64) * 0x9E3779B1 + 1).astype(np.uint32) if crc else None
    blob = container.pack(streams, offs, (8, 30, 32), Bs, total, E, block_crc=c, stored=flags)
    return blob, flags, streams, offs, Bs, total, c


@pytest.mark.parametrize("kind,crc,ver", [("adaptive", False, 0x41), ("planes", False, 0x42), ("adaptive", True, 0x51),
                                          ("planes", True, 0x52)])
@pytest.mark.parametrize("nb", [1, 8, 11, 17])
def test_pack_unpack_block_stored(kind, crc, ver, nb):
    from redux_amd import container
    blob, flags, streams, offs, Bs, total, c = _fake(kind, nb, crc)
    assert blob[4] == ver
    P, bs, tot, o, payload = container.unpack(blob)
    assert (bs, tot) == (Bs, total) and list(o) == list(offs)
    assert payload.tobytes() == streams.tobytes()
    got = container.block_stored(blob)
    assert got.dtype == np.uint8 and got.tolist() == flags.tolist()
    assert container.header_is_wellformed(blob)
    assert container.element_size(blob) == (4 if kind == "planes" else 1)
    assert container.static_table(blob) is None
    assert (container.block_crcs(blob) is None) == (not crc)
    if crc:
        assert container.block_crcs(blob).tolist() == c.tolist()
    assert len(blob) == container.HEADER.size + 4 * nb * (2 if crc else 1) + (nb + 7) // 8 + int(offs[-1])
    assert container.block_stored(container.pack(streams, offs, (8, 30, 32), Bs, total, container.element_size(blob))) is None


def _bitmap_at(blob):
    from redux_amd import container
    nb = container.HEADER.unpack_from(blob, 0)[7]
    return container.HEADER.size + 4 * nb * (2 if blob[4] & 0x10 else 1)


def test_nonzero_padding_bits_rejected():
    import redux_amd as rx
    from redux_amd import container
    blob, *_ = _fake("adaptive", 11)
    at = _bitmap_at(blob) + 1  # byte 1 holds blocks 8..10; bits 3..7 are padding
    bad = blob[:at] + bytes([blob[at] | 0x80]) + blob[at + 1:]
    with pytest.raises(rx.InvalidInput):
        container.unpack(bad)
    with pytest.raises(rx.InvalidInput):
        container.block_stored(bad)


def test_stored_size_must_be_raw_length():
    import redux_amd as rx
    from redux_amd import container
    blob, flags, *_ = _fake("adaptive", 11)
    at = _bitmap_at(blob)
    bad = blob[:at] + bytes([blob[at] | 0x01]) + blob[at + 1:]  # block 0 (3 payload bytes of 100) flagged stored
    with pytest.raises(rx.InvalidInput):
        container.unpack(bad)
    with pytest.raises(rx.InvalidInput):
        container.pack(np.zeros(10, np.uint8), np.array([0, 10], np.uint64), (8, 30, 32), 100, 100, stored=np.ones(1, np.uint8))


@pytest.mark.parametrize("ver", [0x43, 0x53, 0x40, 0x50, 0x44, 0xC1, 0x61])
def test_bad_stored_versions_rejected(ver):
    import redux_amd as rx
    from redux_amd import container
    blob, *_ = _fake("adaptive", 11)
    bad = blob[:4] + bytes([ver]) + blob[5:]
    with pytest.raises(rx.InvalidInput):
        container.unpack(bad)
    assert not container.header_is_wellformed(bad)


def test_static_model_has_no_stored_blocks():
    import redux_amd as rx
    from redux_amd import container
    m = rx.StaticModel(rx.Parameters(8, 30, 32), np.arange(258, dtype=np.uint32) * 4)
    with pytest.raises(rx.InvalidInput):
        container.pack(np.zeros(3, np.uint8), np.array([0, 3], np.uint64), m, 100, 50, stored=np.zeros(1, np.uint8))
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(b"abc", 100, model="static", stored=True)


def test_truncated_bitmap_is_eof():
    import redux_amd as rx
    from redux_amd import container
    blob, *_ = _fake("adaptive", 17)
    cut = _bitmap_at(blob) + 1  # inside the 3-byte bitmap
    with pytest.raises(rx.Eof):
        container.unpack(blob[:cut])
    with pytest.raises(rx.Eof):
        container.block_stored(blob[:cut])


def test_flagless_pack_is_unchanged():
    from redux_amd import container
    blob, flags, streams, offs, Bs, total, _ = _fake("adaptive", 11)
    a = container.pack(streams, offs, (8, 30, 32), Bs, total)
    b = container.pack(streams, offs, (8, 30, 32), Bs, total, stored=None)
    assert a == b and a[4] == 1
    # the flagged container is the flagless one with the bit set and the bitmap inserted
    at = _bitmap_at(blob)
    assert blob[:4] + bytes([1]) + blob[5:at] + blob[at + 2:] == a


# ---- CLI -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--stored"], ["--stored", "--block-size", "0"],
                                   ["--stored", "--block-size", "4096", "--model", "static"]])
def test_cli_stored_usage_errors(tmp_path, extra):
    src = tmp_path / "in.bin"
    src.write_bytes(b"hello" * 100)
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", *extra, "-i", str(src), "-o", str(tmp_path / "out")],
                       cwd=ROOT, capture_output=True)
    assert r.returncode == 1 and b"Usage" in r.stderr


def test_cli_parse_stored():
    from redux_amd import cli
    assert cli.parse(["-c", "--stored", "--block-size", "65536"])["stored"] is True
    assert "stored" not in cli.parse(["-c", "--block-size", "65536"])


# ---- workspace functions: host-side, no device touched --------------------------------------------------------------
def test_workspace_functions():
    from redux_amd import _lib
    L = _lib.lib()
    p = _lib.Params(8, 30, 32)
    for n, bs in ((0, 65536), (1, 65536), (65536 * 5 + 3, 65536), (1 << 20, 4096), (3 << 20, 1 << 20)):
        for E in (1, 2, 4, 8):
            enc = L.redux_encode_stored_workspace_bytes(C.byref(p), n, bs, E)
            dec = L.redux_decode_stored_workspace_bytes(C.byref(p), n, bs, E)
            assert enc >= L.redux_encode_planes_workspace_bytes(C.byref(p), n, bs, E) > 0
            if E > 1:  # (E = 1 decodes straight into the output: no plane buffer)
                assert dec >= L.redux_decode_planes_workspace_bytes(C.byref(p), n, bs, E) > 0
            assert enc >= L.redux_encode_workspace_bytes(C.byref(p), n, bs)
            assert dec >= L.redux_decode_workspace_bytes(C.byref(p), L.redux_block_count(n, bs), bs)
    # outside the coverage: 0
    for q, E in ((_lib.Params(4, 10, 16), 1), (_lib.Params(8, 24, 40), 1), (p, 3)):
        assert L.redux_encode_stored_workspace_bytes(C.byref(q), 1000, 4096, E) == 0
        assert L.redux_decode_stored_workspace_bytes(C.byref(q), 1000, 4096, E) == 0


def test_python_argument_checks():
    import redux_amd as rx
    m = rx.StaticModel(rx.Parameters(8, 30, 32), np.arange(258, dtype=np.uint32) * 4)
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(b"abc", 100, m, stored=np.zeros(1, np.uint8))
    with pytest.raises(rx.InvalidInput):  # stored= needs length=
        rx.decompress_blocks(b"abc", np.array([0, 3], np.uint64), 100, stored=np.zeros(1, np.uint8))
    assert rx.STORE_RATIO == 65536
