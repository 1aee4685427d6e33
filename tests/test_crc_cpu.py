"""Per-block CRC-32 without a GPU: the math k_crc32 (redux_amd/csrc/redux_crc.hpp) rests on, restated in numpy and checked
against zlib for every group width, block size and alignment the GPU tests use; redux_crc32_combine against zlib; the
checksummed container (versions 0x11 / 0x12 / 0x13); the CLI's usage rule for --checksum."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = 0xEDB88320
M32 = 0xFFFFFFFF


# ---- GF(2) mod P, reflected (bit 31 = x^0), as in redux_crc.hpp -------------------------------------------------------
def mulx(b):
    return (b >> 1) ^ (POLY if b & 1 else 0)


def divx(b):
    return (((b ^ POLY) << 1) | 1) & M32 if b & 0x80000000 else (b << 1) & M32


def mulmod(a, b):
    p = 0
    for i in range(31, -1, -1):
        if (a >> i) & 1:
            p ^= b
        b = mulx(b)
    return p


def x8n(n):
    """x^(8n) mod P for any integer n"""
    p = 0x80000000
    step = divx if n < 0 else mulx
    for _ in range(8 * abs(n)):
        p = step(p)
    return p


def tables():
    t = np.zeros((16, 256), dtype=np.uint32)
    for v in range(256):
        r = v
        for _ in range(8):
            r = mulx(r)
        t[0, v] = r
    for j in range(1, 16):
        prev = t[j - 1]
        t[j] = (prev >> 8) ^ t[0][prev & 0xFF]
    return t


T = tables()
C = [x8n(n) for n in range(-15, 1025)]  # kCrc.c
INIT = [mulmod(C[15 - h], M32) for h in range(16)]


def gap_tables(G):
    z = C[15 + 16 * (G - 1)]
    return np.array([[mulmod(z, int(T[j, v])) for v in range(256)] for j in range(16)], dtype=np.uint32)


_GAP = {}


def gap(G):
    if G not in _GAP:
        _GAP[G] = gap_tables(G)
    return _GAP[G]


def step(r, chunk, t):
    w = bytearray(chunk)
    for i in range(4):
        w[i] ^= (r >> (8 * i)) & 0xFF
    out = 0
    for i in range(16):
        out ^= int(t[15 - i, w[i]])
    return out


def piece_term(mem, s, e, G, first):
    """k_crc32's sum over the G lanes of a group for the piece mem[s:e) (s, e: addresses into mem, which stands for the
    device's address space: a0 = s rounded down to 16 must be a valid index).  Returns the register at e."""
    W = 16 * G
    h = s & 15
    a0 = s - h
    R, rem = divmod(e - a0, W)
    acc = 0
    for q in range(G):
        n = R + (1 if 16 * q < rem else 0)
        r = INIT[h] if (q == 0 and first) else 0
        if not n:
            continue
        for i in range(n):
            c = a0 + i * W + 16 * q
            chunk = bytes(mem[k] if s <= k < e else 0 for k in range(c, c + 16))
            r = step(r, chunk, gap(G) if i + 1 < n else T)
        p = a0 + (n - 1) * W + 16 * q + 16
        assert -15 <= e - p < W
        acc ^= mulmod(C[e - p + 15], r)
    return acc


def block_crc(mem, s, length, G, seg=None):
    """the CRC the kernel writes for the block mem[s : s + length), in pieces of `seg` bytes (None: one piece)"""
    if length == 0:
        return 0
    seg = seg or length
    out = 0
    for o0 in range(0, length, seg):
        o1 = min(o0 + seg, length)
        term = piece_term(mem, s + o0, s + o1, G, o0 == 0)
        out ^= mulmod(x8n(length - o1), term)
    return out ^ M32


def group_for(B):
    """redux_hip.hip crc_group(): the widest power of two <= 64 with at least 16 chunks per lane"""
    G = 1
    while G < 64 and 256 * 2 * G <= B:
        G *= 2
    return G


@pytest.mark.parametrize("B", [1, 3, 15, 16, 17, 100, 1000, 1024, 1025, 4095])
def test_group_math_equals_zlib(B):
    rng = np.random.default_rng(B)
    mem = rng.integers(0, 256, size=3 * B + 64, dtype=np.uint8).tobytes()
    G = group_for(B)
    for G_ in {G, 1, 64}:
        for off in (0, 1, 7, 15, 16):
            for length in {B, max(B - 1, 0), B // 2}:
                s = 16 + off
                assert block_crc(mem, s, length, G_) == zlib.crc32(mem[s:s + length]), (G_, off, length)


@pytest.mark.parametrize("off", [0, 5, 15])
def test_segments_equal_zlib(off):
    """blocks split into segments (kCrcSeg at the kernel's scale, a small multiple of 16 here): terms advanced to the
    block end and XORed"""
    rng = np.random.default_rng(off)
    mem = rng.integers(0, 256, size=6000, dtype=np.uint8).tobytes()
    s = 16 + off
    for length in (2048, 3000, 4100, 5000):
        assert block_crc(mem, s, length, 64, seg=1024) == zlib.crc32(mem[s:s + length])
        assert block_crc(mem, s, length, 64, seg=2048) == zlib.crc32(mem[s:s + length])


def test_special_data():
    for fill in (0x00, 0xFF):
        mem = bytes([fill]) * 5000
        for off, length in ((16, 4096), (19, 2500), (31, 1)):
            assert block_crc(mem, off, length, group_for(length)) == zlib.crc32(mem[off:off + length])
    assert block_crc(b"\0" * 64, 16, 0, 1) == zlib.crc32(b"") == 0


def test_identities():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, size=37, dtype=np.uint8).tobytes()
    b = rng.integers(0, 256, size=91, dtype=np.uint8).tobytes()
    raw = lambda m: zlib.crc32(m, 0) ^ mulmod(x8n(len(m)), M32) ^ M32  # noqa: E731  (register from 0, no init/xorout)
    assert raw(a + b) == mulmod(x8n(len(b)), raw(a)) ^ raw(b)
    for h in range(16):  # the init of a lane that reads h zero bytes in front of the block's first byte
        r = INIT[h]
        for _ in range(h):
            r = (r >> 8) ^ int(T[0, r & 0xFF])
        assert r == M32


# ---- C ABI: redux_crc32_combine ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib.lib()


def test_combine_equals_zlib(lib):
    import redux_amd as rx
    rng = np.random.default_rng(11)
    data = rng.integers(0, 256, size=20000, dtype=np.uint8).tobytes()
    for cut in (0, 1, 15, 16, 999, 10000, 19999, 20000):
        a, b = data[:cut], data[cut:]
        assert lib.redux_crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)
        assert rx.crc32_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(data)
    assert lib.redux_crc32_combine(0x12345678, 0, 0) == 0x12345678
    for n in (1, 4096, 1 << 20, (1 << 28) + 3):  # long zero runs (zlib: crc32 of the zeros computed piecewise)
        z = 0
        left = n
        while left:
            k = min(left, 1 << 24)
            z = zlib.crc32(bytes(k), z)
            left -= k
        want = zlib.crc32(b"abc")
        left = n
        while left:
            k = min(left, 1 << 24)
            want = zlib.crc32(bytes(k), want)
            left -= k
        assert lib.redux_crc32_combine(zlib.crc32(b"abc"), z, n) == want


# ---- container ---------------------------------------------------------------------------------------------------------
def _fake(ver_model, nblocks_data=3):
    """a container built by pack() from made-up streams (no GPU): (blob, crcs)"""
    import redux_amd as rx
    from redux_amd import container
    B = 100
    total = B * (nblocks_data - 1) + 37
    nb = nblocks_data
    sizes = np.arange(1, nb + 1, dtype=np.uint64) * 3
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    streams = np.arange(int(offs[-1]), dtype=np.uint64).astype(np.uint8)
    crc = (np.arange(nb, dtype=np.uint64) * 0x9E3779B1 + 5).astype(np.uint32)
    params, E = (8, 30, 32), 1
    if ver_model == "planes":
        E = 4
    elif ver_model == "static":
        cum = np.arange(258, dtype=np.uint32) * 4
        params = rx.StaticModel(rx.Parameters(8, 30, 32), cum)
    return container.pack(streams, offs, params, B, total, E, block_crc=crc), crc, streams, offs, B, total


@pytest.mark.parametrize("kind,ver", [("adaptive", 0x11), ("planes", 0x12), ("static", 0x13)])
def test_pack_unpack_block_crcs(kind, ver):
    from redux_amd import container
    blob, crc, streams, offs, B, total = _fake(kind)
    assert blob[4] == ver
    P, bs, tot, o, payload = container.unpack(blob)
    assert (bs, tot) == (B, total) and list(o) == list(offs)
    assert payload.tobytes() == streams[: int(offs[-1])].tobytes()
    assert list(container.block_crcs(blob)) == list(crc)
    assert container.header_is_wellformed(blob)
    assert container.element_size(blob) == (4 if kind == "planes" else 1)
    assert (container.static_table(blob) is not None) == (kind == "static")
    plain = container.pack(streams, offs, (8, 30, 32), B, total)
    assert container.block_crcs(plain) is None


def test_truncated_crc_table_is_eof():
    import redux_amd as rx
    from redux_amd import container
    blob, crc, *_ = _fake("adaptive")
    cut = container.HEADER.size + 4 * len(crc) + 4 * 2  # inside the CRC table
    with pytest.raises(rx.Eof):
        container.unpack(blob[:cut])
    with pytest.raises(rx.Eof):
        container.block_crcs(blob[:cut])


@pytest.mark.parametrize("ver", [0x10, 0x14, 0x91, 0x21])
def test_bad_flagged_versions_rejected(ver):
    import redux_amd as rx
    from redux_amd import container
    blob, *_ = _fake("adaptive")
    bad = blob[:4] + bytes([ver]) + blob[5:]
    with pytest.raises(rx.InvalidInput):
        container.unpack(bad)
    assert not container.header_is_wellformed(bad)


def test_unflagged_pack_is_unchanged():
    from redux_amd import container
    blob, crc, streams, offs, B, total = _fake("adaptive")
    a = container.pack(streams, offs, (8, 30, 32), B, total)
    b = container.pack(streams, offs, (8, 30, 32), B, total, block_crc=None)
    assert a == b and a[4] == 1


def test_cli_checksum_needs_block_size(tmp_path):
    src = tmp_path / "in.bin"
    src.write_bytes(b"hello" * 100)
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", "--checksum", "-i", str(src), "-o",
                        str(tmp_path / "out")], cwd=ROOT, capture_output=True)
    assert r.returncode == 1 and b"Usage" in r.stderr
    r = subprocess.run([sys.executable, "-m", "redux_amd.cli", "-c", "--checksum", "--block-size", "0", "-i", str(src), "-o",
                        str(tmp_path / "out")], cwd=ROOT, capture_output=True)
    assert r.returncode == 1 and b"Usage" in r.stderr
