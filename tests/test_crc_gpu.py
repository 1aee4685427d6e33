"""Per-block CRC-32 on the device: k_crc32 against zlib (block sizes, lengths, alignments, data), the decoder-layout form, the
six `_crc` coding calls against their siblings and zlib (small chunks, two contexts on one device), the checksummed
container and CLI, and the block swap that only the checksum catches."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5
CORPUS = [os.path.join(GOLDEN, "corpora", "canterbury", f) for f in ("alice29.txt", "kennedy.xls")] + \
         [os.path.join(GOLDEN, "corpora", "calgary", "obj2")]


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def zcrc(data, B):
    data = bytes(data)
    if not data:
        return [0]
    return [zlib.crc32(data[o:o + B]) for o in range(0, len(data), B)]


def host_data(kind, n, seed):
    if kind == "iid":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    return np.full(n, 0x00 if kind == "zero" else 0xFF, dtype=np.uint8)


def on_device(x, off):
    """x at byte offset `off` of a device buffer framed by guard bytes"""
    import torch
    t = torch.full((len(x) + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    d = t[GUARD + off: GUARD + off + len(x)]
    if len(x):
        d.copy_(torch.from_numpy(np.ascontiguousarray(x)).cuda())
    return d


# ---- the kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 15, 16, 17, 1000, 1024, 1025, 4095, 65536, 65537, 1 << 20, 3 * (1 << 20) + 5])
def test_blocks_equal_zlib(rx, B):
    cap = 6 << 20
    for n in sorted({0, min(B - 1, cap), min(B, cap), min(3 * B + 7, cap), min(64 * B + B // 2, cap), 5000}):
        x = host_data("iid", n, seed=B + n)
        want = zcrc(x, B)
        for off in ((0, 1, 7, 15) if n < (1 << 20) else (0, 3)):
            got = rx.crc32_blocks(on_device(x, off), B)
            assert got.tolist() == want, (B, n, off)


@pytest.mark.parametrize("kind", ["zero", "ones"])
def test_constant_data(rx, kind):
    for B, n in ((1000, 50000), (65536, 3 * 65536 + 11), (1 << 20, (1 << 20) + 17)):
        x = host_data(kind, n, 0)
        assert rx.crc32_blocks(on_device(x, 5), B).tolist() == zcrc(x, B)


def test_every_base_offset(rx):
    x = host_data("iid", 70000, 3)
    for off in range(16):
        for B in (17, 4096, 65536):
            assert rx.crc32_blocks(on_device(x[:70000 - off], off), B).tolist() == zcrc(x[:70000 - off], B), (off, B)


def test_one_gib_block(rx):
    import torch
    n = 1 << 30
    d = rx.gen_iid(n)
    got = rx.crc32_blocks(d, n)
    want = 0
    for o in range(0, n, 1 << 27):
        want = zlib.crc32(d[o:o + (1 << 27)].cpu().numpy().tobytes(), want)
    assert got.tolist() == [want]
    got2 = rx.crc32_blocks(d[1:], n)  # unaligned, one byte short
    tail = zlib.crc32(d[n - (1 << 20):].cpu().numpy().tobytes())
    head = zlib.crc32(d[1:1 << 20].cpu().numpy().tobytes())
    mid = rx.crc32_blocks(d[1 << 20:n - (1 << 20)], n)[0]
    whole = rx.crc32_combine(rx.crc32_combine(head, mid, n - (2 << 20)), tail, 1 << 20)
    assert got2.tolist() == [whole]
    del d
    torch.cuda.empty_cache()


def test_sizes_form(rx):
    """the layout redux_decode_blocks_dev writes: block b at b*B, sizes[b] bytes, the rest of its room guard bytes"""
    import torch
    for B, nb in ((1000, 77), (65536, 9), (3 << 19, 3)):
        rng = np.random.default_rng(B)
        sizes = rng.integers(0, B + 1, nb).astype(np.uint32)
        sizes[0], sizes[-1] = B, 0
        buf = np.full(nb * B, FILL, dtype=np.uint8)
        want = []
        for b in range(nb):
            blk = rng.integers(0, 256, int(sizes[b]), dtype=np.uint8)
            buf[b * B: b * B + len(blk)] = blk
            want.append(zlib.crc32(blk.tobytes()))
        d = on_device(buf, 3)
        big = sizes.copy()
        big[1] = B + 1000  # clamped to B
        want_big = list(want)
        want_big[1] = zlib.crc32(buf[B:2 * B].tobytes())
        for s, w in ((sizes, want), (big, want_big)):
            ds = torch.from_numpy(s.view(np.int32)).cuda()
            assert rx.crc32_blocks(d, B, sizes=ds).tolist() == w, B


def test_host_pointer_call(rx):
    x = host_data("iid", 3 * (1 << 20) + 123, 5)
    for B in (1, 4095, 65536):
        if B == 1:
            y = x[:5000]
            assert rx.crc32_blocks(y, B).tolist() == zcrc(y, B)
        else:
            assert rx.crc32_blocks(x, B).tolist() == zcrc(x, B)
    assert rx.crc32_blocks(b"", 65536).tolist() == [0]
    rx.host_set_chunk_bytes(1, 1)
    try:
        assert rx.crc32_blocks(x, 65536).tolist() == zcrc(x, 65536)
    finally:
        rx.host_set_chunk_bytes(0, 0)


# ---- the coding calls ------------------------------------------------------------------------------------------------
def _check_calls(rx, data, B):
    want = zcrc(data, B)
    nb = len(want)
    forms = [("adaptive", {}, (8, 30, 32)), ("static", {}, rx.StaticModel.from_data(data, (8, 30, 32)))]
    forms += [(f"planes{E}", {"element_size": E}, (8, 30, 32)) for E in (2, 4, 8)]
    for name, kw, params in forms:
        crc = np.zeros(nb, dtype=np.uint32)
        o1, f1, s1 = rx.compress_blocks(data, B, params, **kw)
        o2, f2, s2 = rx.compress_blocks(data, B, params, block_crc=crc, **kw)
        assert o1.tobytes() == o2.tobytes() and f1.tolist() == f2.tolist() and s1.tolist() == s2.tolist(), name
        assert crc.tolist() == want, name
        dcrc = np.zeros(nb, dtype=np.uint32)
        dkw = dict(kw)
        if "element_size" in kw:
            dkw["length"] = len(data)
        a1 = rx.decompress_blocks(o1, f1, B, params, **dkw)
        a2 = rx.decompress_blocks(o1, f1, B, params, block_crc=dcrc, **dkw)
        assert all(np.array_equal(p, q) for p, q in zip(a1, a2)), name
        assert dcrc.tolist() == want, name


def test_coding_calls(rx):
    data = open(CORPUS[0], "rb").read() + bytes(range(256)) * 300
    _check_calls(rx, data, 65536)
    _check_calls(rx, data[:70001], 4096)


def test_coding_calls_small_chunks_and_two_contexts(rx):
    data = rx.gen_zipf(64 * 4096 * 3 + 999, seed=3).cpu().numpy().tobytes()
    rx.host_set_chunk_bytes(1, 1)
    try:
        _check_calls(rx, data, 4096)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    rx.host_set_devices([0, 0])
    try:
        rx.host_set_chunk_bytes(1, 1)
        _check_calls(rx, data, 4096)
    finally:
        rx.host_set_chunk_bytes(0, 0)
        rx.host_set_devices([])


# ---- container and CLI -----------------------------------------------------------------------------------------------
def _swap_blocks(blob, i, j):
    """swap the payloads and size entries of blocks i < j of a container (version 1 / 0x11)"""
    from redux_amd import container
    hdr = container.HEADER.unpack_from(blob, 0)
    nb = hdr[7]
    start = container.HEADER.size
    sizes = list(struct.unpack_from(f"<{nb}I", blob, start))
    pay = start + 4 * nb + (4 * nb if blob[4] & 0x10 else 0)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    parts = [blob[pay + offs[b]: pay + offs[b + 1]] for b in range(nb)]
    parts[i], parts[j] = parts[j], parts[i]
    sizes[i], sizes[j] = sizes[j], sizes[i]
    return blob[:start] + struct.pack(f"<{nb}I", *sizes) + blob[start + 4 * nb: pay] + b"".join(parts)


@pytest.mark.parametrize("kind", ["adaptive", "static", 2, 4, 8])
def test_container_round_trip(rx, kind):
    from redux_amd import container
    synth = rx.gen_zipf(5 * 65536 + 77, seed=11).cpu().numpy().tobytes()
    for data in [open(p, "rb").read() for p in CORPUS] + [synth, b"", b"x"]:
        kw = {"model": "static"} if kind == "static" else {"element_size": kind} if isinstance(kind, int) else {}
        blob = container.compress_bytes(data, 65536, (8, 30, 32), checksum=True, **kw)
        assert blob[4] & 0x10
        assert container.block_crcs(blob).tolist() == zcrc(data, 65536)
        assert container.decompress_bytes(blob) == data
        plain = container.compress_bytes(data, 65536, (8, 30, 32), **kw)
        assert not plain[4] & 0x10 and container.block_crcs(plain) is None


def test_block_swap_is_caught_only_with_checksums(rx):
    from redux_amd import container
    data = open(os.path.join(GOLDEN, "corpora", "calgary", "book1"), "rb").read()[: 3 * 65536]  # three full blocks of text
    assert len(data) == 3 * 65536
    plain = container.compress_bytes(data, 65536)
    swapped = _swap_blocks(plain, 0, 2)
    out = container.decompress_bytes(swapped)  # decodes "OK" to the wrong content
    assert len(out) == len(data) and out != data
    checked = container.compress_bytes(data, 65536, checksum=True)
    with pytest.raises(rx.InvalidInput):
        container.decompress_bytes(_swap_blocks(checked, 0, 2))


def test_damaged_crc_table(rx):
    from redux_amd import container
    data = open(CORPUS[1], "rb").read()
    blob = bytearray(container.compress_bytes(data, 65536, checksum=True))
    nb = container.HEADER.unpack_from(blob, 0)[7]
    blob[container.HEADER.size + 4 * nb + 4 * (nb // 2) + 1] ^= 0x01
    with pytest.raises(rx.InvalidInput):
        container.decompress_bytes(bytes(blob))


def test_cli_checksum(rx, tmp_path, capsys):
    from redux_amd import cli, container
    data = open(CORPUS[0], "rb").read()
    src = tmp_path / "in"
    src.write_bytes(data)
    chk, plain, back = tmp_path / "chk", tmp_path / "plain", tmp_path / "back"
    assert cli.main(["-c", "--checksum", "--block-size", "65536", "-i", str(src), "-o", str(chk)]) == 0
    assert cli.main(["-c", "--block-size", "65536", "-i", str(src), "-o", str(plain)]) == 0
    assert chk.read_bytes()[4] == 0x11
    assert plain.read_bytes() == container.compress_bytes(data, 65536)  # opt-in: without --checksum nothing changes
    assert cli.main(["-d", "-i", str(chk), "-o", str(back)]) == 0
    assert back.read_bytes() == data
    capsys.readouterr()
    bad = tmp_path / "bad"
    bad.write_bytes(_swap_blocks(chk.read_bytes(), 0, 1))
    assert cli.main(["-d", "-i", str(bad), "-o", str(back)]) == 3
    err = capsys.readouterr().err
    assert err.startswith("Decompression error: ") and str(rx.InvalidInput()) in err
    assert cli.main(["-c", "--checksum", "-i", str(src), "-o", str(tmp_path / "x")]) == 1
