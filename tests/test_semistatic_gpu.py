"""Semi-static coding on the device: k_byte_hist against np.bincount, k_static_table against the host rule, the
host-pointer table call, the static host pipeline against the CPU oracle, damaged streams, the container / CLI with
--model static and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, corpus_files
from oracle import cbind as ox
from test_semistatic_cpu import rule_ref
from test_static_gpu import oracle_decode_raw, oracle_encode_blocks

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def device_hist(torch, lib, d, counts=None):
    if counts is None:
        counts = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    st = lib.lib().redux_histogram_dev(C.c_void_p(d.data_ptr()) if d.numel() else None, d.numel(),
                                       C.c_void_p(counts.data_ptr()), None, 0, stream_ptr(torch))
    assert st == lib.OK
    return counts


def data_of(kind, n, rx, torch, seed=1):
    if kind == "iid":
        return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    if kind == "zipf":
        return rx.gen_zipf(max(n, 1), seed=seed)[:n].cpu().numpy() if n else np.zeros(0, np.uint8)
    return np.full(n, 0x3C, dtype=np.uint8)


# ---- k_byte_hist --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["iid", "zipf", "one"])
def test_histogram_matches_bincount(rx, lib, kind):
    import torch
    for n in (0, 1, 15, 16, 17, 4095, (1 << 20) + 3):
        x = data_of(kind, n, rx, torch, seed=n + 1)
        want = np.bincount(x, minlength=256)
        for off in (0, 1, 4, 8):
            t = torch.full((n + 2 * GUARD + 16,), FILL, dtype=torch.uint8, device="cuda:0")
            d = t[GUARD + off: GUARD + off + n]
            if n:
                d.copy_(torch.from_numpy(x).cuda())
            counts = device_hist(torch, lib, d)
            torch.cuda.synchronize()
            assert counts.cpu().numpy().tolist() == want.tolist(), (kind, n, off)


def test_histogram_adds_up_over_calls(rx, lib):
    import torch
    x = rx.gen_zipf(3 << 20, seed=9)
    one = device_hist(torch, lib, x)
    two = device_hist(torch, lib, x[: 1234567])
    device_hist(torch, lib, x[1234567:], two)
    torch.cuda.synchronize()
    assert torch.equal(one, two)
    assert one.cpu().numpy().tolist() == np.bincount(x.cpu().numpy(), minlength=256).tolist()


def test_histogram_counts_are_64_bit(rx, lib):
    import torch
    n = (4 << 30) + (1 << 20)
    x = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    x[-1] = 7
    counts = device_hist(torch, lib, x).cpu().numpy()
    del x
    assert int(counts[0]) == n - 1 > 1 << 32 and int(counts[7]) == 1 and int(counts.sum()) == n


# ---- k_static_table and the host-pointer call ------------------------------------------------------------------------
def test_static_table_dev_matches_host_rule(rx, lib):
    import torch
    from test_semistatic_cpu import count_cases
    L = lib.lib()
    cases = dict(count_cases())
    for T in (257, 1000, 1 << 16, (1 << 16) + 1, (1 << 30) - 1):
        for name, counts in cases.items():
            d_counts = torch.from_numpy(counts.astype(np.int64)).cuda()
            d_cum = torch.full((258,), -1, dtype=torch.int32, device="cuda:0")
            cp = lib.Params(8, 30, 32)
            assert L.redux_static_table_dev(C.byref(cp), C.c_void_p(d_counts.data_ptr()), T, C.c_void_p(d_cum.data_ptr()),
                                            stream_ptr(torch)) == lib.OK
            got = d_cum.cpu().numpy().view(np.uint32)
            want = rule_ref(counts, T)
            if want is None:
                assert not got.any(), (name, T)  # the unsupported mark: a table of zeros
            else:
                assert got.tolist() == want.tolist() == rx.static_table_from_counts(counts, total=T).tolist(), (name, T)
    one_big = np.zeros(256, np.uint64)
    one_big[3] = 1 << 63                             # N < 2^64, N R >= 2^64
    all_max = np.full(256, (1 << 64) - 1, np.uint64)  # N itself beyond 64 bits: the 128-bit sum's high word
    cp = lib.Params(8, 30, 32)
    for counts, T in ((one_big, 1 << 16), (all_max, 1 << 16), (all_max, 257)):
        assert rule_ref(counts, T) is None
        d_counts = torch.from_numpy(counts.view(np.int64)).cuda()
        d_cum = torch.full((258,), -1, dtype=torch.int32, device="cuda:0")
        assert L.redux_static_table_dev(C.byref(cp), C.c_void_p(d_counts.data_ptr()), T, C.c_void_p(d_cum.data_ptr()),
                                        stream_ptr(torch)) == lib.OK
        assert not d_cum.cpu().numpy().any(), T  # the unsupported mark
        with pytest.raises(rx.Unsupported):
            rx.static_table_from_counts(counts, total=T)
    assert L.redux_static_table_dev(C.byref(cp), C.c_void_p(d_counts.data_ptr()), 256, C.c_void_p(d_cum.data_ptr()),
                                    stream_ptr(torch)) == lib.INVALID_INPUT


def test_host_and_device_tables_agree(rx):
    import torch
    for name, path in corpus_files("canterbury")[:4] + [("zipf", None)]:
        x = np.fromfile(path, dtype=np.uint8) if path else rx.gen_zipf(5 << 20, seed=3).cpu().numpy()
        want = rule_ref(np.bincount(x, minlength=256), 1 << 16)
        assert rx.static_table(x).tolist() == want.tolist(), name
        assert rx.static_table(torch.from_numpy(x).cuda()).tolist() == want.tolist(), name
        assert rx.static_table(x[1:], (8, 14, 16)).tolist() == rule_ref(np.bincount(x[1:], minlength=256), (1 << 14) - 1).tolist()
    x = rx.gen_zipf((9 << 20) + 77, seed=4).cpu().numpy()
    want = rx.static_table(x)
    try:
        rx.host_set_chunk_bytes(1, 1)  # 64 KiB chunks: 145 of them over the 8 slots
        assert rx.static_table(x).tolist() == want.tolist()
        assert rx.static_table(x[3:]).tolist() == rx.static_table_from_counts(np.bincount(x[3:], minlength=256)).tolist()
    finally:
        rx.host_set_chunk_bytes(0, 0)
    assert rx.static_table(b"").tolist() == list(range(258))


# ---- the static host pipeline ------------------------------------------------------------------------------------------
def split(out, offs):
    return [out[int(offs[i]): int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


@pytest.mark.parametrize("name,path", corpus_files("canterbury", "artificial")[:9])
def test_static_blocks_match_oracle(rx, name, path):
    x = np.fromfile(path, dtype=np.uint8)
    for bs in (4096, 65536):
        m = rx.StaticModel.from_data(x, (8, 30, 32))
        out, offs, st = rx.compress_blocks(x, bs, m)
        assert not st.any()
        want, woffs = oracle_encode_blocks(x, bs, m.cum, (8, 30, 32))
        assert offs.astype(np.int64).tolist() == woffs.tolist() and out.tobytes() == want, (name, bs)
        back, sizes, st2 = rx.decompress_blocks(out, offs, bs, m)
        assert not st2.any()
        assert b"".join(back[b * bs: b * bs + int(sizes[b])].tobytes() for b in range(len(sizes))) == x.tobytes()


def test_static_ragged_lengths_chunks_and_contexts(rx):
    bs = 4096
    rng = np.random.default_rng(5)
    base = rx.gen_zipf(40 * 64 * bs + 12345, seed=6).cpu().numpy()
    for n in (0, 1, bs - 1, bs + 1, 3 * bs + 17):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        m = rx.StaticModel.from_data(x)
        out, offs, _ = rx.compress_blocks(x, bs, m)
        want, woffs = oracle_encode_blocks(x, bs, m.cum, (8, 30, 32))
        assert out.tobytes() == want and offs.astype(np.int64).tolist() == woffs.tolist(), n
    m = rx.StaticModel.from_data(base)
    want = rx.compress_blocks(base, bs, m)
    try:
        rx.host_set_chunk_bytes(1, 1)  # 64 blocks a chunk
        assert rx.host_chunk_plan(len(want[1]) - 1, bs)[1] > 8
        for devices in ([], [0, 0]):
            rx.host_set_devices(devices)
            got = rx.compress_blocks(base, bs, m)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), devices
            back, sizes, st = rx.decompress_blocks(got[0], got[1], bs, m)
            assert not st.any() and np.array_equal(back[: len(base)], base), devices
    finally:
        rx.host_set_devices([])
        rx.host_set_chunk_bytes(0, 0)
    ref, _ = oracle_encode_blocks(base[: 5 * bs], bs, m.cum, (8, 30, 32))
    assert want[0][: int(want[1][5])].tobytes() == ref


def test_static_damaged_streams_match_oracle(rx, lib):
    bs = 4096
    x = np.fromfile(os.path.join(GOLDEN, "corpora", "canterbury", "alice29.txt"), dtype=np.uint8)[: 6 * bs]
    m = rx.StaticModel.from_data(x)
    out, offs, _ = rx.compress_blocks(x, bs, m)
    s = split(out, offs)
    bad = [s[0], s[1][: len(s[1]) // 2], b"", bytes([255] * 40), s[4][:-1], s[5] + b"\x00\x01"]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(len(bad) + 1, dtype=np.uint64)
    boffs[1:] = np.cumsum([len(b) for b in bad])
    got, sizes, status = rx.decompress_blocks(data, boffs, bs, m, check=False)
    for b, stream in enumerate(bad):
        want_st, want_bytes = oracle_decode_raw(stream, bs, m.cum, (8, 30, 32))
        assert int(status[b]) == want_st, b
        if want_st == lib.OK:
            assert int(sizes[b]) == len(want_bytes) and got[b * bs: b * bs + int(sizes[b])].tobytes() == want_bytes, b
    assert int(status[0]) == lib.OK and int(status[1]) != lib.OK


# ---- container, CLI, device coder, C++ mirror -----------------------------------------------------------------------
def test_container_and_cli_with_model_static(rx, tmp_path):
    from redux_amd import cli, container
    src = os.path.join(GOLDEN, "corpora", "large", "bible.txt")
    raw = open(src, "rb").read()
    st, ad, back = tmp_path / "s.rdxb", tmp_path / "a.rdxb", tmp_path / "back"
    assert cli.main(["-c", "-i", src, "-o", str(st), "--block-size", "65536", "--model", "static"]) == 0
    assert cli.main(["-c", "-i", src, "-o", str(ad), "--block-size", "65536"]) == 0
    sb, ab = st.read_bytes(), ad.read_bytes()
    assert sb[4] == 3 and ab[4] == 1
    assert container.static_table(sb).tolist() == rx.static_table(raw).tolist()
    assert cli.main(["-d", "-i", str(st), "-o", str(back)]) == 0
    assert back.read_bytes() == raw
    for data in (b"", b"x", raw[:65536 * 3 + 5]):
        assert container.decompress_bytes(container.compress_bytes(data, 65536, model="static")) == data
    assert cli.main(["-c", "-i", src, "-o", str(tmp_path / "x"), "--model", "static"]) == 1


def test_device_static_coder_from_data(rx):
    import torch
    bs = 65536
    d_in = rx.gen_zipf(64 * bs + 999, seed=12)
    coder = rx.DeviceStaticCoder.from_data(d_in, (8, 30, 32), bs, d_in.numel())
    assert coder.cum[257] == 65536
    out, offs, status, summary = coder.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    host = d_in.cpu().numpy()
    want = rx.compress_blocks(host, bs, rx.StaticModel((8, 30, 32), np.array(list(coder.cum), np.uint32)))
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want[1])
    assert out[: int(want[1][-1])].cpu().numpy().tobytes() == want[0].tobytes()
    d_out, sizes, st, dsum = coder.decode(out[: int(want[1][-1])], offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(d_out[: d_in.numel()], d_in)


def test_cpp_semistatic_mirror(rx, tmp_path):
    from test_semistatic_cpu import build_semistatic_mirror_test
    exe = build_semistatic_mirror_test(tmp_path)
    out = subprocess.run([exe, os.path.join(GOLDEN, "corpora", "canterbury", "lcet10.txt")], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "semistatic mirror ok" in out.stdout, out.stdout + out.stderr
