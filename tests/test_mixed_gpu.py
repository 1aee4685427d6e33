"""The mixed layouts (include/redux_hip.h, "mixed layouts") on the GPU: the transform against the splice of the eight
whole-buffer transforms, the choice against its restatement on the same bits, the coded streams against the streams of the
spliced transform, the round trips (host-pointer pair, device objects, several chunks), checksums, damaged streams, and
container version 10 / `--layout mixed` end to end."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from test_mixed_cpu import B as B64K, choose_ref, mixed_input, mixed_ref
from test_planes_gpu import FILL, guarded, guards_intact, split, typed

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
UNIT = 8


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib(rx):
    from redux_amd import _lib
    return _lib


def tables(nunits):
    """all-k for each k, arange % 8, a reversed order, and bytes with high bits set (taken & 7)"""
    out = [np.full(nunits, k, dtype=np.uint8) for k in range(8)]
    out.append((np.arange(nunits) % 8).astype(np.uint8))
    out.append((7 - np.arange(nunits) % 8).astype(np.uint8))
    out.append(((np.arange(nunits) * 5 + 3) % 8 | 0xF8).astype(np.uint8))
    out.append(((np.arange(nunits) % 8) | (np.arange(nunits) * 8 % 256 & 0xF8)).astype(np.uint8))
    return out


def lengths(B):
    return [0, 1, 8 * B - 1, 8 * B, 8 * B + 1, 3 * 8 * B + 5 * B + 7]


def whole(rx, torch, d_x, B):
    """the eight whole-buffer transforms of d_x on the device, as host arrays"""
    return [(rx.delta_planes if k >= 4 else rx.planes)(d_x, 1 << (k & 3), B).cpu().numpy() for k in range(8)]


def splice(outs, table, n, B):
    U = UNIT * B
    want = np.empty(n, dtype=np.uint8)
    for u in range(-(-n // U)):
        want[u * U: (u + 1) * U] = outs[int(table[u]) & 7][u * U: (u + 1) * U]
    return want


def splice_and_back(rx, torch, x, d_x, outs, table, B):
    """the transform under `table` is the splice, its inverse returns x, and neither writes outside its buffer"""
    n = len(x)
    want = splice(outs, table, n, B)
    tg, d_y = guarded(torch, n)
    rx.mixed_layout(d_x, table, B, out=d_y)
    got = d_y.cpu().numpy()
    assert np.array_equal(got, want), (B, n, table.tolist())
    assert guards_intact(tg, n)
    tg, d_back = guarded(torch, n)
    rx.mixed_layout(d_y, torch.from_numpy(table).cuda(), B, inverse=True, out=d_back)
    assert np.array_equal(d_back.cpu().numpy(), x), (B, n, table.tolist())
    assert guards_intact(tg, n)


# ---- the transform ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [16, 48, 256, 4096, 40, 1000])
def test_mixed_layout_is_the_splice_of_the_whole_buffer_transforms(rx, lib, B):
    import torch
    fast = B % 16 == 0
    for n in lengths(B):
        x = typed(n, seed=B + n % 7) if n else np.zeros(0, dtype=np.uint8)
        d_x = torch.from_numpy(x).cuda()
        outs = whole(rx, torch, d_x, B)
        nunits = rx.mixed_units(n, B)
        assert nunits == max(1, -(-n // (8 * B)))
        for inverse in (False, True):
            name = lib.lib().redux_mixed_kernel_name(n, B, int(inverse)).decode()
            i = int(inverse)
            want_name = "" if n == 0 else "k_mixed_bytes<%d>" % i if not fast or n < 8 * B else \
                "k_mixed_planes<%d>" % i if n % (8 * B) == 0 else "k_mixed_planes<%d> + k_mixed_bytes<%d>" % (i, i)
            assert name == want_name, (n, B, inverse)
        for table in tables(nunits):
            splice_and_back(rx, torch, x, d_x, outs, table, B)
        if n == lengths(B)[-1]:  # the restatement of the rule agrees with the splice of the device's transforms
            t = tables(nunits)[8]
            assert np.array_equal(splice(outs, t, n, B), mixed_ref(x, t, B))


def test_several_workgroups_per_unit_and_rows_past_the_frame_end(rx):
    """B = 32816: 2051 groups per frame, 9 workgroups per unit; E = 1 behind the filter takes a second round of 8 rows of
    which 3 groups are live, E = 8 nine iterations with a ragged last wave"""
    import torch
    B = 32816
    for n in (8 * B, 2 * 8 * B, 2 * 8 * B + 5 * B + 7):
        x = typed(n, seed=B + n % 7)
        d_x = torch.from_numpy(x).cuda()
        outs = whole(rx, torch, d_x, B)
        for table in tables(rx.mixed_units(n, B)):
            splice_and_back(rx, torch, x, d_x, outs, table, B)


def test_sixteen_workgroups_per_unit(rx):
    """B = 65536, the block size of the workload: 4096 groups per frame, 16 workgroups per unit"""
    import torch
    B = 65536
    n = 2 * 8 * B
    x = typed(n, seed=B)
    d_x = torch.from_numpy(x).cuda()
    outs = whole(rx, torch, d_x, B)
    for table in tables(2)[8:10]:
        splice_and_back(rx, torch, x, d_x, outs, table, B)


@pytest.mark.parametrize("so,do", [(1, 0), (0, 15), (15, 1)])
def test_unaligned_buffers_take_the_general_path(rx, lib, so, do):
    import torch
    B = 256
    n = 3 * 8 * B + 5 * B + 7
    x = typed(n, seed=so * 16 + do)
    ts, d_x = guarded(torch, n, so)
    d_x.copy_(torch.from_numpy(x))
    aligned = torch.from_numpy(x).cuda()
    outs = whole(rx, torch, aligned, B)
    for table in tables(4)[8:]:
        want = splice(outs, table, n, B)
        td, d_y = guarded(torch, n, do)
        assert rx.api.mixed_kernel_name(d_x, d_y, B) == "k_mixed_bytes<0>"
        assert rx.api.mixed_kernel_name(aligned, aligned, B) == "k_mixed_planes<0> + k_mixed_bytes<0>"
        rx.mixed_layout(d_x, table, B, out=d_y)
        assert np.array_equal(d_y.cpu().numpy(), want) and guards_intact(td, n, do) and guards_intact(ts, n, so)
        tb, d_back = guarded(torch, n, so)
        assert rx.api.mixed_kernel_name(d_y, d_back, B, inverse=True) == "k_mixed_bytes<1>"
        rx.mixed_layout(d_y, table, B, inverse=True, out=d_back)
        assert np.array_equal(d_back.cpu().numpy(), x) and guards_intact(tb, n, so)


def test_the_grid_walks_1024_units(rx):
    import torch
    B, nunits = 16, 1024
    n = nunits * 8 * B
    x = typed(n, seed=9)
    d_x = torch.from_numpy(x).cuda()
    outs = whole(rx, torch, d_x, B)
    rng = np.random.default_rng(3)
    for table in (tables(nunits)[8], rng.integers(0, 256, nunits, dtype=np.uint8)):
        d_y = rx.mixed_layout(d_x, table, B)
        assert np.array_equal(d_y.cpu().numpy(), splice(outs, table, n, B))
        assert np.array_equal(rx.mixed_layout(d_y, table, B, inverse=True).cpu().numpy(), x)


def test_mixed_layout_refusals(rx, lib):
    import torch
    L = lib.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    o = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    t = torch.zeros(8, dtype=torch.uint8, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda src, dst, n, B, tab: L.redux_mixed_layout_dev(src, dst, n, B, tab, 0, s)  # noqa: E731
    assert call(d.data_ptr(), o.data_ptr(), 4096, 0, t.data_ptr()) == lib.INVALID_INPUT
    assert call(d.data_ptr(), o.data_ptr(), 4096, (1 << 30) + 1, t.data_ptr()) == lib.INVALID_INPUT
    assert call(d.data_ptr(), o.data_ptr(), 4096, 64, None) == lib.INVALID_INPUT
    assert call(d.data_ptr(), d.data_ptr(), 4096, 64, t.data_ptr()) == lib.INVALID_INPUT  # in place
    assert call(None, o.data_ptr(), 4096, 64, t.data_ptr()) == lib.INVALID_INPUT
    assert call(None, None, 0, 64, t.data_ptr()) == lib.OK
    with pytest.raises(rx.InvalidInput):
        rx.mixed_layout(d, np.zeros(7, np.uint8), 64)  # 8 units
    assert L.redux_mixed_unit_count(4096, 0) == 0 and L.redux_mixed_unit_count(0, 64) == 1
    assert L.redux_mixed_unit_count(64 * 8 + 1, 64) == 2
    torch.cuda.synchronize()


# ---- the choice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 8, 19, 2051])
def test_choice_equals_the_restatement_on_the_same_bits(rx, nb):
    rng = np.random.default_rng(nb)
    bits = rng.uniform(100.0, 500000.0, (8, nb))
    bits[5] = bits[1]                                   # exact ties -> the lower k
    bits[2, : nb // 2] = bits[6, : nb // 2]
    bits[1, ::3] *= 0.5                                 # (so that the tied rows win some units)
    bits[5, ::3] = bits[1, ::3]
    for mask in (0xFF, 0x81, 0x22):
        table, total = rx.choose_unit_layouts(bits, mask)
        want, S = choose_ref(bits, mask)
        assert table.dtype == np.uint8 and table.tolist() == want.tolist(), (nb, mask)
        restated = float(sum(S[want[u], u] for u in range(len(want))))
        assert abs(total - restated) <= nb * 2.0 ** -10, (nb, mask, total, restated)
    assert 5 not in rx.choose_unit_layouts(bits)[0] and not (rx.choose_unit_layouts(bits, 0x22)[0] != 1).any()
    with pytest.raises(rx.InvalidInput):
        rx.choose_unit_layouts(bits, 0)
    with pytest.raises(rx.InvalidInput):
        rx.choose_unit_layouts(bits[:7])


def test_choice_on_the_device_costs_of_a_mixed_file(rx):
    x = mixed_input("concat")[: 40 * B64K + 777]        # 41 blocks: timestamps (32), bf16 (8 and a short one)
    bits = rx.layout_cost(x, B64K, P)
    table, total = rx.choose_unit_layouts(bits)
    want, S = choose_ref(bits)
    assert table.tolist() == want.tolist() and table[:4].tolist() == [7] * 4 and table[4] in (1, 2, 3)
    est = rx.estimate_layouts(x, B64K, P, mixed=True)
    assert est["mixed"] == int(np.ceil(total / 8 + rx.api.TERMINATION_BYTES * 41)) and est["mixed"] < min(
        v for k, v in est.items() if k != "mixed")
    assert list(est)[:8] == list(rx.LAYOUTS) and rx.estimate_layouts(x, B64K, P) == {k: est[k] for k in rx.LAYOUTS}


# ---- coding -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coded(B, n, seed):
    """(x, table, streams, offsets) of one dictated call, shared by the tests below"""
    import redux_amd as rx
    x = typed(n, seed=seed)
    nunits = rx.mixed_units(n, B)
    table = ((np.arange(nunits) * 3 + 1) % 8).astype(np.uint8)
    out, offs, st = rx.compress_blocks(x, B, P, unit_layouts=table)
    assert not st.any()
    return x, table, out, offs


@pytest.mark.parametrize("B,n", [(4096, 19 * 4096 + 333), (1000, 8 * 1000 * 2 + 17), (256, 0)])
def test_dictated_streams_are_those_of_the_spliced_transform(rx, B, n):
    x, table, out, offs = coded(B, n, 5)
    want = rx.compress_blocks(mixed_ref(x, table, B), B, P)
    assert np.array_equal(out, want[0]) and np.array_equal(offs, want[1])
    back, sizes, st = rx.decompress_blocks(out, offs, B, P, length=n, unit_layouts=table)
    assert not st.any() and np.array_equal(back, x) and int(sizes.sum()) == n
    if n:
        bad = table.copy()
        bad[0] = 8
        with pytest.raises(rx.InvalidInput):
            rx.compress_blocks(x, B, P, unit_layouts=bad)
        with pytest.raises(rx.InvalidInput):
            rx.decompress_blocks(out, offs, B, P, length=n, unit_layouts=bad)
        with pytest.raises(rx.InvalidInput):
            rx.compress_blocks(x, B, P, unit_layouts=table[:-1])


def test_chosen_tables_round_trip_and_masks(rx):
    B = 4096
    x = np.concatenate([mixed_input("timestamps")[: 16 * B], mixed_input("bf16")[: 16 * B], mixed_input("bible")[: 11 * B + 5]])
    out, offs, st, table = rx.compress_blocks(x, B, P, unit_layouts=True)
    want, _ = choose_ref(rx.layout_cost(x, B, P))
    assert table.tolist() == want.tolist() and table[0] == table[1] == 7 and table[5] == 0
    dictated = rx.compress_blocks(x, B, P, unit_layouts=table)
    assert np.array_equal(out, dictated[0]) and np.array_equal(offs, dictated[1])
    back, _, st = rx.decompress_blocks(out, offs, B, P, length=len(x), unit_layouts=table)
    assert not st.any() and np.array_equal(back, x)
    plain = rx.compress_blocks(x, B, P)
    assert len(out) < 0.9 * len(plain[0])
    out2, offs2, _, table2 = rx.compress_blocks(x, B, P, unit_layouts=True, layouts=[(2, None), (2, "delta")])
    assert set(table2.tolist()) <= {1, 5}
    back, _, st = rx.decompress_blocks(out2, offs2, B, P, length=len(x), unit_layouts=table2)
    assert not st.any() and np.array_equal(back, x)
    out0, offs0, _, table0 = rx.compress_blocks(x, B, P, unit_layouts=True, layouts=0x01)
    assert not table0.any() and np.array_equal(out0, plain[0])


def test_device_objects_round_trip(rx):
    import torch
    B = 4096
    x = np.concatenate([mixed_input("timestamps")[: 16 * B], mixed_input("fp32")[: 8 * B], mixed_input("bible")[: 3 * B + 77]])
    n = len(x)
    d_in = torch.from_numpy(x).cuda()
    enc = rx.DeviceEncoder(P, B, n + 4 * B, mixed=True)
    out, offs, status, summary, d_table = enc.encode(d_in)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0] and d_table.dtype == torch.uint8 and d_table.numel() == rx.mixed_units(n, B)
    table = d_table.cpu().numpy()
    want = rx.compress_blocks(x, B, P, unit_layouts=True)
    total = int(offs[-1])
    assert table.tolist() == want[3].tolist() and np.array_equal(out[:total].cpu().numpy(), want[0])
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want[1])
    dec = rx.DeviceDecoder(P, B, len(want[1]) + 3, mixed=True)
    d_out, sizes, dstatus, dsum = dec.decode(out[:total].clone(), offs.clone(), length=n, unit_layouts=d_table.clone())
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and np.array_equal(d_out.cpu().numpy(), x)
    # a dictated table through the encoder object
    forced = ((np.arange(len(table)) + 2) % 8).astype(np.uint8)
    out, offs, status, summary, d_table = enc.encode(d_in, unit_layouts=torch.from_numpy(forced).cuda())
    torch.cuda.synchronize()
    want = rx.compress_blocks(x, B, P, unit_layouts=forced)
    assert d_table.cpu().numpy().tolist() == forced.tolist() and np.array_equal(out[: int(offs[-1])].cpu().numpy(), want[0])
    with pytest.raises(rx.InvalidInput):
        dec.decode(out[: int(offs[-1])], offs, length=n)
    for kw in ({"element_size": 2}, {"filter": "delta"}, {"base": d_in}, {"constant": True}):
        with pytest.raises(rx.InvalidInput):
            rx.DeviceEncoder(P, B, n, mixed=True, **kw)
        with pytest.raises(rx.InvalidInput):
            rx.DeviceDecoder(P, B, 64, mixed=True, **kw)


def test_several_chunks_give_the_single_chunk_result_and_crcs(rx):
    B = 1024
    x = np.concatenate([mixed_input("timestamps")[: 100 * B], mixed_input("bf16")[: 100 * B], mixed_input("bible")[: 71 * B + 333]])
    nb = 272
    want_crc = np.array([zlib.crc32(x[b * B: (b + 1) * B].tobytes()) for b in range(nb)], dtype=np.uint32)
    crc = np.zeros(nb, dtype=np.uint32)
    want = rx.compress_blocks(x, B, P, unit_layouts=True, block_crc=crc)
    assert np.array_equal(crc, want_crc) and rx.host_chunk_plan(nb, B)[1] == 1
    nocrc = rx.compress_blocks(x, B, P, unit_layouts=True)
    assert np.array_equal(nocrc[0], want[0]) and np.array_equal(nocrc[3], want[3])
    assert len(set(want[3].tolist())) >= 2
    try:
        rx.host_set_chunk_bytes(1, 1)  # 64 blocks a chunk
        assert rx.host_chunk_plan(nb, B)[1] >= 4
        crc2 = np.zeros(nb, dtype=np.uint32)
        got = rx.compress_blocks(x, B, P, unit_layouts=True, block_crc=crc2)
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(crc2, want_crc)
        forced = rx.compress_blocks(x, B, P, unit_layouts=want[3])
        assert np.array_equal(forced[0], want[0]) and np.array_equal(forced[1], want[1])
        crc3 = np.zeros(nb, dtype=np.uint32)
        back, _, st = rx.decompress_blocks(got[0], got[1], B, P, length=len(x), unit_layouts=got[3], block_crc=crc3)
        assert not st.any() and np.array_equal(back, x) and np.array_equal(crc3, want_crc)
    finally:
        rx.host_set_chunk_bytes(0, 0)
    crc4 = np.zeros(nb, dtype=np.uint32)
    back, _, st = rx.decompress_blocks(want[0], want[1], B, P, length=len(x), unit_layouts=want[3], block_crc=crc4)
    assert not st.any() and np.array_equal(back, x) and np.array_equal(crc4, want_crc)


def test_damaged_streams_mark_their_blocks_and_stay_in_bounds(rx, lib):
    import torch
    B = 4096
    n = 19 * B + 333
    x, table, out, offs = coded(B, n, 5)
    streams = split(out, offs)
    nb = len(streams)
    assert nb == 20
    bad = list(streams)
    bad[3] = streams[-1]                         # a valid stream of the wrong length
    bad[9] = streams[9][: len(streams[9]) // 3]  # truncated
    bad[nb - 1] = streams[nb - 1][:2]            # the short last unit: truncated
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.int64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    L = lib.lib()
    cp = lib.Params(*P)
    wsb = L.redux_decode_mixed_workspace_bytes(C.byref(cp), n, B)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    ws_ptr = ws.data_ptr() + (-ws.data_ptr()) % 256
    d_data = torch.from_numpy(data.copy()).cuda()
    d_offs = torch.from_numpy(boffs).cuda()
    d_table = torch.from_numpy(table).cuda()
    U = 8 * B
    for off in (0, 5):
        tg, d_out = guarded(torch, n, off)
        sizes = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        status = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        summary = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        st = L.redux_decode_mixed_dev(C.byref(cp), C.c_void_p(d_data.data_ptr()), C.c_void_p(d_offs.data_ptr()),
                                      C.c_void_p(d_table.data_ptr()), n, B, C.c_void_p(d_out.data_ptr()),
                                      C.c_void_p(sizes.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(summary.data_ptr()),
                                      C.c_void_p(ws_ptr), wsb, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == lib.OK
        torch.cuda.synchronize()
        s = status.cpu().numpy()
        assert s[3] == lib.INVALID_INPUT and [b for b in range(nb) if s[b] != lib.OK] == [3, 9, nb - 1]
        assert summary.cpu().tolist()[1] == 3
        assert guards_intact(tg, n, off)
    # the host-pointer call: the same statuses, only out[0 .. n) written
    hout = np.full(n + 64, FILL, dtype=np.uint8)
    hs = np.zeros(nb, dtype=np.uint32)
    hst = np.zeros(nb, dtype=np.int32)
    hoffs = boffs.astype(np.uint64)
    rc = L.redux_decode_blocks_mixed(C.byref(cp), data.ctypes.data, hoffs.ctypes.data, table.ctypes.data, n, B, hout.ctypes.data,
                                     hs.ctypes.data, hst.ctypes.data, None)
    assert rc != lib.OK and [b for b in range(nb) if hst[b] != lib.OK] == [3, 9, nb - 1]
    assert (hout[n:] == FILL).all()
    # units 0 and 1 hold a damaged block each, unit 2 the truncated last one: nothing is clean here; a run with one
    # damaged unit leaves the others whole
    bad = list(streams)
    bad[9] = streams[9][: len(streams[9]) // 3]
    data = np.frombuffer(b"".join(bad), dtype=np.uint8)
    boffs = np.zeros(nb + 1, dtype=np.uint64)
    boffs[1:] = np.cumsum([len(s) for s in bad])
    back, _, st = rx.decompress_blocks(data, boffs, B, P, check=False, length=n, unit_layouts=table)
    assert [b for b in range(nb) if st[b] != lib.OK] == [9]
    assert np.array_equal(back[:U], x[:U]) and np.array_equal(back[2 * U:], x[2 * U:])


def test_entry_point_refusals(rx, lib):
    import torch
    L = lib.lib()
    cp = lib.Params(*P)
    n, B = 8192, 1024
    d = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    t = torch.zeros(1, dtype=torch.uint8, device="cuda:0")
    wsb = L.redux_encode_mixed_workspace_bytes(C.byref(cp), n, B)
    assert wsb > L.redux_encode_workspace_bytes(C.byref(cp), n, B) + n
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device="cuda:0")
    out = torch.empty(L.redux_encode_bound(C.byref(cp), n, B), dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(9, dtype=torch.int64, device="cuda:0")
    st = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    sm = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def enc(block_size, mask, table, params=cp):
        return L.redux_encode_mixed_dev(C.byref(params), d.data_ptr(), n, block_size, mask, table, out.data_ptr(), out.numel(),
                                        offs.data_ptr(), st.data_ptr(), sm.data_ptr(), ws.data_ptr() + (-ws.data_ptr()) % 256, wsb, s)
    assert enc(0, 0xFF, t.data_ptr()) == lib.INVALID_INPUT
    assert enc((1 << 30) + 1, 0xFF, t.data_ptr()) == lib.INVALID_INPUT
    assert enc(B, 0x100, t.data_ptr()) == lib.INVALID_INPUT
    assert enc(B, 0xFF, None) == lib.INVALID_INPUT
    assert enc(B, 0xFF, t.data_ptr(), lib.Params(12, 14, 16)) == lib.UNSUPPORTED  # as redux_block_cost_dev
    assert enc(B, 0xFF, t.data_ptr()) == lib.OK
    torch.cuda.synchronize()
    assert sm.tolist() == [0, 0]
    bits = torch.zeros((8, 8), dtype=torch.float64, device="cuda:0")
    assert L.redux_mixed_choose_dev(bits.data_ptr(), 8, 0, t.data_ptr(), None, s) == lib.INVALID_INPUT
    assert L.redux_mixed_choose_dev(bits.data_ptr(), 8, 0x100, t.data_ptr(), None, s) == lib.INVALID_INPUT
    assert L.redux_mixed_choose_dev(bits.data_ptr(), 8, 0xFF, None, None, s) == lib.INVALID_INPUT
    assert L.redux_mixed_choose_dev(bits.data_ptr(), 8, 0xFF, t.data_ptr(), None, s) == lib.OK
    x = np.zeros(n, dtype=np.uint8)
    tab = np.array([8], dtype=np.uint8)
    ho = np.zeros(out.numel(), dtype=np.uint8)
    hoffs = np.zeros(9, dtype=np.uint64)
    assert L.redux_encode_blocks_mixed(C.byref(cp), x.ctypes.data, n, B, 0, tab.ctypes.data, ho.ctypes.data, ho.size,
                                       hoffs.ctypes.data, None, None) == lib.INVALID_INPUT
    assert L.redux_encode_blocks_mixed(C.byref(cp), x.ctypes.data, n, B, 0x100, tab.ctypes.data, ho.ctypes.data, ho.size,
                                       hoffs.ctypes.data, None, None) == lib.INVALID_INPUT
    torch.cuda.synchronize()


# ---- container and CLI ----------------------------------------------------------------------------------------------
def test_container_of_the_mixed_file_against_estimate_and_auto(rx):
    from redux_amd import container
    data = mixed_input("concat").tobytes()
    nb = 96
    nunits = 12
    bound = 2 * nb + 1
    est = container.estimate_layout_bytes(data, B64K, P, None, mixed=True)
    mixed = container.compress_bytes(data, B64K, P, None, layout="mixed")
    auto = container.compress_bytes(data, B64K, P, None, layout="auto")
    print("mixed: estimate %d, written %d; auto written %d; ratio %.4f" % (est["mixed"], len(mixed), len(auto), len(mixed) / len(auto)))
    assert mixed[4] == 0x0A and container.element_size(mixed) is None and container.filter(mixed) is None
    table = container.unit_layouts(mixed)
    assert len(table) == nunits and table[:4].tolist() == [7] * 4 and table[10:].tolist() == [0, 0]
    assert container.unit_layouts(auto) is None
    assert abs(len(mixed) - est["mixed"]) <= bound
    assert len(mixed) <= len(auto) + nunits + 2 * bound
    assert len(mixed) <= 0.91 * len(auto)
    assert container.decompress_bytes(mixed) == data
    assert {k: v for k, v in est.items() if k != "mixed"} == container.estimate_layout_bytes(data, B64K, P, None)
    # --element-size 2: every unit plain or delta at that size
    two = container.compress_bytes(data, B64K, P, 2, checksum=True, layout="mixed")
    assert two[4] == 0x1A and set(container.unit_layouts(two).tolist()) <= {1, 5}
    assert container.decompress_bytes(two) == data
    want = np.array([zlib.crc32(data[b * B64K: (b + 1) * B64K]) for b in range(nb)], dtype=np.uint32)
    assert np.array_equal(container.block_crcs(two), want)
    # a checksum that does not match is caught
    bad = bytearray(two)
    bad[container.HEADER.size + 4 * nb] ^= 1
    with pytest.raises(rx.InvalidInput):
        container.decompress_bytes(bytes(bad))
    # an empty input: one unit with layout 0
    empty = container.compress_bytes(b"", B64K, P, None, layout="mixed")
    assert empty[4] == 0x0A and container.unit_layouts(empty).tolist() == [0] and container.decompress_bytes(empty) == b""


def test_cli_end_to_end(rx, tmp_path):
    from redux_amd import cli, container
    data = mixed_input("shifted").tobytes()[: 30 * B64K + 4321]
    src, packed, back = tmp_path / "ckpt.bin", tmp_path / "ckpt.rdx", tmp_path / "ckpt.out"
    src.write_bytes(data)
    assert cli.main(["-c", "--block-size", "65536", "--layout", "mixed", "-i", str(src), "-o", str(packed)]) == 0
    buf = packed.read_bytes()
    assert buf[4] == 0x0A and len(container.unit_layouts(buf)) == 4
    assert buf == container.compress_bytes(data, B64K, P, None, layout="mixed")
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == data
    assert cli.main(["-c", "--block-size", "65536", "--layout", "mixed", "--checksum", "--element-size", "2", "-i", str(src),
                     "-o", str(packed)]) == 0
    buf = packed.read_bytes()
    assert buf[4] == 0x1A and set(container.unit_layouts(buf).tolist()) <= {1, 5}
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == data
    assert cli.main(["-c", "--block-size", "65536", "--layout", "mixed", "--filter", "delta", "-i", str(src), "-o", str(packed)]) == 1
    src.write_bytes(b"")
    assert cli.main(["-c", "--block-size", "65536", "--layout", "mixed", "-i", str(src), "-o", str(packed)]) == 0
    buf = packed.read_bytes()
    assert buf[4] == 0x0A and container.unit_layouts(buf).tolist() == [0]
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == b""
