"""Byte planes, the delta filter and stored blocks on every adaptive coder instance below them (the table:
tests/test_layered_instances_cpu.py).

One launch per row of ROWS, through the `_dev` calls.  A case first asserts, by name, that the coder below the wrapper runs
the encode and decode instance the row promises, for the very pointer, length and workspace of the launch.  The input is
tiled on the device from a few distinct FRAMES (E blocks of typed data; frames are independent under every layer) and ends
in a ragged frame whose last block has an odd length; every distinct block of the numpy restatement of the transform
(planes_ref, delta_planes_ref) is coded once by the oracle.  Checked for EVERY block of every launch (the count is the
row's block count: 389, 1,093 or 2,565): offsets, statuses, the summary, for stored the flags (the rule over the oracle's
stream lengths), the stream bytes against the oracle's (a stored block: its transformed bytes); then the decode of the
device's own output equals the input byte for byte and the sizes are the layout's.  Input, encode output and decode output
lie between guard bands of 0xA5 that must stay untouched (the helpers of test_adaptive_instances_gpu, which place a buffer
a given number of bytes off a 16-byte boundary; test_stream_ranges_gpu's own cannot).
  * planes: bf16 / fp32 / int64 patterns; delta: integer series of test_delta_cpu's generators, cast to the element size;
  * stored: frames whose planes are incompressible (S) or skewed (C): group 0 of 64 blocks all coded, 1 all stored,
    2 alternating, 3 a single stored block, 4 a single coded block (group 0 alternates two coded frames, so that two
    neighbouring table entries never hold the same bytes), the rest mixed frame by frame; the ragged last block
    once stored and once coded.  The flag pattern is asserted.
Then: the host-pointer forms with CRCs in at least three chunks against the `_dev` result; k_planes / k_delta_planes /
k_delta_unplanes at block sizes whose frames end inside a wave's turn, and past 2^20 frames; damaged streams on the table
forms of k_decode_wave and k_decode<false, true> and under planes / delta on k_decode_cells<8>."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_adaptive_instances_gpu import FILL, GUARD, compare_rows, guarded, guards_intact
from test_delta_cpu import delta_planes_ref, sorted_i32, timestamps_i64, tones_i16
from test_layered_instances_cpu import (DELTA, PLANES, ROWS, STORED, input_len, layer_dec_name, layer_enc_name, layer_ws_bytes,
                                        copy_bytes, tail_len)
from test_planes_cpu import planes_ref
from test_planes_gpu import typed
from test_stored_cpu import rule

pytestmark = pytest.mark.gpu
INVALID_INPUT, TOO_SMALL = 2, 4


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def _lib():
    from redux_amd import _lib as L
    return L


def _v(t):
    return C.c_void_p(t.data_ptr())


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def transform(layer, x, E, B, inverse=False):
    if layer == DELTA:
        return delta_planes_ref(x, E, B, inverse=inverse)
    return planes_ref(x, E, B, inverse=inverse) if E > 1 else np.ascontiguousarray(x, np.uint8).copy()


# ---- the input: a few distinct frames -----------------------------------------------------------------------------------
def skewed(n, rng):
    return np.minimum(rng.standard_exponential(n) * 14, 255).astype(np.uint8)


def stored_frame(pattern, B, rng):
    """A frame of len(pattern) planes of B bytes, in ORIGINAL order: plane j uniform bytes ("S": the coder expands it) or
    skewed ones ("C", "c": two draws)."""
    planes = [rng.integers(0, 256, B, dtype=np.uint8) if c == "S" else skewed(B, rng) for c in pattern]
    return np.stack(planes, axis=1).reshape(-1)


def frames_of(layer, E, B, seed):
    """name -> frame (E * B bytes in original order)"""
    rng = np.random.default_rng(seed)
    F = E * B
    if layer == PLANES:
        return {f"typed{k}": typed(F, seed + k) for k in range(3)}
    if layer == DELTA:
        out = {}
        for name, gen, dt in (("timestamps", timestamps_i64, "<u8"), ("sorted", sorted_i32, "<u4"), ("tones", tones_i16, "<i2")):
            v = np.resize(gen().view(dt), B).astype(np.int64).astype("<u%d" % E)        # the series mod 2^(8E)
            out[name] = v.view(np.uint8).copy()
        return out
    pats = ["C" * E, "c" * E, "S" * E] + ([] if E == 1 else ["SC" * (E // 2), "S" + "C" * (E - 1), "C" + "S" * (E - 1)])
    return {p: stored_frame(p, B, rng) for p in pats}


def frame_plan(layer, E, nfull, names):
    """The frame of every full frame of the launch, by name."""
    if layer != STORED:
        return [names[f % len(names)] if f % 7 else names[(f // 7) % len(names)] for f in range(nfull)]
    per = 64 // E                                    # frames in a group of 64 blocks
    c, s = "C" * E, "S" * E
    one_s, one_c, alt = ("S" + "C" * (E - 1), "C" + "S" * (E - 1), "SC" * (E // 2)) if E > 1 else (s, c, None)
    plan = []
    for f in range(nfull):
        g, i = divmod(f, per)
        if g == 0:                                   # two coded frames in turn: neighbours in the table differ
            plan.append(c if i % 2 == 0 else c.lower())
        elif g == 1:
            plan.append(s)
        elif g == 2:
            plan.append(alt if alt else (s, c)[i % 2])
        elif g == 3:
            plan.append(one_s if i == per // 4 + 1 else c)
        elif g == 4:
            plan.append(one_c if i == per - 3 else s)
        else:
            plan.append((c, s, alt or s, c, one_s, one_c)[(f * 5 + g) % 6])
    return plan


class Launch:
    """The blocks of one launch and what the oracle makes of each distinct one."""

    def __init__(self, layer, params, E, B, nb, seed, ragged="C", slot=None):
        import torch
        self.layer, self.params, self.E, self.B, self.nb = layer, params, E, B, nb
        self.in_len = input_len(params, B, nb)
        F = E * B
        frames = frames_of(layer, E, B, seed)
        names = sorted(frames)
        nfull = self.in_len // F
        plan = frame_plan(layer, E, nfull, names)
        last_len = self.in_len - nfull * F
        assert 0 < last_len and nfull * E + -(-last_len // B) == nb
        if layer == STORED:
            rng = np.random.default_rng(seed + 99)
            last = rng.integers(0, 256, last_len, dtype=np.uint8) if ragged == "S" else skewed(last_len, rng)
        else:
            last = frames[names[1]][:last_len]
        # units: the distinct blocks of the transformed input; block b of the launch is unit self.unit[b]
        self.frames, self.names, self.plan, self.last = frames, names, plan, last
        t_blocks, self.raw_len = [], []
        for n in names:
            t = transform(layer, frames[n], E, B)
            t_blocks += [t[j * B: (j + 1) * B] for j in range(E)]
        t_last = transform(layer, last, E, B)
        t_blocks += [t_last[o: o + B] for o in range(0, last_len, B)]
        self.t_blocks = t_blocks
        at = {n: k * E for k, n in enumerate(names)}
        unit = [at[n] + j for n in plan for j in range(E)] + list(range(len(names) * E, len(t_blocks)))
        self.unit = np.array(unit, dtype=np.int64)
        assert len(unit) == nb
        slot = slot or 4 * B + 4096
        self.streams, self.lens = [], []
        for t in t_blocks:
            s, st = ox.compress_blocks(t, B, params, slot=slot)
            assert len(s) == 1 and not st.any()
            self.streams.append(s[0])
        L = [len(t) for t in t_blocks]
        self.flag = rule([0] * len(L), [len(s) for s in self.streams], L, 65536) if layer == STORED else np.zeros(len(L), bool)
        self.payload = [t.tobytes() if f else s for t, s, f in zip(t_blocks, self.streams, self.flag)]
        self.d_unit = torch.from_numpy(self.unit).cuda()

    def device_input(self, off):
        """(whole tensor, the input `off` bytes off a 16-byte boundary, its start in the tensor)"""
        import torch
        big, d_in, lo = guarded(self.in_len, off)
        F = self.E * self.B
        stack = torch.from_numpy(np.stack([self.frames[n] for n in self.names])).cuda()
        idx = torch.tensor([self.names.index(n) for n in self.plan], device="cuda:0")
        nfull = len(self.plan)
        d_in[: nfull * F].view(nfull, F).copy_(stack[idx])
        d_in[nfull * F:].copy_(torch.from_numpy(self.last.copy()))
        return big, d_in, lo

    def expected_offsets(self, payload=None):
        import torch
        lens = torch.tensor([len(p) for p in (payload or self.payload)], dtype=torch.int64, device="cuda:0")[self.d_unit]
        return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(lens, 0)])

    def block_lengths(self):
        n = np.full(self.nb, self.B, dtype=np.int64)
        n[-1] = self.in_len - (self.nb - 1) * self.B
        return n


def scatter_rows(flat, starts, data):
    import torch
    if not len(data) or not starts.numel():
        return
    e = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    ar = torch.arange(len(data), device="cuda:0")
    step = max(1, (16 << 20) // len(data))
    for i in range(0, starts.numel(), step):
        st = starts[i: i + step]
        flat[st[:, None] + ar[None, :]] = e[None, :].expand(st.numel(), -1)


def workspace(nbytes):
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device="cuda:0")
    return t, (t.data_ptr() + 255) // 256 * 256


def encode_dev(layer, params, E, B, d_in, in_len, ws):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    nb = lib.redux_block_count(in_len, B)
    wsb = layer_ws_bytes(layer, params, E, B, in_len, ws)
    wst, wsp = workspace(wsb)
    cap = lib.redux_encode_bound(C.byref(cp), in_len, B)
    big, out, lo = guarded(cap)
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    flags = torch.full((nb,), 0xEE, dtype=torch.uint8, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    if layer == STORED:
        rc = lib.redux_encode_stored_dev(C.byref(cp), _v(d_in), in_len, B, E, 65536, _v(out), cap, _v(offs), _v(flags), _v(status),
                                         _v(summ), C.c_void_p(wsp), wsb, None)
    else:
        fn = lib.redux_encode_planes_dev if layer == PLANES else lib.redux_encode_delta_dev
        rc = fn(C.byref(cp), _v(d_in), in_len, B, E, _v(out), cap, _v(offs), _v(status), _v(summ), C.c_void_p(wsp), wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, cap)
    return out, offs, status, summ, flags


def decode_dev(layer, params, E, B, d_streams, d_offs, d_flags, out_len, off=0):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    nb = lib.redux_block_count(out_len, B)
    fn = {PLANES: lib.redux_decode_planes_workspace_bytes, DELTA: lib.redux_decode_delta_workspace_bytes,
          STORED: lib.redux_decode_stored_workspace_bytes}[layer]
    wsb = fn(C.byref(cp), out_len, B, E)
    wst, wsp = workspace(wsb)
    big, out, lo = guarded(out_len, off)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    if layer == STORED:
        rc = lib.redux_decode_stored_dev(C.byref(cp), _v(d_streams), _v(d_offs), _v(d_flags), out_len, B, E, _v(out), out_len, _v(sizes),
                                         _v(status), _v(summ), C.c_void_p(wsp), wsb, None)
    else:
        f2 = lib.redux_decode_planes_dev if layer == PLANES else lib.redux_decode_delta_dev
        rc = f2(C.byref(cp), _v(d_streams), _v(d_offs), out_len, B, E, _v(out), _v(sizes), _v(status), _v(summ), C.c_void_p(wsp), wsb,
                None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, out_len)
    return out, sizes, status, summ


def assemble(launch, payload, flags):
    """The encode output of a launch, put together on the device from per-unit payloads: (bytes, offsets, flags)."""
    import torch
    offs = launch.expected_offsets(payload)
    flat = torch.zeros(int(offs[-1]) + 64, dtype=torch.uint8, device="cuda:0")
    for u, p in enumerate(payload):
        scatter_rows(flat, offs[:-1][launch.d_unit == u], p)
    return flat, offs, torch.from_numpy(np.asarray(flags, dtype=np.uint8)).cuda()[launch.d_unit]


def _seed(key):
    return sum(map(ord, key))


CASES = [(k, r) for k in sorted(ROWS) for r in (("C", "S") if ROWS[k][0] == STORED else ("C",))]


def test_scatter_and_compare_agree_and_see_one_wrong_byte():
    import torch
    data = skewed(3000, np.random.default_rng(1)).tobytes()
    starts = torch.tensor([5, 4000, 9000, 20000], device="cuda:0")
    flat = torch.full((24000,), FILL, dtype=torch.uint8, device="cuda:0")
    scatter_rows(flat, starts, data)
    compare_rows(flat, starts, data, "self-check")
    assert int((flat != FILL).sum()) <= 4 * 3000 and int(flat[4]) == FILL and int(flat[3005]) == FILL
    flat[9000 + 77] ^= 1
    with pytest.raises(AssertionError, match="row 2 .* differs at byte 77 of 3000"):
        compare_rows(flat, starts, data, "self-check")


# ---- 3. every row through the `_dev` calls ---------------------------------------------------------------------------------
@pytest.mark.parametrize("key,ragged", CASES)
def test_layer_on_instance(rx, key, ragged):
    import torch
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    X = Launch(layer, params, E, B, nb, _seed(key), ragged)
    in_len = X.in_len
    big_in, d_in, lo_in = X.device_input(off)
    assert d_in.data_ptr() % 16 == off
    L = _lib()
    cp = L.Params(*params)
    assert layer_dec_name(layer, params, B, nb) == dec
    if layer == STORED:                 # the flag pattern the docstring promises, from the oracle's stream lengths
        f = X.flag[X.unit]
        assert not f[:64].any() and f[64:128].all() and f[128:192].tolist() == [1, 0] * 32
        assert f[192:256].sum() == 1 and f[256:320].sum() == 63 and 0 < f[320:].sum() < nb - 320
        assert bool(f[-1]) == (ragged == "S")
    else:                               # the layer matters: the transformed bytes are not the input's
        assert any(not np.array_equal(X.t_blocks[k * E], X.frames[n][:B]) for k, n in enumerate(X.names))
    want_offs = X.expected_offsets()
    if enc is not None:
        copy = copy_bytes(layer, params, E, B, in_len)
        wsb = layer_ws_bytes(layer, params, E, B, in_len, ws)
        x_ptr = C.c_void_p(4096) if copy else _v(d_in)
        assert L.lib().redux_encode_kernel_name_ws(C.byref(cp), x_ptr, in_len, B, wsb - copy).decode() == enc
        assert layer_enc_name(layer, params, E, B, nb, off, ws) == enc
        out, offs, status, summ, flags = encode_dev(layer, params, E, B, d_in, in_len, ws)
        assert guards_intact(big_in, lo_in, in_len)
        assert summ.tolist() == [0, 0] and not bool(status.any())
        if layer == STORED:
            assert torch.equal(flags, torch.from_numpy(X.flag.astype(np.uint8)).cuda()[X.d_unit])
        if not torch.equal(offs, want_offs):
            b = int(((offs[1:] - offs[:-1]) != (want_offs[1:] - want_offs[:-1])).nonzero()[0])
            raise AssertionError(f"block {b} (unit {int(X.unit[b])}): {int(offs[b + 1] - offs[b])} payload bytes, expected "
                                 f"{int(want_offs[b + 1] - want_offs[b])}")
        for u, p in enumerate(X.payload):
            idx = (X.d_unit == u).nonzero().flatten()
            compare_rows(out, want_offs[idx], p, f"encode, unit {u} ({'stored' if X.flag[u] else 'coded'}), blocks {idx[:4].tolist()}...")
    else:
        out, offs, flags = assemble(X, X.payload, X.flag)
    d_out, sizes, dstatus, dsum = decode_dev(layer, params, E, B, out, offs, flags, in_len, off)
    assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
    assert torch.equal(sizes.to(torch.int64), torch.from_numpy(X.block_lengths()).cuda())
    if not torch.equal(d_out, d_in):
        at = int((d_out != d_in).nonzero()[0])
        raise AssertionError(f"decode differs from the input at byte {at} (block {at // B}, frame {at // (E * B)})")
    del big_in, d_in, out, d_out
    _free()


def test_a_block_that_is_no_whole_number_of_symbols_is_invalid_input(rx):
    """10-bit symbols in blocks of 4096 bytes: the coder drops the trailing 8 bits, the block comes back OK with 4095 bytes,
    and the layout's length rule (k_planes_sizes: "one that comes back OK with another size is reported INVALID_INPUT") says
    so for every full block; the ragged block of 2735 bytes is whole symbols and stays OK."""
    import torch
    layer, params, E, B, nb = PLANES, (10, 22, 32), 2, 4096, 64 * 5 + 5
    assert tail_len(params, B) == 2735 and 2735 * 8 % 10 == 0 and B * 8 % 10 == 8
    X = Launch(layer, params, E, B, nb, 77)
    big_in, d_in, lo_in = X.device_input(0)
    out, offs, status, summ, _ = encode_dev(layer, params, E, B, d_in, X.in_len, "own")
    assert summ.tolist() == [0, 0] and torch.equal(offs, X.expected_offsets())
    d_out, sizes, dstatus, dsum = decode_dev(layer, params, E, B, out, offs, None, X.in_len)
    assert sizes.tolist() == [4095] * (nb - 1) + [2735]
    assert dstatus.tolist() == [INVALID_INPUT] * (nb - 1) + [0] and dsum.tolist() == [INVALID_INPUT, nb - 1]


# ---- the host-pointer forms, with CRCs, in three chunks and more ----------------------------------------------------------------
HOST_KEYS = ["planes_e2_coop_whole_cb32", "delta_e1_pair_by_blocks_cb32", "stored_e1_single16_by_alignment",
             "stored_e4_pair_by_blocks_cb32", "planes_e8_single32_by_workspace", "delta_e2_gen_below_8", "planes_e2_any"]


@pytest.mark.parametrize("key", HOST_KEYS)
def test_host_pointer_forms_with_crc_equal_the_dev_calls(rx, key):
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    X = Launch(layer, params, E, B, nb, _seed(key), "S")
    big_in, d_in, lo_in = X.device_input(off)
    out, offs, status, summ, flags = encode_dev(layer, params, E, B, d_in, X.in_len, ws)
    x = d_in.cpu().numpy()
    total = int(offs[-1])
    kw = {"element_size": E}
    if layer == DELTA:
        kw["filter"] = "delta"
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, len(x), B)]
    chunk = -(-nb // 64 // 4) * 64 * B                         # four chunks of whole waves, or five
    try:
        rx.host_set_chunk_bytes(chunk, chunk)
        assert rx.host_chunk_plan(nb, B)[1] >= 3
        crc = np.zeros(nb, np.uint32)
        hflags = np.full(nb, 0xEE, np.uint8)
        if layer == STORED:
            h_out, h_offs, h_st = rx.compress_blocks(x, B, params, stored=hflags, store_ratio=65536, block_crc=crc, **kw)
            assert hflags.tolist() == flags.cpu().tolist()
        else:
            h_out, h_offs, h_st = rx.compress_blocks(x, B, params, block_crc=crc, **kw)
        assert not h_st.any() and crc.tolist() == want_crc
        assert h_offs.astype(np.int64).tolist() == offs.cpu().tolist()
        assert np.array_equal(h_out, out[:total].cpu().numpy())
        dcrc = np.zeros(nb, np.uint32)
        if layer == STORED:
            kw["stored"] = hflags
        back, sizes, st = rx.decompress_blocks(h_out, h_offs, B, params, length=len(x), block_crc=dcrc, **kw)
        assert not st.any() and np.array_equal(back, x) and dcrc.tolist() == want_crc
        assert sizes.astype(np.int64).tolist() == X.block_lengths().tolist()
    finally:
        rx.host_set_chunk_bytes(0, 0)
    del big_in, d_in, out
    _free()


# ---- 4. the transform kernels where a frame ends inside a wave's turn -------------------------------------------------------------
def run_transform(rx, x, E, B, delta, inverse):
    import torch
    n = len(x)
    ts, src, slo = guarded(n)
    src.copy_(torch.from_numpy(x).cuda())
    td, dst, dlo = guarded(n)
    (rx.delta_planes if delta else rx.planes)(src, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    assert guards_intact(td, dlo, n) and guards_intact(ts, slo, n)
    return dst.cpu().numpy()


@pytest.mark.parametrize("B", [65520, 65552, 100_000, 1 << 20])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_transform_kernels_at_frames_that_end_inside_a_turn(rx, E, B):
    """Three full frames and a short one (a third of a frame, five elements and E - 1 trailing bytes); uniform bytes: taken
    as differences by the inverse their running sums wrap mod 2^(8E) every few elements, in the partial last turn of every
    frame too; and all-0xFF differences, whose sum steps down by one."""
    rng = np.random.default_rng(E * 1000 + B % 997)
    n = 3 * E * B + (B // 3 + 5) * E + E - 1
    inputs = [rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0xFF, np.uint8)]
    for x in inputs:
        for delta in (False, True):
            if E == 1 and not delta:
                continue
            for inverse in (False, True):
                want = delta_planes_ref(x, E, B, inverse=inverse) if delta else planes_ref(x, E, B, inverse=inverse)
                got = run_transform(rx, x, E, B, delta, inverse)
                if not np.array_equal(got, want):
                    at = int(np.nonzero(got != want)[0][0])
                    raise AssertionError(f"E={E} B={B} delta={delta} inverse={inverse}: first difference at byte {at} "
                                         f"(frame {at // (E * B)}, offset {at % (E * B)})")


def test_delta_inverse_past_2_pow_20_frames(rx):
    """B = 16, E = 2: 2^20 + 3 full frames of 32 bytes and a short one: the grid-stride path of k_delta_unplanes."""
    E, B = 2, 16
    nf = (1 << 20) + 3
    rng = np.random.default_rng(20)
    x = rng.integers(0, 256, nf * E * B + 7, dtype=np.uint8)
    # the restatement, vectorised over the full frames (the per-frame loop of delta_planes_ref takes minutes here) ...
    body = x[: nf * E * B].reshape(nf, E, B)                            # planes of a frame
    elems = (body[:, 0, :].astype(np.uint16) | (body[:, 1, :].astype(np.uint16) << 8))
    sums = np.cumsum(elems, axis=1, dtype=np.uint16)
    want = np.concatenate([sums.astype("<u2").view(np.uint8).reshape(-1), delta_planes_ref(x[nf * E * B:], E, B, inverse=True)])
    # ... checked against delta_planes_ref on both ends
    k = 100 * E * B
    assert np.array_equal(want[:k], delta_planes_ref(x[:k], E, B, inverse=True))
    assert np.array_equal(want[-k - 7:], delta_planes_ref(x[-k - 7:], E, B, inverse=True))
    got = run_transform(rx, x, E, B, True, True)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"first difference at byte {at} (frame {at // (E * B)})")
    assert np.array_equal(run_transform(rx, got, E, B, True, False), x)


# ---- 5. damaged streams on the new decode paths ---------------------------------------------------------------------------------
DAMAGED_KEYS = ["stored_e1_coop_windows_100k", "stored_e4_table_generic32", "planes_e8_cells8", "delta_e2_cells8"]


@pytest.mark.parametrize("key", DAMAGED_KEYS)
def test_damaged_streams_on_the_new_decode_paths(rx, key):
    """Three coded blocks with one flipped bit, three cut to two thirds, the rest intact: status and size of every block are
    the oracle's (through the layout's length rule), and so are the bytes the damaged blocks decoded to, seen through the
    inverse transform of their frames; the frames whose blocks are all OK hold the original bytes; the guard bands stay."""
    import torch
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    assert layer_dec_name(layer, params, B, nb) == dec
    X = Launch(layer, params, E, B, nb, _seed(key), "C")
    rng = np.random.default_rng(_seed(key) + 1)
    coded = [b for b in range(nb - 1) if not X.flag[X.unit[b]]]
    picks = [coded[i] for i in (3, len(coded) // 5, len(coded) // 3, len(coded) // 2, len(coded) - 70, len(coded) - 2)]
    payload, flag, unit = list(X.payload), list(X.flag), X.unit.copy()
    lens = X.block_lengths()
    want_st, want_sz = np.zeros(nb, np.int32), lens.astype(np.int32).copy()
    partial = {}
    for i, b in enumerate(picks):
        s = bytearray(X.streams[X.unit[b]])
        if i % 2 == 0:
            s[int(rng.integers(0, len(s) // 3))] ^= 1 << int(rng.integers(0, 8))
        else:
            s = s[: len(s) * 2 // 3]
        st, d, _ = ox.decompress_raw(bytes(s), B, params)
        st = TOO_SMALL if st == ox.IO_ERROR else st
        want_st[b] = INVALID_INPUT if st == 0 and len(d) != lens[b] else st
        want_sz[b] = len(d)
        partial[b] = d
        unit[b] = len(payload)
        payload.append(bytes(s))
        flag.append(False)
    assert (want_st[picks] != 0).sum() >= 3
    X.unit, X.d_unit = unit, torch.from_numpy(unit).cuda()
    flat, offs, flags = assemble(X, payload, flag)
    big_in, d_in, lo_in = X.device_input(0)
    d_out, sizes, status, dsum = decode_dev(layer, params, E, B, flat, offs, flags, X.in_len, off)
    got_st, got_sz = status.cpu().numpy(), sizes.cpu().numpy()
    bad = np.nonzero((got_st != want_st) | (got_sz != want_sz))[0]
    assert not len(bad), (int(bad[0]), int(got_st[bad[0]]), int(got_sz[bad[0]]), int(want_st[bad[0]]), int(want_sz[bad[0]]))
    nbad = int((want_st != 0).sum())
    assert dsum.tolist()[1] == nbad and dsum.tolist()[0] in set(want_st[want_st != 0].tolist())
    F = E * B
    clean = np.ones(-(-X.in_len // F), bool)
    clean[np.nonzero(want_st)[0] // E] = False
    same = (d_out[: len(X.plan) * F].view(-1, F) == d_in[: len(X.plan) * F].view(-1, F)).all(1).cpu().numpy()
    assert same[clean[: len(X.plan)]].all()
    if clean[len(X.plan)]:                        # the ragged last frame (a pick may lie in it)
        assert torch.equal(d_out[len(X.plan) * F:], d_in[len(X.plan) * F:])
    # the bytes of the damaged blocks.  A damaged frame f holds, in the plane buffer, its intact blocks and for each damaged
    # one the oracle's partial output d; the inverse transform works element by element (the running sum of element i needs
    # the elements before it only), so the first m elements of the frame, m = the shortest d, are decided: they equal the
    # inverse of the restated transform with d in place.  (E = 1 without a filter: the block's first len(d) bytes are d.)
    checked = 0
    for f in sorted({b // E for b in picks if b // E < len(X.plan)}):
        t = transform(layer, X.frames[X.plan[f]], E, B).copy()
        m = B
        for b in picks:
            if b // E == f:
                d = np.frombuffer(partial[b], dtype=np.uint8)
                j = b % E
                t[j * B: j * B + len(d)] = d
                m = min(m, len(d))
        want = transform(layer, t, E, B, inverse=True)[: m * E]
        got = d_out[f * F: f * F + m * E].cpu().numpy()
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"frame {f}: the first {m} elements differ from the oracle's partial output at byte {at}")
        checked += m * E
    assert checked > 0
    del big_in, d_in, d_out, flat
    _free()


# ---- 6. the summary of the four decode tails ------------------------------------------------------------------------------------
TAILS = [PLANES, DELTA, STORED, "plane-static"]


def _tables_coder(E, B, params, total, d_in, in_len):
    """plane-static (the table-addressed static coders): the tables of the input on the device, and its streams."""
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    cum = np.zeros(E * 258, np.uint32)
    host = d_in.cpu().numpy()
    assert lib.redux_plane_static_tables(C.byref(cp), host.ctypes.data, in_len, B, E, total, cum.ctypes.data) == 0
    d_cum = torch.from_numpy(cum).cuda()
    nb = lib.redux_block_count(in_len, B)
    cap = lib.redux_plane_static_encode_bound(C.byref(cp), in_len, B)
    wsb = lib.redux_plane_static_encode_workspace_bytes(C.byref(cp), in_len, B, E)
    wst, wsp = workspace(wsb)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_plane_static_encode_dev(C.byref(cp), _v(d_cum), total, _v(d_in), in_len, B, E, _v(out), cap, _v(offs), _v(status),
                                           _v(summ), C.c_void_p(wsp), wsb, None)
    torch.cuda.synchronize()
    assert rc == 0 and summ.tolist() == [0, 0]
    return d_cum, out, offs


def _tables_decode(E, B, params, total, d_cum, d_streams, d_offs, out_len):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    nb = lib.redux_block_count(out_len, B)
    wsb = lib.redux_plane_static_decode_workspace_bytes(C.byref(cp), out_len, B, E)
    wst, wsp = workspace(wsb)
    big, out, lo = guarded(out_len)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    rc = lib.redux_plane_static_decode_dev(C.byref(cp), _v(d_cum), total, _v(d_streams), _v(d_offs), out_len, B, E, _v(out), _v(sizes),
                                           _v(status), _v(summ), C.c_void_p(wsp), wsb, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, out_len)
    return out, sizes, status, summ


def _summary_is_the_statuses(status, summ, want_bad):
    """d_summary = [the status of the first failing block, the number of failing blocks], from the returned statuses.  (Where
    failing blocks differ in status, the device keeps the one whose workgroup came first: any of them.)"""
    st = status.cpu().numpy()
    bad = np.nonzero(st)[0]
    assert bad.tolist() == want_bad, (bad.tolist(), want_bad)
    first, count = summ.tolist()
    assert count == len(bad)
    assert first == int(st[bad[0]]) or (len(set(st[bad].tolist())) > 1 and first in st[bad].tolist()), (first, st[bad].tolist())


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_summary_of_the_four_decode_tails(rx, E):
    """67 blocks of 1,040 bytes and a last block of 5 (more than one 64-block wave, a block count no multiple of any E > 1, a
    block size that is a multiple of 16 and not of 64, a ragged last block) through the planes, delta, stored and
    table-addressed static decode calls: with two damaged streams, and with an out_len one byte short of what the streams
    hold, d_summary is the first failing block's status and the count of failing blocks, as the returned statuses give them."""
    import torch
    params, B, nb, total = (8, 30, 32), 1040, 68, 4096
    in_len = 67 * B + 5
    rng = np.random.default_rng(140 + E)
    d_in = torch.from_numpy(np.minimum(rng.standard_exponential(in_len) * 5, 255).astype(np.uint8)).cuda()   # (every block shrinks)
    lib = _lib().lib()
    for tail in TAILS:
        if tail == "plane-static":
            d_cum, out, offs = _tables_coder(E, B, params, total, d_in, in_len)
            flags = None
            decode = lambda s, n: _tables_decode(E, B, params, total, d_cum, s, offs, n)
        else:
            out, offs, status, summ, flags = encode_dev(tail, params, E, B, d_in, in_len, "own")
            assert summ.tolist() == [0, 0]
            decode = lambda s, n, tail=tail, flags=flags: decode_dev(tail, params, E, B, s, offs, flags, n)
        assert lib.redux_block_count(in_len - 1, B) == nb
        d_out, sizes, status, summ = decode(out, in_len)
        assert summ.tolist() == [0, 0] and torch.equal(d_out, d_in), tail
        # an out_len one byte short: the last block holds a byte too many
        d_out, sizes, status, summ = decode(out, in_len - 1)
        _summary_is_the_statuses(status, summ, [nb - 1])
        assert torch.equal(d_out[: 67 * B - (67 % E) * B], d_in[: 67 * B - (67 % E) * B]), tail     # the frames without it
        # two damaged streams, one in each 64-block wave: the last two thirds of the stream become 0xFF
        o = offs.cpu().numpy()
        picks = [b for b in (3, 65) if tail != STORED or int(flags[b]) == 0]
        assert len(picks) == 2, "the skewed blocks are coded, not stored"
        hurt = out.clone()
        for b in picks:
            n = int(o[b + 1] - o[b])
            hurt[int(o[b]) + n // 3: int(o[b + 1])] = 0xFF
        d_out, sizes, status, summ = decode(hurt, in_len)
        _summary_is_the_statuses(status, summ, picks)
    _free()
