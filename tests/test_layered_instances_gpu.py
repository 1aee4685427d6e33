"""Every layer in front of the adaptive coder on every coder instance below it (the table:
tests/test_layered_instances_cpu.py): byte planes, the delta filter and stored blocks; constant blocks, the mixed layouts,
the zigzag, lag, base XOR and base folded-difference filters, the lag order (higher-order lagged differences) and the record
layout for fixed-width structs (a row's E is then the record size and a frame E blocks).

One launch per row of ROWS, through the `_dev` calls.  A case first asserts, by name, that the coder below the wrapper runs
the encode and decode instance the row promises, for the very pointer, length and workspace of the launch.  The input is
tiled on the device from a few distinct FRAMES (E blocks of typed data; frames are independent under every layer; a unit
of 8 blocks under the mixed layouts) and ends in a ragged frame whose last block has an odd length; every distinct block
of the numpy restatement of the transform (planes_ref, delta_planes_ref, zigzag_planes_ref, lag_planes_ref,
base_planes_ref + pad, base_sub_planes_ref, mixed_ref, record_ref) is coded once by the oracle.  Checked for EVERY block of every
launch (the count is the row's block count: 389, 1,093 or 2,565): offsets, statuses, the summary, the flags of stored and
constant blocks, the stream bytes against the oracle's (a stored block: its transformed bytes; a constant block: its one
byte); then the decode of the device's own output equals the input byte for byte and the sizes are the layout's.  Input,
base, unit table, encode output, flags and decode output lie between guard bands of 0xA5 that must stay untouched (the
helpers of test_adaptive_instances_gpu, which place a buffer a given number of bytes off a 16-byte boundary;
test_stream_ranges_gpu's own cannot).
  * planes: bf16 / fp32 / int64 patterns; delta, zigzag: integer series of test_delta_cpu's generators, cast to the element
    size; lag: test_lag_cpu's interleaved channels, as many as the row's lag where that is <= 8;
  * stored: frames whose planes are incompressible (S) or skewed (C): group 0 of 64 blocks all coded, 1 all stored,
    2 alternating, 3 a single stored block, 4 a single coded block (group 0 alternates two coded frames, so that two
    neighbouring table entries never hold the same bytes), the rest mixed frame by frame; the ragged last block
    once stored and once coded.  The flag pattern is asserted.
  * const: the same pattern over x' with S a constant plane (one repeated element, its bytes another for each plane and not
    zero); with a base the input is the wanted x' XORed with the base, and every other all-constant frame EQUALS the
    base's, all-zero planes behind the XOR.  The expected flags are const_ref of the restated x'.  Asserted from the
    reference before any device call: the pattern, a whole 64-entry wave of idle entries behind the coded blocks in the
    table the library builds, entries that name non-consecutive blocks, and, where the base ends inside a frame, that
    frame and the frames behind it as units of their own.  The ragged last block once constant and once coded.
  * mixed: int64 stamps, floats and plain bytes under a dictated table of all eight layouts with two equal neighbours and
    a layout for the short last unit (nb mod 8 = 5); one row once more with layouts_mask 0xFF, against the oracle on
    mixed_ref(x, the table the call returned).
  * base, base_sub: x = the base with sparse changes: bit flips; small numeric steps and one across a carry per frame.  The
    base by turn absent, as long as the input, ending inside a frame at an odd byte, and once longer than the input.
  * lag_order: test_lag_order_cpu's interleaved tones (two frames) and test_lag_cpu's walks (one), as many channels as the
    lag where that is <= 8, against lag_order_planes_ref; asserted from the reference before any device call: the
    transformed bytes of every frame are neither the input's nor lag_planes_ref's (the order reaches the kernel).
  * record: packed records of R bytes whose columns are by turn a counter, a slowly moving value, noise and a constant,
    three distinct frames of R blocks; the byte delta on or off as the row says; asserted from the reference before any
    device call: the transformed bytes of every frame are not the input's, and those with the delta not those without.
  * one expected byte (constant blocks: also one flag) made wrong on the reference side fails the row of every later layer
    with a message that names the block and the unit.
Then: the host-pointer forms with CRCs in at least three chunks against the `_dev` result (constant blocks on the caller's
buffer at E = 1, and with a base that ends inside a chunk); k_planes / k_delta_planes / k_delta_unplanes and the zigzag and
lag kernels (S = 3, 255, 256) at block sizes whose frames end inside a wave's turn; the delta inverse, the fused and the
byte lag inverse past 2^20 frames (more frames than workgroups: what a workgroup keeps in LDS from frame to frame); the lag
kernels at one frame of 1025 rows; k_const_select past its grid cap; damaged streams on the table forms of k_decode_wave and
k_decode<false, true> and under planes / delta on k_decode_cells<8>.
Left out: damaged streams under the later layers but for one lag-order row and one record row on k_decode_wave with the
fix-up pass (the
decoders' table forms are covered under stored, k_const_fill's refusals in test_const_gpu.py, and the filters share
layout_decode_tail with delta).  The lag-order kernels with several frames per wave and per workgroup: test_lag_order_gpu.py."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_adaptive_instances_gpu import FILL, GUARD, compare_rows, guarded, guards_intact
from test_base_cpu import base_planes_ref, pad
from test_base_sub_cpu import base_sub_planes_ref
from test_const_cpu import const_ref
from test_delta_cpu import delta_planes_ref, sorted_i32, timestamps_i64, tones_i16
from test_lag_cpu import channels, lag_planes_ref
from test_lag_order_cpu import lag_order_planes_ref, tones
from test_layered_instances_cpu import (BASE, BASE_SUB, CONST, DELTA, EXTRA, LAG, LAG_ORDER, MIXED, PLANES, RECORD, ROWS, STORED, WITH_BASE, ZIGZAG,
                                        base_len_of, coded_len, copy_bytes, input_len, layer_dec_name, layer_enc_name,
                                        layer_ws_bytes, mixed_table, reads_copy, tail_len)
from test_mixed_cpu import mixed_ref
from test_planes_cpu import planes_ref
from test_planes_gpu import typed
from test_record_cpu import record_ref
from test_stored_cpu import rule
from test_zigzag_cpu import zigzag_planes_ref

pytestmark = pytest.mark.gpu
INVALID_INPUT, TOO_SMALL = 2, 4
FLAGGED = (STORED, CONST)            # the layers whose calls write and read a u8 flag per block
NONE = np.zeros(0, np.uint8)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def _lib():
    from redux_amd import _lib as L
    return L


def _v(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _free():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def transform(layer, x, E, B, inverse=False, lag=None, base=NONE, table=None, order=None, delta=None):
    """The numpy restatement of what a layer's call puts in front of the coder (inverse: behind the decoder).  base: y, the
    bytes of the base that lie under x; table: the unit table of the mixed layouts; the record layout: E is the record size,
    delta its flag."""
    if layer == RECORD:
        return record_ref(x, E, B, bool(delta), inverse)
    if layer == LAG_ORDER:
        return lag_order_planes_ref(x, E, B, lag, order, inverse=inverse)
    if layer == DELTA:
        return delta_planes_ref(x, E, B, inverse=inverse)
    if layer == ZIGZAG:
        return zigzag_planes_ref(x, E, B, inverse=inverse)
    if layer == LAG:
        return lag_planes_ref(x, E, B, lag, inverse=inverse)
    if layer == BASE or (layer == CONST and len(base)):
        return base_planes_ref(x, base, E, B, inverse=inverse)
    if layer == BASE_SUB:
        return base_sub_planes_ref(x, base, E, B, inverse=inverse)
    if layer == MIXED:
        return mixed_ref(x, table, B, inverse=inverse)
    return planes_ref(x, E, B, inverse=inverse) if E > 1 else np.ascontiguousarray(x, np.uint8).copy()


# ---- the input: a few distinct frames -----------------------------------------------------------------------------------
def skewed(n, rng):
    return np.minimum(rng.standard_exponential(n) * 14, 255).astype(np.uint8)


def stored_frame(pattern, B, rng):
    """A frame of len(pattern) planes of B bytes, in ORIGINAL order: plane j uniform bytes ("S": the coder expands it) or
    skewed ones ("C", "c": two draws)."""
    planes = [rng.integers(0, 256, B, dtype=np.uint8) if c == "S" else skewed(B, rng) for c in pattern]
    return np.stack(planes, axis=1).reshape(-1)


def const_byte(j, seed):
    """the byte of constant plane j: 1 .. 255, another for each of a frame's planes"""
    return (37 * (j + 1) + seed) % 255 + 1


def const_frame(pattern, B, rng, seed):
    """As stored_frame with "S" a constant plane: the frame's elements repeat one element at those bytes, whose bytes differ
    from plane to plane and are not zero."""
    planes = [np.full(B, const_byte(j, seed), np.uint8) if c == "S" else skewed(B, rng) for j, c in enumerate(pattern)]
    return np.stack(planes, axis=1).reshape(-1)


def patterns(E):
    return ["C" * E, "c" * E, "S" * E] + ([] if E == 1 else ["SC" * (E // 2), "S" + "C" * (E - 1), "C" + "S" * (E - 1)])


def frames_of(layer, E, B, seed, lag=None):
    """(name -> frame, name -> the base's bytes under it): frames of E * B bytes in original order.  Constant blocks: the
    frame is what x ^ y' shall be, the input is made from it (Launch.source)."""
    rng = np.random.default_rng(seed)
    F = E * B
    if layer == PLANES:
        return {f"typed{k}": typed(F, seed + k) for k in range(3)}, {}
    if layer == MIXED:                               # frames (units) that ask for different layouts: int64 stamps, floats, bytes
        stamps = np.resize(timestamps_i64().view("<u8"), F // 8).view(np.uint8).copy()
        return {"bytes": skewed(F, rng), "stamps": stamps, "typed": typed(F, seed)}, {}
    if layer in (DELTA, ZIGZAG):
        out = {}
        for name, gen, dt in (("timestamps", timestamps_i64, "<u8"), ("sorted", sorted_i32, "<u4"), ("tones", tones_i16, "<i2")):
            v = np.resize(gen().view(dt), B).astype(np.int64).astype("<u%d" % E)        # the series mod 2^(8E)
            out[name] = v.view(np.uint8).copy()
        return out, {}
    if layer == LAG:                                 # interleaved channels, as many as the lag where that is <= 8
        return {f"channels{k}": np.resize(channels(lag if lag <= 8 else 8, E, seed + k).view("<u%d" % E), B).view(np.uint8).copy()
                for k in range(3)}, {}
    if layer == RECORD:                              # packed records of E bytes: a counter, a slowly moving, a noisy and a
        out = {}                                     # constant column, repeated across the record
        for k in range(3):
            i = np.arange(B, dtype=np.int64)
            cols = [i + 11 * k, 100 + 37 * k + np.cumsum(rng.integers(-2, 3, B)), rng.integers(0, 256, B), np.full(B, 0x40 + k)]
            out[f"records{k}"] = np.stack([cols[p % 4] + (p // 4) * 3 for p in range(E)], axis=1).astype(np.uint8).reshape(-1)
        return out, {}
    if layer == LAG_ORDER:                           # two frames of tones and one of walks, interleaved as for the lag filter
        ch = lag if lag <= 8 else 8
        gens = {"tones0": tones(ch, E, seed), "tones1": tones(ch, E, seed + 1), "walks": channels(ch, E, seed + 2)}
        return {n: np.resize(v.view("<u%d" % E), B).view(np.uint8).copy() for n, v in gens.items()}, {}
    if layer in (BASE, BASE_SUB):                    # x = y with sparse changes
        xs, ys = {}, {}
        for k in range(3):
            y = typed(F, seed + k)
            x = y.copy()
            if layer == BASE:                        # bit flips
                at = rng.choice(F, F // 97, replace=False)
                x[at] ^= (1 << rng.integers(0, 8, len(at))).astype(np.uint8)
            else:                                    # small numeric steps, and one across a carry: ...FF -> ...00
                yv, xv = y.view("<u%d" % E), x.view("<u%d" % E)
                at = rng.choice(B, B // 53, replace=False)
                xv[at] = yv[at] + rng.integers(-3, 4, len(at)).astype(np.int64).astype(xv.dtype)
                yv[B // 2] |= 0xFF
                xv[B // 2: B // 2 + 1] = yv[B // 2: B // 2 + 1] + xv.dtype.type(1)   # (wraps for E = 1)
            xs[f"snap{k}"], ys[f"snap{k}"] = x, y
        return xs, ys
    if layer == CONST:
        pats = patterns(E)
        return {p: const_frame(p, B, rng, seed) for p in pats}, {p: typed(F, seed + k) for k, p in enumerate(pats)}
    return {p: stored_frame(p, B, rng) for p in patterns(E)}, {}


def frame_plan(layer, E, nfull, names):
    """The frame of every full frame of the launch, by name."""
    if layer not in FLAGGED:
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
    """The blocks of one launch and what the oracle makes of each distinct one.  A full frame is one of a few SOURCES, a
    (name, variant) pair: the variant is how the base lies under the frame ("cov": all of it, "cut": the base ends inside,
    "unc": not at all, and so for every layer without a base) or, for the mixed layouts, the frame's (= unit's) layout."""

    def __init__(self, layer, params, E, B, nb, seed, ragged="C", slot=None, lag=None, base=None, table=None, oracle=True, order=None,
                 delta=None):
        import torch
        self.layer, self.params, self.E, self.B, self.nb, self.lag, self.order, self.delta = layer, params, E, B, nb, lag, order, delta
        self.in_len = input_len(params, B, nb)
        F = E * B
        frames, y_frames = frames_of(layer, E, B, seed, lag)
        names = sorted(frames)
        nfull = self.in_len // F
        plan = frame_plan(layer, E, nfull, names)
        last_len = self.in_len - nfull * F
        assert 0 < last_len and nfull * E + -(-last_len // B) == nb
        self.base_len = base_len_of(base, self.in_len, E, B) if layer in WITH_BASE else 0
        self.table = (mixed_table(nfull + 1) if table is None else np.asarray(table, np.uint8)) if layer == MIXED else None
        assert self.table is None or len(self.table) == nfull + 1
        self.frames, self.y_frames, self.names, self.plan = frames, y_frames, names, plan
        self.keys = [(n, self.variant(f)) for f, n in enumerate(plan)]
        self.sources = sorted(set(self.keys))
        self.x_of, self.y_of = {}, {}
        for key in self.sources:
            self.x_of[key], self.y_of[key] = self.source(*key)
        # the ragged last frame: a source of its own
        rng = np.random.default_rng(seed + 99)
        under = min(max(self.base_len - nfull * F, 0), last_len)        # bytes of the base under it
        if layer == STORED:
            last, y_last = rng.integers(0, 256, last_len, dtype=np.uint8) if ragged == "S" else skewed(last_len, rng), NONE
        elif layer == CONST:                         # x' all one byte ("S": every block of it is constant), or skewed
            y_last = rng.integers(0, 256, under, dtype=np.uint8)
            last = (np.full(last_len, 0x5A, np.uint8) if ragged == "S" else skewed(last_len, rng)) ^ pad(y_last, last_len)
        else:
            last = frames[names[1]][:last_len]
            y_last = y_frames[names[1]][:under] if y_frames else NONE
        self.last, self.y_last = last, y_last
        # units: the distinct blocks of the transformed input; block b of the launch is unit self.unit[b]
        t_blocks = []
        for key in self.sources:
            t = self.transformed(self.x_of[key], self.y_of[key], key[1])
            t_blocks += [t[j * B: (j + 1) * B] for j in range(E)]
        t_last = self.transformed(last, y_last, self.variant(nfull))
        t_blocks += [t_last[o: o + B] for o in range(0, last_len, B)]
        self.t_blocks = t_blocks
        at = {key: k * E for k, key in enumerate(self.sources)}
        unit = [at[key] + j for key in self.keys for j in range(E)] + list(range(len(self.sources) * E, len(t_blocks)))
        self.unit = np.array(unit, dtype=np.int64)
        assert len(unit) == nb
        L = [len(t) for t in t_blocks]
        if layer == CONST:                           # the rule over the restated coder input
            self.flag = np.array([bool(const_ref(t, B)[0]) for t in t_blocks])
        slot = slot or 4 * B + 4096
        self.streams = []
        for u, t in enumerate(t_blocks):
            if not oracle or (layer == CONST and self.flag[u]):
                self.streams.append(None)            # (never coded)
                continue
            s, st = ox.compress_blocks(t, B, params, slot=slot)
            assert len(s) == 1 and not st.any()
            self.streams.append(s[0])
        if layer == STORED:
            self.flag = rule([0] * len(L), [len(s) for s in self.streams], L, 65536)
        elif layer != CONST:
            self.flag = np.zeros(len(L), bool)
        # a stored block travels as its bytes, a constant one as its one byte
        self.payload = [(t.tobytes() if layer == STORED else t[:1].tobytes()) if f else s
                        for t, s, f in zip(t_blocks, self.streams, self.flag)]
        self.d_unit = torch.from_numpy(self.unit).cuda() if torch.cuda.is_available() else None   # (the CPU side too)

    def variant(self, f):
        F = self.E * self.B
        if self.layer == MIXED:
            return int(self.table[f])
        if self.base_len >= (f + 1) * F:     # (constant blocks: every other all-constant frame under the base EQUALS the base)
            return "cov0" if self.layer == CONST and f % 2 and f < len(self.plan) and set(self.plan[f]) == {"S"} else "cov"
        return "unc" if self.base_len <= f * F else "cut"

    def source(self, name, variant):
        """(the input's bytes of such a frame, the base's bytes under it)"""
        F = self.E * self.B
        if self.layer not in WITH_BASE:
            return self.frames[name], NONE
        y = self.y_frames[name][: {"cov": F, "cov0": F, "cut": self.base_len % F, "unc": 0}[variant]]
        if self.layer != CONST:
            return self.frames[name], y
        if variant == "cov0":                        # a frame that equals the base's: all-zero planes behind the XOR
            return y.copy(), y
        return self.frames[name] ^ pad(y, F), y

    def transformed(self, x, y, variant):
        return transform(self.layer, x, self.E, self.B, lag=self.lag, base=y, table=[variant] if self.layer == MIXED else None,
                         order=self.order, delta=self.delta)

    def device_input(self, off):
        """(whole tensor, the input `off` bytes off a 16-byte boundary, its start in the tensor)"""
        import torch
        big, d_in, lo = guarded(self.in_len, off)
        F = self.E * self.B
        stack = torch.from_numpy(np.stack([self.x_of[k] for k in self.sources])).cuda()
        idx = torch.tensor([self.sources.index(k) for k in self.keys], device="cuda:0")
        nfull = len(self.plan)
        d_in[: nfull * F].view(nfull, F).copy_(stack[idx])
        d_in[nfull * F:].copy_(torch.from_numpy(self.last.copy()))
        return big, d_in, lo

    def device_base(self, off=0):
        """(whole tensor, the base_len bytes of the base `off` bytes off a 16-byte boundary, its start in the tensor): the
        frames' bases tiled as the input is, the ragged frame's, and for a base longer than the input some bytes more."""
        import torch
        big, d_y, lo = guarded(self.base_len, off)
        if not self.base_len:
            return big, None, lo
        F = self.E * self.B
        nfull = len(self.plan)
        ncov = min(-(-self.base_len // F), nfull)      # full frames the base reaches into
        stack = torch.from_numpy(np.stack([self.y_frames[n] for n in self.names])).cuda()
        idx = torch.tensor([self.names.index(n) for n in self.plan[:ncov]], device="cuda:0")
        body = stack[idx].reshape(-1)[: self.base_len]
        d_y[: body.numel()].copy_(body)
        if self.base_len > nfull * F:
            more = self.base_len - nfull * F - len(self.y_last)
            rest = np.concatenate([self.y_last, np.random.default_rng(5).integers(0, 256, more, dtype=np.uint8)])
            d_y[nfull * F:].copy_(torch.from_numpy(rest))
        return big, d_y, lo

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


def _dev_fn(direction, layer):
    return getattr(_lib().lib(), f"redux_{direction}_{layer}_dev")


def encode_dev(layer, params, E, B, d_in, in_len, ws, lag=None, d_base=None, base_len=0, d_table=None, mask=0, order=None, delta=None):
    """The layer's encode call between guard bands -> (out, offsets, statuses, summary, flags)"""
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
    fbig, flags, flo = guarded(nb)
    flags.fill_(0xEE)
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    # every call is (params, input, [base], shape, [option], output, offsets, [flags], statuses, summary, workspace, stream)
    fn, x, y = _dev_fn("encode", layer), (C.byref(cp), _v(d_in), in_len), (_v(d_base) if base_len else None, base_len)
    dst, end = (_v(out), cap, _v(offs)), (_v(status), _v(summ), C.c_void_p(wsp), wsb, None)
    if layer == STORED:
        rc = fn(*x, B, E, 65536, *dst, _v(flags), *end)
    elif layer == CONST:
        rc = fn(*x, *y, B, E, *dst, _v(flags), *end)
    elif layer == MIXED:
        rc = fn(*x, B, mask, _v(d_table), *dst, *end)
    elif layer == LAG:
        rc = fn(*x, B, E, lag, *dst, *end)
    elif layer == RECORD:               # (block size, record size, delta flag)
        rc = fn(*x, B, E, int(delta), *dst, *end)
    elif layer == LAG_ORDER:
        rc = fn(*x, B, E, lag, order, *dst, *end)
    elif layer in (BASE, BASE_SUB):
        rc = fn(*x, *y, B, E, *dst, *end)
    else:
        rc = fn(*x, B, E, *dst, *end)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_intact(big, lo, cap) and guards_intact(fbig, flo, nb)
    return out, offs, status, summ, flags


def decode_dev(layer, params, E, B, d_streams, d_offs, d_flags, out_len, off=0, lag=None, d_base=None, base_len=0, d_table=None,
               order=None, delta=None):
    import torch
    L = _lib()
    lib, cp = L.lib(), L.Params(*params)
    nb = lib.redux_block_count(out_len, B)
    if layer == MIXED:
        wsb = lib.redux_decode_mixed_workspace_bytes(C.byref(cp), out_len, B)
    else:
        wsb = getattr(lib, f"redux_decode_{layer}_workspace_bytes")(C.byref(cp), out_len, B, E)
    wst, wsp = workspace(wsb)
    big, out, lo = guarded(out_len, off)
    sizes = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    status = torch.full((nb,), -7, dtype=torch.int32, device="cuda:0")
    summ = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    fn, tail = _dev_fn("decode", layer), (_v(sizes), _v(status), _v(summ), C.c_void_p(wsp), wsb, None)
    y = (_v(d_base) if base_len else None, base_len)
    if layer == STORED:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), _v(d_flags), out_len, B, E, _v(out), out_len, *tail)
    elif layer == CONST:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), _v(d_flags), *y, out_len, B, E, _v(out), *tail)
    elif layer == MIXED:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), _v(d_table), out_len, B, _v(out), *tail)
    elif layer == LAG:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), out_len, B, E, lag, _v(out), *tail)
    elif layer == RECORD:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), out_len, B, E, int(delta), _v(out), *tail)
    elif layer == LAG_ORDER:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), out_len, B, E, lag, order, _v(out), *tail)
    elif layer in (BASE, BASE_SUB):
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), *y, out_len, B, E, _v(out), *tail)
    else:
        rc = fn(C.byref(cp), _v(d_streams), _v(d_offs), out_len, B, E, _v(out), *tail)
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


CASES = [(k, r) for k in sorted(ROWS) for r in (("C", "S") if ROWS[k][0] in FLAGGED else ("C",))]


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
def flag_pattern_holds(X, ragged):
    """The flags of a stored or constant launch, from the reference alone: group 0 of 64 blocks none, 1 all, 2 alternating,
    3 one, 4 all but one, the rest mixed; the ragged last block as asked."""
    f, nb = X.flag[X.unit], X.nb
    assert not f[:64].any() and f[64:128].all() and f[128:192].tolist() == [1, 0] * 32
    assert f[192:256].sum() == 1 and f[256:320].sum() == 63 and 0 < f[320:].sum() < nb - 320
    assert bool(f[-1]) == (ragged == "S")


def const_launch_is_what_the_row_is_for(X, base):
    """From the reference alone: the table k_const_table packs (the coded blocks from entry 0, idle entries behind them) has a
    whole 64-entry wave of idle entries and a wave whose entries name non-consecutive blocks; a constant block's payload is
    its one byte x'[b * B], and the constant planes' bytes are not all zero; a base that ends inside a frame leaves that
    frame and the frames behind it units of their own."""
    f, nb, E = X.flag[X.unit], X.nb, X.E
    coded = np.nonzero(~f)[0]
    assert -(-len(coded) // 64) * 64 + 64 <= nb
    assert any((np.diff(coded[w: w + 64]) != 1).any() for w in range(0, len(coded), 64))
    assert len(coded) > 64 * 2 and (coded != np.arange(len(coded)))[64:].all()          # slot j != block b beyond wave 0
    const_units = np.nonzero(X.flag)[0]
    assert all(X.payload[u] == X.t_blocks[u][:1].tobytes() and len(X.payload[u]) == 1 for u in const_units)
    assert len({X.payload[u] for u in const_units}) >= E and any(X.payload[u] != b"\0" for u in const_units)
    kinds = {v.rstrip("0") for _, v in X.keys}
    assert base == "none" or any(v == "cov0" for _, v in X.keys) and any(X.payload[u] == b"\0" for u in const_units)
    assert kinds == {"none": {"unc"}, "full": {"cov"}, "inside": {"cov", "cut", "unc"}}[base]
    if base == "inside":
        cut = [f for f, (_, v) in enumerate(X.keys) if v == "cut"]
        assert len(cut) == 1 and all(v == "unc" for _, v in X.keys[cut[0] + 1:]) and len(X.keys) - cut[0] > 64 // E
        under = {u for k, u in zip(X.keys, X.unit[::E]) if k[1] in ("cov", "cov0")}
        assert not under & {u for k, u in zip(X.keys, X.unit[::E]) if k[1] in ("cut", "unc")}


def order_reaches_the_kernel(X):
    """The lag order, from the reference alone: the transformed bytes of every distinct frame and of the ragged one are neither
    the input's nor the lag filter's of it (order 1), so a call that dropped the order, or the filter, fails its row."""
    E, B = X.E, X.B
    assert X.order in (2, 3) and 3 * X.lag < B
    xs = [X.x_of[src] for src in X.sources] + [X.last]
    ts = [np.concatenate(X.t_blocks[k * E: (k + 1) * E]) for k in range(len(X.sources))] + [np.concatenate(X.t_blocks[len(X.sources) * E:])]
    for x, t in zip(xs, ts):
        assert len(t) == len(x) and not np.array_equal(t, x) and not np.array_equal(t, lag_planes_ref(x, E, B, X.lag))
        if E > 1:
            assert not np.array_equal(t, planes_ref(x, E, B))


def record_layout_reaches_the_kernel(X):
    """The record layout, from the reference alone: the transformed bytes of every distinct frame and of the ragged one are not
    the input's, and the bytes with the delta are not the bytes without it, so a call that dropped the layout, the record size's
    frame or the flag fails its row."""
    R, B = X.E, X.B
    assert X.delta in (False, True) and len(X.last) % B % 2 == 1 and (len(X.last) > B or R == 2)   # a short frame of several blocks
    for x in [X.x_of[src] for src in X.sources] + [X.last]:
        t, other = record_ref(x, R, B, X.delta), record_ref(x, R, B, not X.delta)
        assert len(t) == len(x) and not np.array_equal(t, x) and not np.array_equal(other, x) and not np.array_equal(t, other)


def layer_is_no_identity(X):
    return any(not np.array_equal(X.t_blocks[k * X.E], X.x_of[src][: X.B]) for k, src in enumerate(X.sources))


def compare_flags(flags, X):
    import torch
    want = torch.from_numpy(X.flag.astype(np.uint8)).cuda()[X.d_unit]
    if not torch.equal(flags, want):
        b = int((flags != want).nonzero()[0])
        raise AssertionError(f"block {b} (unit {int(X.unit[b])}): flag {int(flags[b])}, expected {int(want[b])}")


def spoil_reference(X, what):
    """One expected byte or flag made wrong on the reference side (test_a_corrupted_reference_fails_its_row)."""
    if what == "flag":
        u = int(np.nonzero(X.flag)[0][0])
        X.flag[u] = False
    else:
        u = next(int(u) for u in X.unit[X.nb // 2:] if not X.flag[u])
        p = bytearray(X.payload[u])
        p[len(p) // 2] ^= 1
        X.payload[u] = bytes(p)


def run_row(key, ragged, spoil=None, mask=0):
    import torch
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    lag, base, order, delta = EXTRA.get(key, (None, None, None, None))
    X = Launch(layer, params, E, B, nb, _seed(key), ragged, lag=lag, base=base, oracle=not mask, order=order, delta=delta)
    in_len = X.in_len
    big_in, d_in, lo_in = X.device_input(off)
    assert d_in.data_ptr() % 16 == off
    big_y, d_y, lo_y = X.device_base(4 if off else 0)
    L = _lib()
    cp = L.Params(*params)
    assert layer_dec_name(layer, params, B, nb) == dec
    big_t, d_table, lo_t = None, None, 0
    if layer == MIXED:                  # the dictated table: all eight layouts, two equal neighbours, a layout for the short unit
        assert set(X.table.tolist()) == set(range(8)) and (X.table[1:] == X.table[:-1]).any() and X.table[-1] != 0 and nb % 8 == 5
        big_t, d_table, lo_t = guarded(len(X.table))
        d_table.copy_(torch.full_like(d_table, 0xEE) if mask else torch.from_numpy(X.table).cuda())
    if mask:                            # the layouts are chosen on the device: the reference follows the table it returns
        out, offs, status, summ, flags = encode_dev(layer, params, E, B, d_in, in_len, ws, d_table=d_table, mask=mask)
        assert guards_intact(big_t, lo_t, len(X.table)) and bool((d_table <= 7).all())
        X = Launch(layer, params, E, B, nb, _seed(key), ragged, table=d_table.cpu().numpy())
        print(f"{key}: the device chose {np.bincount(X.table, minlength=8).tolist()} units of layouts 0 .. 7")
        assert len(set(X.table.tolist())) >= 2       # (int64 stamps, floats and plain bytes do not share a best layout)
    if layer in FLAGGED:                # the flag pattern the docstring promises, from the reference alone
        flag_pattern_holds(X, ragged)
    if layer == CONST:
        const_launch_is_what_the_row_is_for(X, base)
    if layer == LAG_ORDER:
        order_reaches_the_kernel(X)
    if layer == RECORD:
        record_layout_reaches_the_kernel(X)
    # the layer matters: the transformed bytes are not the input's (a base filter without a base at E = 1 still copies)
    assert layer_is_no_identity(X) or layer in FLAGGED or (layer in (BASE, BASE_SUB) and base == "none" and E == 1)
    if spoil:
        spoil_reference(X, spoil)
    want_offs = X.expected_offsets()
    if enc is not None:
        front = copy_bytes(layer, params, E, B, in_len)
        wsb = layer_ws_bytes(layer, params, E, B, in_len, ws)
        x_ptr = C.c_void_p(4096) if reads_copy(layer, E, base) else _v(d_in)
        assert L.lib().redux_encode_kernel_name_ws(C.byref(cp), x_ptr, coded_len(layer, B, in_len), B, wsb - front).decode() == enc
        assert layer_enc_name(layer, params, E, B, nb, off, ws, base=base) == enc
        if not mask:
            out, offs, status, summ, flags = encode_dev(layer, params, E, B, d_in, in_len, ws, lag, d_y, X.base_len, d_table, order=order,
                                                        delta=delta)
        assert guards_intact(big_in, lo_in, in_len) and guards_intact(big_y, lo_y, X.base_len)
        assert summ.tolist() == [0, 0] and not bool(status.any())
        if layer in FLAGGED:
            compare_flags(flags, X)
        if layer == MIXED:
            assert guards_intact(big_t, lo_t, len(X.table)) and d_table.cpu().tolist() == X.table.tolist()
        if not torch.equal(offs, want_offs):
            b = int(((offs[1:] - offs[:-1]) != (want_offs[1:] - want_offs[:-1])).nonzero()[0])
            raise AssertionError(f"block {b} (unit {int(X.unit[b])}): {int(offs[b + 1] - offs[b])} payload bytes, expected "
                                 f"{int(want_offs[b + 1] - want_offs[b])}")
        kind = {STORED: "stored", CONST: "constant"}.get(layer, "")
        for u, p in enumerate(X.payload):
            idx = (X.d_unit == u).nonzero().flatten()
            compare_rows(out, want_offs[idx], p, f"encode, unit {u} ({kind if X.flag[u] else 'coded'}), blocks {idx[:4].tolist()}...")
    else:
        out, offs, flags = assemble(X, X.payload, X.flag)
    d_out, sizes, dstatus, dsum = decode_dev(layer, params, E, B, out, offs, flags if layer in FLAGGED else None, in_len, off, lag, d_y,
                                             X.base_len, d_table, order=order, delta=delta)
    assert dsum.tolist() == [0, 0] and not bool(dstatus.any())
    assert torch.equal(sizes.to(torch.int64), torch.from_numpy(X.block_lengths()).cuda())
    if not torch.equal(d_out, d_in):
        at = int((d_out != d_in).nonzero()[0])
        raise AssertionError(f"decode differs from the input at byte {at} (block {at // B}, frame {at // (E * B)})")
    assert guards_intact(big_y, lo_y, X.base_len)
    del big_in, d_in, out, d_out, big_y, d_y
    _free()


@pytest.mark.parametrize("key,ragged", CASES)
def test_layer_on_instance(rx, key, ragged):
    run_row(key, ragged)


def test_mixed_layouts_chosen_on_the_device(rx):
    """One mixed row once more with layouts_mask 0xFF: the streams are the oracle's on mixed_ref(x, the table the call
    returned), and the round trip holds."""
    run_row("mixed_coop_whole_cb32", "C", mask=0xFF)


SPOILED = [("const_e8_pair_below_coop_min", "flag"), ("const_e8_pair_below_coop_min", "byte"), ("mixed_pair_by_blocks_cb32", "byte"),
           ("zigzag_e8_pair_below_coop_min", "byte"), ("lag_e8_pair_below_coop_min", "byte"), ("base_e8_pair_below_coop_min", "byte"),
           ("base_sub_e8_pair_below_coop_min", "byte"), ("lag_order_e8_pair_below_coop_min", "byte"),
           ("record_r256_pair_below_coop_min", "byte")]


@pytest.mark.parametrize("key,what", SPOILED)
def test_a_corrupted_reference_fails_its_row(rx, key, what):
    """One row of every later layer with one expected byte (constant blocks: also one flag) made wrong on the reference side:
    the row fails, and the message names the block and the unit."""
    with pytest.raises(AssertionError, match=r"block \d+ \(unit \d+\): flag 1, expected 0" if what == "flag"
                       else r"encode, unit \d+ \(coded\), blocks \[\d+.*: row \d+ .* differs at byte \d+ of \d+"):
        run_row(key, "C", spoil=what)
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
             "stored_e4_pair_by_blocks_cb32", "planes_e8_single32_by_workspace", "delta_e2_gen_below_8", "planes_e2_any",
             # the later layers: constant blocks at E = 1 on the caller's buffer, and with a base that ends inside a chunk
             "const_e1_single16_by_alignment", "const_e2_pair_by_blocks_cb16", "mixed_pair_by_blocks_cb32",
             "zigzag_e4_pair_by_blocks_cb32", "lag_e4_pair_by_blocks_cb32", "base_e4_pair_by_blocks_cb32",
             "base_sub_e2_single32_by_workspace", "lag_order_e4_pair_by_blocks_cb32", "record_r17_pair_by_blocks_cb32"]


@pytest.mark.parametrize("key", HOST_KEYS)
def test_host_pointer_forms_with_crc_equal_the_dev_calls(rx, key):
    import torch
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    lag, base, order, delta = EXTRA.get(key, (None, None, None, None))
    X = Launch(layer, params, E, B, nb, _seed(key), "S", lag=lag, base=base, order=order, delta=delta)
    big_in, d_in, lo_in = X.device_input(off)
    big_y, d_y, lo_y = X.device_base()
    d_table = torch.from_numpy(X.table).cuda() if layer == MIXED else None
    out, offs, status, summ, flags = encode_dev(layer, params, E, B, d_in, X.in_len, ws, lag, d_y, X.base_len, d_table, order=order,
                                                delta=delta)
    x = d_in.cpu().numpy()
    total = int(offs[-1])
    kw = {"unit_layouts": X.table} if layer == MIXED else {"record_size": E} if layer == RECORD else {"element_size": E}
    if layer == RECORD and delta:
        kw["filter"] = "delta"
    if layer in (DELTA, ZIGZAG, LAG):
        kw["filter"] = layer
    if layer == LAG_ORDER:
        kw.update(filter="lag", lag=lag, order=order)
    if layer == LAG:
        kw["lag"] = lag
    if X.base_len:
        kw["base"] = d_y.cpu().numpy()
    if layer == BASE_SUB:
        kw["base_op"] = "sub"
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, len(x), B)]
    chunk = -(-nb // 64 // 4) * 64 * B                         # four chunks of whole waves, or five
    assert base != "inside" or 0 < X.base_len % chunk          # (the base ends inside a chunk)
    try:
        rx.host_set_chunk_bytes(chunk, chunk)
        assert rx.host_chunk_plan(nb, B)[1] >= 3
        crc = np.zeros(nb, np.uint32)
        hflags = np.full(nb, 0xEE, np.uint8)
        if layer in FLAGGED:
            opt = {"stored": hflags, "store_ratio": 65536} if layer == STORED else {"constant": hflags}
            h_out, h_offs, h_st = rx.compress_blocks(x, B, params, block_crc=crc, **opt, **kw)
            assert hflags.tolist() == flags.cpu().tolist()
        else:
            h_out, h_offs, h_st = rx.compress_blocks(x, B, params, block_crc=crc, **kw)
        assert not h_st.any() and crc.tolist() == want_crc
        assert h_offs.astype(np.int64).tolist() == offs.cpu().tolist()
        assert np.array_equal(h_out, out[:total].cpu().numpy())
        dcrc = np.zeros(nb, np.uint32)
        if layer in FLAGGED:
            kw["stored" if layer == STORED else "constant"] = hflags
        back, sizes, st = rx.decompress_blocks(h_out, h_offs, B, params, length=len(x), block_crc=dcrc, **kw)
        assert not st.any() and np.array_equal(back, x) and dcrc.tolist() == want_crc
        assert sizes.astype(np.int64).tolist() == X.block_lengths().tolist()
    finally:
        rx.host_set_chunk_bytes(0, 0)
    del big_in, d_in, out
    _free()


# ---- 4. the transform kernels where a frame ends inside a wave's turn -------------------------------------------------------------
def run_transform(rx, x, E, B, delta, inverse):
    """delta: False (byte planes), True (the delta filter), "zigzag", or the lag S of the lag filter"""
    import torch
    n = len(x)
    ts, src, slo = guarded(n)
    src.copy_(torch.from_numpy(x).cuda())
    td, dst, dlo = guarded(n)
    if delta == "zigzag":
        rx.api.zigzag_planes(src, E, B, inverse=inverse, out=dst)
    elif delta is not True and delta is not False:
        rx.api.lag_planes(src, E, B, delta, inverse=inverse, out=dst)
    else:
        (rx.delta_planes if delta else rx.planes)(src, E, B, inverse=inverse, out=dst)
    torch.cuda.synchronize()
    assert guards_intact(td, dlo, n) and guards_intact(ts, slo, n)
    return dst.cpu().numpy()


def restated(x, E, B, delta, inverse):
    if delta == "zigzag":
        return zigzag_planes_ref(x, E, B, inverse=inverse)
    if delta is not True and delta is not False:
        return lag_planes_ref(x, E, B, delta, inverse=inverse)
    return delta_planes_ref(x, E, B, inverse=inverse) if delta else planes_ref(x, E, B, inverse=inverse)


@pytest.mark.parametrize("B", [65520, 65552, 100_000, 1 << 20])
@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_transform_kernels_at_frames_that_end_inside_a_turn(rx, E, B):
    """Three full frames and a short one (a third of a frame, five elements and E - 1 trailing bytes); uniform bytes: taken
    as differences by the inverse their running sums wrap mod 2^(8E) every few elements, in the partial last turn of every
    frame too; and all-0xFF differences, whose sum steps down by one.  Byte planes, the delta filter, the zigzag filter and
    the lag filter at S = 3, 255 and 256."""
    rng = np.random.default_rng(E * 1000 + B % 997)
    n = 3 * E * B + (B // 3 + 5) * E + E - 1
    inputs = [rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0xFF, np.uint8)]
    for x in inputs:
        for delta in (False, True, "zigzag", 3, 255, 256):
            if E == 1 and delta is False:
                continue
            for inverse in (False, True):
                want = restated(x, E, B, delta, inverse)
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


def test_lag_kernels_at_one_very_long_frame(rx):
    """B = 2^22 + 16, E = 2, S = 5: a frame of 2^18 + 1 groups, 1025 rows of the fused kernels with one group in the last
    row (the carry and the tile are reused 1024 times inside one frame), then a short frame; both directions."""
    E, B, S = 2, (1 << 22) + 16, 5
    assert B // 16 == 1024 * 256 + 1
    x = np.random.default_rng(22).integers(0, 256, E * B + (B // 3 + 5) * E + 1, dtype=np.uint8)
    for inverse in (False, True):
        want = lag_planes_ref(x, E, B, S, inverse=inverse)
        got = run_transform(rx, x, E, B, S, inverse)
        if not np.array_equal(got, want):
            at = int(np.nonzero(got != want)[0][0])
            raise AssertionError(f"inverse={inverse}: first difference at byte {at} (frame {at // (E * B)}, element {at % (E * B) // E})")


def test_fused_lag_inverse_with_more_frames_than_workgroups(rx):
    """E = 1, B = 4112 (257 groups: two rows a frame, so the chains' carry is live), S = 3, 2^20 + 3 frames and a short one,
    past 2^32 bytes: the grid-stride loop of k_lag_unplanes, which reuses carry[] and the tile from frame to frame.  The input
    is tiled on the device from 8 distinct frames in an aperiodic order, the expected output is the same tiling of the
    per-frame restatement, compared on the device; the forward kernel takes the result back to the input."""
    import torch
    E, B, S, nf, short = 1, 4112, 3, (1 << 20) + 3, 1237
    rng = np.random.default_rng(4112)
    frames = rng.integers(0, 256, (8, B), dtype=np.uint8)
    last = rng.integers(0, 256, short, dtype=np.uint8)
    f = torch.arange(nf, device="cuda:0")
    idx = (f * f // 7 + f // 5 + f) % 8                                      # (no period)
    assert len(set(np.diff(np.nonzero((idx[:4096] == 0).cpu().numpy())[0]).tolist())) > 4
    n = nf * B + short
    assert n > 1 << 32
    ts, src, slo = guarded(n)
    src[: nf * B].view(nf, B).copy_(torch.from_numpy(frames).cuda()[idx])
    src[nf * B:].copy_(torch.from_numpy(last).cuda())
    want = torch.from_numpy(np.stack([lag_planes_ref(fr, E, B, S, inverse=True) for fr in frames])).cuda()
    want_last = torch.from_numpy(lag_planes_ref(last, E, B, S, inverse=True)).cuda()
    td, dst, dlo = guarded(n)
    rx.api.lag_planes(src, E, B, S, inverse=True, out=dst)
    torch.cuda.synchronize()
    assert guards_intact(td, dlo, n) and guards_intact(ts, slo, n)
    step = 1 << 17
    for f0 in range(0, nf, step):
        got = dst[f0 * B: min(f0 + step, nf) * B].view(-1, B)
        bad = (got != want[idx[f0: f0 + step]]).any(1)
        if bool(bad.any()):
            fr = f0 + int(bad.nonzero()[0])
            at = int((dst[fr * B: (fr + 1) * B] != want[idx[fr]]).nonzero()[0])
            raise AssertionError(f"frame {fr} (distinct frame {int(idx[fr])}) differs at byte {at}")
    assert torch.equal(dst[nf * B:], want_last)
    tb, back, blo = guarded(n)
    rx.api.lag_planes(dst, E, B, S, inverse=False, out=back)
    torch.cuda.synchronize()
    assert guards_intact(tb, blo, n) and guards_intact(td, dlo, n)
    assert torch.equal(back, src)
    del ts, src, td, dst, tb, back
    _free()


@pytest.mark.parametrize("S", [3, 256])
def test_byte_lag_inverse_past_2_pow_20_frames(rx, S):
    """E = 1, B = 400 (no multiple of 16: the byte kernels; two iterations of 256 elements a frame, so the chains' carry in
    last[][] is live, and par goes on from frame to frame), 2^20 + 3 frames and a short one: the grid-stride loop of
    k_lag_unplanes_bytes.  (About a second, nearly all of it numpy over the 419 MB of the restatement.)"""
    E, B, nf, short = 1, 400, (1 << 20) + 3, 77
    x = np.random.default_rng(400 + S).integers(0, 256, nf * B + short, dtype=np.uint8)
    # the restatement, vectorised over the full frames (the per-frame loop of lag_planes_ref takes minutes here) ...
    body = x[: nf * B].reshape(nf, B)
    r = (body >> 1) ^ np.negative(body & 1)                             # unfold: (z >> 1) ^ (0 - (z & 1)) mod 256
    if S < B // 2:
        for c in range(S):                                               # chain c: elements c, c + S, ...
            r[:, c::S] = np.cumsum(r[:, c::S], axis=1, dtype=np.uint8)
    else:
        r[:, S:] += r[:, : B - S]                                        # (chains of two elements at the most)
    want = np.concatenate([r.reshape(-1), lag_planes_ref(x[nf * B:], E, B, S, inverse=True)])
    # ... checked against lag_planes_ref on both ends
    k = 100 * B
    assert np.array_equal(want[:k], lag_planes_ref(x[:k], E, B, S, inverse=True))
    assert np.array_equal(want[-k - short:], lag_planes_ref(x[-k - short:], E, B, S, inverse=True))
    got = run_transform(rx, x, E, B, S, True)
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"first difference at byte {at} (frame {at // B}, element {at % B})")
    assert np.array_equal(run_transform(rx, got, E, B, S, False), x)


def test_const_select_past_its_grid_cap(rx):
    """B = 16, 2^22 + 5 blocks, the last one of 5 bytes: more workgroups' worth of blocks than k_const_select's grid of 2^20.
    Constant blocks by a rule that has no period of 4 (a workgroup takes four blocks); the flags against const_ref,
    vectorised, which is checked against const_ref itself on both ends."""
    import torch
    B, nb = 16, (1 << 22) + 5
    rng = np.random.default_rng(16)
    body = rng.integers(0, 256, (nb, B), dtype=np.uint8)
    body[:, B // 2] = body[:, 0] ^ 0x55                                  # never constant by chance
    b = np.arange(nb)
    const = (b % 7 == 0) | (b % 7 == 3) | (b % 13 == 5)
    assert len({tuple(const[i: i + 4]) for i in range(0, 4096, 4)}) > 8
    body[const] = (b[const] % 251)[:, None]
    x = body.reshape(-1)[: (nb - 1) * B + 5]
    want = (body == body[:, :1]).all(1).astype(np.uint8)
    want[-1] = (x[-5:] == x[-5]).all()
    assert np.array_equal(want, const.astype(np.uint8) | np.r_[np.zeros(nb - 1, np.uint8), want[-1:]])
    k = 1000 * B
    assert np.array_equal(want[:1000], const_ref(x[:k], B)) and np.array_equal(want[-1000:], const_ref(x[-k + B - 5:], B))
    t, view, lo = guarded(len(x))
    view.copy_(torch.from_numpy(x).cuda())
    ft, flags, flo = guarded(nb)
    assert _lib().lib().redux_const_blocks_dev(_v(view), len(x), B, _v(flags), None) == 0
    torch.cuda.synchronize()
    assert guards_intact(ft, flo, nb) and guards_intact(t, lo, len(x))
    got = flags.cpu().numpy()
    if not np.array_equal(got, want):
        at = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"block {at}: flag {got[at]}, expected {want[at]}")


# ---- 5. damaged streams on the new decode paths ---------------------------------------------------------------------------------
DAMAGED_KEYS = ["stored_e1_coop_windows_100k", "stored_e4_table_generic32", "planes_e8_cells8", "delta_e2_cells8",
                "lag_order_e2_coop_windows_150k",       # (k_decode_wave and the fix-up pass in front of the K-level inverse)
                "record_r2_coop_windows_150k"]          # (... and in front of the record layout's inverse)


@pytest.mark.parametrize("key", DAMAGED_KEYS)
def test_damaged_streams_on_the_new_decode_paths(rx, key):
    """Three coded blocks with one flipped bit, three cut to two thirds, the rest intact: status and size of every block are
    the oracle's (through the layout's length rule), and so are the bytes the damaged blocks decoded to, seen through the
    inverse transform of their frames; the frames whose blocks are all OK hold the original bytes; the guard bands stay."""
    import torch
    layer, params, E, B, nb, off, ws, enc, dec, _ = ROWS[key]
    assert layer_dec_name(layer, params, B, nb) == dec
    lag, _, order, delta = EXTRA.get(key, (None, None, None, None))
    X = Launch(layer, params, E, B, nb, _seed(key), "C", lag=lag, order=order, delta=delta)
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
    d_out, sizes, status, dsum = decode_dev(layer, params, E, B, flat, offs, flags, X.in_len, off, lag, order=order, delta=delta)
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
        t = transform(layer, X.frames[X.plan[f]], E, B, lag=lag, order=order, delta=delta).copy()
        m = B
        for b in picks:
            if b // E == f:
                d = np.frombuffer(partial[b], dtype=np.uint8)
                j = b % E
                t[j * B: j * B + len(d)] = d
                m = min(m, len(d))
        want = transform(layer, t, E, B, inverse=True, lag=lag, order=order, delta=delta)[: m * E]
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
