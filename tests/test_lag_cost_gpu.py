"""Lag estimates on the GPU (include/redux_hip.h, "lag estimates"): k_lag_cost and k_lag_cost_bytes against k_block_cost
of what redux_lag_planes_dev writes, lag by lag, and against the library's host rule on the numpy restatement of the filter.
Shapes are the smallest at which a lane group, a row, a frame, the masked first chunk, a fold or a workgroup boundary can go
wrong.  Every input lies between poisoned bytes: a byte read before a frame's first, or past the input's last, would show in
the counts."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_lag_auto_cpu import block_counts, block_count_ref, sampled_columns
from test_lag_cpu import lag_planes_ref

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
TOL = 2.0 ** -10          # bits (tests/test_layout_cost_gpu.py): both sides sum at most 258 f64 terms below 2^27 bits
GUARD = 8                 # doubles on either side of the result
LEAD = 4096               # poisoned bytes in front of the input: more than the 256 * 8 bytes the largest lag reaches back
POISON = 0xA7


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _data(kind, n):
    rng = np.random.default_rng(len(kind) * 1000003 + n)
    if kind == "iid":
        return rng.integers(0, 256, n).astype(np.uint8)
    if kind == "one":                                                    # one byte value: at lag 1 every folded difference
        return np.full(n, 0xC3, dtype=np.uint8)                          # behind a frame's first element is zero
    v = np.stack([np.cumsum(rng.integers(-40, 41, n // 6 + 1)) + 3000 * c for c in range(3)], 1)   # "walk": three channels
    return v.reshape(-1).astype("<i2").view(np.uint8)[:n].copy()


# rows a wave counts between folds (redux_layout_cost.hpp: kLayoutFoldRows = 65535 // (16 E)); a row is 1 KiB of each plane
FOLD_ROWS = {1: 4095, 2: 2047, 4: 1023, 8: 511}
LAGS = [1, 2, 3, 15, 16, 17, 255, 256]
AROUND_16_BYTES = {1: [15, 16, 17], 2: [7, 8, 9], 4: [3, 4, 5], 8: [1, 2, 3]}  # S * E below, at and above a 16-byte chunk


def _lags(E):
    return sorted(set(LAGS + AROUND_16_BYTES[E])) + [3]  # (a repeated lag at the end)


def _above_fold(E):
    return FOLD_ROWS[E] * 1024 + 16


# (E, block size, input length, offset of d_in from a 16-byte boundary, data, lags)
CASES = []
for _E in (1, 2, 4, 8):
    CASES += [
        (_E, 64, 0, 0, "iid", [1, 256]), (_E, 64, 1, 0, "iid", [1, 2]), (_E, 64, max(_E - 1, 1), 0, "iid", [1, 3]),
        (_E, 64, 63, 0, "walk", _lags(_E)),
        # one frame at B = 64: 64 elements, so the lags from 64 on only fold and give equal rows
        (_E, 64, _E * 64, 0, "walk", _lags(_E) + [63, 64, 65]),
        # three frames and a short one whose length is no multiple of E
        (_E, 4096, 3 * _E * 4096 + 4096 + 5, 0, "walk", _lags(_E)),
        # a frame of fewer groups than a wave has lanes, and a last row that is not full (B / 16 = 100 groups)
        (_E, 256, _E * 256 * 3, 0, "walk", _lags(_E)), (_E, 1600, _E * 1600 * 2 + 77, 0, "walk", _lags(_E)),
        # B = 48 is three groups of 16: the fast path with three lanes; 40 and 1000 are no multiples of 16: the byte path
        (_E, 48, 1000, 0, "walk", _lags(_E)), (_E, 40, 1000, 0, "walk", _lags(_E)), (_E, 1000, _E * 1000 * 2 + 9, 0, "walk", [1, 3, 17, 256]),
        # a buffer off a 16-byte boundary: the byte path
        (_E, 4096, 2 * _E * 4096, 1, "walk", [1, 3, 16]), (_E, 4096, _E * 4096 + 100, 15, "iid", [2, 3, 255]),
        # 8,192 blocks of 256 bytes: more jobs than launched workgroups, the grid-stride walk
        (_E, 256, 2 << 20, 0, "walk", [1, 3, 256]),
        # the counter fold inside a block: one byte value, 16 bytes above the bound of kLayoutFoldRows
        (_E, _above_fold(_E), _E * _above_fold(_E), 0, "one", [1, 2]),
    ]
# E = 1, B = 5120: five rows of 64 groups, no multiple of the eight rows of a step; one, four and five lags (one wave of a
# workgroup, all four, and one of a second job)
CASES += [(1, 5120, 3 * 5120 + 100, 0, "walk", _l) for _l in ([3], [1, 3, 2, 256], [3, 1, 17, 2, 255])]


def _place(a, shift):
    """a device copy of `a` that starts `shift` bytes after a 16-byte boundary, with poison before and behind it"""
    import torch
    buf = torch.full((len(a) + LEAD + 64,), POISON, dtype=torch.uint8, device="cuda")
    at = LEAD + (-(buf.data_ptr() + LEAD)) % 16 + shift
    d = buf[at: at + len(a)]
    d.copy_(torch.from_numpy(a))
    return d


def _run(lib, d, E, B, lags, step=1, params=P):
    """redux_lag_cost_dev on the device tensor d, into a result that was filled with NaN and lies between NaN guards
    -> f64[len(lags), block_count]"""
    import torch
    L = lib.lib()
    n = d.numel()
    nb = L.redux_lag_cost_block_count(n, B, E, step)
    assert nb == block_count_ref(n, B, E, step)
    out = torch.full((len(lags) * nb + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    cp = lib.Params(*params)
    h_lags = np.asarray(lags, dtype=np.uint32)
    st = L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, E, h_lags.ctypes.data, len(lags), step,
                              C.c_void_p(out.data_ptr() + 8 * GUARD), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    h_lags[:] = 0  # (the list was consumed by the call)
    assert st == lib.OK
    h = out.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + len(lags) * nb:]).all(), "guard words around d_bits were written"
    got = h[GUARD: GUARD + len(lags) * nb].reshape(len(lags), nb)
    assert not np.isnan(got).any(), "a block of the result was not written"
    return got


def _composed(rx, d, E, B, S):
    """k_block_cost of what redux_lag_planes_dev writes: the parent's kernels"""
    import torch
    if d.numel() == 0:
        return rx.block_cost(torch.empty(0, dtype=torch.uint8, device="cuda"), B, P)
    return rx.block_cost(rx.api.lag_planes(d.clone(), E, B, S), B, P)


def _host(rx, a, E, B, S):
    return rx.adaptive_cost_from_counts(block_counts(lag_planes_ref(a, E, B, S), B), P)


@pytest.mark.parametrize("E,B,n,shift,kind,lags", CASES)
def test_lag_cost_equals_block_cost_of_the_filtered_input(rx, lib, E, B, n, shift, kind, lags):
    a = _data(kind, n)
    d = _place(a, shift)
    got = _run(lib, d, E, B, lags)
    worst_host = worst_dev = 0.0
    for j, S in enumerate(lags):
        host, composed = _host(rx, a, E, B, S), _composed(rx, d, E, B, S)
        assert got[j].shape == host.shape == composed.shape, (S, got[j].shape, host.shape, composed.shape)
        worst_host, worst_dev = max(worst_host, np.abs(got[j] - host).max()), max(worst_dev, np.abs(got[j] - composed).max())
        assert np.abs(got[j] - host).max() <= TOL and np.abs(got[j] - composed).max() <= TOL, (E, B, n, shift, S)
    print("E %d, B %d, %d bytes, +%d, %s, %d lags: max |lag_cost - host rule| = %.3g, - block_cost(lag_planes) = %.3g bits"
          % (E, B, n, shift, kind, len(lags), worst_host, worst_dev))
    if lags[-1] == 3 and lags.index(3) < len(lags) - 1:  # a repeated lag: equal, independent rows
        assert np.array_equal(got[lags.index(3)], got[-1])
    N = min(n, E * B) // E
    flat = [j for j, S in enumerate(lags) if S >= N]  # S >= every frame's element count: only folds, all such rows equal
    assert all(np.array_equal(got[flat[0]], got[j]) for j in flat)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_all_256_lags_in_one_call(rx, lib, E):
    B = 1024
    a = _data("walk", 3 * E * B + B + 5)
    d = _place(a, 0)
    lags = list(range(1, 257))
    got = _run(lib, d, E, B, lags)
    host = np.stack([_host(rx, a, E, B, S) for S in lags])
    composed = np.stack([_composed(rx, d, E, B, S) for S in lags])
    print("E %d: 256 lags, max |lag_cost - host rule| = %.3g, - block_cost(lag_planes) = %.3g bits"
          % (E, np.abs(got - host).max(), np.abs(got - composed).max()))
    assert np.abs(got - host).max() <= TOL and np.abs(got - composed).max() <= TOL
    if E == 2:
        assert int(np.argmin(got.sum(axis=1))) + 1 == 3  # (three int16 channels)


@pytest.mark.parametrize("E,B,shift", [(1, 256, 0), (2, 4096, 0), (4, 256, 0), (8, 64, 0), (2, 256, 1), (4, 40, 0)])
def test_frame_sampling_keeps_the_selected_columns(rx, lib, E, B, shift):
    a = _data("walk", 3 * E * B + (B + 5 if E > 1 else B // 2 + 5))  # four frames, the last a short one
    d = _place(a, shift)
    lags = [1, 3, 17, 256, 3]
    full = _run(lib, d, E, B, lags)
    nb = full.shape[1]
    for step in (2, 3, 4, 5, 1 << 31):  # 2: the short frame is not selected; 3: it is; 5 and above: the first frame alone
        got = _run(lib, d, E, B, lags, step)
        cols = sampled_columns(nb, E, step)
        assert got.shape == (len(lags), len(cols)) and np.array_equal(got, full[:, cols]), (E, B, shift, step)
    assert sampled_columns(nb, E, 5) == list(range(E)) and sampled_columns(nb, E, 3)[E:] == list(range(3 * E, nb))


def test_api_lag_cost_and_estimates(rx):
    import torch
    from redux_amd import api, container
    E, B = 2, 4096
    a = _data("walk", 3 * E * B + B + 5)
    lags = [1, 2, 3, 6, 256]
    host = np.stack([_host(rx, a, E, B, S) for S in lags])
    got = rx.lag_cost(a.tobytes(), E, lags, B)                              # host data, uploaded
    assert got.shape == host.shape and got.dtype == np.float64 and np.abs(got - host).max() <= TOL
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = rx.lag_cost(torch.from_numpy(a).cuda(), E, np.array(lags), B, P, frame_step=3)  # a device tensor, on a side stream
    nb = host.shape[1]
    assert np.abs(dev - host[:, sampled_columns(nb, E, 3)]).max() <= TOL
    est = rx.estimate_lags(a, E, B, lags)
    assert est == {S: int(np.ceil(host[j].sum() / 8 + api.TERMINATION_BYTES * nb)) for j, S in enumerate(lags)}
    every = rx.estimate_lags(a, E, B)
    assert list(every) == list(range(1, 257)) and all(every[S] == est[S] for S in lags) and min(every, key=every.get) == 3
    cols = sampled_columns(nb, E, 2)
    assert rx.estimate_lags(a, E, B, [3], frame_step=2) == {3: int(np.ceil(host[2][cols].sum() / 8 + api.TERMINATION_BYTES * len(cols)))}
    for checksum in (False, True):
        over = container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="lag")
        assert container.estimate_lag_bytes(a, E, B, lags, checksum=checksum) == {S: est[S] + over for S in lags}
    assert rx.choose_lag(a, E, B) == (3, every)                            # four frames: one exact pass
    with pytest.raises(rx.Unsupported):
        rx.lag_cost(a, E, [1], 65536, (8, 14, 16))                         # a 64 KiB block can freeze the 14-bit model


def test_refusals_and_kernel_names(lib):
    import torch
    L = lib.lib()
    d = torch.zeros(4096 + 32, dtype=torch.uint8, device="cuda")
    at = d.data_ptr() + (-d.data_ptr()) % 16
    out = torch.zeros(256 * 4, dtype=torch.float64, device="cuda")
    lags = np.array([1, 2, 3, 256], dtype=np.uint32)

    def call(params=P, B=64, E=2, lg=lags, nl=4, T=1, pin=at, bits=out.data_ptr(), n=4096):
        cp = lib.Params(*params)
        return L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(pin) if pin else None, n, B, E, lg.ctypes.data if lg is not None else None,
                                    nl, T, C.c_void_p(bits) if bits else None, None)
    assert call() == lib.OK
    assert call(B=0) == lib.INVALID_INPUT and call(B=(1 << 30) + 1) == lib.INVALID_INPUT
    assert call(E=3) == lib.INVALID_INPUT and call(E=0) == lib.INVALID_INPUT and call(E=16) == lib.INVALID_INPUT
    assert call(nl=0) == lib.INVALID_INPUT and call(lg=np.ones(257, np.uint32), nl=257) == lib.INVALID_INPUT
    assert call(lg=np.array([1, 0, 3, 4], np.uint32)) == lib.INVALID_INPUT and call(lg=np.array([1, 2, 3, 257], np.uint32)) == lib.INVALID_INPUT
    assert call(T=0) == lib.INVALID_INPUT and call(lg=None) == lib.INVALID_INPUT and call(bits=None) == lib.INVALID_INPUT
    assert call(pin=None) == lib.INVALID_INPUT and call(pin=None, n=0) == lib.OK
    assert call(lg=np.full(256, 256, np.uint32), nl=256, B=1024) == lib.OK   # 256 rows of 4 blocks
    assert call(params=(12, 14, 16)) == lib.UNSUPPORTED                      # symbol_bits != 8
    assert call(params=(8, 24, 40)) == lib.UNSUPPORTED                       # code_bits > 32
    assert call(params=(8, 14, 16), B=16383 - 256, n=4096) == lib.UNSUPPORTED  # 256 + block_size >= freq_max = 2^14 - 1
    assert call(params=(8, 14, 16), B=16383 - 257, n=4096) == lib.OK
    torch.cuda.synchronize()
    B = 256
    for E in (1, 2, 4, 8):
        fast, general = b"k_lag_cost<%d>" % E, b"k_lag_cost_bytes<%d>" % E
        n = 4096 // (E * B) * (E * B)
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(at), n, B, E) == fast
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(at), n + 5, B, E) == fast + b" + " + general
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(at + 1), n, B, E) == general          # the unaligned buffer
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(at + 16), 1000, 48, E) == fast + b" + " + general
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(at), n, 40, E) == general
        assert L.redux_lag_cost_kernel_name(n, B, E) == fast and L.redux_lag_cost_kernel_name(0, B, E) == general
    assert L.redux_lag_cost_kernel_name(4096, 4096, 3) == b"" and L.redux_lag_cost_kernel_name(4096, 0, 2) == b""
