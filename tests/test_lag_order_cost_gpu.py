"""Order estimates on the GPU (include/redux_hip.h, "order estimates"): k_lag_order_cost and k_lag_order_cost_bytes against
k_block_cost of what redux_lag_order_planes_dev writes, candidate by candidate, and against the library's host rule on the
numpy restatement of the filter.  Shapes are the smallest at which a lane group, a row, a frame, the masked chunk of each of
the three predecessors, a fold or the grid stride can go wrong.  Every input lies between poisoned bytes: a byte read before a
frame's first, or past the input's last, would show in the counts."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_lag_auto_cpu import block_counts, block_count_ref, sampled_columns
from test_lag_order_cpu import lag_order_planes_ref

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
TOL = 2.0 ** -10          # bits (tests/test_lag_cost_gpu.py): both sides sum at most 258 f64 terms below 2^27 bits
GUARD = 8                 # doubles on either side of the result
LEAD = 8192               # poisoned bytes in front of the input: more than the 3 * 256 * 8 bytes the furthest term reaches back
POISON = 0xA7
ORDERS = (1, 2, 3)


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
    if kind == "one":                                                    # one byte value: behind the first K S elements of a
        return np.full(n, 0xC3, dtype=np.uint8)                          # frame every folded difference is zero
    v = np.stack([np.cumsum(rng.integers(-40, 41, n // 6 + 1)) + 3000 * c for c in range(3)], 1)   # "walk": three channels
    return v.reshape(-1).astype("<i2").view(np.uint8)[:n].copy()


# rows a wave counts between folds (redux_layout_cost.hpp: kLayoutFoldRows = 65535 // (16 E)); a row is 1 KiB of each plane
FOLD_ROWS = {1: 4095, 2: 2047, 4: 1023, 8: 511}
# S E, 2 S E and 3 S E below, at and above a multiple of 16 bytes: S E = 16 at S = 16 / E with its neighbours; 2 S E = 16 at
# S = 8 / E (E = 8: every 2 S E is a multiple of 16); 3 S E = 48 at S = 16 / E again, and S = 5, 6 (E = 1), 2, 3 (E = 2, 4) and
# 1 (E = 8) put 3 S E on either side of 16 or 24
AROUND = {1: [5, 6, 7, 8, 9, 15, 16, 17], 2: [2, 3, 4, 5, 7, 8, 9], 4: [1, 2, 3, 4, 5], 8: [1, 2, 3]}


def _cands(lags, orders=ORDERS):
    return [(S, K) for S in lags for K in orders]  # (by lag first: every workgroup mixes the orders)


def _lags(E):
    return sorted(set([1, 2, 3, 255, 256] + AROUND[E]))


def _above_fold(E):
    return FOLD_ROWS[E] * 1024 + 16


# (E, block size, input length, offset of d_in from a 16-byte boundary, data, candidates)
CASES = []
for _E in (1, 2, 4, 8):
    CASES += [
        (_E, 64, 0, 0, "iid", _cands([1, 256])), (_E, 64, 1, 0, "iid", _cands([1, 2])), (_E, 64, max(_E - 1, 1), 0, "iid", _cands([1, 3])),
        # one frame at B = 64, N = 64 elements: lags around N / 3, N / 2 and N.  22 .. 32 have 2 S <= N < 3 S (the third term
        # never exists), 33 .. 63 have S < N < 2 S, and from 64 on S >= N: only folds, every order gives the same row
        (_E, 64, _E * 64, 0, "walk", _cands([20, 21, 22, 31, 32, 33, 63, 64, 65, 256]) + [(21, 3)]),
        # three frames and a short one whose length is no multiple of E
        (_E, 4096, 3 * _E * 4096 + 4096 + 5, 0, "walk", _cands(_lags(_E)) + [(3, 2)]),
        # a frame of fewer groups than a wave has lanes, and a last row that is not full (B / 16 = 100 groups)
        (_E, 256, _E * 256 * 3, 0, "walk", _cands(_lags(_E))), (_E, 1600, _E * 1600 * 2 + 77, 0, "walk", _cands(_lags(_E))),
        # B = 48 is three groups of 16: the fast path with three lanes; 40 and 1000 are no multiples of 16: the byte path
        (_E, 48, 1000, 0, "walk", _cands(_lags(_E))), (_E, 40, 1000, 0, "walk", _cands(_lags(_E))),
        (_E, 1000, _E * 1000 * 2 + 9, 0, "walk", _cands([1, 3, 17, 256])),
        # a buffer off a 16-byte boundary: the byte path
        (_E, 4096, 2 * _E * 4096, 1, "walk", _cands([1, 3, 16])), (_E, 4096, _E * 4096 + 100, 15, "iid", _cands([2, 3, 255])),
        # 8,192 blocks of 256 bytes, three candidates: more jobs than launched workgroups, the grid-stride walk
        (_E, 256, 2 << 20, 0, "walk", [(1, 1), (3, 2), (256, 3)]),
        # the counter fold inside a block: one byte value, 16 bytes above the bound of kLayoutFoldRows, at order 3
        (_E, _above_fold(_E), _E * _above_fold(_E), 0, "one", [(1, 3), (2, 3)]),
    ]
# E = 1, B = 5120: five rows of 64 groups, a multiple of neither k_lag_order_cost's four rows a step nor k_lag_cost's eight;
# one, four and five candidates (one wave of a workgroup, all four, and one of a second job), the orders mixed
CASES += [(1, 5120, 3 * 5120 + 100, 0, "walk", _c) for _c in
          ([(3, 2)], [(1, 1), (3, 3), (2, 2), (256, 1)], [(3, 3), (1, 1), (17, 2), (3, 1), (255, 3)])]


def _place(a, shift):
    """a device copy of `a` that starts `shift` bytes after a 16-byte boundary, with poison before and behind it"""
    import torch
    buf = torch.full((len(a) + LEAD + 64,), POISON, dtype=torch.uint8, device="cuda")
    at = LEAD + (-(buf.data_ptr() + LEAD)) % 16 + shift
    d = buf[at: at + len(a)]
    d.copy_(torch.from_numpy(a))
    return d


def _run(lib, d, E, B, cands, step=1, params=P):
    """redux_lag_order_cost_dev on the device tensor d, into a result that was filled with NaN and lies between NaN guards
    -> f64[len(cands), block_count]"""
    import torch
    L = lib.lib()
    n = d.numel()
    nb = L.redux_lag_cost_block_count(n, B, E, step)
    assert nb == block_count_ref(n, B, E, step)
    out = torch.full((len(cands) * nb + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    cp = lib.Params(*params)
    h_lags = np.asarray([S for S, _ in cands], dtype=np.uint32)
    h_orders = np.asarray([K for _, K in cands], dtype=np.uint32)
    st = L.redux_lag_order_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, E, h_lags.ctypes.data,
                                    h_orders.ctypes.data, len(cands), step, C.c_void_p(out.data_ptr() + 8 * GUARD),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    h_lags[:] = 0  # (both lists were consumed by the call)
    h_orders[:] = 0
    assert st == lib.OK
    h = out.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + len(cands) * nb:]).all(), "guard words around d_bits were written"
    got = h[GUARD: GUARD + len(cands) * nb].reshape(len(cands), nb)
    assert not np.isnan(got).any(), "a block of the result was not written"
    return got


def _run_lag_cost(lib, d, E, B, lags):
    """redux_lag_cost_dev, the parent's order-1 estimate -> f64[len(lags), block_count]"""
    import torch
    L = lib.lib()
    n = d.numel()
    out = torch.full((len(lags), L.redux_lag_cost_block_count(n, B, E, 1)), float("nan"), dtype=torch.float64, device="cuda")
    cp = lib.Params(*P)
    h_lags = np.asarray(lags, dtype=np.uint32)
    assert L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, E, h_lags.ctypes.data, len(lags), 1,
                                C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == lib.OK
    return out.cpu().numpy()


def _composed(rx, d, E, B, S, K):
    """k_block_cost of what redux_lag_order_planes_dev writes: the parent's kernels"""
    import torch
    if d.numel() == 0:
        return rx.block_cost(torch.empty(0, dtype=torch.uint8, device="cuda"), B, P)
    return rx.block_cost(rx.api.lag_order_planes(d.clone(), E, B, S, K), B, P)


def _host(rx, a, E, B, S, K):
    return rx.adaptive_cost_from_counts(block_counts(lag_order_planes_ref(a, E, B, S, K), B), P)


@pytest.mark.parametrize("E,B,n,shift,kind,cands", CASES)
def test_lag_order_cost_equals_block_cost_of_the_filtered_input(rx, lib, E, B, n, shift, kind, cands):
    a = _data(kind, n)
    d = _place(a, shift)
    got = _run(lib, d, E, B, cands)
    worst_host = worst_dev = 0.0
    refs = {}
    for j, (S, K) in enumerate(cands):
        if (S, K) not in refs:
            refs[S, K] = (_host(rx, a, E, B, S, K), _composed(rx, d, E, B, S, K))
        host, composed = refs[S, K]
        assert got[j].shape == host.shape == composed.shape, (S, K, got[j].shape, host.shape, composed.shape)
        worst_host, worst_dev = max(worst_host, np.abs(got[j] - host).max()), max(worst_dev, np.abs(got[j] - composed).max())
        assert np.abs(got[j] - host).max() <= TOL and np.abs(got[j] - composed).max() <= TOL, (E, B, n, shift, S, K)
    print("E %d, B %d, %d bytes, +%d, %s, %d candidates: max |lag_order_cost - host rule| = %.3g, - block_cost(lag_order_planes) = %.3g bits"
          % (E, B, n, shift, kind, len(cands), worst_host, worst_dev))
    if cands.index(cands[-1]) < len(cands) - 1:  # a repeated candidate: equal, independent rows
        assert np.array_equal(got[cands.index(cands[-1])], got[-1])
    N = min(n, E * B) // E
    flat = [j for j, (S, K) in enumerate(cands) if S >= N]  # S >= every frame's element count: only folds, at every order
    assert all(np.array_equal(got[flat[0]], got[j]) for j in flat)
    if B == 64 and n == E * 64:
        assert len(flat) == 9  # (lags 64, 65 and 256 at three orders)
    # the order-1 rows against redux_lag_cost_dev's
    ones = [j for j, (S, K) in enumerate(cands) if K == 1]
    if ones:
        lag_rows = _run_lag_cost(lib, d, E, B, [cands[j][0] for j in ones])
        diff = np.abs(got[ones] - lag_rows).max()
        print("    order 1 against redux_lag_cost_dev, %d rows: max |difference| = %.3g bits" % (len(ones), diff))
        assert diff == 0.0  # (the same integer counts through the same sums: nothing may move)


@pytest.mark.parametrize("E", [1, 2, 4, 8])
def test_256_candidates_in_one_call(rx, lib, E):
    B = 1024
    a = _data("walk", 3 * E * B + B + 5)
    d = _place(a, 0)
    cands = _cands(range(1, 86)) + [(256, 3)]  # 85 lags at three orders, and the largest reach back
    assert len(cands) == 256
    got = _run(lib, d, E, B, cands)
    host = np.stack([_host(rx, a, E, B, S, K) for S, K in cands])
    composed = np.stack([_composed(rx, d, E, B, S, K) for S, K in cands])
    print("E %d: 256 candidates, max |lag_order_cost - host rule| = %.3g, - block_cost(lag_order_planes) = %.3g bits"
          % (E, np.abs(got - host).max(), np.abs(got - composed).max()))
    assert np.abs(got - host).max() <= TOL and np.abs(got - composed).max() <= TOL
    if E == 2:
        assert cands[int(np.argmin(got.sum(axis=1)))] == (3, 1)  # (three int16 walks: lag 3, and order 1 on a walk)


@pytest.mark.parametrize("E,B,shift", [(1, 256, 0), (2, 4096, 0), (4, 256, 0), (8, 64, 0), (2, 256, 1), (4, 40, 0)])
def test_frame_sampling_keeps_the_selected_columns(rx, lib, E, B, shift):
    a = _data("walk", 3 * E * B + (B + 5 if E > 1 else B // 2 + 5))  # four frames, the last a short one
    d = _place(a, shift)
    cands = [(1, 1), (3, 2), (3, 3), (17, 2), (256, 3), (3, 2)]
    full = _run(lib, d, E, B, cands)
    nb = full.shape[1]
    for step in (2, 3, 4, 5, 1 << 31):  # 2: the short frame is not selected; 3: it is; 5 and above: the first frame alone
        got = _run(lib, d, E, B, cands, step)
        cols = sampled_columns(nb, E, step)
        assert got.shape == (len(cands), len(cols)) and np.array_equal(got, full[:, cols]), (E, B, shift, step)


def test_api_lag_order_cost_and_estimates(rx):
    import torch
    from redux_amd import api, container
    E, B = 2, 4096
    a = _data("walk", 3 * E * B + B + 5)
    cands = [(1, 1), (3, 1), (3, 2), (3, 3), (256, 3)]
    host = np.stack([_host(rx, a, E, B, S, K) for S, K in cands])
    got = rx.lag_order_cost(a.tobytes(), E, cands, B)                       # host data, uploaded
    assert got.shape == host.shape and got.dtype == np.float64 and np.abs(got - host).max() <= TOL
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = rx.lag_order_cost(torch.from_numpy(a).cuda(), E, np.array(cands), B, P, frame_step=3)  # a device tensor, a side stream
    nb = host.shape[1]
    assert np.abs(dev - host[:, sampled_columns(nb, E, 3)]).max() <= TOL
    est = rx.estimate_lag_orders(a, E, B, cands + [(3, 2)])
    assert est == {c: int(np.ceil(host[j].sum() / 8 + api.TERMINATION_BYTES * nb)) for j, c in enumerate(cands)}
    assert est[(3, 1)] == rx.estimate_lags(a, E, B, [3])[3]
    cols = sampled_columns(nb, E, 2)
    assert rx.estimate_lag_orders(a, E, B, [(3, 2)], P, frame_step=2) == \
        {(3, 2): int(np.ceil(host[2][cols].sum() / 8 + api.TERMINATION_BYTES * len(cols)))}
    for checksum in (False, True):
        over = container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="lag")
        assert container.estimate_lag_order_bytes(a, E, B, cands, checksum=checksum) == {c: est[c] + over for c in cands}
    choice, table = rx.choose_lag_order(a, E, B, 3)
    assert choice == (3, 1) and table == {c: est[c] for c in ((3, 1), (3, 2), (3, 3))}   # a walk: order 1
    lag, every = rx.choose_lag(a, E, B)
    choice, table = rx.choose_lag_order(a, E, B)                             # four frames: the first stage is exact
    assert choice == (3, 1) and sorted({S for S, _ in table}) == api.lag_finalists(every) and len(table) <= 12
    assert table[choice] <= every[lag] and table[choice] <= table[(1, 1)] == every[1]
    with pytest.raises(rx.Unsupported):
        rx.lag_order_cost(a, E, [(1, 1)], 65536, (8, 14, 16))               # a 64 KiB block can freeze the 14-bit model


def test_refusals_write_nothing_and_kernel_names(lib):
    import torch
    L = lib.lib()
    d = torch.zeros(4096 + 32, dtype=torch.uint8, device="cuda")
    at = d.data_ptr() + (-d.data_ptr()) % 16
    out = torch.full((256 * 4,), float("nan"), dtype=torch.float64, device="cuda")
    lags = np.array([1, 2, 3, 256], dtype=np.uint32)
    orders = np.array([1, 2, 3, 3], dtype=np.uint32)

    def call(params=P, B=64, E=2, lg=lags, od=orders, nc=4, T=1, pin=at, bits=out.data_ptr(), n=4096):
        cp = lib.Params(*params)
        return L.redux_lag_order_cost_dev(C.byref(cp), C.c_void_p(pin) if pin else None, n, B, E, lg.ctypes.data if lg is not None else None,
                                          od.ctypes.data if od is not None else None, nc, T, C.c_void_p(bits) if bits else None, None)
    assert call(B=0) == lib.INVALID_INPUT and call(B=(1 << 30) + 1) == lib.INVALID_INPUT
    assert call(E=3) == lib.INVALID_INPUT and call(E=0) == lib.INVALID_INPUT and call(E=16) == lib.INVALID_INPUT
    assert call(nc=0) == lib.INVALID_INPUT
    assert call(lg=np.ones(257, np.uint32), od=np.ones(257, np.uint32), nc=257) == lib.INVALID_INPUT
    assert call(lg=np.array([1, 0, 3, 4], np.uint32)) == lib.INVALID_INPUT and call(lg=np.array([1, 2, 3, 257], np.uint32)) == lib.INVALID_INPUT
    assert call(od=np.array([1, 0, 3, 3], np.uint32)) == lib.INVALID_INPUT and call(od=np.array([1, 2, 3, 4], np.uint32)) == lib.INVALID_INPUT
    assert call(T=0) == lib.INVALID_INPUT and call(lg=None) == lib.INVALID_INPUT and call(od=None) == lib.INVALID_INPUT
    assert call(bits=None) == lib.INVALID_INPUT and call(pin=None) == lib.INVALID_INPUT
    assert call(params=(12, 14, 16)) == lib.UNSUPPORTED                      # symbol_bits != 8
    assert call(params=(8, 24, 40)) == lib.UNSUPPORTED                       # code_bits > 32
    assert call(params=(8, 14, 16), B=16383 - 256, n=4096) == lib.UNSUPPORTED  # 256 + block_size >= freq_max = 2^14 - 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call wrote to d_bits"
    assert call(params=(8, 14, 16), B=16383 - 257, n=4096) == lib.OK
    assert call() == lib.OK and call(pin=None, n=0) == lib.OK
    assert call(lg=np.full(256, 256, np.uint32), od=np.full(256, 3, np.uint32), nc=256, B=1024) == lib.OK   # 256 rows of 4 blocks
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    B = 256
    for E in (1, 2, 4, 8):
        fast, general = b"k_lag_order_cost<%d>" % E, b"k_lag_order_cost_bytes<%d>" % E
        n = 4096 // (E * B) * (E * B)
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(at), n, B, E) == fast
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(at), n + 5, B, E) == fast + b" + " + general
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(at + 1), n, B, E) == general          # the unaligned buffer
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(at + 16), 1000, 48, E) == fast + b" + " + general
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(at), n, 40, E) == general
        assert L.redux_lag_order_cost_kernel_name(n, B, E) == fast and L.redux_lag_order_cost_kernel_name(0, B, E) == general
    assert L.redux_lag_order_cost_kernel_name(4096, 4096, 3) == b"" and L.redux_lag_order_cost_kernel_name(4096, 0, 2) == b""
