"""Layout estimates on the GPU (include/redux_hip.h, "layout estimates"): k_layout_cost and k_layout_cost_bytes against
k_block_cost of the transformed input and against the library's host rule on the numpy restatement of the eight layouts.
Shapes are the smallest at which a lane group, a row, a frame, a fold or a workgroup boundary can go wrong."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_layout_auto_cpu import block_counts, transform_ref

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
TOL = 2.0 ** -10          # bits (tests/test_estimate_gpu.py): both sides sum at most 258 f64 terms below 2^27 bits
GUARD = 8                 # doubles on either side of the result
MARK = -12345.678
ALL = 0xFF


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
    if kind == "one":                                                    # one byte value, the last byte another
        a = np.full(n, 0xC3, dtype=np.uint8)
        a[-1:] = 0x3C
        return a
    if kind == "walk":                                                   # an int64 series: the delta layouts differ from the plain
        v = 1_700_000_000_000 + np.cumsum(rng.integers(900, 1100, n // 8 + 1))
        return v.astype("<i8").view(np.uint8)[:n].copy()
    return rng.choice(np.array([0, 255], dtype=np.uint8), n)            # "two"


# rows a wave counts between folds (redux_layout_cost.hpp: kLayoutFoldRows = 65535 // (16 E)); a row is 1 KiB of each plane
FOLD_ROWS = {1: 4095, 2: 2047, 4: 1023, 8: 511}


def _above_fold(E):
    """the smallest block size (a multiple of 16) at which a lane group of 64 / E lanes must fold inside a block"""
    return FOLD_ROWS[E] * 1024 + 16


def _mask(E):
    k = {1: 0, 2: 1, 4: 2, 8: 3}[E]
    return 1 << k | 1 << (4 + k)


# (block size, input length, offset of d_in from a 16-byte boundary, data, layouts)
CASES = [
    (4096, 0, 0, "iid", ALL), (4096, 1, 0, "iid", ALL), (4096, 63, 0, "walk", ALL),
    # exactly one frame of each element size
    (4096, 4096, 0, "walk", ALL), (4096, 2 * 4096, 0, "walk", ALL), (4096, 4 * 4096, 0, "walk", ALL), (4096, 8 * 4096, 0, "walk", ALL),
    # three frames and a short last frame whose length is no multiple of E
    (4096, 3 * 4096 + 4096 + 5, 0, "iid", ALL), (4096, 3 * 2 * 4096 + 4096 + 5, 0, "walk", ALL),
    (4096, 3 * 4 * 4096 + 4096 + 5, 0, "walk", ALL), (4096, 3 * 8 * 4096 + 4096 + 5, 0, "walk", ALL),
    # a frame of fewer groups than a wave has lanes, and a last row that is not full (B / 16 = 100 groups)
    (256, 8 * 256 * 3, 0, "walk", ALL), (1600, 8 * 1600 * 2 + 77, 0, "walk", ALL),
    # a block of 48 bytes IS three groups of 16: full frames of three lanes on the fast path, the rest on the general one
    (48, 1000, 0, "walk", ALL),
    # the general path: a block size that is no multiple of 16 (40, 1000), a buffer that is not aligned
    (40, 1000, 0, "walk", ALL), (1000, 8 * 1000 * 2 + 9, 0, "walk", ALL),
    (4096, 2 * 8 * 4096, 1, "walk", ALL), (4096, 8 * 4096 + 100, 15, "two", ALL),
    # more frames than launched workgroups: the grid-stride walk
    (256, 2 << 20, 0, "walk", ALL),
    # the counter fold inside a block: one byte value, so that one u16 counter of a lane takes every byte of its group
    (1 << 20, 8 << 20, 0, "one", _mask(8)),
    (_above_fold(8), 8 * _above_fold(8), 0, "one", _mask(8)), (_above_fold(4), 4 * _above_fold(4), 0, "one", _mask(4)),
    (_above_fold(2), 2 * _above_fold(2), 0, "one", _mask(2)), (_above_fold(1), _above_fold(1), 0, "one", _mask(1)),
]


def _run(lib, a, B, shift, mask, params=P):
    """redux_layout_cost_dev on a copy of `a` that starts `shift` bytes after a 16-byte boundary, into a result that was
    filled with NaN and lies between guards -> (f64[8, nblocks], the device copy of a)"""
    import torch
    L = lib.lib()
    buf = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + shift
    d = buf[at: at + len(a)]
    d.copy_(torch.from_numpy(a))
    nb = L.redux_block_count(len(a), B)
    out = torch.full((8 * nb + 2 * GUARD,), MARK, dtype=torch.float64, device="cuda")
    out[GUARD: GUARD + 8 * nb] = float("nan")
    cp = lib.Params(*params)
    st = L.redux_layout_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if len(a) else None, len(a), B, mask,
                                 C.c_void_p(out.data_ptr() + 8 * GUARD), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.OK
    h = out.cpu().numpy()
    assert (h[:GUARD] == MARK).all() and (h[GUARD + 8 * nb:] == MARK).all(), "guard words around d_bits were written"
    return h[GUARD: GUARD + 8 * nb].reshape(8, nb), d


@pytest.mark.parametrize("B,n,shift,kind,mask", CASES)
def test_layout_cost_equals_block_cost_of_the_transformed_input(rx, lib, B, n, shift, kind, mask):
    import torch
    a = _data(kind, n)
    got, d = _run(lib, a, B, shift, mask)
    for k, (E, filt) in enumerate(rx.LAYOUTS):
        if not mask >> k & 1:
            assert np.isnan(got[k]).all(), "row %d was written without being asked for" % k
            continue
        host = rx.adaptive_cost_from_counts(block_counts(transform_ref(a, k, B), B), P)
        if n:
            d_t = rx.delta_planes(d.clone(), E, B) if filt else rx.planes(d.clone(), E, B) if E > 1 else d
            composed = rx.block_cost(d_t, B, P)
        else:
            composed = rx.block_cost(torch.empty(0, dtype=torch.uint8, device="cuda"), B, P)
        e_host, e_dev = np.abs(got[k] - host).max(), np.abs(got[k] - composed).max()
        print("B %d, %d bytes, +%d, %s, layout %d: max |layout_cost - host rule| = %.3g, - block_cost(transform) = %.3g bits"
              % (B, n, shift, kind, k, e_host, e_dev))
        assert got[k].shape == host.shape == composed.shape and e_host <= TOL and e_dev <= TOL, (k, E, filt)


def test_only_the_selected_rows_are_written(rx, lib):
    a = _data("walk", 8 * 4096 * 2 + 300)
    got, _ = _run(lib, a, 4096, 0, 0x81)
    assert [k for k in range(8) if not np.isnan(got[k]).any()] == [0, 7]
    assert all(np.isnan(got[k]).all() for k in range(1, 7))
    for k in (0, 7):
        assert np.abs(got[k] - rx.adaptive_cost_from_counts(block_counts(transform_ref(a, k, 4096), 4096), P)).max() <= TOL


def test_api_layout_cost_and_estimates(rx):
    import torch
    a = _data("walk", 8 * 4096 * 3 + 4096 + 5)
    host = np.stack([rx.adaptive_cost_from_counts(block_counts(transform_ref(a, k, 4096), 4096), P) for k in range(8)])
    got = rx.layout_cost(a.tobytes(), 4096)                                # host data, uploaded
    assert got.shape == host.shape and np.abs(got - host).max() <= TOL
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        part = rx.layout_cost(torch.from_numpy(a).cuda(), 4096, P, [(8, "delta"), 2])  # a device tensor, on a side stream
    assert np.isnan(part[[0, 1, 3, 4, 5, 6]]).all() and np.abs(part[[2, 7]] - host[[2, 7]]).max() <= TOL
    nb = host.shape[1]
    est = rx.estimate_layouts(a, 4096, P)
    assert list(est) == list(rx.LAYOUTS)
    assert est == {key: int(np.ceil(host[k].sum() / 8 + rx.api.TERMINATION_BYTES * nb)) for k, key in enumerate(rx.LAYOUTS)}
    assert rx.estimate_layouts(a, 4096, P, element_size=4) == {(4, None): est[(4, None)], (4, "delta"): est[(4, "delta")]}
    with pytest.raises(rx.InvalidInput):
        rx.layout_cost(a, 4096, P, 0)
    with pytest.raises(rx.InvalidInput):
        rx.layout_cost(a, 4096, P, [(3, None)])
    with pytest.raises(rx.InvalidInput):
        rx.estimate_layouts(a, 4096, P, element_size=3)
    with pytest.raises(rx.Unsupported):
        rx.layout_cost(a, 65536, (8, 14, 16))                              # a 64 KiB block can freeze the 14-bit model


def test_refusals(lib):
    import torch
    L = lib.lib()
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    pin, pout = C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr())

    def call(params, B, mask):
        cp = lib.Params(*params)
        return L.redux_layout_cost_dev(C.byref(cp), pin, 4096, B, mask, pout, None)

    assert call(P, 4096, 0xFF) == lib.OK
    assert call(P, 0, 0xFF) == lib.INVALID_INPUT
    assert call(P, (1 << 30) + 1, 0xFF) == lib.INVALID_INPUT
    assert call(P, 4096, 0) == lib.INVALID_INPUT
    assert call(P, 4096, 0x100) == lib.INVALID_INPUT
    assert call(P, 4096, 0x1FF) == lib.INVALID_INPUT
    assert call((12, 14, 16), 64, 0xFF) == lib.UNSUPPORTED               # symbol_bits != 8
    assert call((8, 24, 40), 64, 0xFF) == lib.UNSUPPORTED                # code_bits > 32
    assert call((8, 14, 16), 16383 - 256, 0xFF) == lib.UNSUPPORTED       # 256 + block_size >= freq_max = 2^14 - 1
    assert call((8, 14, 16), 16383 - 257, 0xFF) == lib.OK
    torch.cuda.synchronize()


def test_kernel_name(lib):
    import torch
    L = lib.lib()
    B = 4096
    for k in range(8):
        E = 1 << (k & 3)
        fast, general = b"k_layout_cost<%d>" % E, b"k_layout_cost_bytes<%d>" % E
        assert L.redux_layout_cost_kernel_name(E * B, B, k) == fast
        assert L.redux_layout_cost_kernel_name(5 * E * B, B, k) == fast
        assert L.redux_layout_cost_kernel_name(E * B - 1, B, k) == general                 # a short frame alone
        assert L.redux_layout_cost_kernel_name(0, B, k) == general
        assert L.redux_layout_cost_kernel_name(3 * E * B + B + 5, B, k) == fast + b" + " + general   # ... behind full frames
        assert L.redux_layout_cost_kernel_name(1000, 40, k) == general                     # no multiple of 16
        assert L.redux_layout_cost_kernel_name(40 * E * 10, 40, k) == general
        assert L.redux_layout_cost_kernel_name(48 * E * 10, 48, k) == fast                 # (48 is three groups of 16)
        assert L.redux_layout_cost_kernel_name(1000, 48, k) == fast + b" + " + general
        d = torch.zeros(5 * E * B + 32, dtype=torch.uint8, device="cuda")
        at = d.data_ptr() + (-d.data_ptr()) % 16
        assert L.redux_layout_cost_kernel_name_at(C.c_void_p(at), 5 * E * B, B, k) == fast
        assert L.redux_layout_cost_kernel_name_at(C.c_void_p(at + 1), 5 * E * B, B, k) == general  # the unaligned buffer
    assert L.redux_layout_cost_kernel_name(4096, 4096, 8) == b"" and L.redux_layout_cost_kernel_name(4096, 0, 0) == b""
