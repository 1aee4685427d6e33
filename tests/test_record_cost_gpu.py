"""Record estimates on the GPU (include/redux_hip.h, "record estimates"): k_record_cost and k_record_cost_bytes against
k_block_cost of what redux_record_planes_dev writes, candidate by candidate, and against the library's host rule on the numpy
restatement of the layout; then choose_record and record_size="auto" end to end.  Shapes are the smallest at which a column
range, an odd range end, the masked first record, a counter, a copy of a histogram or the job table can go wrong.  Every input
lies between poisoned bytes: a byte read before a frame's first, or past the input's last, would show in the counts."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_lag_auto_cpu import block_counts
from test_lag_cost_gpu import TOL, GUARD, _place
from test_record_cost_cpu import ORACLE, numpy_estimate, sample_ref, selected_columns
from test_record_cpu import generated_tables, record_ref

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
B = 4096  # the block size of the end-to-end claims
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST, SLOW = "k_record_cost", "k_record_cost_bytes"
BOTH = FAST + " + " + SLOW


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _data(kind, n, R=0):
    rng = np.random.default_rng(len(kind) * 1000003 + n + R)
    if kind == "iid":
        return rng.integers(0, 256, n).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint8)
    if kind == "two":                                                    # two byte values
        return (rng.integers(0, 2, n) * 0x5A + 3).astype(np.uint8)
    if kind == "const0":                                                 # R = 2: column 0 constant, column 1 random
        a = rng.integers(0, 256, n).astype(np.uint8)
        a[0::2] = 0xC3
        return a
    # "table": records of R bytes whose columns differ: a counter, a slow walk, few values, noise
    nrec = n // R + 1
    cols = [np.arange(nrec) >> (p % 5) if p % 4 == 0 else np.cumsum(rng.integers(-2, 3, nrec)) if p % 4 == 1
            else rng.integers(0, 3, nrec) * 7 if p % 4 == 2 else rng.integers(0, 256, nrec) for p in range(R)]
    return np.stack(cols, 1).astype(np.uint8).reshape(-1)[:n].copy()


def _run(lib, d, Bk, cands, Q=0, params=P, expect=None):
    """redux_record_cost_dev on the device tensor d, into a result that was filled with NaN and lies between NaN guards
    -> (f64[len(cands), redux_block_count] with NaN where nothing was written, the rows' own counts)"""
    import torch
    L = lib.lib()
    n = d.numel()
    stride = L.redux_block_count(n, Bk) if expect is None else 16
    counts = [L.redux_record_cost_block_count(n, Bk, R, Q) for R, _ in cands]
    assert expect is not None or counts == [sample_ref(n, Bk, R, Q)[2] for R, _ in cands]
    out = torch.full((len(cands) * stride + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    cp = lib.Params(*params)
    h_r = np.asarray([R for R, _ in cands], dtype=np.uint32)
    h_d = np.asarray([f for _, f in cands], dtype=np.uint8)
    st = L.redux_record_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, Bk, h_r.ctypes.data, h_d.ctypes.data, len(cands),
                                 Q, C.c_void_p(out.data_ptr() + 8 * GUARD), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    h_r[:] = 0  # (the lists were consumed by the call)
    h_d[:] = 0
    if expect is not None:
        assert st == expect
        assert np.isnan(out.cpu().numpy()).all(), "a refused call wrote to d_bits"
        return None, counts
    assert st == lib.OK
    h = out.cpu().numpy()
    assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + len(cands) * stride:]).all(), "guard words around d_bits were written"
    got = h[GUARD: GUARD + len(cands) * stride].reshape(len(cands), stride)
    for c, k in enumerate(counts):
        assert not np.isnan(got[c, :k]).any(), "a block of the result was not written"
        assert np.isnan(got[c, k:]).all(), "an entry past a row's count was written"
    return got, counts


def _composed(rx, d, R, Bk, F):
    """k_block_cost of what redux_record_planes_dev writes: the parent's kernels"""
    import torch
    if d.numel() == 0:
        return rx.block_cost(torch.empty(0, dtype=torch.uint8, device="cuda"), Bk, P)
    return rx.block_cost(rx.api.record_planes(d.clone(), R, Bk, delta=bool(F)), Bk, P)


def _host(rx, a, R, Bk, F):
    return rx.adaptive_cost_from_counts(block_counts(record_ref(a, R, Bk, bool(F)), Bk), P)


def _name(lib, d, Bk, R):
    return lib.lib().redux_record_cost_kernel_name_at(C.c_void_p(d.data_ptr()), d.numel(), Bk, R).decode()


def _check(rx, lib, a, Bk, R, shift, name):
    """both filters of R in one call against the host rule and the composed device path -> the worst differences"""
    d = _place(a, shift)
    assert _name(lib, d, Bk, R) == name, (R, Bk, len(a), shift)
    got, _ = _run(lib, d, Bk, [(R, 0), (R, 1)])
    worst = [0.0, 0.0]
    for F in (0, 1):
        host, composed = _host(rx, a, R, Bk, F), _composed(rx, d, R, Bk, F)
        assert got[F].shape == host.shape == composed.shape
        dh, dc = np.abs(got[F] - host).max(), np.abs(got[F] - composed).max()
        worst = [max(worst[0], dh), max(worst[1], dc)]
        assert dh <= TOL and dc <= TOL, (R, Bk, len(a), shift, F, dh, dc)
    return worst


SWEEP_R = (2, 3, 7, 16, 20, 23, 64, 255, 256)


def _sweep_len(R, Bk):
    """two full frames, then a short one of Bk // 2 + 1 records and R // 2 trailing bytes: its columns end inside blocks"""
    return 2 * R * Bk + R * (Bk // 2 + 1) + R // 2


@pytest.mark.parametrize("Bk", [64, 1024 + 16, 4096])
@pytest.mark.parametrize("R", SWEEP_R)
def test_record_cost_equals_block_cost_of_the_record_layout(rx, lib, R, Bk):
    a = _data("table", _sweep_len(R, Bk), R)
    worst = _check(rx, lib, a, Bk, R, 0, BOTH)
    print("R %d B %d: max |record_cost - host rule| = %.3g, - block_cost(record_planes) = %.3g bits" % (R, Bk, *worst))


@pytest.mark.parametrize("R", SWEEP_R)
def test_unaligned_source_and_odd_block_sizes_take_the_byte_path(rx, lib, R):
    _check(rx, lib, _data("table", _sweep_len(R, 64), R), 64, R, 1, SLOW)   # a byte off a 16-byte boundary
    if R in (3, 23, 256):
        Bk = 4099
        _check(rx, lib, _data("table", R * Bk + R * 700 + 1, R), Bk, R, 0, SLOW)
    _check(rx, lib, _data("table", R * 64 - 1, R), 64, R, 0, SLOW)           # less than a frame
    _check(rx, lib, _data("iid", R - 1), 64, R, 0, SLOW)                     # less than a record: N = 0


@pytest.mark.parametrize("Bk", [65536, 131072])
def test_a_count_of_the_block_size_and_above_65535(rx, lib, Bk):
    """R = 2, one frame: column 0 is constant, so one counter reaches Bk = 65,536 (one past a 16-bit counter) and 131,072;
    with the delta the column's first byte stands alone and the count is Bk - 1.  (8, 30, 32) allows both block sizes."""
    a = _data("const0", 2 * Bk)
    _check(rx, lib, a, Bk, 2, 0, FAST)
    d = _place(a, 0)
    _run(lib, d, Bk, [(2, 0)], params=(8, 14, 16), expect=lib.UNSUPPORTED)


@pytest.mark.parametrize("kind", ["zeros", "two"])
@pytest.mark.parametrize("R", [3, 256])
def test_many_lanes_on_one_counter(rx, lib, R, kind):
    _check(rx, lib, _data(kind, 2 * R * 4096), 4096, R, 0, FAST)


@pytest.mark.parametrize("R", [255, 256])
def test_split_column_ranges_on_few_large_frames(rx, lib, R):
    _check(rx, lib, _data("table", 2 * R * 4096, R), 4096, R, 0, FAST)


def test_lists_of_one_of_256_and_with_repeats_have_independent_rows(rx, lib):
    Bk = 64
    a = _data("table", 3 * 129 * Bk + 77, 23)
    d = _place(a, 0)
    cands = [(R, F) for R in range(2, 130) for F in (0, 1)]
    assert len(cands) == 256
    full, _ = _run(lib, d, Bk, cands)
    rev, _ = _run(lib, d, Bk, cands[::-1])
    assert np.array_equal(full, rev[::-1])
    for c, (R, F) in enumerate(cands):
        one, _ = _run(lib, d, Bk, [(R, F)])
        assert np.array_equal(one[0], full[c]), (R, F)
        if R in (2, 23, 33, 129):
            assert np.abs(one[0] - _host(rx, a, R, Bk, F)).max() <= TOL
    rep = [(23, 1), (3, 0), (23, 1), (129, 1), (3, 0), (23, 1)]
    got, _ = _run(lib, d, Bk, rep)
    for c, cand in enumerate(rep):
        assert np.array_equal(got[c], full[cands.index(cand)]), cand


@pytest.mark.parametrize("R,frames,tail", [(3, 300, 0), (3, 300, 100), (255, 5, 0), (255, 5, 255 * 20 + 7)])
def test_sampled_rows_are_the_selected_columns_of_the_exact_rows(rx, lib, R, frames, tail):
    Bk = 64
    a = _data("table", frames * R * Bk + tail, R)
    d = _place(a, 0)
    cands = [(R, 0), (R, 1), (2, 1), (16, 0)]
    exact, _ = _run(lib, d, Bk, cands)
    for Q in (1, 64):
        got, counts = _run(lib, d, Bk, cands, Q)   # (checks the rows' lengths, and that nothing is written past them)
        for c, (Rc, _) in enumerate(cands):
            cols = selected_columns(len(a), Bk, Rc, Q)
            assert len(cols) == counts[c]
            assert np.array_equal(got[c, :counts[c]], exact[c, cols]), (Rc, Q)
    assert sample_ref(300 * 3 * Bk, Bk, 3, 1)[0] == 300 and sample_ref(300 * 3 * Bk, Bk, 3, 64)[0] == 14
    assert sample_ref(5 * 255 * Bk, Bk, 255, 64)[0] == 5 and sample_ref(5 * 255 * Bk + 7, Bk, 255, 64)[0] == 6


def test_empty_input_and_refused_calls(rx, lib):
    import torch
    L = lib.lib()
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    got, counts = _run(lib, empty, 64, [(2, 0), (23, 1), (256, 1)])
    assert counts == [1, 1, 1] and got.shape == (3, 1)
    assert np.abs(got[:, 0] - rx.adaptive_cost_from_counts(np.zeros((1, 256), np.uint64), P)[0]).max() <= TOL
    got, counts = _run(lib, empty, 64, [(2, 0)], Q=64)
    assert counts == [1]
    d = _place(_data("iid", 1000), 0)
    for cands, kw in (([(1, 0)], {}), ([(257, 0)], {}), ([(0, 1)], {}), ([(3, 2)], {}), ([(3, 0), (3, 255)], {}), ([(3, 0)] * 257, {}),
                      ([(3, 0)], {"Bk": 0}), ([(3, 0)], {"Bk": (1 << 30) + 1})):
        _run(lib, d, kw.get("Bk", 64), cands, expect=lib.INVALID_INPUT)
    out = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    cp = lib.Params(*P)
    h_r, h_d = np.array([3], np.uint32), np.array([0], np.uint8)
    args = dict(p=C.byref(cp), d=C.c_void_p(d.data_ptr()), r=h_r.ctypes.data, f=h_d.ctypes.data, nc=1, bits=C.c_void_p(out.data_ptr()))
    for kw in ({"p": None}, {"d": None}, {"r": None}, {"f": None}, {"nc": 0}, {"bits": None}):
        x = {**args, **kw}
        assert L.redux_record_cost_dev(x["p"], x["d"], 1000, 64, x["r"], x["f"], x["nc"], 0, x["bits"], None) == lib.INVALID_INPUT, kw
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["imu23", "ticks20"])
def test_choose_record_and_record_size_auto_on_the_generated_tables(rx, name, tmp_path):
    from redux_amd import api, cli, container
    x, _ = generated_tables(40000)[name]
    want, coded = ORACLE[name]
    choice, est = api.choose_record(x, B, P)
    print(name, "choice", choice, "estimates", est)
    assert choice == want and None in est and len(est) == 5
    host = numpy_estimate(x, B)
    ref = {**host([k for k in est if k is not None], 0), **host(None, 0)}
    assert all(abs(est[k] - ref[k]) <= 1 for k in est), (est, ref)
    assert abs(est[choice] - {"imu23": 377980, "ticks20": 136031}[name]) <= 1
    blob = container.compress_bytes(x.tobytes(), B, P, record_size="auto")
    assert blob == container.compress_bytes(x.tobytes(), B, P, record_size=want[0], filter="delta")
    nb = -(-len(x) // B)
    payload = len(blob) - container.overhead_bytes("adaptive", nb, filter="delta", record_size=want[0])
    print(name, "payload", payload, "estimate", est[choice], "oracle", coded)
    assert abs(payload - est[choice]) <= est[choice] / 1000
    assert container.estimate_record_bytes(x, B, [want], P)[want] == est[choice] + len(blob) - payload
    assert container.decompress_bytes(blob) == x.tobytes()
    src, packed, back = tmp_path / "in", tmp_path / "packed", tmp_path / "back"
    src.write_bytes(x.tobytes())
    assert cli.main(["-c", "--block-size", str(B), "--record-size", "auto", "-i", str(src), "-o", str(packed)]) == 0
    assert packed.read_bytes() == blob
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0
    assert back.read_bytes() == x.tobytes()


def test_record_size_auto_on_text_is_never_estimated_above_the_plain_container(rx):
    """alice29.txt at B = 4096: the choice is recorded, not asserted.  It has no fixed-width records."""
    from redux_amd import api, container
    x = open(os.path.join(ROOT, "tests", "golden", "corpora", "canterbury", "alice29.txt"), "rb").read()
    choice, est = api.choose_record(x, B, P)
    print("alice29.txt: choice", choice, "plain", est[None], "smallest", sorted(est.items(), key=lambda kv: kv[1])[:4], "of", len(est))
    assert est[choice] <= est[None] and choice in (None, api.best_record(est))
    blob = container.compress_bytes(x, B, P, record_size="auto", checksum=True)
    if choice is None:
        assert blob == container.compress_bytes(x, B, P, checksum=True)
    else:
        assert blob == container.compress_bytes(x, B, P, record_size=choice[0], filter=choice[1], checksum=True)
    assert container.decompress_bytes(blob) == x
