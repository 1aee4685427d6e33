"""Size estimates on the GPU (include/redux_hip.h, "size estimates"): k_block_cost and k_table_cost against the library's host
rule (which test_estimate_cpu.py holds against the oracle and the definition), and `model="auto"` end to end: every
candidate's estimate against the container that model really writes, and the choice made from them.  Shapes are the smallest
at which a lane, vector, fold or workgroup boundary can go wrong."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
TOL = 2.0 ** -10          # bits: both sides sum at most 258 f64 terms below 2^27 bits (ulp 2^-26 at 4 MiB), a few ulp each
GUARD = 8                 # doubles on either side of a result
MARK = -12345.678


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@pytest.fixture(scope="module")
def lib():
    from redux_amd import _lib
    return _lib


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _read(name):
    return open(os.path.join(GOLDEN, "corpora", *name.split("/")), "rb").read()


@functools.lru_cache(maxsize=None)
def _data(kind, n):
    rng = np.random.default_rng(len(kind) * 1000003 + n)
    if kind == "iid":
        return rng.integers(0, 256, n).astype(np.uint8)
    if kind == "one":
        return np.full(n, 0xC3, dtype=np.uint8)
    return rng.choice(np.array([0, 255], dtype=np.uint8), n)          # "two"


def _block_counts(a, B):
    nb = max(1, -(-len(a) // B))
    return np.stack([np.bincount(a[b * B: (b + 1) * B], minlength=256) for b in range(nb)]).astype(np.uint64)


LONG = (4 << 20) + 4096   # a lane counts 65,600 bytes of one value: past what a packed u16 counter holds, so the fold runs

# (block size, input length, offset of d_in from a 16-byte boundary, data)
BLOCK_CASES = [
    (1, 1, 0, "iid"), (1, 130, 0, "iid"), (1, 65, 1, "one"),
    (63, 63, 15, "two"), (63, 63 * 2 - 5, 1, "iid"), (63, 63 * 65, 0, "two"),
    (64, 64, 0, "one"), (64, 64 * 2, 1, "iid"), (64, 64 * 130, 15, "iid"),
    (4096, 4096, 0, "two"), (4096, 4096 * 2 - 100, 1, "one"), (4096, 4096 * 65, 0, "iid"), (4096, 4096 * 130 - 1, 15, "two"),
    (65536, 65536, 1, "two"), (65536, 65536 * 2 - 7, 15, "one"), (65536, 65536 * 65, 0, "iid"), (65536, 65536 * 130 - 3000, 0, "two"),
    (65537, 65537, 0, "one"), (65537, 65537 * 2, 0, "iid"), (65537, 65537 * 65 - 11, 1, "one"),
    (1 << 20, 1 << 20, 0, "iid"), (1 << 20, (2 << 20) - 4097, 15, "two"), (1 << 20, (1 << 20) + 1, 1, "one"),
    (1, 0, 0, "iid"), (4096, 0, 0, "iid"), (1 << 20, 0, 1, "iid"),
    (LONG, LONG, 0, "one"), (LONG, 2 * LONG - 5, 1, "one"),
]


def _run_block_cost(lib, a, B, shift, params=P):
    """redux_block_cost_dev on a copy of `a` that starts `shift` bytes after a 16-byte boundary, into a guarded result"""
    import torch
    L = lib.lib()
    buf = torch.zeros(len(a) + 32, dtype=torch.uint8, device="cuda")
    at = (-buf.data_ptr()) % 16 + shift
    d = buf[at: at + len(a)]
    d.copy_(torch.from_numpy(a))
    nb = L.redux_block_count(len(a), B)
    out = torch.full((nb + 2 * GUARD,), MARK, dtype=torch.float64, device="cuda")
    cp = lib.Params(*params)
    st = L.redux_block_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if len(a) else None, len(a), B,
                                C.c_void_p(out.data_ptr() + 8 * GUARD), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == lib.OK
    h = out.cpu().numpy()
    assert (h[:GUARD] == MARK).all() and (h[GUARD + nb:] == MARK).all(), "guard words around d_bits were written"
    return h[GUARD: GUARD + nb]


@pytest.mark.parametrize("B,n,shift,kind", BLOCK_CASES)
def test_block_cost_equals_the_host_rule(rx, lib, B, n, shift, kind):
    a = _data(kind, n)
    want = rx.adaptive_cost_from_counts(_block_counts(a, B), P)
    got = _run_block_cost(lib, a, B, shift)
    err = np.abs(got - want).max()
    print("block_size %d, %d bytes, +%d, %s: max |device - host| = %.3g bits" % (B, n, shift, kind, err))
    assert got.shape == want.shape and err <= TOL


def test_block_cost_api_on_a_side_stream(rx, lib):
    import torch
    a = _data("iid", 65536 * 3 + 17)
    want = rx.adaptive_cost_from_counts(_block_counts(a, 65536), P)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got_dev = rx.block_cost(dev(a), 65536, P)                       # a device tensor, in place
        got_guarded = _run_block_cost(lib, a, 65536, 0)
    got_host = rx.block_cost(a.tobytes(), 65536)                        # host data, uploaded
    for got in (got_dev, got_guarded, got_host):
        assert got.dtype == np.float64 and np.abs(got - want).max() <= TOL
    assert np.abs(rx.block_cost(a, 4096, (8, 14, 16)) - rx.adaptive_cost_from_counts(_block_counts(a, 4096), (8, 14, 16))).max() <= TOL
    with pytest.raises(rx.Unsupported):
        rx.block_cost(a, 65536, (8, 14, 16))                            # a 64 KiB block can freeze the 14-bit model
    with pytest.raises(rx.Unsupported):
        rx.block_cost(a, 64, (8, 24, 40))


# ---- k_table_cost ----------------------------------------------------------------------------------------------------
def _pair_counts(a):
    c = np.zeros((256, 256), dtype=np.uint64)
    np.add.at(c, (a[:-1], a[1:]), 1)
    return c


def _table_cases(rx):
    alice = np.frombuffer(_read("canterbury/alice29.txt"), dtype=np.uint8)
    one = np.bincount(alice, minlength=256).astype(np.uint64)
    rng = np.random.default_rng(4)
    rows = np.stack([np.bincount(alice[:50000], minlength=256), rng.integers(0, 1 << 20, 256), rng.integers(0, 3, 256),
                     np.zeros(256, dtype=np.int64)]).astype(np.uint64)
    tabs = np.stack([rx.static_table_from_counts(rows[0]), rx.static_table_from_counts(rows[1]),
                     np.arange(258, dtype=np.uint32),                   # the all-ones table (total 257) under small counts
                     rx.static_table_from_counts(rows[0])])             # a zero row under a real table
    pair = _pair_counts(alice)
    hole = np.arange(258, dtype=np.uint32)
    hole[8:] -= 1                                                       # byte 7: frequency 0
    back = np.arange(258, dtype=np.uint32)
    back[8] = 3                                                         # byte 7: a negative frequency
    bad_rows = np.zeros((4, 256), dtype=np.uint64)
    bad_rows[:3, 7] = 5
    bad_tabs = np.stack([hole, back, np.zeros(258, dtype=np.uint32), hole])   # +inf, +inf, +inf (T == 0), 0 (zero row)
    return {"n=1": (one[None, :], rx.static_table_from_counts(one)[None, :]), "n=4": (rows, tabs),
            "n=256": (pair, rx.context_static_tables_from_counts(pair)), "bad": (bad_rows, bad_tabs)}


@pytest.mark.parametrize("case", ["n=1", "n=4", "n=256", "bad"])
def test_table_cost_dev_equals_the_host_rule(rx, lib, case):
    import torch
    counts, cums = _table_cases(rx)[case]
    want = rx.table_cost_from_counts(counts, cums)
    n = len(counts)
    d_c, d_t = dev(counts.view(np.int64).reshape(-1)), dev(cums.view(np.int32).reshape(-1))
    out = torch.full((n + 2 * GUARD,), MARK, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        st = lib.lib().redux_table_cost_dev(C.c_void_p(d_c.data_ptr()), C.c_void_p(d_t.data_ptr()), n,
                                            C.c_void_p(out.data_ptr() + 8 * GUARD), C.c_void_p(s.cuda_stream))
        assert st == lib.OK
        h = out.cpu().numpy()
    assert (h[:GUARD] == MARK).all() and (h[GUARD + n:] == MARK).all()
    got = h[GUARD: GUARD + n]
    api_got = rx.table_cost(d_c, d_t)
    for g in (got, api_got, rx.table_cost(counts, cums)):
        assert np.array_equal(np.isinf(g), np.isinf(want))
        fin = np.isfinite(want)
        assert (np.abs(g[fin] - want[fin]) <= TOL).all()               # (rows below 2^32 bits: ulp 2^-21)
    if case == "bad":
        assert np.isinf(want[:3]).all() and want[3] == 0.0


# ---- end to end ------------------------------------------------------------------------------------------------------
B = 65536
VERSION_MODEL = {1: "adaptive", 2: "adaptive", 3: "static", 4: "plane-static", 5: "segment-static", 7: "context-static"}


def _bf16():
    x = np.random.default_rng(16).standard_normal(1 << 19).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16).tobytes()        # 1 MiB of bf16


INPUTS = {"alice29.txt": ("canterbury/alice29.txt", 1), "kennedy.xls": ("canterbury/kennedy.xls", 1),
          "random.txt": ("artificial/random.txt", 1), "bible.txt": ("large/bible.txt", 1), "bf16": (None, 2),
          "a.txt": ("artificial/a.txt", 1)}


@functools.lru_cache(maxsize=None)
def _end_to_end(name):
    """(data, element size, estimates, {model: container}, auto's container), computed once per input"""
    from redux_amd import api, container
    path, E = INPUTS[name]
    data = _bf16() if path is None else _read(path)
    est = container.estimate_bytes(data, B, P, E)
    blobs = {m: container.compress_bytes(data, B, P, E, model=m) for m in api.estimate_candidates(E)}
    return data, E, est, blobs, container.compress_bytes(data, B, P, E, model="auto")


@pytest.mark.parametrize("name", ["alice29.txt", "kennedy.xls", "random.txt", "bible.txt", "bf16"])
def test_estimates_and_auto_end_to_end(name):
    from redux_amd import api, container
    data, E, est, blobs, auto = _end_to_end(name)
    nb = max(1, -(-len(data) // B))
    assert tuple(est) == api.estimate_candidates(E)
    for m, blob in blobs.items():
        print("%s %s: estimated %d, actual %d" % (name, m, est[m], len(blob)))
    for m, blob in blobs.items():
        assert abs(len(blob) - est[m]) <= 2 * nb + 1, (name, m, len(blob), est[m])
    chosen = container.choose_model(est)
    assert VERSION_MODEL[auto[4] & 0x0F] == chosen and auto == blobs[chosen]   # the chosen model's own container
    assert container.decompress_bytes(auto) == data
    assert len(auto) <= min(len(b) for b in blobs.values()) + 4 * nb + 2
    if name == "bible.txt":
        assert chosen == "context-static"
    if name == "kennedy.xls":
        assert chosen != "context-static"
    if E > 1:
        assert container.element_size(auto) == E


def test_auto_on_one_byte():
    from redux_amd import container
    data, E, est, blobs, auto = _end_to_end("a.txt")
    assert container.choose_model(est) != "context-static" and VERSION_MODEL[auto[4] & 0x0F] != "context-static"
    assert container.decompress_bytes(auto) == data
    assert container.decompress_bytes(container.compress_bytes(b"", B, model="auto")) == b""


def test_estimate_payload_of_a_device_tensor(rx):
    from redux_amd import container
    data = _read("canterbury/alice29.txt")
    want, _ = rx.api._estimate(data, B, P, 1, None, None)
    got = rx.estimate_payload(dev(np.frombuffer(data, dtype=np.uint8).copy()), B)
    assert got == want and list(rx.estimate_payload(data, B, models=("static",))) == ["static"]
    nb = -(-len(data) // B)
    est = container.estimate_bytes(data, B)
    assert est["adaptive"] == got["adaptive"] + container.overhead_bytes("adaptive", nb)
    with pytest.raises(rx.InvalidInput):
        rx.estimate_payload(data, B, models=("plane-static",))          # no candidate for element size 1
