"""Lag estimates and lag="auto" (include/redux_hip.h, "lag estimates"): the choice rule on hand-made estimate tables, the
row length of a sampled call against a numpy restatement, the host-only refusals of the ABI, the value claim on the CPU --
the lag with the smallest counted cost is the number of channels, on every frame and on a sample of four -- the Python
refusals before the library is touched, the CLI tables and the Rust declarations.  No GPU call.

The value claim rests on GENERATED data, the interleaved random walks and four-column records of tests/test_lag_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import test_rust_shim_cpu as shim
from test_lag_cpu import lag_planes_ref

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- the choice rule ---------------------------------------------------------------------------------------------------
def run_rule(nframes, first, exact=None, E=2, Bk=16):
    """choose_lag on an input of nframes frames whose estimates are the tables `first` (first pass) and `exact` (the
    finalists' pass) -> (S, the returned dict, the (lags, frame_step) of every pass)"""
    from redux_amd import api
    calls = []

    def estimate(lags, T):
        calls.append((None if lags is None else list(lags), T))
        table = first if len(calls) == 1 else exact
        return {S: table[S] for S in (range(1, 257) if lags is None else lags)}
    S, est = api.choose_lag(bytes(nframes * E * Bk), E, Bk, estimate=estimate)
    return S, est, calls


def test_choice_rule_on_hand_made_tables():
    from redux_amd import api
    assert api.LAG_SAMPLE_FRAMES == 64 and api.LAG_FINALISTS == 3 and api.LAG_MAX == 256
    flat = {S: 1000 for S in range(1, 257)}
    # up to 64 frames: one exact pass over all 256 lags; exact ties go to the smaller S
    for F in (1, 2, 63, 64):
        S, est, calls = run_rule(F, {**flat, 7: 900, 9: 900, 200: 901})
        assert S == 7 and calls == [(None, 1)] and est[7] == 900 and len(est) == 256, F
    assert run_rule(3, flat)[0] == 1
    assert run_rule(3, {**flat, 256: 999})[0] == 256
    # the frame step of the first pass
    assert [api.lag_frame_step(F) for F in (1, 64, 65, 128, 129, 130, 6400, 6401)] == [1, 1, 2, 2, 3, 3, 100, 101]
    for F, T in ((65, 2), (128, 2), (129, 3)):
        first = {**flat, 3: 500, 6: 520, 9: 540, 12: 560}
        S, est, calls = run_rule(F, first, {1: 800, 3: 700, 6: 650, 9: 900})
        # the finalists are the three smallest sampled estimates and lag 1; the second pass is exact and decides
        assert calls == [(None, T), ([1, 3, 6, 9], 1)] and S == 6 and est == {1: 800, 3: 700, 6: 650, 9: 900}, F
    # lag 1 is always a finalist, also when it is the worst of the sample, and wins when the exact pass says so
    first = {**flat, 1: 5000, 4: 10, 8: 20, 16: 30}
    S, est, calls = run_rule(200, first, {1: 40, 4: 50, 8: 60, 16: 70})
    assert calls[1] == ([1, 4, 8, 16], 1) and S == 1
    # lag 1 among the three smallest: three finalists, no repeat
    S, est, calls = run_rule(200, {**flat, 1: 5, 4: 10, 8: 20, 16: 30}, {1: 9, 4: 9, 8: 10})
    assert calls[1] == ([1, 4, 8], 1) and S == 1  # the exact tie goes to the smaller S
    # ties of the sample go to the smaller S: of four equal candidates the three smallest lags go on
    S, est, calls = run_rule(200, {**flat, 10: 7, 20: 7, 30: 7, 40: 7}, {1: 3, 10: 2, 20: 2, 30: 2})
    assert calls[1] == ([1, 10, 20, 30], 1) and S == 10
    assert api.lag_finalists({**flat, 1: 0}) == [1, 2, 3] and api.lag_finalists(flat) == [1, 2, 3]
    assert api.lag_finalists({**flat, 255: 1, 256: 1, 254: 1}) == [1, 254, 255, 256]
    assert api.best_lag({5: 3, 2: 3, 9: 4}) == 2


# ---- the row length of a sampled call -----------------------------------------------------------------------------------
def block_count_ref(n, Bk, E, T):
    nb = max(1, -(-n // Bk))
    frames = -(-nb // E)
    return sum(min(E, nb - f * E) for f in range(0, frames, T))


def test_block_count_matches_the_restatement(rx):
    from redux_amd import _lib
    L = _lib.lib()
    for E in (1, 2, 4, 8):
        for Bk in (1, 16, 48, 4096):
            for n in (0, 1, Bk - 1, Bk, Bk + 1, E * Bk - 1, E * Bk, E * Bk + 1, 3 * E * Bk, 3 * E * Bk + 5, 4 * E * Bk + (E - 1) * Bk + 1,
                      7 * E * Bk - 1, 130 * E * Bk + Bk // 2):
                n = max(n, 0)
                assert L.redux_lag_cost_block_count(n, Bk, E, 1) == L.redux_block_count(n, Bk), (E, Bk, n)
                for T in (1, 2, 3, 4, 5, 7, 64, 131, 1 << 31):
                    assert L.redux_lag_cost_block_count(n, Bk, E, T) == block_count_ref(n, Bk, E, T), (E, Bk, n, T)
    # a short last frame selected (3 full frames and one of 2 blocks, step 3: frames 0 and 3) and not selected (step 2)
    assert L.redux_lag_cost_block_count(3 * 4 * 64 + 65, 64, 4, 3) == 4 + 2
    assert L.redux_lag_cost_block_count(3 * 4 * 64 + 65, 64, 4, 2) == 4 + 4
    assert L.redux_lag_cost_block_count(0, 64, 4, 1) == 1 and L.redux_lag_cost_block_count(0, 64, 4, 9) == 1
    for bad in ((100, 0, 2, 1), (100, 64, 3, 1), (100, 64, 0, 1), (100, 64, 2, 0)):
        assert L.redux_lag_cost_block_count(*bad) == 0, bad


# ---- the host-only refusals of the ABI ----------------------------------------------------------------------------------
def test_abi_refuses_bad_arguments_before_any_device_work(rx):
    from redux_amd import _lib
    L = _lib.lib()
    ok = _lib.Params(*PARAMS)
    d_in, d_bits = C.c_void_p(4096), C.c_void_p(1 << 20)  # (never dereferenced: every call below is refused on the host)
    lags = np.array([1, 2, 3, 256], dtype=np.uint32)
    lp = lags.ctypes.data

    def call(p=ok, d=d_in, n=1024, Bk=64, E=2, lg=lp, nl=4, T=1, bits=d_bits):
        return L.redux_lag_cost_dev(C.byref(p) if p is not None else None, d, n, Bk, E, lg, nl, T, bits, None)
    for kw in ({"Bk": 0}, {"Bk": (1 << 30) + 1}, {"E": 0}, {"E": 3}, {"E": 16}, {"nl": 0}, {"nl": 257}, {"T": 0}, {"lg": None},
               {"bits": None}, {"d": None}, {"p": None}):
        assert call(**kw) == _lib.INVALID_INPUT, kw
    for bad in (0, 257, 1 << 16, 0xFFFFFFFF):
        for at in range(4):
            one = lags.copy()
            one[at] = bad
            assert call(lg=one.ctypes.data) == _lib.INVALID_INPUT, (bad, at)
    many = np.zeros(257, dtype=np.uint32)  # (the 257th lag is not looked at: the count is refused first)
    assert call(lg=many.ctypes.data, nl=257) == _lib.INVALID_INPUT
    # UNSUPPORTED where redux_block_cost_dev is: a block that could freeze the model
    small = _lib.Params(8, 14, 16)
    assert call(p=small, Bk=65536) == _lib.UNSUPPORTED
    assert L.redux_block_cost_dev(C.byref(small), d_in, 1024, 65536, d_bits, None) == _lib.UNSUPPORTED
    # the names
    for E in (1, 2, 4, 8):
        fast, slow = b"k_lag_cost<%d>" % E, b"k_lag_cost_bytes<%d>" % E
        assert L.redux_lag_cost_kernel_name(3 * E * 64, 64, E) == fast
        assert L.redux_lag_cost_kernel_name(3 * E * 64 + 1, 64, E) == fast + b" + " + slow
        assert L.redux_lag_cost_kernel_name(E * 64 - 1, 64, E) == slow and L.redux_lag_cost_kernel_name(0, 64, E) == slow
        assert L.redux_lag_cost_kernel_name(3 * E * 40, 40, E) == slow
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(4096), 3 * E * 64, 64, E) == fast
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(4096 + 1), 3 * E * 64, 64, E) == slow
        assert L.redux_lag_cost_kernel_name_at(C.c_void_p(4096 + 15), 3 * E * 64 + 1, 64, E) == slow
    for bad in ((100, 0, 2), (100, (1 << 30) + 1, 2), (100, 64, 3), (100, 64, 0)):
        assert L.redux_lag_cost_kernel_name(*bad) == b"", bad


def test_python_estimates_check_their_arguments_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api, container

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    x = np.zeros(256, np.uint8)
    for kw in ({"element_size": 3}, {"element_size": 0}, {"element_size": True}, {"block_size": 0}, {"block_size": (1 << 30) + 1},
               {"lags": []}, {"lags": [0]}, {"lags": [257]}, {"lags": [1, 2.0]}, {"lags": ["3"]}, {"lags": [True]}, {"lags": 3},
               {"lags": list(range(1, 257)) + [1]}, {"frame_step": 0}, {"frame_step": -1}, {"frame_step": 1.0}):
        a = {"element_size": 2, "block_size": 64, "lags": [1, 2], "frame_step": 1, **kw}
        with pytest.raises(rx.InvalidInput):
            api.lag_cost(x, a["element_size"], a["lags"], a["block_size"], PARAMS, a["frame_step"])
        with pytest.raises(rx.InvalidInput):
            api.estimate_lags(x, a["element_size"], a["block_size"], a["lags"], PARAMS, a["frame_step"])
        with pytest.raises(rx.InvalidInput):
            container.estimate_lag_bytes(x, a["element_size"], a["block_size"], a["lags"], PARAMS, frame_step=a["frame_step"])
    for E, Bk in ((3, 64), (2, 0), (2, (1 << 30) + 1)):
        with pytest.raises(rx.InvalidInput):
            api.choose_lag(x, E, Bk)


# ---- the value claim, on the CPU ----------------------------------------------------------------------------------------
def channels(C_, E, seed):
    rng = np.random.default_rng(seed)
    n = 3 * B + 100
    w = np.stack([np.cumsum(np.round(rng.normal(0, 50, n))) + 5000 * c * (-1) ** c for c in range(C_)], 1)
    return w.reshape(-1).astype(np.int64).astype("<i%d" % E).view(np.uint8)


def records(seed):
    rng = np.random.default_rng(seed)
    m = 3 * B + 100
    cols = [np.cumsum(rng.integers(990, 1010, m)), np.arange(m) * 3 + 7,
            np.cumsum(np.round(rng.normal(0, 20, m))), rng.integers(0, 2, m)]
    return np.stack(cols, 1).reshape(-1).astype(np.int64).astype("<i4").view(np.uint8)


def block_counts(y, Bk):
    """u64[nblocks, 256]: the byte counts of every block of Bk bytes of y (one empty block for no bytes)"""
    nb = max(1, -(-len(y) // Bk))
    return np.stack([np.bincount(y[b * Bk: (b + 1) * Bk], minlength=256) for b in range(nb)]).astype(np.uint64)


def cost_table_ref(x, E, Bk, lags=range(1, 257)):
    """the host rule: float64[len(lags), nblocks], the adaptive cost of every block of lag_planes_ref(x, E, Bk, S)"""
    from redux_amd import api
    return np.stack([api.adaptive_cost_from_counts(block_counts(lag_planes_ref(x, E, Bk, S), Bk), PARAMS) for S in lags])


def sampled_columns(nblocks, E, T):
    """the blocks of the frames 0, T, 2T, ... in order: the columns a sampled call keeps"""
    frames = -(-nblocks // E)
    return [b for f in range(0, frames, T) for b in range(f * E, min(f * E + E, nblocks))]


CLAIMS = [(C_, E) for C_ in (2, 3, 6) for E in (2, 4)] + [("records", 4)]


@pytest.mark.parametrize("C_,E", CLAIMS)
def test_the_counted_lag_is_the_number_of_channels(C_, E):
    x = records(1) if C_ == "records" else channels(C_, E, 100 + 10 * C_ + E)
    want = 4 if C_ == "records" else C_
    bits = cost_table_ref(x, E, B)
    total = bits.sum(axis=1)
    order = np.argsort(total, kind="stable")
    print("%s, E = %d: lag %d at %.0f bits, runner-up lag %d at %.3f x" % (C_, E, order[0] + 1, total[order[0]], order[1] + 1,
                                                                          total[order[1]] / total[order[0]]))
    assert int(order[0]) + 1 == want, (C_, E, order[:4] + 1)
    # the same when only every ceil(F / 4)-th frame is counted
    nb = bits.shape[1]
    frames = -(-nb // E)
    T = -(-frames // 4)
    cols = sampled_columns(nb, E, T)
    assert 0 < len(cols) < nb
    assert int(np.argmin(bits[:, cols].sum(axis=1))) + 1 == want, (C_, E, T)


# ---- Python refusals before the library is touched ----------------------------------------------------------------------
def test_python_api_refuses_lag_auto_where_nothing_chooses(rx, monkeypatch):
    from redux_amd import _lib, api, container
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    # the four calls that do not choose
    for lag in ("auto", "Auto", "AUTO", "", "3"):
        kw = {"filter": "lag", "lag": lag}
        for call in (lambda: rx.compress_blocks(b"abcd", 4, **kw),
                     lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                     lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, **kw),
                     lambda: rx.DeviceDecoder(PARAMS, 4096, 1, **kw),
                     lambda: api.lag_planes(None, 2, 4096, lag),
                     lambda: container.pack(flags, offs, PARAMS, 4, 4, filter="lag", lag=lag)):
            with pytest.raises(rx.InvalidInput):
                call()
        with pytest.raises(rx.InvalidInput):
            api._resolve_front(None, **kw)
    data = b"abcd" * 4
    # every exclusion of filter="lag" holds for lag="auto"
    for kw in ({"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
               {"model": "context-static"}, {"model": "auto"}, {"stored": True}, {"base": b"abcd"}, {"skip_constant": True},
               {"layout": "auto"}, {"layout": "mixed"}, {"base": b"abcd", "base_op": "sub"}, {"element_size": 3},
               {"segment_blocks": 64}, {"block_size": 0}):
        kw = {"block_size": 16, **kw}
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, filter="lag", lag="auto", **kw)
    # only the literal "auto", and only with its filter
    for kw in ({"filter": "lag", "lag": "Auto"}, {"filter": "lag", "lag": "AUTO"}, {"filter": "lag", "lag": " auto"},
               {"filter": "lag", "lag": ""}, {"filter": "lag", "lag": b"auto"}, {"filter": "zigzag", "lag": "auto"},
               {"filter": "delta", "lag": "auto"}, {"lag": "auto"}, {"filter": "Lag", "lag": "auto"}):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, 16, **kw)
    assert len(api.LAYOUTS) == 8 and all(f in (None, "delta") for _, f in api.LAYOUTS)  # the choice of a layout does not see the filter


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_lag_auto(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    some = ["-c", "--block-size", "65536", "--filter", "lag", "--lag", "auto"]
    assert cli.parse(some) == {**base, "filter": "lag", "lag": "auto"}
    assert cli.parse(["-c", "--lag", "auto", "--filter", "lag", "--block-size", "65536"]) == {**base, "filter": "lag", "lag": "auto"}
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "lag", "--lag", "auto"]) == \
            {**base, "block_size": 4096, "element_size": int(E), "filter": "lag", "lag": "auto"}
    assert cli.parse(some + ["--checksum"]) == {**base, "filter": "lag", "lag": "auto", "checksum": True}
    assert cli.parse(["-c", "--block-size", "65536", "--filter", "lag", "--lag", "3"]) == {**base, "filter": "lag", "lag": 3}
    head = ["-c", "--block-size", "65536"]
    for bad in (head + ["--lag", "auto"], head + ["--filter", "zigzag", "--lag", "auto"], head + ["--filter", "delta", "--lag", "auto"],
                head + ["--filter", "lag", "--lag", "Auto"], head + ["--filter", "lag", "--lag", "AUTO"],
                head + ["--filter", "lag", "--lag", "auto "], head + ["--filter", "lag", "--lag", "x"],
                head + ["--filter", "lag", "--lag", "3.0"], head + ["--filter", "lag", "--lag", ""],
                head + ["--filter", "lag", "--lag", "0"], head + ["--filter", "lag", "--lag", "257"], head + ["--filter", "lag", "--lag"],
                head + ["--filter", "lag"], ["-c", "--filter", "lag", "--lag", "auto"],
                ["-c", "--block-size", "0", "--filter", "lag", "--lag", "auto"], ["-d", "--filter", "lag", "--lag", "auto", "--block-size", "0"],
                some + ["--stored"], some + ["--base", "f"], some + ["--skip-constant"], some + ["--layout", "auto"],
                some + ["--layout", "mixed"], some + ["--model", "static"], some + ["--element-size", "2", "--model", "plane-static"],
                some + ["--model", "segment-static"], some + ["--model", "context-static"], some + ["--model", "auto"]):
        assert cli.parse(bad) is None, bad
    for bad in (head + ["--lag", "auto"], head + ["--filter", "lag", "--lag", "Auto"], some + ["--stored"]):
        assert cli.main(bad) == 1, bad
    assert "delta|zigzag|lag" in cli.USAGE and "--lag" in cli.USAGE and "auto" in cli.USAGE.split("--lag")[1].split("]")[0]
    assert "--filter lag --lag S" in cli.__doc__ and "version 13" in cli.__doc__ and "--filter lag --lag auto" in cli.__doc__
    assert "opt-in" in cli.__doc__ and "or S, for you" not in cli.__doc__


# ---- Rust ---------------------------------------------------------------------------------------------------------------
def test_rust_declares_the_lag_estimates():
    rust, hdr = shim.rust_externs(), shim.header_decls()
    for name in ("redux_lag_cost_block_count", "redux_lag_cost_dev", "redux_lag_cost_kernel_name", "redux_lag_cost_kernel_name_at"):
        assert name in rust and name in hdr, name
        (rargs, rret), (cargs, cret) = rust[name], hdr[name]
        assert len(rargs) == len(cargs), name
        assert all(shim.same(rk, ck) for rk, ck in zip(rargs, cargs)) and shim.same(rret, cret), name
    assert len(rust["redux_lag_cost_dev"][0]) == 10 and hdr["redux_lag_cost_block_count"][1] == ("int", 64)
