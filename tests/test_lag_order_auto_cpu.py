"""Order estimates and order="auto" (include/redux_hip.h, "order estimates"): the choice rule on hand-made estimate tables,
the value claim on the CPU oracle -- the order with the smallest counted cost is the order the oracle codes smallest, and the
estimate is within a byte per block of the oracle's payload -- the Python refusals before the library is touched, the CLI
table of `--order-auto`, the ABI's names and the host-side list checks under a sanitizer.  No GPU call.

The value claim rests on GENERATED data, the tones and the interleaved random walks of tests/test_lag_order_cpu.py: no recorded
PCM or sensor log is among the fixtures."""
import os
import subprocess

import numpy as np
import pytest

import test_rust_shim_cpu as shim
from test_lag_auto_cpu import block_counts
from test_lag_cpu import channels
from test_lag_order_cpu import CASES, lag_order_planes_ref, tones
from test_planes_cpu import oracle_bytes

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- the choice rule ---------------------------------------------------------------------------------------------------
def run_rule(nframes, first, exact, lag=None, E=2, Bk=16):
    """choose_lag_order on an input of nframes frames whose estimates are the tables `first` ({S: bytes}, the first stage)
    and `exact` ({(S, K): bytes}) -> ((S, K), the returned dict, the (candidates, frame_step) of every pass)"""
    from redux_amd import api
    calls = []

    def estimate(cands, T):
        calls.append((None if cands is None else list(cands), T))
        if cands is None:
            return {S: first[S] for S in range(1, 257)}
        return {c: exact(c) if callable(exact) else exact[c] for c in cands}
    choice, est = api.choose_lag_order(bytes(nframes * E * Bk), E, Bk, lag, estimate=estimate)
    return choice, est, calls


def three(*lags):
    """every order of every lag, by order first: the candidate list of the exact pass"""
    return [(S, K) for K in (1, 2, 3) for S in lags]


def test_choice_rule_on_hand_made_tables():
    from redux_amd import api
    assert api.LAG_ORDER_COST_MAX == 256 and api.LAG_ORDER_MAX == 3
    flat = {S: 1000 for S in range(1, 257)}
    # a fixed lag: one exact pass over its three orders, no first stage, whatever the length
    for F in (1, 64, 65, 1000):
        choice, est, calls = run_rule(F, None, {(5, 1): 90, (5, 2): 80, (5, 3): 85}, lag=5)
        assert choice == (5, 2) and calls == [(three(5), 1)] and est == {(5, 1): 90, (5, 2): 80, (5, 3): 85}, F
    assert run_rule(3, None, {(5, 1): 90, (5, 2): 80, (5, 3): 70}, lag=np.int64(5))[0] == (5, 3)
    # ties go to the smaller order
    assert run_rule(3, None, {(7, 1): 50, (7, 2): 50, (7, 3): 50}, lag=7)[0] == (7, 1)
    assert run_rule(3, None, {(7, 1): 51, (7, 2): 50, (7, 3): 50}, lag=7)[0] == (7, 2)
    assert run_rule(3, None, {(256, 1): 51, (256, 2): 51, (256, 3): 50}, lag=256)[0] == (256, 3)
    # lag None: choose_lag's first stage (exact up to 64 frames, sampled above), its finalists with lag 1 among them, then one
    # exact pass over every order of every finalist, ordered by order first
    for F, T in ((1, 1), (64, 1), (65, 2), (128, 2), (129, 3), (6401, 101)):
        first = {**flat, 3: 500, 6: 520, 9: 540, 12: 560}
        assert api.lag_finalists(first) == [1, 3, 6, 9]
        exact = {c: 700 for c in three(1, 3, 6, 9)}
        exact[(6, 3)] = 600
        choice, est, calls = run_rule(F, first, exact)
        assert calls == [(None, T), (three(1, 3, 6, 9), 1)], F
        assert choice == (6, 3) and est == exact and len(calls[1][0]) <= 12
    # lag 1 and order 1 are always among the candidates, also when lag 1 is the worst of the sample; they win an exact tie
    first = {**flat, 1: 5000, 4: 10, 8: 20, 16: 30}
    choice, est, calls = run_rule(200, first, lambda c: 40)
    assert calls[1][0] == three(1, 4, 8, 16) and choice == (1, 1)
    assert all((S, 1) in est for S in (1, 4, 8, 16))
    # then the smaller S: equal estimates at order 2 of lags 4 and 8 beat everything else
    choice, est, calls = run_rule(200, first, lambda c: 30 if c in ((8, 2), (4, 2)) else 40)
    assert choice == (4, 2)
    # the smaller K comes before the smaller S: (8, 1) against (4, 2)
    assert run_rule(200, first, lambda c: 30 if c in ((8, 1), (4, 2)) else 40)[0] == (8, 1)
    # lag 1 among the three smallest: three finalists, nine candidates
    choice, est, calls = run_rule(200, {**flat, 1: 5, 4: 10, 8: 20, 16: 30}, lambda c: 9 + c[1])
    assert calls[1][0] == three(1, 4, 8) and choice == (1, 1)
    # never above the order-1 minimum of the same pass, whatever the table holds
    rng = np.random.default_rng(5)
    for _ in range(50):
        first = {S: int(v) for S, v in zip(range(1, 257), rng.integers(100, 200, 256))}
        table = {}
        choice, est, calls = run_rule(200, first, lambda c: table.setdefault(c, int(rng.integers(100, 120))))
        assert est[choice] <= min(v for (S, K), v in est.items() if K == 1)
        assert {S for S, _ in est} == set(api.lag_finalists(first)) and 1 in {S for S, _ in est}
        assert choice == min(est, key=lambda c: (est[c], c[1], c[0]))
    assert api.best_lag_order({(5, 2): 3, (2, 3): 3, (9, 2): 3, (1, 1): 4}) == (5, 2)
    assert api.lag_order_candidates([2, 7]) == three(2, 7) == [(2, 1), (7, 1), (2, 2), (7, 2), (2, 3), (7, 3)]


# ---- the value claim, on the CPU oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,want", [("tones", 3), ("walks", 1)])
@pytest.mark.parametrize("C_,E", CASES)
def test_the_counted_order_is_the_order_the_oracle_codes_smallest(rx, C_, E, kind, want):
    """The bound is a byte per block.  Measured: at most 10 bytes between estimate and oracle payload, over 7 to 49 blocks."""
    from redux_amd import api
    x = tones(C_, E, 7) if kind == "tones" else channels(C_, E, 7)
    est, coded = {}, {}
    for K in (1, 2, 3):
        y = lag_order_planes_ref(x, E, B, C_, K)
        bits = rx.adaptive_cost_from_counts(block_counts(y, B), PARAMS)
        est[(C_, K)] = int(np.ceil(bits.sum() / 8 + api.TERMINATION_BYTES * len(bits)))
        coded[(C_, K)] = oracle_bytes(y, B)
    nb = max(1, -(-len(x) // B))
    worst = max(abs(est[c] - coded[c]) for c in est)
    print("%s, %d channels, E = %d: estimates %s, oracle %s, largest difference %d bytes over %d blocks"
          % (kind, C_, E, list(est.values()), list(coded.values()), worst, nb))
    choice, _ = api.choose_lag_order(x, E, B, C_, estimate=lambda cands, T: {c: est[c] for c in cands})
    assert choice == min(coded, key=lambda c: (coded[c], c[1])) == (C_, want)
    assert worst <= nb, (est, coded)


# ---- Python refusals before the library is touched ----------------------------------------------------------------------
def test_python_refuses_bad_order_auto_and_bad_candidates_before_any_library_call(rx, monkeypatch):
    from redux_amd import _lib, api, container
    flags = np.zeros(1, np.uint8)
    offs = np.array([0, 1], np.uint64)

    def touched():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    data = b"abcd" * 4
    lag3 = {"filter": "lag", "lag": 3, "order": "auto"}
    # order="auto" without its filter or without a lag, under another spelling, and with everything order 2 is refused with
    for kw in ({"order": "auto"}, {"filter": "lag", "order": "auto"}, {"filter": "zigzag", "order": "auto"},
               {"filter": "delta", "order": "auto"}, {"lag": 3, "order": "auto"}, {"filter": "Lag", "lag": 3, "order": "auto"},
               {**lag3, "order": "Auto"}, {**lag3, "order": "AUTO"}, {**lag3, "order": " auto"}, {**lag3, "order": ""},
               {**lag3, "order": b"auto"}, {**lag3, "lag": 0}, {**lag3, "lag": 257}, {**lag3, "lag": "Auto"}, {**lag3, "lag": 3.0},
               {**lag3, "model": "static"}, {**lag3, "model": "plane-static", "element_size": 2}, {**lag3, "model": "segment-static"},
               {**lag3, "model": "context-static"}, {**lag3, "model": "auto"}, {**lag3, "stored": True}, {**lag3, "base": b"abcd"},
               {**lag3, "skip_constant": True}, {**lag3, "layout": "auto"}, {**lag3, "layout": "mixed"},
               {**lag3, "base": b"abcd", "base_op": "sub"}, {**lag3, "element_size": 3}, {**lag3, "segment_blocks": 64},
               {**lag3, "block_size": 0}, {**lag3, "lag": "auto", "stored": True}, {**lag3, "lag": "auto", "model": "static"},
               {**lag3, "lag": "auto", "block_size": 0}, {**lag3, "lag": "auto", "element_size": 3}):
        kw = {"block_size": 16, **kw}
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, **kw)
    # lag "auto" with an integer order above 1 stays refused
    for K in (2, 3):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, 16, filter="lag", lag="auto", order=K)
    # the calls that do not choose keep refusing a string order
    for order in ("auto", "Auto", "2"):
        kw = {"filter": "lag", "lag": 3, "order": order}
        for call in (lambda: rx.compress_blocks(b"abcd", 4, **kw),
                     lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, **kw),
                     lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, **kw),
                     lambda: rx.DeviceDecoder(PARAMS, 4096, 1, **kw),
                     lambda: api.lag_order_planes(None, 2, 4096, 3, order),
                     lambda: container.pack(flags, offs, PARAMS, 4, 4, **kw)):
            with pytest.raises(rx.InvalidInput):
                call()
    # a bad candidate list, and bad scalar arguments
    x = np.zeros(256, np.uint8)
    ok = [(1, 1), (3, 2)]
    for kw in ({"candidates": []}, {"candidates": [(1, 1)] * 257}, {"candidates": [(1, 0)]}, {"candidates": [(1, 4)]},
               {"candidates": [(0, 1)]}, {"candidates": [(257, 1)]}, {"candidates": [(True, 1)]}, {"candidates": [(1, True)]},
               {"candidates": [(1.0, 1)]}, {"candidates": [(1, 2.0)]}, {"candidates": [("1", 1)]}, {"candidates": [(1,)]},
               {"candidates": [(1, 1, 1)]}, {"candidates": [1, 2]}, {"candidates": 3}, {"candidates": None},
               {"candidates": ok + [(3, -1)]}, {"element_size": 3}, {"element_size": 0}, {"element_size": True},
               {"block_size": 0}, {"block_size": (1 << 30) + 1}, {"frame_step": 0}, {"frame_step": -1}, {"frame_step": 1.0}):
        a = {"element_size": 2, "block_size": 64, "candidates": ok, "frame_step": 1, **kw}
        with pytest.raises(rx.InvalidInput):
            api.lag_order_cost(x, a["element_size"], a["candidates"], a["block_size"], PARAMS, a["frame_step"])
        with pytest.raises(rx.InvalidInput):
            api.estimate_lag_orders(x, a["element_size"], a["block_size"], a["candidates"], PARAMS, a["frame_step"])
        with pytest.raises(rx.InvalidInput):
            container.estimate_lag_order_bytes(x, a["element_size"], a["block_size"], a["candidates"], PARAMS, frame_step=a["frame_step"])
    for args in ((3, 64, None), (2, 0, None), (2, (1 << 30) + 1, 3), (2, 64, 0), (2, 64, 257), (2, 64, True), (2, 64, 3.0),
                 (2, 64, "auto")):
        with pytest.raises(rx.InvalidInput):
            api.choose_lag_order(x, *args)
    assert api._candidate_list([(np.int64(3), np.uint8(2)), [256, 3]]) == [(3, 2), (256, 3)]
    assert len(api._candidate_list([(1, 1)] * 256)) == 256


def test_overhead_of_versions_13_and_14_is_the_same_size(rx):
    from redux_amd import container
    for E in (1, 2, 4, 8):
        for nb, checksum in ((1, False), (5, False), (5, True)):
            streams = np.zeros(nb, np.uint8)
            offs = np.arange(nb + 1, dtype=np.uint64)
            crc = np.zeros(nb, np.uint32) if checksum else None
            sizes = []
            for K in (1, 2, 3):
                blob = container.pack(streams, offs, PARAMS, 64, nb * 64, element_size=E, block_crc=crc, filter="lag", lag=3, order=K)
                assert container.order(blob) == K and container.lag(blob) == 3
                sizes.append(len(blob) - nb)
            assert sizes == [container.overhead_bytes("adaptive", nb, E, checksum=checksum, filter="lag")] * 3, (E, nb, checksum)


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_order_auto_flag(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    some = ["-c", "--block-size", "65536", "--filter", "lag", "--lag", "3"]
    auto = ["-c", "--block-size", "65536", "--filter", "lag", "--lag", "auto"]
    assert cli.parse(some + ["--order-auto"]) == {**base, "filter": "lag", "lag": 3, "order": "auto"}
    assert cli.parse(auto + ["--order-auto"]) == {**base, "filter": "lag", "lag": "auto", "order": "auto"}
    assert cli.parse(["-c", "--order-auto", "--lag", "256", "--filter", "lag", "--block-size", "65536"]) == \
        {**base, "filter": "lag", "lag": 256, "order": "auto"}
    for E in ("1", "2", "4", "8"):
        assert cli.parse(["-c", "--block-size", "4096", "--element-size", E, "--filter", "lag", "--lag", "auto", "--order-auto"]) == \
            {**base, "block_size": 4096, "element_size": int(E), "filter": "lag", "lag": "auto", "order": "auto"}
    assert cli.parse(some + ["--order-auto", "--checksum"]) == {**base, "filter": "lag", "lag": 3, "order": "auto", "checksum": True}
    # calls that do not use it get the dicts they got
    assert cli.parse(some) == {**base, "filter": "lag", "lag": 3}
    assert cli.parse(some + ["--order", "2"]) == {**base, "filter": "lag", "lag": 3, "order": 2}
    assert cli.parse(auto) == {**base, "filter": "lag", "lag": "auto"}
    head = ["-c", "--block-size", "65536"]
    for bad in (some + ["--order-auto", "--order", "2"], some + ["--order", "2", "--order-auto"], some + ["--order", "1", "--order-auto"],
                some + ["--order-auto", "--order", "1"], some + ["--order-auto", "--order-auto"], some + ["--order", "auto"],
                auto + ["--order", "auto"], some + ["--order-auto", "x"], some + ["--order-Auto"], some + ["--order-auto=1"],
                head + ["--order-auto"], head + ["--filter", "zigzag", "--order-auto"], head + ["--filter", "delta", "--order-auto"],
                head + ["--filter", "lag", "--order-auto"], head + ["--lag", "3", "--order-auto"],
                ["-c", "--filter", "lag", "--lag", "3", "--order-auto"], ["-c", "--block-size", "0", "--filter", "lag", "--lag", "3", "--order-auto"],
                ["-d", "--order-auto"], ["-d", "--block-size", "65536", "--filter", "lag", "--lag", "3", "--order-auto"],
                some + ["--order-auto", "--stored"], some + ["--order-auto", "--base", "f"], some + ["--order-auto", "--skip-constant"],
                some + ["--order-auto", "--layout", "auto"], some + ["--order-auto", "--layout", "mixed"],
                some + ["--order-auto", "--model", "static"], some + ["--order-auto", "--model", "auto"],
                some + ["--order-auto", "--model", "segment-static"], auto + ["--order-auto", "--stored"],
                auto + ["--order-auto", "--model", "context-static"]):
        assert cli.parse(bad) is None, bad
    for bad in (some + ["--order-auto", "--order", "2"], head + ["--order-auto"], ["-d", "--order-auto"], some + ["--order-auto", "--stored"]):
        assert cli.main(bad) == 1, bad
    assert "--order <1|2|3>" in cli.USAGE and "[--order-auto]" in cli.USAGE
    assert "`--order-auto`" in cli.__doc__ and "[--order-auto]" in cli.__doc__ and "choose_lag_order" in cli.__doc__
    assert "generated" in cli.__doc__.split("`--order-auto` (")[1].split("`--base FILE`")[0]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_order_estimates(rx):
    from redux_amd import _lib
    rust, hdr = shim.rust_externs(), shim.header_decls()
    for name in ("redux_lag_order_cost_dev", "redux_lag_order_cost_kernel_name", "redux_lag_order_cost_kernel_name_at"):
        assert name in _lib.SIGNATURES and name in rust and name in hdr, name
        (rargs, rret), (cargs, cret) = rust[name], hdr[name]
        assert len(rargs) == len(cargs) == len(_lib.SIGNATURES[name][1]), name
        assert all(shim.same(rk, ck) for rk, ck in zip(rargs, cargs)) and shim.same(rret, cret), name
    assert len(hdr["redux_lag_order_cost_dev"][0]) == len(hdr["redux_lag_cost_dev"][0]) + 1
    for name in ("lag_order_cost", "estimate_lag_orders", "choose_lag_order"):
        assert getattr(rx, name) is getattr(rx.api, name)
    assert "#define REDUX_LAG_ORDER_COST_MAX 256" in shim.HEADER


def test_abi_refuses_bad_candidates_before_any_device_work(rx):
    import ctypes as C
    from redux_amd import _lib
    L = _lib.lib()
    ok = _lib.Params(*PARAMS)
    d_in, d_bits = C.c_void_p(4096), C.c_void_p(1 << 20)  # (never dereferenced: every call below is refused on the host)
    lags = np.array([1, 2, 3, 256], dtype=np.uint32)
    orders = np.array([1, 2, 3, 3], dtype=np.uint32)

    def call(p=ok, d=d_in, n=1024, Bk=64, E=2, lg=lags, od=orders, nc=4, T=1, bits=d_bits):
        return L.redux_lag_order_cost_dev(C.byref(p) if p is not None else None, d, n, Bk, E, lg.ctypes.data if lg is not None else None,
                                          od.ctypes.data if od is not None else None, nc, T, bits, None)
    for kw in ({"Bk": 0}, {"Bk": (1 << 30) + 1}, {"E": 0}, {"E": 3}, {"E": 16}, {"nc": 0}, {"nc": 257}, {"T": 0}, {"lg": None},
               {"od": None}, {"bits": None}, {"d": None}, {"p": None}):
        assert call(**kw) == _lib.INVALID_INPUT, kw
    for at in range(4):
        for bad in (0, 257, 1 << 16, 0xFFFFFFFF):
            one = lags.copy()
            one[at] = bad
            assert call(lg=one) == _lib.INVALID_INPUT, (bad, at)
        for bad in (0, 4, 256, 0xFFFFFFFF):
            one = orders.copy()
            one[at] = bad
            assert call(od=one) == _lib.INVALID_INPUT, (bad, at)
    small = _lib.Params(8, 14, 16)
    assert call(p=small, Bk=65536) == _lib.UNSUPPORTED
    for E in (1, 2, 4, 8):
        fast, slow = b"k_lag_order_cost<%d>" % E, b"k_lag_order_cost_bytes<%d>" % E
        assert L.redux_lag_order_cost_kernel_name(3 * E * 64, 64, E) == fast
        assert L.redux_lag_order_cost_kernel_name(3 * E * 64 + 1, 64, E) == fast + b" + " + slow
        assert L.redux_lag_order_cost_kernel_name(E * 64 - 1, 64, E) == slow and L.redux_lag_order_cost_kernel_name(0, 64, E) == slow
        assert L.redux_lag_order_cost_kernel_name(3 * E * 40, 40, E) == slow
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(4096), 3 * E * 64, 64, E) == fast
        assert L.redux_lag_order_cost_kernel_name_at(C.c_void_p(4096 + 1), 3 * E * 64, 64, E) == slow
    for bad in ((100, 0, 2), (100, (1 << 30) + 1, 2), (100, 64, 3), (100, 64, 0)):
        assert L.redux_lag_order_cost_kernel_name(*bad) == b"", bad


# ---- the host-side list checks under a sanitizer --------------------------------------------------------------------------
def test_candidate_list_checks_under_address_and_undefined_sanitizers(tmp_path):
    """redux_lag_order_cost_dev's list handling is split from the launch (redux_lag_order_cost_list.hpp): a stand-alone
    program runs it on heap lists of exactly ncand entries, so a read past either list is an error"""
    exe = str(tmp_path / "lag_order_cost_list_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "lag_order_cost_list_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout, run.stderr)
