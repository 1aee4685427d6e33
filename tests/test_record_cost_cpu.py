"""Record estimates and record_size="auto" (include/redux_hip.h, "record estimates"): the sampling arithmetic against a Python
restatement, lengths past 2^32 included; the refusals of the C entry points before any device work and the kernel names; the
choice rule on hand-made estimates; the value claim on the host rule -- the adaptive cost of the counts of record_ref -- on the
two GENERATED tables of tests/test_record_cpu.py and on random bytes; the Python refusals before the library is touched; the
CLI's `--record-size auto`; the ABI's names; and the host-side list checks under a sanitizer.  No GPU call.

No recorded table is among the fixtures: the value claim rests on generated data."""
import os
import subprocess

import numpy as np
import pytest

import test_rust_shim_cpu as shim
from test_lag_auto_cpu import block_counts
from test_record_cpu import generated_tables, record_ref

PARAMS = (8, 30, 32)
B = 4096  # the block size of the value claim
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = {"imu23": ((23, "delta"), 378060), "ticks20": ((20, "delta"), 136086)}  # the oracle's payload bytes at B


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- the sampling rule ---------------------------------------------------------------------------------------------------
def sample_ref(n, Bk, R, Q):
    """the rule as the header states it -> (T, the selected frames' count, the blocks of the row)"""
    nframes = max(1, -(-n // (R * Bk)))
    T = 1
    if Q > 0:
        want = -(-Q // R)
        T = 1 if nframes <= want else -(-nframes // want)
    nblocks = max(1, -(-n // Bk))
    nsel = len(range(0, nframes, T))
    last = (nsel - 1) * T
    return T, nsel, (nsel - 1) * R + min(R, nblocks - last * R)


def selected_columns(n, Bk, R, Q):
    """the blocks of the frames 0, T, 2T, ... in order: the columns of the exact row that a sampled row keeps"""
    T, _, _ = sample_ref(n, Bk, R, Q)
    nblocks = max(1, -(-n // Bk))
    return [b for f in range(0, -(-nblocks // R), T) for b in range(f * R, min(f * R + R, nblocks))]


def test_frame_step_and_block_count_match_the_restatement(rx):
    from redux_amd import _lib, api
    L = _lib.lib()
    for R in (2, 3, 23, 255, 256):
        for Bk in (16, 4096, 65536):
            for Q in (0, 1, 64, 1000):
                for n in (0, 1, R - 1, R * Bk, R * Bk + 1, 100 * R * Bk, 100 * R * Bk + Bk + 3, (1 << 33) + 5):
                    T, nsel, row = sample_ref(n, Bk, R, Q)
                    assert L.redux_record_cost_frame_step(n, Bk, R, Q) == T, (R, Bk, Q, n)
                    assert L.redux_record_cost_block_count(n, Bk, R, Q) == row, (R, Bk, Q, n)
                    assert api.record_cost_sample(n, Bk, R, Q)[:2] == (T, row)
                    if n <= 100 * R * Bk + Bk + 3:
                        assert len(selected_columns(n, Bk, R, Q)) == row
                    if Q == 0:
                        assert T == 1 and row == L.redux_block_count(n, Bk)
                    else:  # about Q blocks: whole frames, so fewer than Q + R unless every frame is costed
                        assert row <= L.redux_block_count(n, Bk) and (T == 1 or row < Q + 2 * R)
    # past 2^32: counts only
    n = (1 << 33) + 5
    assert sample_ref(n, 65536, 23, 64) == (1900, 3, 69) and L.redux_record_cost_block_count(n, 65536, 23, 0) == 131073
    assert L.redux_record_cost_frame_step(n, 16, 2, 1) == 268435457 and L.redux_record_cost_block_count(n, 16, 2, 1) == 2
    # the input bytes a sampled row stands for
    assert api.record_cost_sample(49, 16, 3, 0) == (1, 4, 49) and api.record_cost_sample(49, 16, 3, 1) == (2, 3, 48)
    assert api.record_cost_sample(0, 16, 3, 64) == (1, 1, 0)


def test_bad_arguments_give_zero_or_invalid_input_before_any_device_call(rx):
    import ctypes as C
    from redux_amd import _lib
    L = _lib.lib()
    for bad in ((100, 0, 3, 0), (100, (1 << 30) + 1, 3, 0), (100, 64, 0, 0), (100, 64, 1, 0), (100, 64, 257, 64), (100, 64, 1 << 16, 1)):
        assert L.redux_record_cost_frame_step(*bad) == 0 and L.redux_record_cost_block_count(*bad) == 0, bad
    ok = _lib.Params(*PARAMS)
    d_in, d_bits = C.c_void_p(4096), C.c_void_p(1 << 20)  # (never dereferenced: every call below is refused on the host)
    records = np.array([2, 23, 23, 256], dtype=np.uint32)
    deltas = np.array([0, 1, 1, 0], dtype=np.uint8)

    def call(p=ok, d=d_in, n=1024, Bk=64, rs=records, ds=deltas, nc=4, Q=0, bits=d_bits):
        return L.redux_record_cost_dev(C.byref(p) if p is not None else None, d, n, Bk, rs.ctypes.data if rs is not None else None,
                                       ds.ctypes.data if ds is not None else None, nc, Q, bits, None)
    for kw in ({"Bk": 0}, {"Bk": (1 << 30) + 1}, {"nc": 0}, {"nc": 257}, {"nc": 0xFFFFFFFF}, {"rs": None}, {"ds": None}, {"bits": None},
               {"d": None}, {"p": None}):
        assert call(**kw) == _lib.INVALID_INPUT, kw
    for at in range(4):
        for bad in (0, 1, 257, 1 << 16, 0xFFFFFFFF):
            one = records.copy()
            one[at] = bad
            assert call(rs=one) == _lib.INVALID_INPUT, (bad, at)
        for bad in (2, 128, 255):
            one = deltas.copy()
            one[at] = bad
            assert call(ds=one) == _lib.INVALID_INPUT, (bad, at)
    assert call(p=_lib.Params(8, 14, 16), Bk=65536) == _lib.UNSUPPORTED


def test_kernel_name_tells_the_paths_apart(rx):
    import ctypes as C
    from redux_amd import _lib
    L = _lib.lib()
    fast, slow = b"k_record_cost", b"k_record_cost_bytes"
    for R in (2, 3, 23, 255, 256):
        assert L.redux_record_cost_kernel_name(3 * R * 64, 64, R) == fast
        assert L.redux_record_cost_kernel_name(3 * R * 64 + 1, 64, R) == fast + b" + " + slow
        assert L.redux_record_cost_kernel_name(R * 64 - 1, 64, R) == slow and L.redux_record_cost_kernel_name(0, 64, R) == slow
        assert L.redux_record_cost_kernel_name(3 * R * 40, 40, R) == slow and L.redux_record_cost_kernel_name(3 * R * 4099, 4099, R) == slow
        assert L.redux_record_cost_kernel_name_at(C.c_void_p(4096), 3 * R * 64, 64, R) == fast
        assert L.redux_record_cost_kernel_name_at(C.c_void_p(4096 + 1), 3 * R * 64, 64, R) == slow
        assert L.redux_record_cost_kernel_name((1 << 33) + 5, 65536, R) == fast + b" + " + slow
    for bad in ((100, 0, 3), (100, (1 << 30) + 1, 3), (100, 64, 1), (100, 64, 0), (100, 64, 257)):
        assert L.redux_record_cost_kernel_name(*bad) == b"", bad


# ---- the choice rule on constructed estimates ------------------------------------------------------------------------------
def run_rule(nbytes, Bk, sampled, exact, plain):
    """choose_record on nbytes zeros whose estimates are the functions `sampled` (stage 1), `exact` and the number `plain`
    -> (choice, the returned dict, the (candidates, sample_blocks) of every pass)"""
    from redux_amd import api
    calls = []

    def estimate(cands, Q):
        calls.append((None if cands is None else list(cands), Q))
        if cands is None:
            return {None: plain}
        return {c: (sampled if Q else exact)(c) for c in cands}
    choice, est = api.choose_record(bytes(nbytes), Bk, estimate=estimate)
    return choice, est, calls


def test_choice_rule_on_constructed_estimates(rx):
    from redux_amd import api
    assert api.RECORD_COST_MAX == 256 and api.RECORD_SAMPLE_BLOCKS == 64 and api.RECORD_FINALISTS == 4
    allc = api.record_candidates()
    assert len(allc) == 510 and allc[0] == (2, None) and allc[1] == (2, "delta") and allc[-1] == (256, "delta")
    # few frames: stage 1 is exact for every candidate (256 * 16 * 1 frame each at most), its figures stand, the plain cost is added
    choice, est, calls = run_rule(16 * 16, 16, lambda c: 900 if c != (7, "delta") else 800, None, 850)
    assert calls == [(allc, 64), (None, 0)] and choice == (7, "delta") and len(est) == 511 and est[None] == 850
    # many frames: the four best by sampled bytes per costed input byte, one exact pass, the plain cost
    n, Bk = 1000 * 256 * 16, 16

    def sampled(c):  # every candidate at rate 1.0, four below it: costed bytes differ, so equal rates are unequal byte counts
        rate = {(23, "delta"): 0.30, (46, "delta"): 0.35, (69, "delta"): 0.40, (23, None): 0.50}.get(c, 1.0)
        return int(rate * api.record_cost_sample(n, Bk, c[0], 64)[2])
    four = [(23, "delta"), (46, "delta"), (69, "delta"), (23, None)]
    choice, est, calls = run_rule(n, Bk, sampled, lambda c: 1000 + 10 * four.index(c), 5000)
    assert calls == [(allc, 64), (four, 0), (None, 0)] and choice == (23, "delta")
    assert est == {**{c: 1000 + 10 * i for i, c in enumerate(four)}, None: 5000}
    # the exact pass decides, not the sample
    assert run_rule(n, Bk, sampled, lambda c: 900 if c == (69, "delta") else 1000, 5000)[0] == (69, "delta")
    # equal estimates: the smaller R, then no filter; None wins a tie against any candidate
    assert run_rule(n, Bk, sampled, lambda c: 1000, 5000)[0] == (23, None)
    assert run_rule(n, Bk, sampled, lambda c: 1000 if c[1] else 1001, 5000)[0] == (23, "delta")
    assert run_rule(n, Bk, sampled, lambda c: 1000, 1000)[0] is None
    assert run_rule(n, Bk, sampled, lambda c: 1000, 1001)[0] == (23, None)
    assert run_rule(n, Bk, sampled, lambda c: 1000, 999)[0] is None
    assert api.best_record({(5, "delta"): 3, (5, None): 3, (4, "delta"): 3, (9, None): 2, None: 3}) == (9, None)
    assert api.best_record({(5, "delta"): 3, (5, None): 3, (4, "delta"): 3, (9, None): 4}) == (4, "delta")
    assert api.best_record({(5, "delta"): 3, (5, None): 3, (9, None): 4, None: 3}) is None
    # the finalists: four, ties to the smaller R, then to no filter; by rate where the costed bytes are given
    flat = {c: 100 for c in allc}
    assert api.record_finalists(flat) == [(2, None), (2, "delta"), (3, None), (3, "delta")]
    assert len(api.record_finalists({**flat, None: 1})) == 4 and None not in api.record_finalists({**flat, None: 1})
    assert api.record_finalists({**flat, (200, "delta"): 99, (100, None): 99}) == [(100, None), (200, "delta"), (2, None), (2, "delta")]
    costed = {c: 1000 for c in allc}
    costed[(50, None)] = 2000  # the same bytes for twice the input: half the rate
    assert api.record_finalists(flat, costed)[0] == (50, None) and len(api.record_finalists(flat, costed)) == 4
    assert api.record_finalists({(3, None): 5, (2, "delta"): 5}) == [(2, "delta"), (3, None)]


# ---- the value claim, on the host rule -------------------------------------------------------------------------------------
def numpy_estimate(x, Bk):
    """choose_record's `estimate` from numpy: the adaptive cost of the byte counts of record_ref, frame by frame (frames are
    independent, so a sampled pass transforms its selected frames alone)"""
    from redux_amd import api
    x = np.ascontiguousarray(x, np.uint8)

    def total(bits):
        return int(np.ceil(float(bits.sum()) / 8 + api.TERMINATION_BYTES * len(bits)))

    def estimate(cands, Q):
        if cands is None:
            bits = api.adaptive_cost_from_counts(block_counts(x, Bk), PARAMS)
            return {None: total(bits), "noise": api.record_noise_bytes(bits, len(x) // Bk)}
        out = {}
        for R, f in cands:
            T = sample_ref(len(x), Bk, R, Q)[0]
            frame = R * Bk
            rows = [api.adaptive_cost_from_counts(block_counts(record_ref(x[at: at + frame], R, Bk, f is not None), Bk), PARAMS)
                    for at in range(0, max(1, len(x)), T * frame)]
            out[(R, f)] = total(np.concatenate(rows))
        return out
    return estimate


@pytest.fixture(scope="module")
def claims():
    """{name: (choice, estimates)} of choose_record under numpy_estimate, for the two generated tables and random bytes"""
    from redux_amd import api
    data = {name: x for name, (x, _) in generated_tables().items()}
    data["random"] = np.random.default_rng(0).integers(0, 256, 65536, dtype=np.uint8)
    return {name: api.choose_record(x, B, estimate=numpy_estimate(x, B)) for name, x in data.items()}


@pytest.mark.parametrize("name", ["imu23", "ticks20"])
def test_the_rule_finds_the_record_size_and_the_filter_of_the_generated_tables(claims, name):
    """Measured: imu23 (23, delta) 377,980 against the oracle's 378,060; ticks20 (20, delta) 136,031 against 136,086."""
    choice, est = claims[name]
    want, coded = ORACLE[name]
    print(name, "choice", choice, "estimates", est)
    assert choice == want and None in est and len(est) == 5
    assert abs(est[choice] - coded) <= coded / 1000, (est[choice], coded)
    assert est[choice] < est[None]


def test_random_bytes_keep_the_plain_container(claims):
    """Measured on 64 KiB of default_rng(0).integers(0, 256) at B = 4096: plain 66,348 bytes estimated; the smallest of the 510
    candidates, all costed exactly, are (235, None) 66,323, (108, delta) 66,325, (24, None) 66,326, and the oracle agrees
    (66,352 plain, 66,324 behind record_ref(x, 235)): every candidate deals iid bytes into other blocks, and the smallest of
    510 such draws lies about 3 standard deviations of that noise below the plain cost.  record_noise_bytes of the plain
    block costs is printed; the gain of 25 bytes is fewer than the 6.4 deviations RECORD_NOISE_SIGMAS asks for: None."""
    from redux_amd import api
    choice, est = claims["random"]
    low = sorted(est, key=lambda c: est[c])[:5]
    print("random: choice", choice, "plain", est[None], "smallest", [(c, est[c]) for c in low])
    assert "noise" not in est
    assert choice is None and api.best_record(est) is not None and est[api.best_record(est)] < est[None]


@pytest.mark.parametrize("seed,n,top", [(5, 65536, 256), (1, 1 << 20, 256), (2, 1 << 19, 16)])
def test_the_smallest_of_510_draws_of_noise_is_not_chosen(seed, n, top):
    """iid bytes of other seeds, lengths and alphabets (the largest gains seen over seeds 0 to 5, at 1 MiB, where stage 2
    runs on four finalists, and with 16 symbols): 36, 114 and 24 bytes."""
    from redux_amd import api
    x = np.random.default_rng(seed).integers(0, top, n, dtype=np.uint8)
    choice, est = api.choose_record(x, B, estimate=numpy_estimate(x, B))
    print("seed", seed, "choice", choice, "plain", est[None], "smallest", min(v for k, v in est.items() if k is not None))
    assert choice is None


def test_noise_scale_is_read_off_the_plain_block_costs(rx):
    from redux_amd import api
    assert api.record_noise_bytes([]) == 0.0 and api.record_noise_bytes([800.0]) == 0.0 and api.record_noise_bytes([8.0] * 9) == 0.0
    # nine blocks whose costs have the sample deviation 16 bits: 16 * sqrt(9) / 8 = 6 bytes
    bits = np.array([100, 116, 84, 116, 84, 116, 84, 116, 84], dtype=np.float64)
    s = np.sqrt(((bits - bits.mean()) ** 2).sum() / 8)
    assert abs(api.record_noise_bytes(bits) - s * 3 / 8) < 1e-12 and abs(api.record_noise_bytes(bits) - 6.0) < 0.1
    # a short last block is left out of the deviation, not of the count: 16 * sqrt(10) / 8; one full block: no deviation
    short = np.append(bits, 3.0)
    assert abs(api.record_noise_bytes(short, 9) - s * np.sqrt(10) / 8) < 1e-12 and api.record_noise_bytes(short) > 2 * 6.0
    assert api.record_noise_bytes([800.0, 300.0], 1) == 0.0 and api.record_noise_bytes([800.0, 300.0], 0) == 0.0
    assert api.RECORD_NOISE_SIGMAS == 6.4
    # a gain inside the noise goes to None, one outside it is taken; a hook that reports no noise keeps ties only
    calls = []

    def rule(plain, noise):
        def estimate(cands, Q):
            calls.append(cands)
            return {None: plain, "noise": noise} if cands is None else {c: 1000 for c in cands}
        choice, est = api.choose_record(bytes(256), 16, estimate=estimate)
        assert "noise" not in est and est[None] == plain
        return choice
    assert rule(1064, 10.0) is None and rule(1065, 10.0) == (2, None) and rule(1001, 0.0) == (2, None) and rule(1000, 0.0) is None


# ---- Python refusals before the library is touched -------------------------------------------------------------------------
def test_python_refuses_bad_record_auto_before_any_library_or_torch_call(rx, monkeypatch):
    from redux_amd import _lib, api, container
    offs = np.array([0, 1], np.uint64)

    def touched():
        raise AssertionError("the library or torch was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(api, "_torch", touched)
    data = b"abcd" * 4
    auto = {"record_size": "auto"}
    for kw in ({**auto, "filter": "delta"}, {**auto, "filter": "zigzag"}, {**auto, "filter": "lag", "lag": 3}, {**auto, "filter": "Delta"},
               {"record_size": "Auto"}, {"record_size": "AUTO"}, {"record_size": " auto"}, {"record_size": ""}, {"record_size": b"auto"},
               {**auto, "model": "static"}, {**auto, "model": "segment-static"}, {**auto, "model": "context-static"}, {**auto, "model": "auto"},
               {**auto, "stored": True}, {**auto, "base": b"abcd"}, {**auto, "skip_constant": True}, {**auto, "layout": "auto"},
               {**auto, "layout": "mixed"}, {**auto, "segment_blocks": 64}, {**auto, "lag": "auto"}, {**auto, "lag": 3}, {**auto, "order": "auto"},
               {**auto, "order": 1}, {**auto, "element_size": 4}, {**auto, "element_size": 2}, {**auto, "base_op": "sub"},
               {**auto, "block_size": 0}, {**auto, "block_size": (1 << 30) + 1}):
        kw = {"block_size": 16, **kw}
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, **kw)
    # the calls that do not choose keep refusing a string
    for call in (lambda: rx.compress_blocks(b"abcd", 4, record_size="auto"),
                 lambda: rx.decompress_blocks(b"\0", offs, 4, length=4, record_size="auto"),
                 lambda: rx.DeviceEncoder(PARAMS, 4096, 4096, record_size="auto"),
                 lambda: rx.DeviceDecoder(PARAMS, 4096, 1, record_size="auto"),
                 lambda: api.record_planes(None, "auto", 16),
                 lambda: container.pack(np.zeros(1, np.uint8), offs, PARAMS, 4, 4, record_size="auto"),
                 lambda: container.overhead_bytes("adaptive", 1, record_size="auto")):
        with pytest.raises(rx.InvalidInput):
            call()
    # a bad candidate list, and bad scalar arguments
    x = np.zeros(256, np.uint8)
    ok = [(2, None), (23, "delta")]
    with pytest.raises(rx.InvalidInput):
        api.record_cost(x, [(2, None)] * 257, 64)  # (one call's list; estimate_records splits up to 510 into calls of 256)
    for kw in ({"candidates": []}, {"candidates": [(2, None)] * 511}, {"candidates": [(1, None)]}, {"candidates": [(257, None)]},
               {"candidates": [(0, "delta")]}, {"candidates": [(True, None)]}, {"candidates": [(3.0, None)]}, {"candidates": [("3", None)]},
               {"candidates": [(3, "zigzag")]}, {"candidates": [(3, "Delta")]}, {"candidates": [(3, 2)]}, {"candidates": [(3, -1)]},
               {"candidates": [(3, 1.0)]}, {"candidates": [(3,)]}, {"candidates": [(3, None, None)]}, {"candidates": [2, 3]},
               {"candidates": 3}, {"candidates": ok + [(3, b"delta")]}, {"block_size": 0}, {"block_size": (1 << 30) + 1},
               {"block_size": True}, {"block_size": 64.0}, {"sample_blocks": -1}, {"sample_blocks": 1 << 32}, {"sample_blocks": 1.0},
               {"sample_blocks": True}):
        a = {"block_size": 64, "candidates": ok, "sample_blocks": 0, **kw}
        with pytest.raises(rx.InvalidInput):
            api.record_cost(x, a["candidates"], a["block_size"], PARAMS, a["sample_blocks"])
        with pytest.raises(rx.InvalidInput):
            api.estimate_records(x, a["block_size"], a["candidates"], PARAMS, a["sample_blocks"])
        with pytest.raises(rx.InvalidInput):
            container.estimate_record_bytes(x, a["block_size"], a["candidates"], PARAMS, sample_blocks=a["sample_blocks"])
    with pytest.raises(rx.InvalidInput):
        api.record_cost(x, None, 64)
    for Bk in (0, (1 << 30) + 1, True, 64.0, "64"):
        with pytest.raises(rx.InvalidInput):
            api.choose_record(x, Bk)
    assert api._record_candidate_list([(np.int64(3), None), [256, "delta"], (4, False), (5, True), (6, 0), (7, np.uint8(1))]) == \
        [(3, None), (256, "delta"), (4, None), (5, "delta"), (6, None), (7, "delta")]
    assert len(api._record_candidate_list([(2, None)] * 256)) == 256


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def test_cli_record_size_auto(rx):
    from redux_amd import cli
    base = {"compress": True, "input": None, "output": None, "block_size": 65536}
    auto = ["-c", "--block-size", "65536", "--record-size", "auto"]
    assert cli.parse(auto) == {**base, "record_size": "auto"}
    assert cli.parse(auto + ["--checksum"]) == {**base, "record_size": "auto", "checksum": True}
    assert cli.parse(["-c", "--record-size", "auto", "--block-size", "4096", "--element-size", "1", "--model", "adaptive"]) == \
        {**base, "block_size": 4096, "record_size": "auto", "element_size": 1, "model": "adaptive"}
    # calls that do not use it get the dicts they got
    assert cli.parse(["-c", "--block-size", "65536", "--record-size", "23"]) == {**base, "record_size": 23}
    assert cli.parse(["-c", "--block-size", "65536", "--record-size", "23", "--filter", "delta"]) == {**base, "record_size": 23, "filter": "delta"}
    head = ["-c", "--block-size", "65536"]
    for bad in (auto + ["--filter", "delta"], ["-c", "--block-size", "65536", "--filter", "delta", "--record-size", "auto"],
                auto + ["--filter", "zigzag"], auto + ["--filter", "lag", "--lag", "23"], auto + ["--lag", "23"], auto + ["--lag", "auto"],
                auto + ["--order", "1"], auto + ["--order-auto"], auto + ["--stored"], auto + ["--base", "f"], auto + ["--skip-constant"],
                auto + ["--layout", "auto"], auto + ["--layout", "mixed"], auto + ["--model", "static"], auto + ["--model", "segment-static"],
                auto + ["--model", "context-static"], auto + ["--model", "auto"], auto + ["--element-size", "2"], auto + ["--element-size", "8"],
                ["-c", "--record-size", "auto"], ["-c", "--block-size", "0", "--record-size", "auto"], ["-d", "--record-size", "auto"],
                ["-d", "--block-size", "65536", "--record-size", "auto"], head + ["--record-size", "Auto"], head + ["--record-size", "AUTO"],
                head + ["--record-size", "auto "], head + ["--record-size"], head + ["--record-size=auto"]):
        assert cli.parse(bad) is None, bad
    for bad in (auto + ["--filter", "delta"], auto + ["--stored"], ["-d", "--record-size", "auto"], ["-c", "--record-size", "auto"]):
        assert cli.main(bad) == 1, bad
    # the pinned strings of the record layout's own test are still there
    assert "--record-size <2..256>" in cli.USAGE and "--record-size R [--filter delta]" in cli.__doc__ and "version 15" in cli.__doc__
    assert "[--record-size <2..256>|auto]" in cli.USAGE and "`--record-size auto`" in cli.__doc__ and "choose_record" in cli.__doc__
    assert "generated" in cli.__doc__.split("`--record-size auto` (")[1].split("`--range START:LENGTH`")[0]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_abi_declares_the_record_estimates(rx):
    from redux_amd import _lib, container
    rust, hdr = shim.rust_externs(), shim.header_decls()
    names = ("redux_record_cost_frame_step", "redux_record_cost_block_count", "redux_record_cost_dev", "redux_record_cost_kernel_name",
             "redux_record_cost_kernel_name_at")
    for name in names:
        assert name in _lib.SIGNATURES and name in rust and name in hdr, name
        (rargs, rret), (cargs, cret) = rust[name], hdr[name]
        assert len(rargs) == len(cargs) == len(_lib.SIGNATURES[name][1]), name
        assert all(shim.same(rk, ck) for rk, ck in zip(rargs, cargs)) and shim.same(rret, cret), name
    assert len(hdr["redux_record_cost_dev"][0]) == 10 and hdr["redux_record_cost_block_count"][1] == ("int", 64)
    assert hdr["redux_record_cost_frame_step"][1] == ("int", 32)
    for name in ("record_cost", "estimate_records", "choose_record", "RECORD_COST_MAX"):
        assert getattr(rx, name) is getattr(rx.api, name)
    assert callable(container.estimate_record_bytes)
    assert "#define REDUX_RECORD_COST_MAX 256" in shim.HEADER


# ---- the host-side list checks and sampling arithmetic under a sanitizer --------------------------------------------------
def test_list_checks_and_sampling_under_address_and_undefined_sanitizers(tmp_path):
    """redux_record_cost_dev's list handling and sampling arithmetic are split from the launch (redux_record_cost_list.hpp): a
    stand-alone program runs them on heap lists of exactly ncand entries, so a read past either list is an error"""
    exe = str(tmp_path / "record_cost_list_test")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "cpp", "record_cost_list_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "ok" in run.stdout, (run.stdout, run.stderr)
