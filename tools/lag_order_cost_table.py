#!/usr/bin/env python3
"""Order estimates, measured in one GPU run (results: profiles/lag_order_cost.txt).

For E = 1, 2, 4, 8 on `--gib` GiB (default 4) at 64 KiB blocks of two interleaved channels of GENERATED tones in E-byte
integers, the input of tools/lag_order_table.py, every entry warmed up once and then taken in turn in every round (device
events; per entry the median, the fastest and the slowest; the clocks are not touched):

  1. fused     redux_lag_order_cost_dev over the 12 candidates lags 1, 2, 3, 4 x orders 1, 2, 3 at frame_step 1, in the order
               api.lag_order_candidates gives them (by order first): k_lag_order_cost, no transformed copy.  The same list by
               lag first is timed next to it: reported, not gated.
  2. composed  the same 12 rows the way they could be had before: 12 transforms into a scratch buffer (redux_lag_planes_dev
               at order 1, redux_lag_order_planes_dev above), each followed by redux_block_cost_dev.  THE CRITERION: fused
               takes no longer than composed at every E; a row that misses it says MISS.  The two results are compared
               block by block.
  3. choice    the whole of api.choose_lag_order with lag None (both stages, their sums and read-backs) next to the whole of
               api.choose_lag.  Reported, not gated.
  4. coder     the adaptive coder kernel of an encode call on the lag-2 order-3 transform of the same bytes
               (DeviceEncoder.encode_slots), the yardstick rows 1 to 3 are read against.

Then the container bytes behind orders 1, 2 and 3 at the known lag -- the streams of the device encoder summed plus
container.overhead_bytes -- next to the choice of api.choose_lag_order, which is what order="auto" writes, on the tones and on
three interleaved GENERATED random walks (the input of tools/lag_table.py).  No recorded signal is measured.

usage: python tools/lag_order_cost_table.py [--gib N] [--rounds R] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import _lib, api, container  # noqa: E402
from tools import lag_table  # noqa: E402
from tools.lag_order_table import B, CHANNELS, PARAMS, measure, tones  # noqa: E402

LAGS = (1, 2, 3, 4)
CANDS = api.lag_order_candidates(LAGS)


def container_sizes(src, E, lag, n, nb):
    """{K: container bytes of src behind the lag filter at `lag` and order K}"""
    sizes = {}
    for K in (1, 2, 3):
        e = rx.DeviceEncoder(PARAMS, B, n, element_size=E, filter="lag", lag=lag, order=K)
        _, f, _, s = e.encode(src)
        torch.cuda.synchronize()
        assert s.tolist() == [0, 0]
        sizes[K] = int(f[-1]) + container.overhead_bytes("adaptive", nb, E, filter="lag")
        del e, f
        torch.cuda.empty_cache()
    return sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.rounds >= 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.gib << 30
    nb = n // B
    L = _lib.lib()
    cp = _lib.Params(*PARAMS)
    say(f"# {rx.version()}  source hash {L.redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"# {a.gib} GiB = {nb} blocks of 64 KiB: {CHANNELS} interleaved channels of generated tones in E-byte integers; one warm-up, then "
        f"{a.rounds} rounds of every entry in turn; ms: median [fastest .. slowest]; the clocks were not touched")
    misses = []
    for E in (1, 2, 4, 8):
        src = tones(n, E)
        scratch = torch.empty_like(src)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fused_bits = torch.empty((len(CANDS), nb), dtype=torch.float64, device="cuda:0")
        composed_bits = torch.empty((len(CANDS), nb), dtype=torch.float64, device="cuda:0")
        h_lags = np.asarray([S for S, _ in CANDS], dtype=np.uint32)
        h_orders = np.asarray([K for _, K in CANDS], dtype=np.uint32)
        by_lag = sorted(CANDS)
        l_lags = np.asarray([S for S, _ in by_lag], dtype=np.uint32)
        l_orders = np.asarray([K for _, K in by_lag], dtype=np.uint32)
        by_lag_bits = torch.empty((len(CANDS), nb), dtype=torch.float64, device="cuda:0")

        def fused():
            api._raise(L.redux_lag_order_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), n, B, E, h_lags.ctypes.data,
                                                  h_orders.ctypes.data, len(CANDS), 1, C.c_void_p(fused_bits.data_ptr()), stream))

        def fused_by_lag():
            api._raise(L.redux_lag_order_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), n, B, E, l_lags.ctypes.data,
                                                  l_orders.ctypes.data, len(CANDS), 1, C.c_void_p(by_lag_bits.data_ptr()), stream))

        def composed():
            for j, (S, K) in enumerate(CANDS):
                if K == 1:
                    api.lag_planes(src, E, B, S, out=scratch)
                else:
                    api.lag_order_planes(src, E, B, S, K, out=scratch)
                api._raise(L.redux_block_cost_dev(C.byref(cp), C.c_void_p(scratch.data_ptr()), n, B,
                                                  C.c_void_p(composed_bits[j].data_ptr()), stream))

        chosen, lag_chosen = [], []
        t = api.lag_order_planes(src, E, B, CHANNELS, 3)  # what the coder sees
        enc = rx.DeviceEncoder(PARAMS, B, n)
        f12, c12 = "fused, 12 candidates", "composed, 12 candidates"
        runs = {f12: fused, "fused, the same by lag first": fused_by_lag, c12: composed,
                "choose_lag_order": lambda: chosen.append(api.choose_lag_order(src, E, B, None, PARAMS)),
                "choose_lag": lambda: lag_chosen.append(api.choose_lag(src, E, B, PARAMS)), "coder forward": lambda: enc.encode_slots(t)}
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        diff = float((fused_bits - composed_bits).abs().max().item())
        rows = [by_lag.index(c) for c in CANDS]
        assert torch.equal(by_lag_bits[rows], fused_bits), f"E={E}: a row depends on its place in the list"
        ok = med[f12] <= med[c12]
        if not ok:
            misses.append(E)
        for k, v in ms.items():
            tail = ""
            if k == f12:
                tail = f"  {med[k] / med[c12]:.2f} x composed  {'ok' if ok else 'MISS'}"
            elif k.startswith("fused"):
                tail = f"  {med[k] / med[c12]:.2f} x composed"
            elif k in ("choose_lag_order", "choose_lag"):
                tail = f"  {med[k] / med['coder forward']:.2f} x coder"
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]{tail}")
        picks = sorted({c for c, _ in chosen})
        finalists = sorted({S for _, table in chosen for S, _ in table})
        say(f"E={E} fused against composed, {len(CANDS) * nb} blocks: max |difference| = {diff:g} bits; choose_lag_order picked {picks} "
            f"among the orders of lags {finalists}; choose_lag picked {sorted({S for S, _ in lag_chosen})}")
        del enc, t, scratch, fused_bits, composed_bits, by_lag_bits
        torch.cuda.empty_cache()
        # what order="auto" writes: the chosen candidate's ordinary container
        sizes = container_sizes(src, E, CHANNELS, n, nb)
        (S, K), table = chosen[-1]
        say(f"E={E} tones, container bytes of {n} at lag {CHANNELS}: order 1 {sizes[1]}, order 2 {sizes[2]} ({sizes[2] / sizes[1]:.3f}), "
            f"order 3 {sizes[3]} ({sizes[3] / sizes[1]:.3f}); order auto: lag {S} order {K}"
            + (f", {sizes[K]} bytes, estimated payload {table[(S, K)]}" if S == CHANNELS else ""))
        del src
        torch.cuda.empty_cache()
        walks = lag_table.channels(n, E)
        (S, K), table = api.choose_lag_order(walks, E, B, None, PARAMS)
        sizes = container_sizes(walks, E, lag_table.CHANNELS, n, nb)
        say(f"E={E} walks, container bytes of {n} at lag {lag_table.CHANNELS}: order 1 {sizes[1]}, order 2 {sizes[2]} "
            f"({sizes[2] / sizes[1]:.3f}), order 3 {sizes[3]} ({sizes[3] / sizes[1]:.3f}); order auto: lag {S} order {K}"
            + (f", {sizes[K]} bytes, estimated payload {table[(S, K)]}" if S == lag_table.CHANNELS else ""))
        del walks
        torch.cuda.empty_cache()
    say("# the criterion (fused <= composed at every E): "
        + ("met by every row" if not misses else "MISSED at " + ", ".join(f"E={E}" for E in misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
