#!/usr/bin/env python3
"""Lag estimates, measured in one GPU run (results: profiles/lag_cost.txt).

For E = 1, 2, 4, 8 on `--gib` GiB (default 4) at 64 KiB blocks of three interleaved random walks of E-byte integers, the
input of tools/lag_table.py, every entry warmed up once and then taken in turn in every round (device events; per entry the
median, the fastest and the slowest; the clocks are not touched):

  1. fused     redux_lag_cost_dev over the four lags 1, 2, 3, 4 at frame_step 1: k_lag_cost, no transformed copy.
  2. composed  the same four rows the way they could be had before: four redux_lag_planes_dev into a scratch buffer, each
               followed by redux_block_cost_dev (k_lag_planes + k_block_cost).  THE CRITERION: fused takes less time than
               composed at every E; a row that misses it says MISS.  The two results are compared block by block.
  3. sample    the first pass of api.choose_lag (256 lags on 64 frames) as one redux_lag_cost_dev call, and the whole of
               api.choose_lag (both passes, their sums and read-backs).  Reported, not gated.
  4. coder     the adaptive coder kernel of an encode call on the lag-3 transform of the same bytes (DeviceEncoder.encode_slots),
               the yardstick rows 1 to 3 are read against.

usage: python tools/lag_cost_table.py [--gib N] [--rounds R] [--out FILE]
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
from redux_amd import _lib, api  # noqa: E402
from tools.lag_table import B, CHANNELS, PARAMS, channels, measure  # noqa: E402

LAGS = (1, 2, 3, 4)


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
    say(f"# {a.gib} GiB = {nb} blocks of 64 KiB: {CHANNELS} interleaved walks of E-byte integers; one warm-up, then {a.rounds} rounds of "
        "every entry in turn; ms: median [fastest .. slowest]; the clocks were not touched")
    misses = []
    for E in (1, 2, 4, 8):
        src = channels(n, E)
        scratch = torch.empty_like(src)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        fused_bits = torch.empty((len(LAGS), nb), dtype=torch.float64, device="cuda:0")
        composed_bits = torch.empty((len(LAGS), nb), dtype=torch.float64, device="cuda:0")
        h_lags = np.asarray(LAGS, dtype=np.uint32)
        every = np.arange(1, api.LAG_MAX + 1, dtype=np.uint32)
        step = api.lag_frame_step(nb // E)
        sample_bits = torch.empty((api.LAG_MAX, L.redux_lag_cost_block_count(n, B, E, step)), dtype=torch.float64, device="cuda:0")

        def fused():
            api._raise(L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), n, B, E, h_lags.ctypes.data, len(LAGS), 1,
                                            C.c_void_p(fused_bits.data_ptr()), stream))

        def composed():
            for j, S in enumerate(LAGS):
                api.lag_planes(src, E, B, S, out=scratch)
                api._raise(L.redux_block_cost_dev(C.byref(cp), C.c_void_p(scratch.data_ptr()), n, B,
                                                  C.c_void_p(composed_bits[j].data_ptr()), stream))

        def sample():
            api._raise(L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), n, B, E, every.ctypes.data, len(every), step,
                                            C.c_void_p(sample_bits.data_ptr()), stream))

        chosen = []
        t = api.lag_planes(src, E, B, CHANNELS)  # what the coder sees
        enc = rx.DeviceEncoder(PARAMS, B, n)
        runs = {"fused, lags 1 2 3 4": fused, "composed, lags 1 2 3 4": composed, "first pass, 256 lags": sample,
                "choose_lag": lambda: chosen.append(api.choose_lag(src, E, B, PARAMS)), "coder forward": lambda: enc.encode_slots(t)}
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        diff = float((fused_bits - composed_bits).abs().max().item())
        picks = sorted({S for S, _ in chosen})
        ok = med["fused, lags 1 2 3 4"] < med["composed, lags 1 2 3 4"]
        if not ok:
            misses.append(E)
        for k, v in ms.items():
            tail = ""
            if k.startswith("fused"):
                tail = f"  {med[k] / med['composed, lags 1 2 3 4']:.2f} x composed  {'ok' if ok else 'MISS'}"
            elif k in ("first pass, 256 lags", "choose_lag"):
                tail = f"  {med[k] / med['coder forward']:.2f} x coder"
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]{tail}")
        say(f"E={E} fused against composed, {len(LAGS) * nb} blocks: max |difference| = {diff:g} bits; first pass: frame step {step}, "
            f"{sample_bits.shape[1] // E} frames; choose_lag picked {picks}")
        del enc, t, src, scratch, fused_bits, composed_bits, sample_bits
        torch.cuda.empty_cache()
    say("# the criterion (fused < composed at every E): "
        + ("met by every row" if not misses else "MISSED at " + ", ".join(f"E={E}" for E in misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
