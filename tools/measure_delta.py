#!/usr/bin/env python3
"""The delta filter for integer series, measured in one GPU run (results: profiles/r11_delta.txt).

  1. the transform alone: forward and inverse of 4 GiB at 64 KiB blocks for E = 1, 2, 4, 8 -- k_delta_planes and
     k_delta_unplanes next to k_planes forward and inverse (E = 1: a device copy) and a plain torch copy of the same
     4 GiB, all five taken in turn in every round, so that each is compared with yardsticks of the same minutes.  Per
     kernel: median, fastest and slowest round as 2 * len / time; the spread of k_planes is what a difference has to beat.
  2. the block coder at 65,536 x 64 KiB of an int64 timestamp series generated on the device (increments uniform in
     [900, 1100)), byte planes against delta + byte planes: encode and decode GB/s (input bytes / time of the whole
     stream-ordered call, transform included) and the compressed ratio; every decode is checked against the input.

usage: python tools/measure_delta.py [--mib N] [--rounds R] [--out FILE]   (N: MiB of coder input, default 4096)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redux_amd as rx  # noqa: E402

B = 65536
PARAMS = (8, 30, 32)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    return sorted(once(fn) for _ in range(reps))[reps // 2]


def timestamps(n):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261017)
    inc = torch.randint(900, 1100, (n // 8,), device="cuda:0", generator=g, dtype=torch.int64)
    t = torch.cumsum(inc, 0)
    del inc
    t += 1_700_000_000_000_000
    return t.view(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    n = 4 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 255)
    dst = torch.empty_like(src)
    say(f"# transform: 4 GiB, B = 64 KiB, {a.rounds} rounds of all five in turn; TB/s = 2 * len / time: median [slowest .. fastest]")
    for E in (1, 2, 4, 8):
        runs = {"torch copy_": lambda: dst.copy_(src),
                "k_planes forward": lambda: rx.planes(src, E, B, out=dst),
                "k_delta_planes (forward)": lambda: rx.delta_planes(src, E, B, out=dst),
                "k_planes inverse": lambda: rx.planes(src, E, B, inverse=True, out=dst),
                "k_delta_unplanes (inverse)": lambda: rx.delta_planes(src, E, B, inverse=True, out=dst)}
        for fn in runs.values():  # warm up every shape
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                ms[k].append(once(fn))
        med = {}
        for k, v in ms.items():
            v.sort()
            med[k] = v[len(v) // 2]
            say(f"E={E} {k}: {med[k]:.3f} ms = {2 * n / med[k] / 1e9:.2f} TB/s [{2 * n / v[-1] / 1e9:.2f} .. {2 * n / v[0] / 1e9:.2f}]")
        say(f"E={E} forward / k_planes forward: {med['k_delta_planes (forward)'] / med['k_planes forward']:.3f} x the time; "
            f"inverse / k_planes inverse: {med['k_delta_unplanes (inverse)'] / med['k_planes inverse']:.3f} x; "
            f"inverse / torch copy_: {med['k_delta_unplanes (inverse)'] / med['torch copy_']:.3f} x")
        back = torch.empty_like(src)
        rx.delta_planes(src, E, B, out=dst)
        rx.delta_planes(dst, E, B, inverse=True, out=back)
        torch.cuda.synchronize()
        assert torch.equal(back, src), f"E={E}: inverse of forward differs"
        del back
    del src, dst
    torch.cuda.empty_cache()

    n = a.mib << 20
    nb = n // B
    say(f"# coder: int64 timestamps, {nb} x 64 KiB = {n >> 20} MiB, params {PARAMS}, element size 8; GB/s = input bytes / time of the whole call")
    x = timestamps(n)
    for filt in (None, "delta"):
        enc = rx.DeviceEncoder(PARAMS, B, n, element_size=8, filter=filt)
        ms_e = timed(lambda: enc.encode(x), 3)
        out, offs, status, summary = enc.encode(x)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0]
        total = int(offs[-1])
        streams = out[:total].clone()
        offs = offs.clone()
        del enc, out
        torch.cuda.empty_cache()
        dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=8, filter=filt)
        ms_d = timed(lambda: dec.decode(streams, offs, length=n), 3)
        d_out, _, _, dsum = dec.decode(streams, offs, length=n)
        torch.cuda.synchronize()
        assert dsum.tolist() == [0, 0] and torch.equal(d_out, x), f"filter={filt}: decode differs"
        say(f"{'delta + byte planes' if filt else 'byte planes'}: ratio {total / n:.4f}  encode {ms_e:.2f} ms = {n / ms_e / 1e6:.1f} GB/s  "
            f"decode {ms_d:.2f} ms = {n / ms_d / 1e6:.1f} GB/s")
        del dec, streams, offs, d_out
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
