#!/usr/bin/env python3
"""The zigzag-folded delta filter, measured in one GPU run (results: profiles/zigzag_filter.txt).

  1. sizes: the stream bytes (summed over blocks) of compress_blocks behind the byte planes, the delta filter and the
     folded delta filter, params (8, 30, 32), for generated series at E = 2, 4, 8: a random walk with steps N(0, 50), a sine
     of amplitude 2000 with noise N(0, 20), timestamps (the running sum of uniform 990 .. 1009), each three full frames
     plus 100 elements at B = 4096 and B = 65536, and an int64 timestamp file of 2 MiB at B = 65536.  Every size is
     checked against the CPU oracle on the numpy restatement of the transform (the streams are bit-exact, so the sizes
     agree to the byte), and every decode against the input.
  2. the transform alone: forward and inverse of 4 GiB at 64 KiB blocks for E = 1, 2, 4, 8, redux_zigzag_planes_dev next
     to redux_delta_planes_dev, taken in turn in every round, so that both see the same minutes.  Per kernel: median,
     slowest and fastest round as 2 * len / time; the spread of delta's own rounds is what a difference has to beat.

usage: python tools/zigzag_table.py [--gib N] [--rounds R] [--no-oracle] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import redux_amd as rx  # noqa: E402

PARAMS = (8, 30, 32)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def series(B):
    """{name: {E: bytes}}: three full frames of B elements plus 100, from np.random.default_rng(1)"""
    n = 3 * B + 100
    rng = np.random.default_rng(1)
    walk = np.cumsum(np.round(rng.normal(0, 50, n))).astype(np.int64)
    sine = np.round(2000 * np.sin(2 * np.pi * np.arange(n) / 500.0) + rng.normal(0, 20, n)).astype(np.int64)
    stamps = np.cumsum(rng.integers(990, 1010, n)).astype(np.int64)
    return {"random walk N(0, 50)": {E: walk.astype("<i%d" % E).view(np.uint8) for E in (2, 4, 8)},
            "sine 2000 + noise N(0, 20)": {E: sine.astype("<i%d" % E).view(np.uint8) for E in (2, 4, 8)},
            "timestamps 990..1009": {E: stamps.astype("<u%d" % E).view(np.uint8) for E in (2, 4, 8)}}


def sizes(x, E, B, oracle):
    """stream bytes behind the byte planes, the delta filter and the folded one; checked against the oracle and decoded"""
    got = []
    for f in (None, "delta", "zigzag"):
        out, offs, st = rx.compress_blocks(x, B, PARAMS, element_size=E, filter=f)
        assert not st.any()
        back, _, st = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=len(x), filter=f)
        assert not st.any() and np.array_equal(back, x), (E, B, f)
        got.append(int(offs[-1]))
    if oracle:
        from oracle import cbind as ox
        from test_delta_cpu import delta_planes_ref
        from test_planes_cpu import planes_ref
        from test_zigzag_cpu import zigzag_planes_ref
        for g, t in zip(got, (planes_ref, delta_planes_ref, zigzag_planes_ref)):
            streams, st = ox.compress_blocks(t(x, E, B), B, PARAMS)
            assert not st.any() and sum(len(s) for s in streams) == g, (E, B, t.__name__)
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"# sizes: stream bytes summed over blocks, params {PARAMS}; three full frames + 100 elements"
        + ("" if a.no_oracle else "; every size equals the CPU oracle's on the restated transform"))
    say("series | E | B | plain planes | delta | zigzag | zigzag / delta")
    for B in (4096, 65536):
        for name, by_e in series(B).items():
            for E, x in by_e.items():
                p, d, z = sizes(x, E, B, not a.no_oracle)
                say(f"{name} | {E} | {B} | {p} | {d} | {z} | {z / d:.3f}")
    rng = np.random.default_rng(11)
    x = (1_700_000_000_000_000 + np.cumsum(rng.integers(900, 1100, 262144))).astype("<u8").view(np.uint8)
    p, d, z = sizes(x, 8, 65536, not a.no_oracle)
    say(f"int64 timestamp file, 2 MiB | 8 | 65536 | {p} | {d} | {z} | {z / d:.3f}")

    n = a.gib << 30
    B = 65536
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    dst = torch.empty_like(src)
    say(f"# transform: {a.gib} GiB of random bytes in HBM, B = 64 KiB, {a.rounds} rounds of all four in turn; "
        "TB/s = 2 * len / time: median [slowest .. fastest]")
    for E in (1, 2, 4, 8):
        runs = {"delta forward": lambda: rx.delta_planes(src, E, B, out=dst),
                "zigzag forward": lambda: rx.zigzag_planes(src, E, B, out=dst),
                "delta inverse": lambda: rx.delta_planes(src, E, B, inverse=True, out=dst),
                "zigzag inverse": lambda: rx.zigzag_planes(src, E, B, inverse=True, out=dst)}
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
            say(f"E={E} {k}: {med[k]:.3f} ms = {2 * n / med[k] / 1e9:.2f} TB/s [{2 * n / v[-1] / 1e9:.2f} .. {2 * n / v[0] / 1e9:.2f}]"
                f"  spread {(v[-1] - v[0]) / med[k] * 100:.1f} %")
        say(f"E={E} zigzag / delta: forward {med['zigzag forward'] / med['delta forward']:.3f} x the time, "
            f"inverse {med['zigzag inverse'] / med['delta inverse']:.3f} x")
        back = torch.empty_like(src)
        rx.zigzag_planes(src, E, B, out=dst)
        rx.zigzag_planes(dst, E, B, inverse=True, out=back)
        torch.cuda.synchronize()
        assert torch.equal(back, src), f"E={E}: inverse of forward differs"
        del back
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
