#!/usr/bin/env python3
"""The snapshot-stride filter, measured in one GPU run (results: profiles/stride_filter.txt).

  1. sizes: the GENERATED series of tests/test_stride_cpu.py (series(), seed 29) at B = 4096, params (8, 30, 32): stream bytes
     of filter="stride" from the GPU next to the CPU oracle's on the numpy restatement (bit-exact, so the sums agree to the
     byte) and next to the best of plain, planes, zigzag and lag 3 on the oracle; every decode is checked against the input.
     No recorded series is measured here.
  2. kernel times, section 6s's protocol: 4 GiB of random bytes in HBM as 65,536 blocks of 64 KiB; device events; one
     warm-up, then 7 rounds of ALL entries in turn; median [slowest .. fastest].  Clocks are not touched.  Entries:
     redux_stride_planes_dev forward, and inverse (the layout's inverse and the running sums together), for E = 1, 2, 4, 8
     at S*E = 4 KiB, 360,000 B, 1 MiB + E, 64 MiB, 1 GiB and at S = 1 (the segmented sums).  In the same run: torch copy_,
     k_base_planes<E, BaseSubFold<E>> (redux_base_sub_planes_dev forward against a second buffer), and the yardsticks: the
     adaptive encoder's coder kernel without compaction (DeviceEncoder.encode_slots) and the plain decode call
     (DeviceDecoder.decode) on the same bytes.  The standing condition: every entry takes less time than the coder kernel of
     its direction; a row that does not is printed as MISSED.

usage: python tools/stride_table.py [--gib N] [--rounds R] [--no-sizes] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import redux_amd as rx  # noqa: E402
from base_table import once  # noqa: E402

PARAMS = (8, 30, 32)


def sizes(say):
    from oracle import cbind as ox
    from test_stride_cpu import best_existing, series, stride_planes_ref
    B = 4096
    say(f"# sizes: GENERATED series (default_rng(29)), B = {B}, params {PARAMS}: stream bytes behind filter=\"stride\" from the GPU "
        "(equal to the CPU oracle's on the restated transform) against the best of plain, planes, zigzag and lag 3 on the oracle.  "
        "No recorded series was measured.")
    say("series | E | S | stride | best existing | ratio")
    for name, (data, E, S) in series().items():
        x = np.frombuffer(data, dtype=np.uint8)
        out, offs, _ = rx.compress_blocks(x, B, PARAMS, element_size=E, filter="stride", stride=S)
        want, _ = ox.compress_blocks(stride_planes_ref(x, E, S, B).tobytes(), B, PARAMS)
        assert int(offs[-1]) == sum(len(s) for s in want), name
        back, _, st = rx.decompress_blocks(out, offs, B, PARAMS, element_size=E, length=len(x), filter="stride", stride=S)
        assert not st.any() and np.array_equal(back, x), name
        best = best_existing(data, E, B)
        say(f"{name} | {E} | {S} | {int(offs[-1])} | {best} | {int(offs[-1]) / best:.3f}")


def kernels(say, gib, rounds):
    n, B = gib << 30, 65536
    nb = n // B
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    other = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    dst = torch.empty_like(src)
    enc = rx.DeviceEncoder(PARAMS, B, n)
    out, offs, _, summary = enc.encode(src)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    streams, offs = out[: int(offs[-1])].clone(), offs.clone()
    dec = rx.DeviceDecoder(PARAMS, B, nb)
    runs = {"torch copy_": lambda: dst.copy_(src),
            "encode coder kernel (no compaction)": lambda: enc.encode_slots(src),
            "plain decode call": lambda: dec.decode(streams, offs)}
    strides = {}
    for E in (1, 2, 4, 8):
        runs[f"E={E} base_sub forward"] = lambda E=E: rx.base_sub_planes(src, other, E, B, out=dst)
        for label, nbytes in (("4 KiB", 4096), ("360,000 B", 360000), ("1 MiB + E", (1 << 20) + E), ("64 MiB", 64 << 20),
                              ("1 GiB", 1 << 30), ("S = 1", E)):
            S = nbytes // E
            if S * E >= n:
                continue
            strides[(E, label)] = S
            runs[f"E={E} S*E={label} forward"] = lambda E=E, S=S: rx.stride_planes(src, E, B, S, out=dst)
            runs[f"E={E} S*E={label} inverse"] = lambda E=E, S=S: rx.stride_planes(src, E, B, S, inverse=True, out=dst)
    say(f"# kernels: {gib} GiB of random bytes in HBM as {nb} blocks of 64 KiB, one warm-up then {rounds} rounds of all {len(runs)} "
        "entries in turn, device events, clocks untouched; ms: median [slowest .. fastest]; GB/s = input bytes / median")
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ms[k].append(once(fn))
    med = {}
    for k, v in ms.items():
        v.sort()
        med[k] = v[len(v) // 2]
    yard = {"forward": med["encode coder kernel (no compaction)"], "inverse": med["plain decode call"]}
    missed = 0
    for k, v in ms.items():
        way = k.rsplit(" ", 1)[-1]
        verdict = ""
        if "S*E=" in k:
            E, label = int(k[2]), k.split("S*E=")[1].rsplit(" ", 1)[0]
            name = rx.stride_kernel_name(n, B, E, strides[(E, label)], way == "inverse", src, dst)
            ok = med[k] < yard[way]
            missed += not ok
            verdict = f"  {med[k] / yard[way]:.3f} x the {way} coder  {'ok' if ok else 'MISSED'}  [{name}]"
        say(f"{k}: {med[k]:.3f} ms [{v[-1]:.3f} .. {v[0]:.3f}] = {n / med[k] / 1e6:.1f} GB/s  spread {(v[-1] - v[0]) / med[k] * 100:.1f} %{verdict}")
    say(f"# rows above their direction's coder kernel: {missed}")
    for (E, label), S in strides.items():  # the inverse of the forward is the input, at every shape timed
        back = torch.empty_like(src)
        rx.stride_planes(src, E, B, S, out=dst)
        rx.stride_planes(dst, E, B, S, inverse=True, out=back)
        torch.cuda.synchronize()
        assert torch.equal(back, src), f"E={E} S*E={label}: inverse of forward differs"
        del back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-sizes", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    if not a.no_sizes:
        sizes(say)
    kernels(say, a.gib, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
