#!/usr/bin/env python3
"""The XOR-against-base filter, measured in one GPU run (results: profiles/base_filter.txt).

  1. sizes: seeded SYNTHETIC pairs of snapshots -- N(0, 0.02) weights w and w * (1 + r * N(0, 1)) for a relative update r of
     1e-2, 1e-3 and 1e-4, as fp32 and as bf16, plus an identical pair and an unrelated pair -- and for each the container
     bytes of the second snapshot coded plain, with --element-size, and with --element-size and --base.  No real checkpoint
     series is measured here.
  2. kernel times: 4 GiB, B = 64 KiB, E = 2 and 4: k_base_planes and k_base_unplanes next to k_planes, k_delta_planes and
     the two-step route the fused kernel replaces (torch.bitwise_xor into a scratch tensor, then redux_planes_dev), all taken
     in turn in every round, by device events after a warm-up of every shape: median [slowest .. fastest].  Bytes moved per
     input byte: k_planes 2, the fused kernels 3, the two-step route 5.
  3. the block coder end to end with the base: a synthetic fp32 pair generated on the device (update N(0, 2e-5)), encode and
     decode GB/s (input bytes / time of the whole stream-ordered call, transform included) and the ratio, byte planes alone
     against base + byte planes; every decode is checked against the input.

usage: python tools/base_table.py [--mib N] [--rounds R] [--out FILE]   (N: MiB of coder input in part 3, default 4096)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redux_amd as rx  # noqa: E402
from redux_amd import container  # noqa: E402

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


def as_bytes(w, dtype):
    """fp32 values -> the bytes of their fp32 or bf16 form"""
    if dtype == "fp32":
        return w.astype("<f4").view(np.uint8)
    return torch.from_numpy(w.astype(np.float32)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint8)


def pairs(n_elements, seed=20261018):
    """(name, dtype, E, base bytes, snapshot bytes) of every synthetic pair"""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
    out = []
    for dtype, E in (("fp32", 4), ("bf16", 2)):
        for r in (1e-2, 1e-3, 1e-4):
            w2 = (w * (1 + np.float32(r) * rng.standard_normal(n_elements).astype(np.float32))).astype(np.float32)
            out.append((f"relative update {r:g}", dtype, E, as_bytes(w, dtype), as_bytes(w2, dtype)))
        out.append(("identical pair", dtype, E, as_bytes(w, dtype), as_bytes(w, dtype)))
        other = (rng.standard_normal(n_elements) * 0.02).astype(np.float32)
        out.append(("unrelated pair", dtype, E, as_bytes(other, dtype), as_bytes(w, dtype)))
    return out


def sizes(say, n_elements):
    say(f"# sizes: SYNTHETIC pairs, {n_elements} elements each, N(0, 0.02) weights, seeded; B = 64 KiB, params {PARAMS}; container "
        "bytes of the second snapshot and their ratio to its size.  No real checkpoint series was measured.")
    say("# pair | dtype | input bytes | plain | --element-size E | --element-size E --base | base / element-size")
    for name, dtype, E, y, x in pairs(n_elements):
        plain = len(container.compress_bytes(x, B, PARAMS))
        planes = len(container.compress_bytes(x, B, PARAMS, element_size=E))
        blob = container.compress_bytes(x, B, PARAMS, element_size=E, base=y)
        assert container.decompress_bytes(blob, base=y) == x.tobytes(), (name, dtype)
        say(f"{name} | {dtype} | {len(x)} | {plain} ({plain / len(x):.4f}) | {planes} ({planes / len(x):.4f}) | "
            f"{len(blob)} ({len(blob) / len(x):.4f}) | {len(blob) / planes:.3f}")


def kernels(say, rounds):
    n = 4 << 30
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 255)
    base = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 255)
    dst = torch.empty_like(src)
    scratch = torch.empty_like(src)
    say(f"# kernels: 4 GiB, B = 64 KiB, {rounds} rounds of all seven in turn after a warm-up, device events; ms: median "
        "[fastest .. slowest]; GB/s = bytes moved / median (k_planes, k_delta_planes, copy_: 2 per input byte; k_base_*: 3; two-step: 5)")

    def two_step(E):
        torch.bitwise_xor(src, base, out=scratch)
        rx.planes(scratch, E, B, out=dst)

    for E in (2, 4):
        runs = {"torch copy_": (2, lambda: dst.copy_(src)),
                "k_planes forward": (2, lambda: rx.planes(src, E, B, out=dst)),
                "k_planes inverse": (2, lambda: rx.planes(src, E, B, inverse=True, out=dst)),
                "k_delta_planes (forward)": (2, lambda: rx.delta_planes(src, E, B, out=dst)),
                "k_base_planes (forward)": (3, lambda: rx.base_planes(src, base, E, B, out=dst)),
                "k_base_unplanes (inverse)": (3, lambda: rx.base_planes(src, base, E, B, inverse=True, out=dst)),
                "torch.bitwise_xor + k_planes (two steps)": (5, lambda: two_step(E))}
        for _, fn in runs.values():  # warm up every shape
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, (_, fn) in runs.items():
                ms[k].append(once(fn))
        med = {}
        for k, v in ms.items():
            v.sort()
            med[k] = v[len(v) // 2]
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {runs[k][0] * n / med[k] / 1e6:.0f} GB/s")
        say(f"E={E} k_base_planes / k_planes forward: {med['k_base_planes (forward)'] / med['k_planes forward']:.3f} x the time "
            f"(3 bytes against 2: 1.5 expected); k_base_unplanes / k_planes inverse: "
            f"{med['k_base_unplanes (inverse)'] / med['k_planes inverse']:.3f} x; two steps / k_base_planes: "
            f"{med['torch.bitwise_xor + k_planes (two steps)'] / med['k_base_planes (forward)']:.3f} x (5 bytes against 3: 1.67 expected)")
        # both routes give the same bytes, and the inverse gives the input back
        rx.base_planes(src, base, E, B, out=dst)
        two_step_out = torch.empty_like(dst)
        torch.bitwise_xor(src, base, out=scratch)
        rx.planes(scratch, E, B, out=two_step_out)
        rx.base_planes(dst, base, E, B, inverse=True, out=scratch)
        torch.cuda.synchronize()
        assert torch.equal(dst, two_step_out) and torch.equal(scratch, src), f"E={E}: the fused kernels and the two-step route differ"
        del two_step_out
    del src, base, dst, scratch
    torch.cuda.empty_cache()


def coder(say, mib):
    n = mib << 20
    nb = n // B
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261018)
    w = torch.randn(n // 4, device="cuda:0", generator=g) * 0.02
    w2 = w + 2e-5 * torch.randn(n // 4, device="cuda:0", generator=g)
    y, x = w.view(torch.uint8), w2.view(torch.uint8)
    say(f"# coder: SYNTHETIC fp32 pair generated on the device (N(0, 0.02) weights, N(0, 2e-5) update), {nb} x 64 KiB = {n >> 20} MiB, "
        f"params {PARAMS}, element size 4; GB/s = input bytes / time of the whole call")
    for base in (None, y):
        enc = rx.DeviceEncoder(PARAMS, B, n, element_size=4, base=base)
        ms_e = timed(lambda: enc.encode(x), 5)
        out, offs, status, summary = enc.encode(x)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0]
        total = int(offs[-1])
        streams = out[:total].clone()
        offs = offs.clone()
        del enc, out
        torch.cuda.empty_cache()
        dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=4, base=base)
        ms_d = timed(lambda: dec.decode(streams, offs, length=n), 5)
        d_out, _, _, dsum = dec.decode(streams, offs, length=n)
        torch.cuda.synchronize()
        assert dsum.tolist() == [0, 0] and torch.equal(d_out, x), "decode differs"
        say(f"{'base + byte planes' if base is not None else 'byte planes'}: ratio {total / n:.4f}  encode {ms_e:.2f} ms = "
            f"{n / ms_e / 1e6:.1f} GB/s  decode {ms_d:.2f} ms = {n / ms_d / 1e6:.1f} GB/s  (medians of 5)")
        del dec, streams, offs, d_out
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--elements", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    sizes(say, a.elements)
    kernels(say, a.rounds)
    coder(say, a.mib)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
