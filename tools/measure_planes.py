#!/usr/bin/env python3
"""The byte-plane layout of typed data, measured in one GPU run (results: profiles/r05_planes.txt).

  1. k_planes alone: forward and inverse of 4 GiB at 64 KiB blocks for E = 2, 4, 8, as 2 * len / kernel time, next to a
     plain torch copy of the same 4 GiB (the yardstick, tools/copy_bw.py);
  2. the block coder at 65,536 x 64 KiB of seeded bf16 (N(0, 0.02)) and fp32 (N(0, 1)) data generated on the device, with
     and without the layout: encode and decode GB/s (input bytes / time of the whole stream-ordered call, layout
     included) and the compressed ratio; every decode is checked against the input.

usage: python tools/measure_planes.py [--mib N] [--out FILE]   (N: MiB of coder input, default 4096)
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redux_amd as rx  # noqa: E402

B = 65536
PARAMS = (8, 30, 32)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def data(kind, n):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261015)
    if kind == "bf16":
        t = (torch.randn(n // 2, device="cuda:0", generator=g) * 0.02).to(torch.bfloat16)
    else:
        t = torch.randn(n // 4, device="cuda:0", generator=g)
    return t.view(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
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
    ms = timed(lambda: dst.copy_(src), 10)
    say(f"torch copy_ 4 GiB: {ms:.3f} ms = {2 * n / ms / 1e9:.2f} TB/s (yardstick)")
    for E in (2, 4, 8):
        for inverse in (False, True):
            ms = timed(lambda: rx.planes(src, E, B, inverse=inverse, out=dst), 10)
            say(f"k_planes E={E} {'inverse' if inverse else 'forward'} 4 GiB, B=64 KiB: {ms:.3f} ms = {2 * n / ms / 1e9:.2f} TB/s")
        back = torch.empty_like(src)
        rx.planes(dst, E, B, inverse=True, out=back)
        rx.planes(src, E, B, out=dst)
        rx.planes(dst, E, B, inverse=True, out=back)
        torch.cuda.synchronize()
        assert torch.equal(back, src), f"E={E}: inverse of forward differs"
        del back
    del src, dst
    torch.cuda.empty_cache()

    n = a.mib << 20
    nb = n // B
    say(f"# coder: {nb} x 64 KiB = {n >> 20} MiB, params {PARAMS}; GB/s = input bytes / time of the whole call")
    for kind in ("bf16", "fp32"):
        x = data(kind, n)
        E_native = 2 if kind == "bf16" else 4
        for E in (1, E_native):
            enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E)
            ms_e = timed(lambda: enc.encode(x), 3)
            out, offs, status, summary = enc.encode(x)
            torch.cuda.synchronize()
            assert summary.tolist() == [0, 0]
            total = int(offs[-1])
            streams = out[:total].clone()
            offs = offs.clone()
            del enc
            torch.cuda.empty_cache()
            dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E)
            ms_d = timed(lambda: dec.decode(streams, offs, length=n), 3)
            d_out, _, _, dsum = dec.decode(streams, offs, length=n)
            torch.cuda.synchronize()
            assert dsum.tolist() == [0, 0] and torch.equal(d_out, x), f"{kind} E={E}: decode differs"
            say(f"{kind} element_size={E}: ratio {total / n:.4f}  encode {ms_e:.2f} ms = {n / ms_e / 1e6:.1f} GB/s  "
                f"decode {ms_d:.2f} ms = {n / ms_d / 1e6:.1f} GB/s")
            del dec, streams, offs, d_out
            torch.cuda.empty_cache()
        del x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
