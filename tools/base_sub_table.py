#!/usr/bin/env python3
"""The folded difference against a base, measured in one GPU run (results: profiles/base_sub_filter.txt).

  1. sizes: the seeded SYNTHETIC pairs of tools/base_table.py (pairs(), seed 20261018) at B = 65536 with 2^19 elements and
     at B = 4096 with 3 * 4096 + 100 elements, params (8, 30, 32): container bytes and stream bytes (summed over blocks) of
     the second snapshot coded against the first with the XOR (version 8) and with the folded difference (version 12).
     Every stream sum is checked against the CPU oracle on the numpy restatement of the transform (the streams are
     bit-exact, so the sums agree to the byte), every decode against the input, and what base_op="auto" picks is listed.
     No real checkpoint series is measured here.
  2. kernel times: 4 GiB of random bytes and a random base in HBM, B = 64 KiB, E = 1, 2, 4, 8: redux_base_sub_planes_dev
     forward and inverse next to redux_base_planes_dev forward and inverse and torch copy_, all taken in turn in every round
     after a warm-up, by device events: median [slowest .. fastest].  The yardstick is the XOR kernels in the same run (the
     same traffic: two reads and one write per byte); each folded-difference median is reported against XOR's own spread.
  3. the block coder end to end: section 6k's synthetic fp32 pair generated on the device (N(0, 0.02) weights, N(0, 2e-5)
     update), coded with both operations: ratio, encode and decode GB/s (input bytes / time of the whole stream-ordered
     call, transform included); every decode is checked against the input.

usage: python tools/base_sub_table.py [--gib N] [--mib N] [--rounds R] [--no-oracle] [--out FILE]
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
from redux_amd import container  # noqa: E402
from base_table import once, pairs, timed  # noqa: E402

PARAMS = (8, 30, 32)
OPS = ("xor", "sub")


def sizes(say, n_elements, B, oracle):
    say(f"# sizes: SYNTHETIC pairs, {n_elements} elements each, B = {B}, params {PARAMS}: container bytes and stream bytes of the "
        "second snapshot against the first"
        + ("" if not oracle else "; every stream sum equals the CPU oracle's on the restated transform")
        + ".  No real checkpoint series was measured.")
    say("pair | dtype / E | container XOR | container folded difference | ratio | streams XOR | streams folded difference | ratio | auto picks")
    if oracle:
        from oracle import cbind as ox
        from test_base_cpu import base_planes_ref
        from test_base_sub_cpu import base_sub_planes_ref
        refs = {"xor": base_planes_ref, "sub": base_sub_planes_ref}
    for name, dtype, E, y, x in pairs(n_elements):
        blob, streams = {}, {}
        for op in OPS:
            blob[op] = container.compress_bytes(x, B, PARAMS, element_size=E, base=y, base_op=op)
            assert container.decompress_bytes(blob[op], base=y) == x.tobytes(), (name, dtype, op)
            streams[op] = int(container._parse(blob[op]).offsets[-1])
            if oracle:
                want, st = ox.compress_blocks(refs[op](x, y, E, B), B, PARAMS)
                assert not st.any() and sum(len(s) for s in want) == streams[op], (name, dtype, op)
        auto = container.compress_bytes(x, B, PARAMS, element_size=E, base=y, base_op="auto")
        assert auto in blob.values()
        say(f"{name} | {dtype} / {E} | {len(blob['xor'])} | {len(blob['sub'])} | {len(blob['sub']) / len(blob['xor']):.3f} | "
            f"{streams['xor']} | {streams['sub']} | {streams['sub'] / streams['xor']:.3f} | {container.base_op(auto)}")


def kernels(say, gib, rounds):
    n = gib << 30
    B = 65536
    src = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    base = torch.empty(n, dtype=torch.uint8, device="cuda:0").random_(0, 256)
    dst = torch.empty_like(src)
    say(f"# kernels: {gib} GiB of random bytes and a random base in HBM, B = 64 KiB, {rounds} rounds of all five in turn after a "
        "warm-up, device events; ms: median [slowest .. fastest]; TB/s = bytes moved / median (copy_: 2 per input byte; the base "
        "kernels: 3)")
    for E in (1, 2, 4, 8):
        runs = {"torch copy_": (2, lambda: dst.copy_(src)),
                "xor forward": (3, lambda: rx.base_planes(src, base, E, B, out=dst)),
                "sub forward": (3, lambda: rx.base_sub_planes(src, base, E, B, out=dst)),
                "xor inverse": (3, lambda: rx.base_planes(src, base, E, B, inverse=True, out=dst)),
                "sub inverse": (3, lambda: rx.base_sub_planes(src, base, E, B, inverse=True, out=dst))}
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
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[-1]:.3f} .. {v[0]:.3f}] = {runs[k][0] * n / med[k] / 1e9:.2f} TB/s"
                f"  spread {(v[-1] - v[0]) / med[k] * 100:.1f} %")
        for way in ("forward", "inverse"):
            xs, m = ms["xor " + way], med["sub " + way]
            where = "inside" if xs[0] <= m <= xs[-1] else "%.1f %% %s" % (
                (xs[0] - m) / med["xor " + way] * 100 if m < xs[0] else (m - xs[-1]) / med["xor " + way] * 100,
                "below" if m < xs[0] else "above")
            say(f"E={E} sub / xor {way}: {m / med['xor ' + way]:.3f} x the time; the sub median lies {where} XOR's band "
                f"[{xs[0]:.3f} .. {xs[-1]:.3f}] ms")
        back = torch.empty_like(src)
        rx.base_sub_planes(src, base, E, B, out=dst)
        rx.base_sub_planes(dst, base, E, B, inverse=True, out=back)
        torch.cuda.synchronize()
        assert torch.equal(back, src), f"E={E}: inverse of forward differs"
        del back
    del src, base, dst
    torch.cuda.empty_cache()


def coder(say, mib):
    B = 65536
    n = mib << 20
    nb = n // B
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261018)
    w = torch.randn(n // 4, device="cuda:0", generator=g) * 0.02
    w2 = w + 2e-5 * torch.randn(n // 4, device="cuda:0", generator=g)
    y, x = w.view(torch.uint8), w2.view(torch.uint8)
    say(f"# coder: SYNTHETIC fp32 pair generated on the device (N(0, 0.02) weights, N(0, 2e-5) update), {nb} x 64 KiB = {n >> 20} MiB, "
        f"params {PARAMS}, element size 4; GB/s = input bytes / time of the whole call.  Host-pointer rates, a file on disk and "
        "real checkpoints were not measured.")
    for op in OPS:
        enc = rx.DeviceEncoder(PARAMS, B, n, element_size=4, base=y, base_op=op)
        ms_e = timed(lambda: enc.encode(x), 5)
        out, offs, status, summary = enc.encode(x)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0]
        total = int(offs[-1])
        streams = out[:total].clone()
        offs = offs.clone()
        del enc, out
        torch.cuda.empty_cache()
        dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=4, base=y, base_op=op)
        ms_d = timed(lambda: dec.decode(streams, offs, length=n), 5)
        d_out, _, _, dsum = dec.decode(streams, offs, length=n)
        torch.cuda.synchronize()
        assert dsum.tolist() == [0, 0] and torch.equal(d_out, x), "decode differs"
        say(f"base_op={op}: ratio {total / n:.4f}  encode {ms_e:.2f} ms = {n / ms_e / 1e6:.1f} GB/s  decode {ms_d:.2f} ms = "
            f"{n / ms_d / 1e6:.1f} GB/s  (medians of 5)")
        del dec, streams, offs, d_out
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        ap.error("--rounds: at least 7")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    sizes(say, 1 << 19, 65536, not a.no_oracle)
    sizes(say, 3 * 4096 + 100, 4096, not a.no_oracle)
    kernels(say, a.gib, a.rounds)
    coder(say, a.mib)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
