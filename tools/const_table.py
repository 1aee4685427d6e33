#!/usr/bin/env python3
"""Constant blocks, measured in one GPU run (results: profiles/const_blocks.txt).

SYNTHETIC pairs of snapshots generated on the device, bf16 (E = 2, relative update 1e-3) and fp32 (E = 4, update
N(0, 2e-5)), N(0, 0.02) weights, B = 64 KiB, params (8, 30, 32).  A seeded choice of 0 %, 50 %, 90 %, 99 % and 100 % of the
frames of the second snapshot is left equal to the first; the rest is updated.  No real checkpoint series is measured.

For every share, in one run on the same buffers:
  1. k_const_select over the coder input x' (the byte-plane layout of snapshot ^ base), next to k_byte_hist
     (redux_histogram_dev) and a device-to-device copy of the same bytes, all three in turn in every round, device events
     after a warm-up: median [fastest .. slowest];
  2. DeviceEncoder / DeviceDecoder with base= alone and with base= and constant=True: ms and GB/s (input bytes / time of
     the whole stream-ordered call, layout and detection included), medians of 5; every decode is checked against the input;
  3. the container bytes both would make: header + base record + size table + (bitmap) + payloads, computed from the device
     calls' offsets (a 4 GiB container is not assembled on the host).
The one ordering asserted: at 100 % unchanged the calls with the option are faster than the calls without it.

The inputs are 4 GiB less 1 MiB: the `_dev` encode call with the option takes less than 4 GiB (the table form of the
encoder addresses x' with 32-bit lane offsets), so 4095 MiB is the largest whole number of MiB, and of frames, it codes in
one call.

usage: python tools/const_table.py [--mib N] [--rounds R] [--out FILE]   (N < 4096)
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redux_amd as rx  # noqa: E402

B = 65536
PARAMS = (8, 30, 32)
SHARES = (0, 50, 90, 99, 100)


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    return sorted(once(fn) for _ in range(reps))[reps // 2]


def snapshots(dtype, n, g):
    """(base bytes, fully updated snapshot bytes), n bytes each"""
    if dtype == "fp32":
        w = torch.randn(n // 4, device="cuda:0", generator=g) * 0.02
        w2 = w + 2e-5 * torch.randn(n // 4, device="cuda:0", generator=g)
        return w.view(torch.uint8), w2.view(torch.uint8)
    w = torch.randn(n // 2, device="cuda:0", generator=g) * 0.02
    w2 = (w * (1 + 1e-3 * torch.randn(n // 2, device="cuda:0", generator=g))).to(torch.bfloat16)
    return w.to(torch.bfloat16).view(torch.uint8), w2.view(torch.uint8)


def histogram(d, counts):
    rx._lib.lib().redux_histogram_dev(C.c_void_p(d.data_ptr()), d.numel(), C.c_void_p(counts.data_ptr()), None, 0,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))


def measure(say, dtype, E, n, rounds):
    nb = n // B
    F = E * B
    nframes = n // F
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261018)
    y, full = snapshots(dtype, n, g)
    order = torch.randperm(nframes, device="cuda:0", generator=g)
    xp = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    scratch = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    head = 32 + 12 + 4 * nb
    say(f"# {dtype}: E = {E}, {nb} x 64 KiB = {n >> 20} MiB, {nframes} frames; update: "
        f"{'N(0, 2e-5) absolute' if dtype == 'fp32' else '1e-3 relative'}")
    for share in SHARES:
        keep = torch.zeros(nframes, dtype=torch.bool, device="cuda:0")
        keep[order[: nframes * share // 100]] = True
        x = torch.where(keep[:, None], y.view(nframes, F), full.view(nframes, F)).view(-1)
        rx.base_planes(x, y, E, B, out=xp)
        flags = rx.constant_blocks(xp, B)
        nconst = int(flags.sum())
        # 1. the detection next to the histogram and a copy, over the same x'
        runs = {"k_const_select": lambda: rx.constant_blocks(xp, B), "k_byte_hist": lambda: histogram(xp, counts),
                "d2d copy": lambda: scratch.copy_(xp)}
        for fn in runs.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(once(fn))
        txt = []
        for k, v in ms.items():
            v.sort()
            txt.append(f"{k} {v[len(v) // 2]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]")
        say(f"{dtype} {share:3d} % unchanged frames: {nconst} of {nb} blocks constant | " + " | ".join(txt))
        # 2. and 3. the coder with and without the option
        res = {}
        for const in (False, True):
            enc = rx.DeviceEncoder(PARAMS, B, n, element_size=E, base=y, constant=const)
            ms_e = timed(lambda: enc.encode(x))
            r = enc.encode(x)
            torch.cuda.synchronize()
            assert r[3].tolist() == [0, 0]
            total = int(r[1][-1])
            streams, offs = r[0][:total].clone(), r[1].clone()
            cflags = r[4].clone() if const else None
            del enc, r
            torch.cuda.empty_cache()
            dec = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, base=y, constant=const)
            kw = {"constant": cflags} if const else {}
            ms_d = timed(lambda: dec.decode(streams, offs, length=n, **kw))
            d_out, _, _, dsum = dec.decode(streams, offs, length=n, **kw)
            torch.cuda.synchronize()
            assert dsum.tolist() == [0, 0] and torch.equal(d_out, x), "decode differs"
            if const:
                assert torch.equal(cflags, flags)
            size = head + total + ((nb + 7) // 8 if const else 0)
            res[const] = (ms_e, ms_d, size)
            say(f"{dtype} {share:3d} %   {'--base --skip-constant' if const else '--base               '}: container {size} bytes "
                f"({size / n:.5f})  encode {ms_e:.2f} ms = {n / ms_e / 1e6:.1f} GB/s  decode {ms_d:.2f} ms = {n / ms_d / 1e6:.1f} GB/s")
            del dec, streams, offs, d_out
            torch.cuda.empty_cache()
        say(f"{dtype} {share:3d} %   with / without: size {res[True][2] / res[False][2]:.4f}  encode time {res[True][0] / res[False][0]:.3f}  "
            f"decode time {res[True][1] / res[False][1]:.3f}")
        if share == 100:
            assert res[True][0] < res[False][0] and res[True][1] < res[False][1], "100 % unchanged: the option is not faster"
        del x
    del y, full, xp, scratch
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4095)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        ap.error("--rounds: at least 5")
    if not 0 < a.mib < 4096:
        ap.error("--mib: below 4096 (redux_encode_const_dev takes less than 4 GiB)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"# SYNTHETIC pairs generated on the device, seeded; B = 64 KiB, params {PARAMS}; a seeded choice of the frames is left "
        "unchanged.  No real checkpoint series was measured.  Kernel times: device events, median [fastest .. slowest] of "
        f"{a.rounds} rounds of all three in turn; coder: medians of 5, GB/s = input bytes / time of the whole call; container "
        "bytes computed from the calls' offsets (header 32 + base record 12 + 4 per block + bitmap + payloads).")
    try:
        for dtype, E in (("bf16", 2), ("fp32", 4)):
            measure(say, dtype, E, a.mib << 20, a.rounds)
    finally:  # (what was measured is kept when the ordering check at 100 % fails)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
