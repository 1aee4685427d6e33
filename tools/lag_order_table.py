#!/usr/bin/env python3
"""Higher-order lagged differences, measured in one GPU run (results: profiles/lag_order_filter.txt).

  1. the transform alone: forward and inverse of `--gib` GiB (default 4) at 64 KiB blocks for E = 1, 2, 4, 8, the lags 1, 3, 16,
     256 and the orders 2 and 3, redux_lag_order_planes_dev (k_lag_order_planes / k_lag_order_unplanes) next to
     redux_lag_planes_dev (k_lag_planes / k_lag_unplanes) at the same E and S, and next to the adaptive coder of that direction
     on the same bytes: the encoder's coder kernel (DeviceEncoder.encode_slots: phase 1, no compaction) and the plain decode
     call (redux_decode_blocks_dev: the decoder kernel and its summary).  The input is two interleaved channels of GENERATED
     tones (three sinusoids and white noise of standard deviation 4 per channel, the `tones` generator of
     tests/test_lag_order_cpu.py on the device; 256 MiB of it repeated; at E = 1 the values wrap, which the timings do not
     mind); the coders run on its lag-2 order-2 transform.  All entries are taken in turn in every round, so that they see the
     same minutes.  Per entry: the median over the rounds, the fastest and the slowest.  THE CONDITION (the lag filter's):
     every transform takes no longer than the coder of its direction; a row that misses it says MISS.
  2. container bytes of that input behind the lag filter at lag 2 and orders 1, 2 and 3: the streams of the device encoder
     summed plus container.overhead_bytes, each decoded again and compared.

usage: python tools/lag_order_table.py [--gib N] [--rounds R] [--out FILE]
"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import api, container  # noqa: E402

PARAMS = (8, 30, 32)
LAGS = (1, 3, 16, 256)
ORDERS = (2, 3)
B = 65536
CHANNELS = 2


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def tones(n, E):
    """n bytes: CHANNELS interleaved channels of E-byte integers, each 6000, 2500 and 900 times a sinusoid of 0.003 (c + 1),
    0.011 and 0.031 cycles a sample plus N(0, 4) noise; a piece of 256 MiB, repeated"""
    piece = min(n, 256 << 20)
    m = piece // (E * CHANNELS) + 1
    g = torch.Generator(device="cuda:0").manual_seed(7 + E)
    t = torch.arange(m, device="cuda:0", dtype=torch.float64)
    cols = []
    for c in range(CHANNELS):
        ph = torch.rand(3, device="cuda:0", generator=g, dtype=torch.float64) * 6.28
        s = sum(a * torch.sin(2 * math.pi * f * t + ph[k]) for k, (a, f) in enumerate(((6000, 0.003 * (c + 1)), (2500, 0.011), (900, 0.031))))
        cols.append(torch.round(s + torch.randn(m, device="cuda:0", generator=g, dtype=torch.float64) * 4).to(torch.int64))
    dt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[E]
    p = torch.stack(cols, 1).reshape(-1).to(dt).view(torch.uint8)[:piece]
    return p.repeat((n + piece - 1) // piece)[:n].contiguous()


def measure(runs, rounds):
    """{name: sorted ms over the rounds}, every entry warmed up and then taken in turn in every round"""
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            ms[k].append(once(fn))
    return {k: sorted(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.gib << 30
    nb = n // B
    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"# {a.gib} GiB = {nb} blocks of 64 KiB: {CHANNELS} interleaved channels of generated tones in E-byte integers; {a.rounds} rounds of "
        "every entry in turn after one warm-up; ms: median [fastest .. slowest]; the clocks were not touched")
    misses = []
    for E in (1, 2, 4, 8):
        src = tones(n, E)
        dst = torch.empty_like(src)
        t = api.lag_order_planes(src, E, B, CHANNELS, 2)  # what the coders see
        enc = rx.DeviceEncoder(PARAMS, B, n)
        out, offs, _, summary = enc.encode(t)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0]
        total = int(offs[-1])
        streams, d_offs = out[:total].clone(), offs.clone()
        dec = rx.DeviceDecoder(PARAMS, B, nb)
        runs = {"coder forward": lambda: enc.encode_slots(t), "coder inverse": lambda: dec.decode(streams, d_offs)}
        for S in LAGS:
            runs[f"lag {S} forward"] = lambda S=S: api.lag_planes(src, E, B, S, out=dst)
            runs[f"lag {S} inverse"] = lambda S=S: api.lag_planes(t, E, B, S, inverse=True, out=dst)
            for K in ORDERS:
                runs[f"lag {S} order {K} forward"] = lambda S=S, K=K: api.lag_order_planes(src, E, B, S, K, out=dst)
                runs[f"lag {S} order {K} inverse"] = lambda S=S, K=K: api.lag_order_planes(t, E, B, S, K, inverse=True, out=dst)
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        for k in ("coder forward", "coder inverse"):
            v = ms[k]
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]")
        for S in LAGS:
            for d in ("forward", "inverse"):
                k, v = f"lag {S} {d}", ms[f"lag {S} {d}"]
                say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]  {med[k] / med['coder ' + d]:.2f} x coder")
                for K in ORDERS:
                    k, v = f"lag {S} order {K} {d}", ms[f"lag {S} order {K} {d}"]
                    ok = med[k] <= med[f"coder {d}"]
                    if not ok:
                        misses.append((E, S, K, d))
                    say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {2 * n / med[k] / 1e9:.2f} TB/s  "
                        f"{med[k] / med[f'lag {S} {d}']:.2f} x lag  {med[k] / med['coder ' + d]:.2f} x coder  {'ok' if ok else 'MISS'}")
        for S in LAGS:  # inverse of forward, at the size timed; order 1 against the lag kernels
            for K in (1,) + ORDERS:
                back = torch.empty_like(src)
                api.lag_order_planes(src, E, B, S, K, out=dst)
                if K == 1:
                    api.lag_planes(src, E, B, S, out=back)
                    torch.cuda.synchronize()
                    assert torch.equal(back, dst), f"E={E} S={S}: order 1 is not the lag filter"
                api.lag_order_planes(dst, E, B, S, K, inverse=True, out=back)
                torch.cuda.synchronize()
                assert torch.equal(back, src), f"E={E} S={S} K={K}: inverse of forward differs"
                del back
        del enc, dec, out, offs, streams, d_offs, t, dst
        torch.cuda.empty_cache()
        # the container bytes
        sizes = {}
        for K in (1, 2, 3):
            kw = {"element_size": E, "filter": "lag", "lag": CHANNELS, "order": K}
            e = rx.DeviceEncoder(PARAMS, B, n, **kw)
            o, f, _, s = e.encode(src)
            torch.cuda.synchronize()
            assert s.tolist() == [0, 0]
            sizes[K] = int(f[-1]) + container.overhead_bytes("adaptive", nb, E, filter="lag")
            d = rx.DeviceDecoder(PARAMS, B, nb, **kw)
            got = d.decode(o[: int(f[-1])], f, length=n)
            torch.cuda.synchronize()
            assert got[3].tolist() == [0, 0] and torch.equal(got[0], src), f"E={E} K={K}: the round trip differs"
            del e, d, o, f, got
            torch.cuda.empty_cache()
        say(f"E={E} container bytes of {n} at lag {CHANNELS}: order 1 {sizes[1]}, order 2 {sizes[2]} ({sizes[2] / sizes[1]:.3f}), "
            f"order 3 {sizes[3]} ({sizes[3] / sizes[1]:.3f})")
        del src
        torch.cuda.empty_cache()
    say("# the condition (transform <= coder of its direction): "
        + ("met by every row" if not misses else "MISSED by " + ", ".join(f"E={E} S={S} K={K} {d}" for E, S, K, d in misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
