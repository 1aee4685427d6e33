#!/usr/bin/env python3
"""The lagged delta filter, measured in one GPU run (results: profiles/lag_filter.txt).

  1. the transform alone: forward and inverse of `--gib` GiB (default 4) at 64 KiB blocks for E = 1, 2, 4, 8 and the lags
     1, 2, 3, 4, 6, 8, 16, 64, 256, redux_lag_planes_dev next to redux_zigzag_planes_dev (k_delta_planes<E, true> /
     k_delta_unplanes<E, true>) and next to the adaptive coder of that direction on the same bytes: the encoder's coder
     kernel (DeviceEncoder.encode_slots: phase 1, no compaction) and the plain decode call (redux_decode_blocks_dev: the decoder
     kernel and its summary).  The input is three interleaved random walks of E-byte integers (steps N(0, 50), levels 5000
     apart: the `channels` generator of tests/test_lag_cpu.py, 256 MiB of it repeated); the coders run on its lag-3 transform.
     All of them are taken in turn in every round, so that they see the same minutes.  Per entry: the median over the rounds,
     the slowest and the fastest.  THE CONDITION: every lag transform takes no longer than the coder of its direction; a row
     that misses it says MISS.
  2. the whole calls: redux_encode_lag_dev / redux_decode_lag_dev (DeviceEncoder / DeviceDecoder) at lag 1 and 3 next to their
     zigzag namesakes, the same way.
  3. container bytes of that input: the streams summed plus container.overhead_bytes, behind the planes alone, the zigzag
     filter and the lag filter with lag 3.

usage: python tools/lag_table.py [--gib N] [--rounds R] [--out FILE]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import api, container  # noqa: E402

PARAMS = (8, 30, 32)
LAGS = (1, 2, 3, 4, 6, 8, 16, 64, 256)
B = 65536
CHANNELS = 3


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def channels(n, E):
    """n bytes: CHANNELS interleaved int walks of E bytes, steps N(0, 50), levels 5000 apart; a piece of 256 MiB, repeated"""
    piece = min(n, 256 << 20)
    m = piece // (E * CHANNELS) + 1
    g = torch.Generator(device="cuda:0").manual_seed(100 + 10 * CHANNELS + E)
    w = torch.cumsum(torch.round(torch.randn(m, CHANNELS, device="cuda:0", generator=g) * 50).to(torch.int64), 0)
    w += torch.tensor([5000 * c * (-1) ** c for c in range(CHANNELS)], device="cuda:0")
    dt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[E]
    p = w.reshape(-1).to(dt).view(torch.uint8)[:piece]
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
    say(f"# {a.gib} GiB = {nb} blocks of 64 KiB: {CHANNELS} interleaved walks of E-byte integers; {a.rounds} rounds of every entry in turn; "
        "ms: median [fastest .. slowest]; the clocks were not touched")
    misses = []
    for E in (1, 2, 4, 8):
        src = channels(n, E)
        dst = torch.empty_like(src)
        t = api.lag_planes(src, E, B, CHANNELS)  # what the coders see
        enc = rx.DeviceEncoder(PARAMS, B, n)
        out, offs, _, summary = enc.encode(t)
        torch.cuda.synchronize()
        assert summary.tolist() == [0, 0]
        total = int(offs[-1])
        streams, d_offs = out[:total].clone(), offs.clone()
        dec = rx.DeviceDecoder(PARAMS, B, nb)
        runs = {"coder forward": lambda: enc.encode_slots(t), "coder inverse": lambda: dec.decode(streams, d_offs),
                "zigzag forward": lambda: rx.zigzag_planes(src, E, B, out=dst),
                "zigzag inverse": lambda: rx.zigzag_planes(t, E, B, inverse=True, out=dst)}
        for S in LAGS:
            runs[f"lag {S} forward"] = lambda S=S: api.lag_planes(src, E, B, S, out=dst)
            runs[f"lag {S} inverse"] = lambda S=S: api.lag_planes(t, E, B, S, inverse=True, out=dst)
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        for k in ("coder forward", "coder inverse", "zigzag forward", "zigzag inverse"):
            v = ms[k]
            say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]")
        for S in LAGS:
            for d in ("forward", "inverse"):
                k, v = f"lag {S} {d}", ms[f"lag {S} {d}"]
                ok = med[k] <= med[f"coder {d}"]
                if not ok:
                    misses.append((E, S, d))
                say(f"E={E} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {2 * n / med[k] / 1e9:.2f} TB/s  "
                    f"{med[k] / med['zigzag ' + d]:.2f} x zigzag  {med[k] / med['coder ' + d]:.2f} x coder  {'ok' if ok else 'MISS'}")
        for S in (1, 3, 64):  # inverse of forward, at the size timed
            back = torch.empty_like(src)
            api.lag_planes(src, E, B, S, out=dst)
            api.lag_planes(dst, E, B, S, inverse=True, out=back)
            torch.cuda.synchronize()
            assert torch.equal(back, src), f"E={E} S={S}: inverse of forward differs"
            del back
        del enc, dec, out, offs, streams, d_offs
        # the whole calls, and the container bytes
        sizes, calls = {}, {}
        coders = {}
        for name, kw in (("planes", {}), ("zigzag", {"filter": "zigzag"}), ("lag 1", {"filter": "lag", "lag": 1}),
                         ("lag 3", {"filter": "lag", "lag": 3})):
            e = rx.DeviceEncoder(PARAMS, B, n, element_size=E, **kw)
            o, f, _, s = e.encode(src)
            torch.cuda.synchronize()
            assert s.tolist() == [0, 0]
            sizes[name] = int(f[-1]) + container.overhead_bytes("adaptive", nb, E, filter=kw.get("filter"))
            if name == "planes":
                del e, o, f
                continue
            st, fo = o[: int(f[-1])].clone(), f.clone()
            d = rx.DeviceDecoder(PARAMS, B, nb, element_size=E, **kw)
            coders[name] = (e, d, st, fo)
            calls[f"encode {name}"] = lambda e=e: e.encode(src)
            calls[f"decode {name}"] = lambda d=d, st=st, fo=fo: d.decode(st, fo, length=n)
        got = coders["lag 3"][1].decode(coders["lag 3"][2], coders["lag 3"][3], length=n)
        torch.cuda.synchronize()
        assert got[3].tolist() == [0, 0] and torch.equal(got[0], src), f"E={E}: the lag-3 round trip differs"
        assert torch.equal(coders["lag 1"][2], coders["zigzag"][2]), f"E={E}: lag 1 is not the zigzag filter"
        ms = measure(calls, a.rounds)
        for k, v in ms.items():
            say(f"E={E} whole call, {k}: {v[len(v) // 2]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]")
        say(f"E={E} container bytes of {n}: planes {sizes['planes']}, zigzag {sizes['zigzag']}, lag 3 {sizes['lag 3']} "
            f"({sizes['lag 3'] / min(sizes['planes'], sizes['zigzag']):.3f} x the smaller)")
        del coders, calls, src, dst, t, got
        torch.cuda.empty_cache()
    say("# the condition (lag transform <= coder of its direction): "
        + ("met by every row" if not misses else "MISSED by " + ", ".join(f"E={E} S={S} {d}" for E, S, d in misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
