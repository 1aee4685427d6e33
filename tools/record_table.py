#!/usr/bin/env python3
"""The record layout for fixed-width structs, measured in one GPU run (results: profiles/record_layout.txt).

  1. sizes: imu23 and ticks20, the two GENERATED tables of packed structs of tests/test_record_cpu.py, at `--records` records
     (default 4,000,000) and 64 KiB blocks: container bytes (the streams summed plus container.overhead_bytes) plain, behind the
     best lag setting (filter "lag" at E = 1, S = R; for ticks20 also planes and lag at E = 2 and 4 with S = R / E), behind
     the record layout alone and behind the record layout with the byte delta.
  2. timings: forward and inverse of `--gib` GiB (default 4) at 64 KiB blocks, with and without the byte delta, for R = 3, 12,
     20, 23, 64, 255, 256 (redux_record_planes_dev), next to a plain device copy, k_planes<8> (redux_planes_dev at E = 8),
     k_lag_planes<1> / k_lag_unplanes<1> at S = 23, and the adaptive coder of each direction on the same bytes: the encoder's
     coder kernel (DeviceEncoder.encode_slots: phase 1, no compaction) and the plain decode call (redux_decode_blocks_dev).
     The input is imu23 repeated; the coders run on its record layout with the delta at R = 23.  All entries are taken in
     turn in every round, so that they see the same minutes.  Per entry: the median over the rounds, the fastest and the
     slowest.  THE CONDITION: every record transform takes less time than the coder of its direction; a row that misses it
     says MISS.  The ratios to the copy and to the existing transforms are recorded without a bar.

usage: python tools/record_table.py [--gib N] [--records N] [--rounds R] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import api, container  # noqa: E402

PARAMS = (8, 30, 32)
SIZES = (3, 12, 20, 23, 64, 255, 256)
B = 65536


def once(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def generated_tables(n):
    """imu23 and ticks20 of tests/test_record_cpu.py at n records -> {name: (uint8 array, record size)}"""
    rng = np.random.default_rng(5)
    t = np.arange(n)
    imu = np.zeros(n, dtype=[("ts", "<i8"), ("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("flags", "<u2"), ("st", "u1")])
    imu["ts"] = 1700000000000000 + np.cumsum(rng.integers(900, 1100, n))
    imu["x"] = np.sin(t / 300) + rng.normal(0, .01, n)
    imu["y"] = 9.8 + rng.normal(0, .02, n)
    imu["z"] = np.cumsum(rng.normal(0, .01, n))
    imu["flags"] = rng.choice([0, 1, 4, 0x8000], n, p=[.9, .05, .04, .01])
    imu["st"] = rng.integers(0, 3, n)
    tk = np.zeros(n, dtype=[("id", "<u4"), ("px", "<i4"), ("qty", "<u2"), ("side", "u1"), ("pad", "u1"), ("ts", "<u8")])
    tk["id"] = np.arange(n) + rng.integers(0, 3, n)
    tk["px"] = 100000 + np.cumsum(rng.integers(-5, 6, n))
    tk["qty"] = rng.geometric(.05, n)
    tk["side"] = rng.integers(0, 2, n)
    tk["pad"] = 0
    tk["ts"] = 1700000000000 + np.cumsum(rng.integers(0, 50, n))
    return {"imu23": (imu.view(np.uint8).reshape(-1).copy(), 23), "ticks20": (tk.view(np.uint8).reshape(-1).copy(), 20)}


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


def container_bytes(d, **kw):
    """the container of the device tensor d under these DeviceEncoder options: streams summed plus the overhead"""
    n = d.numel()
    enc = rx.DeviceEncoder(PARAMS, B, n, **kw)
    res = enc.encode(d)
    torch.cuda.synchronize()
    assert res[3].tolist() == [0, 0]
    return int(res[1][-1]) + container.overhead_bytes("adaptive", max(1, -(-n // B)), kw.get("element_size", 1),
                                                      filter=kw.get("filter"), record_size=kw.get("record_size"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {rx.version()}  source hash {rx._lib.lib().redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    # ---- 1. sizes ----
    say(f"# sizes: GENERATED tables of {a.records} records, blocks of 64 KiB, container bytes (streams + overhead)")
    tables = generated_tables(a.records)
    for name, (x, R) in tables.items():
        d = torch.from_numpy(x).cuda()
        lag = {"lag E=1 S=%d" % R: container_bytes(d, filter="lag", lag=R)}
        if name == "ticks20":
            for E in (2, 4):
                lag["planes E=%d" % E] = container_bytes(d, element_size=E)
                lag["lag E=%d S=%d" % (E, R // E)] = container_bytes(d, element_size=E, filter="lag", lag=R // E)
        plain = container_bytes(d)
        alone = container_bytes(d, record_size=R)
        both = container_bytes(d, record_size=R, filter="delta")
        best = min(lag, key=lag.get)
        dec = rx.DeviceDecoder(PARAMS, B, -(-len(x) // B), record_size=R, filter="delta")
        enc = rx.DeviceEncoder(PARAMS, B, len(x), record_size=R, filter="delta")
        out, offs, _, _ = enc.encode(d)
        back = dec.decode(out[: int(offs[-1])], offs, length=len(x))
        torch.cuda.synchronize()
        assert back[3].tolist() == [0, 0] and torch.equal(back[0], d), f"{name}: the round trip differs"
        say(f"{name} (R = {R}, {len(x)} bytes): plain {plain}; " + ", ".join(f"{k} {v}" for k, v in lag.items())
            + f"; record layout {alone}; record layout + byte delta {both} = {both / len(x):.3f} of the input, "
            f"{both / min(plain, lag[best]):.3f} of the best existing ({best if lag[best] < plain else 'plain'})")
        del d, enc, dec, out, offs, back
    torch.cuda.empty_cache()
    # ---- 2. timings ----
    n = a.gib << 30
    nb = n // B
    say(f"# timings: {a.gib} GiB = {nb} blocks of 64 KiB, imu23 repeated; {a.rounds} rounds of every entry in turn; "
        "ms: median [fastest .. slowest]; the clocks were not touched")
    piece = torch.from_numpy(tables["imu23"][0]).cuda()
    src = piece.repeat((n + piece.numel() - 1) // piece.numel())[:n].contiguous()
    del piece
    dst = torch.empty_like(src)
    t = api.record_planes(src, 23, B, delta=True)  # what the coders see
    enc = rx.DeviceEncoder(PARAMS, B, n)
    out, offs, _, summary = enc.encode(t)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    streams, d_offs = out[: int(offs[-1])].clone(), offs.clone()
    dec = rx.DeviceDecoder(PARAMS, B, nb)
    runs = {"coder forward": lambda: enc.encode_slots(t), "coder inverse": lambda: dec.decode(streams, d_offs),
            "copy": lambda: dst.copy_(src),
            "planes E=8 forward": lambda: rx.planes(src, 8, B, out=dst),
            "planes E=8 inverse": lambda: rx.planes(t, 8, B, inverse=True, out=dst),
            "lag E=1 S=23 forward": lambda: api.lag_planes(src, 1, B, 23, out=dst),
            "lag E=1 S=23 inverse": lambda: api.lag_planes(t, 1, B, 23, inverse=True, out=dst)}
    for R in SIZES:
        for delta in (False, True):
            f = "+delta" if delta else "      "
            runs[f"record {R}{f} forward"] = lambda R=R, delta=delta: api.record_planes(src, R, B, delta=delta, out=dst)
            runs[f"record {R}{f} inverse"] = lambda R=R, delta=delta: api.record_planes(t, R, B, delta=delta, inverse=True, out=dst)
    ms = measure(runs, a.rounds)
    med = {k: v[len(v) // 2] for k, v in ms.items()}
    misses = []
    for k, v in ms.items():
        line = f"{k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}] = {2 * n / med[k] / 1e9:.2f} TB/s read + written"
        if k.startswith("record"):
            d = k.rsplit(" ", 1)[1]
            ok = med[k] < med[f"coder {d}"]
            if not ok:
                misses.append(k)
            line += (f"  {med[k] / med['copy']:.2f} x copy  {med[k] / med['planes E=8 ' + d]:.2f} x planes<8>  "
                     f"{med[k] / med['lag E=1 S=23 ' + d]:.2f} x lag<1>  {med[k] / med['coder ' + d]:.3f} x coder  {'ok' if ok else 'MISS'}")
        say(line)
    for R in SIZES:  # inverse of forward, at the size timed
        for delta in (False, True):
            back = torch.empty_like(src)
            api.record_planes(src, R, B, delta=delta, out=dst)
            api.record_planes(dst, R, B, delta=delta, inverse=True, out=back)
            torch.cuda.synchronize()
            assert torch.equal(back, src), f"R={R} delta={delta}: inverse of forward differs"
            del back
    say("# the condition (record transform < coder of its direction): "
        + ("met by every row" if not misses else "MISSED by " + ", ".join(misses)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
