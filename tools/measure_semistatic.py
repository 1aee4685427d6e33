#!/usr/bin/env python3
"""Semi-static coding measured in one GPU run (results: profiles/r06_semistatic.txt).

  1. k_byte_hist alone on 4 GiB of iid, Zipf and one-byte-value data: ms and TB/s of input read, next to a torch sum of
     the same bytes read once (the HBM yardstick); k_static_table alone in microseconds;
  2. the static coder at 65,536 x 64 KiB of Zipf data with the table built on the device: encode and decode GB/s (input
     bytes / time of the whole stream-ordered call); semi-static encode end to end (histogram + table + read-back +
     encode) against adaptive encode of the same bytes;
  3. compressed_over_input of the static model (one table per file, default total 2^16) and of the adaptive model on
     Zipf and on every corpus file under tests/golden/corpora, through the host-pointer calls, 64 KiB blocks: the streams
     alone, and the container files `redux -c --block-size 65536 [--model static]` writes.  The static container carries
     the 1,032-byte table; the winner is decided on the container sizes.

usage: python tools/measure_semistatic.py [--mib N] [--out FILE]   (N: MiB of coder input, default 4096)
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import _lib  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    L = _lib.lib()
    cp = _lib.Params(*PARAMS)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    say(f"# {rx.version()}  source hash {L.redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    n = 4 << 30
    x = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    cum = torch.zeros(258, dtype=torch.int32, device="cuda:0")
    hist = lambda t: L.redux_histogram_dev(C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(counts.data_ptr()), None, 0, stream())  # noqa: E731
    ms = timed(lambda: x.view(torch.int64).sum(), 10)
    say(f"torch int64 sum of 4 GiB: {ms:.3f} ms = {n / ms / 1e9:.2f} TB/s (read yardstick)")
    times = {}
    for kind in ("iid", "zipf", "one"):
        if kind == "iid":
            rx.gen_iid(n, out=x)
        elif kind == "zipf":
            rx.gen_zipf(n, out=x)
        else:
            x.fill_(0x3C)
        ms = timed(lambda: hist(x), 10)
        times[kind] = ms
        counts.zero_()
        hist(x)
        assert counts.cpu().numpy().tolist() == torch.bincount(x, minlength=256).cpu().numpy().tolist(), kind
        say(f"k_byte_hist 4 GiB {kind}: {ms:.3f} ms = {n / ms / 1e9:.2f} TB/s")
    say(f"one-byte-value / iid time: {times['one'] / times['iid']:.3f}")
    us = timed(lambda: L.redux_static_table_dev(C.byref(cp), C.c_void_p(counts.data_ptr()), 1 << 16, C.c_void_p(cum.data_ptr()),
                                                stream()), 50) * 1000
    say(f"k_static_table (one workgroup, 256 threads): {us:.1f} us")
    del x
    torch.cuda.empty_cache()

    n = a.mib << 20
    nb = n // B
    say(f"# coder: {nb} x 64 KiB = {n >> 20} MiB of Zipf bytes (gen_zipf), params {PARAMS}; GB/s = input bytes / time of the call")
    x = rx.gen_zipf(n)
    coder = rx.DeviceStaticCoder.from_data(x, PARAMS, B, n)
    tab = np.array(list(coder.cum), dtype=np.uint32)
    assert tab.tolist() == rx.static_table_from_counts(torch.bincount(x, minlength=256).cpu().numpy()).tolist()
    ms_h = timed(lambda: (counts.zero_(), hist(x), L.redux_static_table_dev(C.byref(cp), C.c_void_p(counts.data_ptr()), 1 << 16,
                                                                             C.c_void_p(cum.data_ptr()), stream())), 5)
    ms_e = timed(lambda: coder.encode(x), 3)
    out, offs, status, summary = coder.encode(x)
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    total = int(offs[-1])
    streams, offs = out[:total].clone(), offs.clone()
    ms_d = timed(lambda: coder.decode(streams, offs), 3)
    d_out, _, _, dsum = coder.decode(streams, offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(d_out[:n], x)
    say(f"static (device table, total {int(tab[-1])}): ratio {total / n:.4f}  encode {ms_e:.2f} ms = {n / ms_e / 1e6:.1f} GB/s  "
        f"decode {ms_d:.2f} ms = {n / ms_d / 1e6:.1f} GB/s")
    say(f"histogram + table: {ms_h:.3f} ms = {100 * ms_h / ms_e:.1f} % of the static encode")
    del d_out, streams
    torch.cuda.empty_cache()

    # end to end: histogram + table + read-back + encode, reusing the coder's buffers (allocation is not part of coding)
    def semi_encode():
        coder.cum = (C.c_uint32 * 258)(*[int(v) for v in rx.static_table(x, PARAMS)])
        return coder.encode(x)
    ms_semi = timed(semi_encode, 3)
    del coder
    torch.cuda.empty_cache()
    enc = rx.DeviceEncoder(PARAMS, B, n)
    ms_a = timed(lambda: enc.encode(x), 3)
    o2, f2, _, s2 = enc.encode(x)
    torch.cuda.synchronize()
    ad_ratio = int(f2[-1]) / n
    say(f"semi-static encode end to end: {ms_semi:.2f} ms = {n / ms_semi / 1e6:.1f} GB/s   adaptive encode: {ms_a:.2f} ms = "
        f"{n / ms_a / 1e6:.1f} GB/s (ratio {ad_ratio:.4f})")
    del enc, o2, f2, x
    torch.cuda.empty_cache()

    say("# compressed_over_input, 64 KiB blocks, host-pointer calls: static (one table per input) vs adaptive (per block)")
    say("# streams: the coded blocks alone; file: the container (header + block sizes, + the 1,032-byte table for static)")
    say("# gain: adaptive stream bytes - static stream bytes; the table pays for itself where gain > 1032")
    rows = [("zipf 256 MiB (gen_zipf)", rx.gen_zipf(256 << 20, seed=77).cpu().numpy())]
    cdir = os.path.join(ROOT, "tests", "golden", "corpora")
    for c in sorted(os.listdir(cdir)):
        for f in sorted(os.listdir(os.path.join(cdir, c))):
            rows.append((f"{c}/{f}", np.fromfile(os.path.join(cdir, c, f), dtype=np.uint8)))
    from redux_amd import container
    stream_wins, file_wins = 0, []
    for name, d in rows:
        m = rx.StaticModel.from_data(d, PARAMS)
        so, sf, _ = rx.compress_blocks(d, B, m)
        ao, af, _ = rx.compress_blocks(d, B, PARAMS)
        back, sizes, _ = rx.decompress_blocks(so, sf, B, m)
        assert b"".join(back[i * B: i * B + int(sizes[i])].tobytes() for i in range(len(sizes))) == d.tobytes(), name
        sfile = container.compress_bytes(d.tobytes(), B, PARAMS, model="static")
        afile = container.compress_bytes(d.tobytes(), B, PARAMS)
        assert len(sfile) - len(afile) == container.TABLE + int(sf[-1]) - int(af[-1]), name
        n = max(len(d), 1)
        gain = int(af[-1]) - int(sf[-1])
        stream_wins += gain > 0
        if len(sfile) < len(afile):
            file_wins.append(name)
        say(f"{name:28s} {len(d):>10d} B  streams static {int(sf[-1]) / n:.4f} adaptive {int(af[-1]) / n:.4f}  gain {gain:>7d} B  "
            f"file static {len(sfile) / n:.4f} adaptive {len(afile) / n:.4f}  {'static' if len(sfile) < len(afile) else 'adaptive'} file smaller")
    say(f"streams alone: static smaller on {stream_wins} of {len(rows)} inputs")
    say(f"files (table included): static smaller on {len(file_wins)} of {len(rows)} inputs: {', '.join(file_wins)}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
