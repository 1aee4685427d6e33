#!/usr/bin/env python3
"""Plane-static coding measured in one GPU run (results: profiles/r09_plane_static.txt).

Device-event times, medians of `--reps` runs, two alternating rounds of every comparison, device-resident blocks of 64 KiB:
  1. k_plane_hist (E = 2, 4) against k_byte_hist on the same x' buffer;
  2. plane-static encode / decode (bf16 E = 2, fp32 E = 4: the k_*_segment_static* kernels with a single segment, as
     the printed kernel names say) against (a) the one-table static calls on the same x' and (b) the adaptive planes
     calls on the same input; compressed_over_input of each;
  3. semi-static end to end (layout + histogram + tables + encode) against adaptive planes encode;
  4. E = 1 through the one-table entry points (the existing static path).

usage: python tools/measure_plane_static.py [--mib N] [--reps R] [--out FILE]   (N: MiB of input, default 4096)
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


def typed(kind, n):
    """bf16 = N(0, 0.02), fp32 = N(0, 1), generated on the device"""
    g = torch.Generator(device="cuda:0").manual_seed(5)
    if kind == "bf16":
        v = torch.empty(n // 2, dtype=torch.float32, device="cuda:0").normal_(0, 0.02, generator=g).to(torch.bfloat16)
    else:
        v = torch.empty(n // 4, dtype=torch.float32, device="cuda:0").normal_(0, 1, generator=g)
    return v.view(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.mib << 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    L = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    gbs = lambda ms: n / ms / 1e6  # noqa: E731
    say(f"# {rx.version()} source {L.redux_source_hash().decode()}; {n >> 20} MiB in {n // B} blocks of {B}; medians of {a.reps}")
    for kind, E in (("bf16", 2), ("fp32", 4)):
        d_in = typed(kind, n)
        d_x = rx.planes(d_in, E, B)
        counts1 = torch.zeros(256, dtype=torch.int64, device="cuda:0")
        countsE = torch.zeros(E * 256, dtype=torch.int64, device="cuda:0")
        flat = lambda: L.redux_histogram_dev(C.c_void_p(d_x.data_ptr()), n, C.c_void_p(counts1.data_ptr()), None, 0, stream())  # noqa: E731
        plane = lambda: L.redux_plane_histogram_dev(C.c_void_p(d_x.data_ptr()), n, B, E, C.c_void_p(countsE.data_ptr()), None, 0, stream())  # noqa: E731
        ps = rx.DevicePlaneStaticCoder.from_data(d_in, PARAMS, E, B, n)
        one = rx.DeviceStaticCoder.from_data(d_x, PARAMS, B, n)
        ad_e = rx.DeviceEncoder(PARAMS, B, n, element_size=E)
        ad_d = rx.DeviceDecoder(PARAMS, B, n // B, element_size=E)
        res = {}

        def enc(c, src, key):
            out, offs, _, summary = c.encode(src)
            torch.cuda.synchronize()
            assert summary.tolist() == [0, 0]
            res[key] = (out, offs, int(offs[-1]) / n)

        enc(ps, d_in, "ps")
        enc(one, d_x, "one")
        enc(ad_e, d_in, "ad")
        say(f"{kind} E={E}: compressed_over_input plane-static {res['ps'][2]:.4f} (+{E * 1032} table bytes), one static table over x' "
            f"{res['one'][2]:.4f}, adaptive planes {res['ad'][2]:.4f}")
        say(f"  kernels: {L.redux_plane_static_encode_kernel_name(C.byref(ps.cp), ps.total, n, B, E).decode()} / "
            f"{L.redux_plane_static_decode_kernel_name(C.byref(ps.cp), ps.total, n // B, E).decode()}")

        def e2e():
            c = rx.DevicePlaneStaticCoder.from_data(d_in, PARAMS, E, B, n)
            c.ws, c.ws_off, c.out, c.offsets, c.status, c.summary = ps.ws, ps.ws_off, ps.out, ps.offsets, ps.status, ps.summary
            c.encode(d_in)

        ps_streams = res["ps"][0][: int(res["ps"][1][-1])].clone()
        ps_offs = res["ps"][1].clone()
        one_streams = res["one"][0][: int(res["one"][1][-1])].clone()
        one_offs = res["one"][1].clone()
        ad_streams = res["ad"][0][: int(res["ad"][1][-1])].clone()
        ad_offs = res["ad"][1].clone()
        for rnd in (1, 2):
            say(f"  round {rnd}: k_byte_hist {timed(flat, a.reps):.3f} ms, k_plane_hist {timed(plane, a.reps):.3f} ms")
            say(f"  round {rnd}: encode GB/s plane-static {gbs(timed(lambda: ps.encode(d_in), a.reps)):.1f} (layout included), "
                f"one-table static on x' {gbs(timed(lambda: one.encode(d_x), a.reps)):.1f} (no layout), "
                f"adaptive planes {gbs(timed(lambda: ad_e.encode(d_in), a.reps)):.1f}, "
                f"semi-static end to end {gbs(timed(e2e, a.reps)):.1f}")
            say(f"  round {rnd}: decode GB/s plane-static {gbs(timed(lambda: ps.decode(ps_streams, ps_offs, n), a.reps)):.1f} (inverse layout included), "
                f"one-table static {gbs(timed(lambda: one.decode(one_streams, one_offs), a.reps)):.1f} (no layout), "
                f"adaptive planes {gbs(timed(lambda: ad_d.decode(ad_streams, ad_offs, length=n), a.reps)):.1f}")
        dec = ps.decode(ps_streams, ps_offs, n)[0]
        assert torch.equal(dec, d_in)
        del ps, one, ad_e, ad_d, res, d_in, d_x, dec
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
