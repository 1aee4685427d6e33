"""Segment-static coding against plane-static and the adaptive planes path on device-resident typed data.

    python tools/measure_segment_static.py [--blocks 65536] [--block-size 65536] [--out profiles/r10_segment_static.txt]

Shape: `blocks` x `block-size` bytes of mixed-sigma bf16 (E = 2: tensors of 2^19 to 2^22 elements, sigma log-uniform in
[0.002, 0.5], the high halves of fp32) and of fp32 with the same sigmas (E = 4).  Timing: device events, medians of 5, two
alternating rounds (every row is timed once per round, the rows in the same order; both medians are printed).  Rows: ratio,
encode and decode GB/s for k in 1, 2, 4, 8 with the decoder instance each k selected; plane-static (the same kernels with a
single segment) and the adaptive planes path on the same data; k_segment_hist against k_plane_hist on the same bytes;
k_static_tables for the full table set; build_encode_dev end to end.  Last: the k0 the default rule picks (the smallest k
whose decode rate is at least the adaptive planes decoder's)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import redux_amd as rx  # noqa: E402
from redux_amd import _lib  # noqa: E402

P = (8, 30, 32)
TOTAL = 1 << 16


def mixed(nbytes, E, seed=7):
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda:0") if E == 4 else torch.empty(nbytes // 2, dtype=torch.int16, device="cuda:0")
    n, at = out.numel(), 0
    while at < n:
        m = min(int(2 ** rng.uniform(19, 22)), n - at)
        sigma = float(np.exp(rng.uniform(np.log(0.002), np.log(0.5))))
        v = torch.randn(m, generator=g, device="cuda:0") * sigma
        out[at: at + m] = v if E == 4 else (v.view(torch.int32) >> 16).to(torch.int16)
        at += m
    return out.view(torch.uint8)


def ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--block-size", type=int, default=65536)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, n = a.block_size, a.blocks * a.block_size
    L = _lib.lib()
    cp = _lib.Params(*P)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# %s, source %s; %d x %d bytes; ms are medians of 5, round 1 / round 2" % (rx.version(), L.redux_source_hash().decode(), a.blocks, B))
    for E, name in ((2, "bf16"), (4, "fp32")):
        x = mixed(n, E)
        gbs = lambda t: n / t / 1e6
        rows = {}
        # the coders
        seg = {k: rx.DeviceSegmentStaticCoder(P, E, B, n, 64 * E * k) for k in (1, 2, 4, 8)}
        plane = rx.DevicePlaneStaticCoder.from_data(x, P, E, B, n)
        enc = rx.DeviceEncoder(P, B, n, element_size=E)
        dec = rx.DeviceDecoder(P, B, a.blocks, element_size=E)
        streams = {}
        for k, c in seg.items():
            out, offs, _, summ = c.encode_build(x)
            torch.cuda.synchronize()
            assert summ.tolist() == [0, 0]
            end = int(offs[-1])
            streams[k] = (out[:end].clone(), offs.clone())
            tables = c.ntables(n) * 1032
            back = c.decode(*streams[k], n)[0]
            assert torch.equal(back, x)
            rows[k] = [(end + tables) / n, L.redux_segment_static_decode_kernel_name(C.byref(cp), TOTAL, a.blocks, E, 64 * E * k).decode()]
        p_out, p_offs, _, _ = plane.encode(x)
        p_s = (p_out[: int(p_offs[-1])].clone(), p_offs.clone())
        a_out, a_offs = enc.encode(x)[:2]
        a_s = (a_out[: int(a_offs[-1])].clone(), a_offs.clone())
        d_x = rx.planes(x, E, B)
        counts = torch.zeros(seg[1].ntables(n) * 256, dtype=torch.int64, device="cuda:0")
        d_cum = torch.zeros(seg[1].ntables(n) * 258, dtype=torch.int32, device="cuda:0")
        s0 = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        t = {}
        for rnd in (0, 1):
            for k, c in seg.items():
                t.setdefault(("enc", k), []).append(ms(lambda: c.encode(x)))
                t.setdefault(("dec", k), []).append(ms(lambda: c.decode(*streams[k], n)))
                t.setdefault(("build", k), []).append(ms(lambda: c.encode_build(x)))
            t.setdefault(("enc", "plane"), []).append(ms(lambda: plane.encode(x)))
            t.setdefault(("dec", "plane"), []).append(ms(lambda: plane.decode(*p_s, n)))
            t.setdefault(("enc", "adaptive"), []).append(ms(lambda: enc.encode(x)))
            t.setdefault(("dec", "adaptive"), []).append(ms(lambda: dec.decode(*a_s, n)))
            for k in (1, 8):
                t.setdefault(("hist", k), []).append(ms(lambda: L.redux_segment_histogram_dev(
                    C.c_void_p(d_x.data_ptr()), n, B, E, 64 * E * k, C.c_void_p(counts.data_ptr()), s0)))
            t.setdefault(("hist", "plane"), []).append(ms(lambda: L.redux_plane_histogram_dev(
                C.c_void_p(d_x.data_ptr()), n, B, E, C.c_void_p(counts.data_ptr()), None, 0, s0)))
            t.setdefault(("tables", 1), []).append(ms(lambda: L.redux_segment_static_tables_dev(
                C.byref(cp), C.c_void_p(counts.data_ptr()), a.blocks, E, 64 * E, TOTAL, C.c_void_p(d_cum.data_ptr()), s0)))
        two = lambda key: "%.3f / %.3f ms (%.0f / %.0f GB/s)" % (t[key][0], t[key][1], gbs(t[key][0]), gbs(t[key][1]))
        say("## %s, E = %d" % (name, E))
        for k in (1, 2, 4, 8):
            say("segment-static k=%d: ratio %.4f (%d tables); encode %s; decode %s; build+encode %s; %s"
                % (k, rows[k][0], seg[k].ntables(n), two(("enc", k)), two(("dec", k)), two(("build", k)), rows[k][1]))
        say("plane-static: ratio %.4f; encode %s; decode %s" % ((int(p_offs[-1]) + E * 1032) / n, two(("enc", "plane")), two(("dec", "plane"))))
        say("adaptive planes: ratio %.4f; encode %s; decode %s" % (int(a_offs[-1]) / n, two(("enc", "adaptive")), two(("dec", "adaptive"))))
        say("k_segment_hist k=1 %s; k=8 %s; k_plane_hist %s" % (two(("hist", 1)), two(("hist", 8)), two(("hist", "plane"))))
        say("k_static_tables, %d tables: %.3f / %.3f ms" % (seg[1].ntables(n), t[("tables", 1)][0], t[("tables", 1)][1]))
        ad = max(t[("dec", "adaptive")])
        ok = [k for k in (1, 2, 4, 8) if max(t[("dec", k)]) <= ad]
        say("default rule: k0 = %s (smallest k whose decode is at least as fast as adaptive planes decode in both rounds)" % (ok[0] if ok else "none"))
        del seg, plane, enc, dec, streams, x, d_x
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
