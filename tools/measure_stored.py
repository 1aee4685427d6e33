#!/usr/bin/env python3
"""Stored blocks measured in one GPU run (results: profiles/r08_stored.txt).

  1. 65,536 device-resident blocks of 64 KiB (4 GiB): iid (every block stored) and Zipf (none stored), the stored `_dev`
     calls against the plain ones (redux_encode_blocks_dev / redux_decode_blocks_dev), alternating, device-event ms;
  2. bf16 N(0, 0.02) with element_size 2 and fp32 N(0, 1) with element_size 4 at t = 65536 and 64512: ratio, blocks
     stored, encode and decode ms, against the planes calls;
  3. a torch copy of 4 GiB (the yardstick of k_store_unpack's 2 * bytes / kernel time);
  4. Zipf in 2,048 blocks of 1 MiB: the stored decoder's table form runs k_decode where the plain call runs
     k_decode_cells<8> (one launch each);
  5. the host-pointer calls at 1 GiB of iid (wall time, median).
Every decode is checked against its input.

usage: python tools/measure_stored.py [--reps R] [--skip-host] [--only-iid] [--out FILE] [--stats DIR]
The kernel trace: rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/measure_stored.py --only-iid --skip-host; then
--stats <dir> appends the per-kernel table of that trace to the report.
"""
import argparse
import ctypes as C
import csv
import glob
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import _lib  # noqa: E402

B, NB = 65536, 65536
N = B * NB


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


def wall(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return sorted(t)[len(t) // 2]


class Calls:
    """the plain / planes and the stored `_dev` calls over one device-resident input"""

    def __init__(self, d_in, E, B=B, NB=NB):
        self.L, self.cp, self.E, self.d_in = _lib.lib(), _lib.Params(8, 30, 32), E, d_in
        self.B, self.NB, self.N = B, NB, B * NB
        L, cp = self.L, C.byref(self.cp)
        self.cap = L.redux_encode_bound(cp, self.N, self.B)
        self.out = torch.empty(self.cap, dtype=torch.uint8, device="cuda:0")
        self.offs = torch.empty(self.NB + 1, dtype=torch.int64, device="cuda:0")
        self.flags = torch.zeros(self.NB, dtype=torch.uint8, device="cuda:0")
        self.st = torch.empty(self.NB, dtype=torch.int32, device="cuda:0")
        self.sum = torch.zeros(2, dtype=torch.int32, device="cuda:0")
        self.sz = torch.empty(self.NB, dtype=torch.int32, device="cuda:0")
        self.dec = torch.empty(self.N, dtype=torch.uint8, device="cuda:0")
        ws = max(L.redux_encode_stored_workspace_bytes(cp, self.N, self.B, E), L.redux_encode_planes_workspace_bytes(cp, self.N, self.B, E),
                 L.redux_decode_stored_workspace_bytes(cp, self.N, self.B, E), L.redux_decode_planes_workspace_bytes(cp, self.N, self.B, E))
        self.ws_b = ws
        self.ws = torch.empty(ws, dtype=torch.uint8, device="cuda:0")

    def p(self, t):
        return C.c_void_p(t.data_ptr())

    def s(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def enc_plain(self):
        self.sum.zero_()
        assert self.L.redux_encode_planes_dev(C.byref(self.cp), self.p(self.d_in), self.N, self.B, self.E, self.p(self.out), self.cap,
                                              self.p(self.offs), self.p(self.st), self.p(self.sum), self.p(self.ws), self.ws_b,
                                              self.s()) == 0

    def enc_stored(self, t):
        self.sum.zero_()
        assert self.L.redux_encode_stored_dev(C.byref(self.cp), self.p(self.d_in), self.N, self.B, self.E, t, self.p(self.out), self.cap,
                                              self.p(self.offs), self.p(self.flags), self.p(self.st), self.p(self.sum),
                                              self.p(self.ws), self.ws_b, self.s()) == 0

    def dec_plain(self):
        self.sum.zero_()
        if self.E == 1:
            rc = self.L.redux_decode_blocks_dev(C.byref(self.cp), self.p(self.out), self.p(self.offs), self.NB, self.B, self.p(self.dec), self.N,
                                                self.p(self.sz), self.p(self.st), self.p(self.sum), self.p(self.ws), self.ws_b,
                                                self.s())
        else:
            rc = self.L.redux_decode_planes_dev(C.byref(self.cp), self.p(self.out), self.p(self.offs), self.N, self.B, self.E,
                                                self.p(self.dec), self.p(self.sz), self.p(self.st), self.p(self.sum),
                                                self.p(self.ws), self.ws_b, self.s())
        assert rc == 0

    def dec_stored(self):
        assert self.L.redux_decode_stored_dev(C.byref(self.cp), self.p(self.out), self.p(self.offs), self.p(self.flags), self.N, self.B,
                                              self.E, self.p(self.dec), self.N, self.p(self.sz), self.p(self.st), self.p(self.sum),
                                              self.p(self.ws), self.ws_b, self.s()) == 0

    def check(self):
        torch.cuda.synchronize()
        return self.sum.tolist() == [0, 0] and torch.equal(self.dec, self.d_in)


def stats_table(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    out = ["rocprofv3 --kernel-trace --stats (a run of its own: --only-iid --skip-host; every launch of the run, the first",
           "included):", "kernel                                   calls   avg ms   min ms"]
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        name = r["Name"].split("(")[0][:40]
        out.append(f"{name:40} {int(r['Calls']):5}  {float(r['AverageNs']) / 1e6:7.3f}  {float(r['MinNs']) / 1e6:7.3f}")
        if name.startswith("redux::k_store_unpack") or name.startswith("k_store_unpack"):
            out.append(f"  k_store_unpack: 2 * 4 GiB / avg = {2 * N / float(r['AverageNs']) / 1e3:.2f} TB/s, "
                       f"/ min = {2 * N / float(r['MinNs']) / 1e3:.2f} TB/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--only-iid", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if a.stats:
        with open(a.out, "a") as f:
            f.write("\n".join(stats_table(a.stats)) + "\n")
        return 0
    L = _lib.lib()
    say(f"# {rx.version()}  source hash {L.redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"65,536 device-resident blocks of 64 KiB; device-event ms, median of {a.reps}, two alternating rounds")
    x = torch.empty(N, dtype=torch.uint8, device="cuda:0")
    y = torch.empty_like(x)
    ms = timed(lambda: y.copy_(x), a.reps)
    say(f"torch copy of 4 GiB: {ms:.3f} ms = {2 * N / ms / 1e9:.2f} TB/s (2 * bytes: k_store_unpack's yardstick)")
    del y
    kinds = ["iid"] if a.only_iid else ["iid", "zipf", "bf16", "fp32"]
    say("data  E  t        ratio    stored   enc plain  enc stored   dec plain  dec stored   (decode = input)")
    for kind in kinds:
        E = {"bf16": 2, "fp32": 4}.get(kind, 1)
        if kind == "iid":
            rx.gen_iid(N, out=x)
        elif kind == "zipf":
            rx.gen_zipf(N, out=x)
        elif kind == "bf16":
            x.view(torch.bfloat16).copy_(torch.randn(N // 2, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1)) * 0.02)
        else:
            x.view(torch.float32).normal_(0, 1, generator=torch.Generator("cuda:0").manual_seed(2))
        c = Calls(x, E)
        for t in ((65536,) if E == 1 else (65536, 64512)):
            r = {}
            for _ in range(2 if not a.only_iid else 1):
                r.setdefault("ep", []).append(timed(c.enc_plain, a.reps))
                r.setdefault("es", []).append(timed(lambda: c.enc_stored(t), a.reps))
            c.enc_plain()
            c.dec_plain()
            ok_p = c.check()
            plain_bytes = int(c.offs[-1])
            c.enc_stored(t)
            torch.cuda.synchronize()
            stored_bytes, nstored = int(c.offs[-1]), int(c.flags.sum())
            c.dec_stored()
            ok_s = c.check()
            for _ in range(2 if not a.only_iid else 1):
                c.enc_plain()
                r.setdefault("dp", []).append(timed(c.dec_plain, a.reps))
                c.enc_stored(t)
                r.setdefault("ds", []).append(timed(c.dec_stored, a.reps))
            f = lambda k: "/".join(f"{v:.2f}" for v in r[k])  # noqa: E731
            say(f"{kind:5} {E}  {t:5}  {plain_bytes / N:.5f}->{stored_bytes / N:.5f}  {nstored:6}  {f('ep'):>10}  {f('es'):>10}  "
                f"{f('dp'):>10}  {f('ds'):>10}   ({'ok' if ok_p and ok_s else 'MISMATCH'})")
            if not (ok_p and ok_s):
                return 1
        del c
        torch.cuda.empty_cache()
    del x
    torch.cuda.empty_cache()
    if not a.only_iid:  # blocks above 64 KiB: the stored decoder's table form runs k_decode where the plain one runs k_decode_cells<8>
        Bl, nbl = 1 << 20, 2048
        xl = rx.gen_zipf(Bl * nbl, seed=3)
        c = Calls(xl, 1, Bl, nbl)
        c.enc_plain()
        ep = timed(c.enc_plain, 1)
        dp = timed(c.dec_plain, 1)
        ok_p = c.check()
        es = timed(lambda: c.enc_stored(65536), 1)
        ds = timed(c.dec_stored, 1)
        ok_s = c.check()
        say(f"zipf 1 MiB blocks x {nbl}: enc plain {ep:.2f}  enc stored {es:.2f}  dec plain {dp:.2f} "
            f"({L.redux_decode_kernel_name_n(C.byref(c.cp), None, Bl, nbl).decode()[:24]})  dec stored {ds:.2f} "
            "(k_decode<false, true>, table form)  "
            f"{int(c.flags.sum())} stored ({'ok' if ok_p and ok_s else 'MISMATCH'})")
        del c, xl
        torch.cuda.empty_cache()
    if not a.skip_host:
        n, nb = 1 << 30, (1 << 30) // B
        data = rx.gen_iid(n, seed=7).cpu().numpy()
        flags = np.zeros(nb, np.uint8)
        t = {}
        for _ in range(2):
            t.setdefault("enc", []).append(wall(lambda: rx.compress_blocks(data, B), a.reps))
            t.setdefault("enc_stored", []).append(wall(lambda: rx.compress_blocks(data, B, stored=flags), a.reps))
        o1, f1, _ = rx.compress_blocks(data, B)
        o2, f2, _ = rx.compress_blocks(data, B, stored=flags)
        for _ in range(2):
            t.setdefault("dec", []).append(wall(lambda: rx.decompress_blocks(o1, f1, B), a.reps))
            t.setdefault("dec_stored", []).append(wall(lambda: rx.decompress_blocks(o2, f2, B, length=n, stored=flags), a.reps))
        ok = rx.decompress_blocks(o2, f2, B, length=n, stored=flags)[0].tobytes() == data.tobytes()
        say(f"host-pointer calls, 1 GiB of iid, 64 KiB blocks (wall s, median of {a.reps}, two alternating rounds; "
            f"{int(flags.sum())} of {nb} blocks stored, {'round trip ok' if ok else 'MISMATCH'}):")
        for k in ("enc", "enc_stored", "dec", "dec_stored"):
            say(f"  {k:10} " + "  ".join(f"{v:.4f} s = {n / v / 1e9:.1f} GB/s" for v in t[k]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
