#!/usr/bin/env python3
"""Per-block CRC-32 measured in one GPU run (results: profiles/r07_crc.txt).

  1. k_crc32 alone (redux_crc32_blocks_dev) on 4 GiB of iid and of all-zero data in blocks of 1 KiB, 64 KiB and 1 MiB, and
     one 1 GiB block: ms and TB/s of input read, next to a torch int64 sum of the same bytes (the HBM read yardstick);
     every result is checked against zlib on a sample of blocks;
  2. the host-pointer calls at 1 GiB of Zipf data in 64 KiB blocks: redux_encode_blocks against redux_encode_blocks_crc and
     redux_decode_blocks against redux_decode_blocks_crc (wall time of the synchronous call, median of --reps).

usage: python tools/measure_crc.py [--mib N] [--reps R] [--skip-host] [--out FILE]   (N: MiB of kernel input, default 4096)
The kernel trace of the same launches: rocprofv3 --kernel-trace --stats -d <dir> -- python tools/measure_crc.py --skip-host
"""
import argparse
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import _lib  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    L = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    say(f"# {rx.version()}  source hash {L.redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    n = a.mib << 20
    x = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ms = timed(lambda: x.view(torch.int64).sum(), a.reps)
    say(f"torch int64 sum of {a.mib} MiB: {ms:.3f} ms = {n / ms / 1e9:.2f} TB/s (read yardstick)")
    crc = torch.empty(n // 1024 + 1, dtype=torch.int32, device="cuda:0")
    say("kernel     data  block      ms     TB/s  (zlib spot check)")
    for kind in ("iid", "zero"):
        if kind == "iid":
            rx.gen_iid(n, out=x)
        else:
            x.zero_()
        for B in (1024, 65536, 1 << 20, 1 << 30):
            if B > n:
                continue
            nb = L.redux_block_count(n, B)
            run = lambda: L.redux_crc32_blocks_dev(C.c_void_p(x.data_ptr()), n, B, C.c_void_p(crc.data_ptr()), stream())  # noqa: E731
            assert run() == _lib.OK
            ms = timed(run, a.reps)
            got = crc[:nb].cpu().numpy().view(np.uint32)
            picks = sorted({0, nb // 2, nb - 1})
            if B == 1 << 30:  # one zlib pass over the first block
                want, blk = 0, x[:B]
                for o in range(0, B, 1 << 27):
                    want = zlib.crc32(blk[o:o + (1 << 27)].cpu().numpy().tobytes(), want)
                ok = int(got[0]) == want
            else:
                ok = all(int(got[b]) == zlib.crc32(x[b * B:(b + 1) * B].cpu().numpy().tobytes()) for b in picks)
            label = f"{B >> 10} KiB" if B < (1 << 20) else f"{B >> 20} MiB"
            say(f"k_crc32  {kind:>5}  {label:>7}  {ms:7.3f}  {n / ms / 1e9:6.2f}  ({'ok' if ok else 'MISMATCH'})")
            if not ok:
                return 1
    del x, crc
    torch.cuda.empty_cache()
    if not a.skip_host:
        B, P = 65536, rx.Parameters(8, 30, 32)
        cp = P._c()
        n = 1 << 30
        data = rx.gen_zipf(n, seed=7).cpu().numpy()
        nb = n // B
        cap = L.redux_encode_bound(C.byref(cp), n, B)
        out = np.empty(cap, dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        st = np.zeros(nb, dtype=np.int32)
        bc = np.zeros(nb, dtype=np.uint32)
        enc = lambda: L.redux_encode_blocks(C.byref(cp), data.ctypes.data, n, B, out.ctypes.data, cap, offs.ctypes.data, st.ctypes.data)  # noqa: E731
        enc_c = lambda: L.redux_encode_blocks_crc(C.byref(cp), data.ctypes.data, n, B, out.ctypes.data, cap, offs.ctypes.data,  # noqa: E731
                                                  st.ctypes.data, bc.ctypes.data)
        dec_out = np.empty(n, dtype=np.uint8)
        sizes = np.zeros(nb, dtype=np.uint32)
        dc = np.zeros(nb, dtype=np.uint32)
        t = {}
        for rep in range(2):  # alternating, twice
            t.setdefault("enc", []).append(wall(enc, a.reps // 2))
            t.setdefault("enc_crc", []).append(wall(enc_c, a.reps // 2))
        dec = lambda: L.redux_decode_blocks(C.byref(cp), out.ctypes.data, offs.ctypes.data, nb, B, dec_out.ctypes.data, n,  # noqa: E731
                                            sizes.ctypes.data, st.ctypes.data)
        dec_c = lambda: L.redux_decode_blocks_crc(C.byref(cp), out.ctypes.data, offs.ctypes.data, nb, B, dec_out.ctypes.data, n,  # noqa: E731
                                                  sizes.ctypes.data, st.ctypes.data, dc.ctypes.data)
        for rep in range(2):
            t.setdefault("dec", []).append(wall(dec, a.reps // 2))
            t.setdefault("dec_crc", []).append(wall(dec_c, a.reps // 2))
        ok = bc[::997].tolist() == [zlib.crc32(data[b * B:(b + 1) * B].tobytes()) for b in range(0, nb, 997)] and \
            np.array_equal(bc, dc)
        say(f"host-pointer calls, 1 GiB of Zipf data, 64 KiB blocks (wall s, median of {a.reps // 2}, two alternating rounds):")
        for k in ("enc", "enc_crc", "dec", "dec_crc"):
            say(f"  {k:8} " + "  ".join(f"{v:.4f} s = {n / v / 1e9:.1f} GB/s" for v in t[k]))
        say(f"  encode with block_crc / without: {min(t['enc_crc']) / min(t['enc']):.3f};  decode: "
            f"{min(t['dec_crc']) / min(t['dec']):.3f}  (CRCs {'equal zlib and each other' if ok else 'MISMATCH'})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
