#!/usr/bin/env python3
"""k_byte_hist of 4 GiB (iid, Zipf, one byte value) in the library REDUX_LIB names: one line per input.
Run by tools/ab/hist_variants.sh once per variant build (a fresh process each: the library is chosen at import)."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import redux_amd as rx  # noqa: E402
from redux_amd import _lib  # noqa: E402


def main():
    L = _lib.lib()
    n = 4 << 30
    x = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    counts = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    name = os.path.basename(os.environ.get("REDUX_LIB", "product"))
    for kind in ("iid", "zipf", "one"):
        if kind == "iid":
            rx.gen_iid(n, out=x)
        elif kind == "zipf":
            rx.gen_zipf(n, out=x)
        else:
            x.fill_(0x3C)
        ms = []
        for i in range(11):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            assert L.redux_histogram_dev(C.c_void_p(x.data_ptr()), n, C.c_void_p(counts.data_ptr()), None, 0, s) == 0
            e1.record()
            torch.cuda.synchronize()
            if i:
                ms.append(e0.elapsed_time(e1))
        t = sorted(ms)[len(ms) // 2]
        print(f"{name:34s} {kind:5s} {t:.3f} ms = {n / t / 1e9:.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
