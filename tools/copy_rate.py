#!/usr/bin/env python3
"""The copy yardstick of the encoder's row gather: tools/ubench/copy_rate.hip, a grid-stride uint4 copy, on the bytes
k_compact_rows moves at the headline shape (65,536 iid blocks of 64 KiB leave 4.30 GB of streams: read once, written once).

    python tools/copy_rate.py [--bytes N] [--warmup 10] [--reps 10] [--per-cu 2,3,4,6,8,16,32]

builds tools/ubench/bin/copy_rate when it is missing or older than its source, runs it once per grid size (workgroups of 256
threads per CU) and prints every line and the best median: the rate a gather's time for the same bytes is compared with,
in the same session on the same chip."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "ubench", "copy_rate.hip")
BIN = os.path.join(ROOT, "tools", "ubench", "bin", "copy_rate")


def build():
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= os.path.getmtime(SRC):
        return
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "--offload-arch=gfx950", "-O3", "-o", BIN, SRC])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=4_300_000_000)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--per-cu", default="2,3,4,6,8,16,32")
    ap.add_argument("--build-only", action="store_true")
    a = ap.parse_args()
    build()
    if a.build_only:
        return 0
    best = None
    for per_cu in a.per_cu.split(","):
        run = subprocess.run([BIN, str(a.bytes), str(a.warmup), str(a.reps), per_cu], capture_output=True, text=True)
        sys.stdout.write(run.stdout)
        if run.returncode != 0:  # (nothing more on a device that has failed a launch)
            sys.stderr.write(run.stderr)
            return run.returncode
        ms, rate = re.search(r"median ([0-9.]+) ms .* = ([0-9.]+) TB/s", run.stdout).groups()
        if best is None or float(rate) > best[1]:
            best = (float(ms), float(rate), per_cu)
    print("yardstick: %.3f TB/s read+write (%.4f ms for 2 x %d bytes, %s workgroups per CU)" % (best[1], best[0], a.bytes, best[2]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
