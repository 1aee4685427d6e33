"""Range reads on an MI355X: what k_segment_copy moves next to a torch copy of the same bytes, and what a range read of a large
container costs next to reading all of it.

    python tools/measure_range.py [--gib 4] [--repeats 5] [--out profiles/range_reads.txt]

Part 1, k_segment_copy through redux_segment_copy_dev, each figure the median of --repeats timed calls after one untimed call,
with the range, from HIP events around the call (so the upload of the tile table is in it), next to torch's copy_ of the
same number of bytes in the same run (tools/copy_bw.py's yardstick): 1 GiB as one segment with source and destination at the
same phase and at relative phases 1, 4, 8 and 15; 1 GiB as 16,384 segments of 64 KiB at random phases; 256 MiB as segments of
1 KiB at random phases.  Every result is compared with the source before it is timed.
Part 2, container.Reader on a container of --gib GiB of Zipf bytes held in memory, at blocks of 64 KiB and of 4 KiB: 1, 16 and
256 ranges of 1 MiB at random places as ONE read_many call and as one read call per range, next to decompress_bytes of the
whole container, host clock around calls that return the bytes, with the bytes fetched from the container.
Part 3, DeviceDecoder.decode_ranges on --device-gib GiB of streams kept in device memory, the same range sets, host clock
around calls that end in a synchronise, next to decode() of everything.
No figure is fixed in advance: the lines say what was measured.  profiles/range_reads.txt holds the outputs of the runs named
at its top (--parts picks the parts of a run; REDUX_LIB names another build of the library to measure)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def timed(torch, fn, repeats):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def clocked(fn, repeats):
    fn()
    ms = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms), min(ms), max(ms)


def cell(t):
    return f"{t[0]:9.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def rate(nbytes, t):
    return f"{2 * nbytes / t[0] / 1e9:5.2f} TB/s read+write"


def copies(torch, rx, api, repeats):
    say("== k_segment_copy next to torch copy_ (HIP events around the call, median (min .. max)) ==")
    rng = np.random.default_rng(1)
    n = 1 << 30
    src = torch.empty(n + 4096, dtype=torch.uint8, device="cuda").random_(0, 255)
    dst = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
    s0, d0 = (-src.data_ptr()) % 16, (-dst.data_ptr()) % 16
    t = timed(torch, lambda: dst[:n].copy_(src[:n]), repeats)
    say(f"torch copy_ of 1 GiB (u8)                                  {cell(t)}  {rate(n, t)}")

    def run(name, segs, nbytes):
        segs = api._segments_arg(segs)
        dst.zero_()
        rx.segment_copy(src, dst, segs)
        for i in rng.integers(0, len(segs), 16).tolist() + [0, len(segs) - 1]:  # spot checks, ends included
            s, d, k = (int(v) for v in segs[i])
            assert torch.equal(dst[d: d + k], src[s: s + k]), (name, i)
        t = timed(torch, lambda: api._segment_copy(torch, src, dst, segs), repeats)
        say(f"{name:58s} {cell(t)}  {rate(nbytes, t)}  ({len(api.segment_tiles(segs))} tiles)")
    for ph in (0, 1, 4, 8, 15):
        run(f"1 GiB, one segment, source {ph:2d} bytes past the destination's phase", [(s0 + ph, d0, n)], n)
    k = 65536
    run("1 GiB, 16,384 segments of 64 KiB, random phases",
        [(i * k + int(rng.integers(0, 16)), i * k + int(rng.integers(0, 16)), k - 16) for i in range(16384)], 16384 * (k - 16))
    k, m = 1024, 1 << 18
    t = timed(torch, lambda: dst[: m * k].copy_(src[: m * k]), repeats)
    say(f"torch copy_ of 256 MiB (u8)                                {cell(t)}  {rate(m * k, t)}")
    run("256 MiB, 262,144 segments of 1 KiB, random phases",
        [(i * (k + 16) + int(rng.integers(0, 16)), i * (k + 16) + int(rng.integers(0, 16)), k) for i in range(m)], m * k)
    say()


def range_sets(total, rng):
    return {r: [(int(s), 1 << 20) for s in rng.integers(0, total - (1 << 20), r)] for r in (1, 16, 256)}


def containers(torch, rx, container, gib, repeats):
    say(f"== container.Reader on {gib} GiB of Zipf bytes (host clock, median (min .. max); ranges of 1 MiB at random places) ==")
    data = rx.gen_zipf(gib << 30).cpu().numpy()
    for bs in (65536, 4096):
        t0 = time.perf_counter()
        blob = container.compress_bytes(data, bs, checksum=True)
        say(f"block size {bs}: container of {len(blob)} bytes with checksums, written in {time.perf_counter() - t0:.2f} s")
        sets = range_sets(len(data), np.random.default_rng(bs))
        whole = clocked(lambda: container.decompress_bytes(blob), max(1, repeats // 2))
        say(f"  decompress_bytes of everything                 {cell(whole)}")
        for r, ranges in sets.items():
            reader = container.Reader(blob)
            opened = reader.bytes_read
            got = reader.read_many(ranges)
            assert all(g == data[s: s + n].tobytes() for g, (s, n) in zip(got, ranges))
            fetched = reader.bytes_read - opened
            one = clocked(lambda: reader.read_many(ranges), repeats)
            each = clocked(lambda: [reader.read(*x) for x in ranges], 1 if r > 16 else repeats)
            say(f"  {r:3d} ranges: one read_many {cell(one)}   a read per range {cell(each)}   "
                f"{fetched} bytes fetched ({opened} at open)")
        del blob
    say()


def device(torch, rx, gib, repeats):
    say(f"== DeviceDecoder.decode_ranges on {gib} GiB of Zipf bytes in device memory (host clock to a synchronise) ==")
    n = gib << 30
    d_in = rx.gen_zipf(n)
    for bs in (65536, 4096):
        enc = rx.DeviceEncoder((8, 30, 32), bs, n)
        out, offs, _, summary = enc.encode(d_in)
        assert summary.tolist() == [0, 0]
        h_offs = offs.cpu().numpy()
        streams = out[: int(h_offs[-1])].clone()
        d_offs = offs.clone()
        del enc, out, offs
        dec = rx.DeviceDecoder((8, 30, 32), bs, len(h_offs) - 1)

        def sync(fn):
            fn()
            torch.cuda.synchronize()
        whole = clocked(lambda: sync(lambda: dec.decode(streams, d_offs, length=n)), repeats)
        say(f"block size {bs}: decode() of everything              {cell(whole)}")
        for r, ranges in range_sets(n, np.random.default_rng(bs)).items():
            got, where = dec.decode_ranges(streams, h_offs, n, ranges)
            assert all(torch.equal(got[w: w + k], d_in[s: s + k]) for w, (s, k) in zip(where, ranges))
            one = clocked(lambda: sync(lambda: dec.decode_ranges(streams, h_offs, n, ranges, out=got)), repeats)
            say(f"  {r:3d} ranges: one decode_ranges {cell(one)}")
        del dec, streams
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--device-gib", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parts", default="123")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_reads.txt"))
    a = ap.parse_args()
    import torch
    import redux_amd as rx
    from redux_amd import api, container
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    say(f"{rx.version()}  {torch.cuda.get_device_name(0)}  kernel {rx.api._lib.lib().redux_segment_copy_kernel_name().decode()}")
    say()
    if "1" in a.parts:
        copies(torch, rx, api, a.repeats)
    if "2" in a.parts:
        containers(torch, rx, container, a.gib, a.repeats)
    if "3" in a.parts:
        device(torch, rx, a.device_gib, a.repeats)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
