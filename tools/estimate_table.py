"""Size estimates on an MI355X: what k_block_cost costs next to the passes it stands beside, and how close the estimates
of every model come to the containers the models really write.

    python tools/estimate_table.py [--gib 4] [--repeats 5] [--zipf-mib 16] > profiles/estimate.txt

Part 1, on --gib GiB of iid and of Zipf bytes generated in HBM, blocks of 64 KiB at (8, 30, 32): k_block_cost
(redux_block_cost_dev), k_byte_hist (redux_histogram_dev) and the adaptive encoder (its coder kernels alone, and the whole
call with compaction) on the same buffer in the same run; each figure is the median of --repeats timed calls after one
untimed call, with the range, from HIP events around the C call.
Part 2, for --zipf-mib MiB of the Zipf bytes and every file under tests/golden/corpora: container.estimate_bytes beside the
length of container.compress_bytes for every candidate model, the model `auto` chose, and whether that was the smallest.
No rate or hit count is fixed in advance: the lines say what was measured.  profiles/estimate.txt is this output."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def line(what, nbytes, t):
    med, lo, hi = t
    print(f"  {what:52s} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f}; {nbytes / med / 1e6:7.1f} GB/s)")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--zipf-mib", type=int, default=16)
    a = ap.parse_args()
    import torch
    import redux_amd as rx
    from redux_amd import _lib, container
    L = _lib.lib()
    B, P = 65536, (8, 30, 32)
    cp = _lib.Params(*P)
    n = a.gib << 30
    print(f"{rx.version()}  source {L.redux_source_hash().decode()}  {torch.cuda.get_device_name(0)}")
    print(f"part 1: {a.gib} GiB in HBM, blocks of {B} bytes, parameters {P}, median of {a.repeats} after one warm-up call")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    enc = rx.DeviceEncoder(P, B, n)
    counts = torch.zeros(256, dtype=torch.int64, device="cuda:0")
    bits = torch.zeros(n // B, dtype=torch.float64, device="cuda:0")
    d_in = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    zipf_head = None
    for name, gen in (("iid", rx.gen_iid), ("zipf", rx.gen_zipf)):
        gen(n, out=d_in)
        torch.cuda.synchronize()
        print(f" {name}:")
        ptr = C.c_void_p(d_in.data_ptr())
        hist = line("k_byte_hist (redux_histogram_dev)", n,
                    timed(torch, lambda: L.redux_histogram_dev(ptr, n, C.c_void_p(counts.data_ptr()), None, 0, s), a.repeats))
        cost = line("k_block_cost (redux_block_cost_dev)", n,
                    timed(torch, lambda: L.redux_block_cost_dev(C.byref(cp), ptr, n, B, C.c_void_p(bits.data_ptr()), s), a.repeats))
        line("adaptive encode, coder kernels (encode_slots)", n, timed(torch, lambda: enc.encode_slots(d_in), a.repeats))
        line("adaptive encode, whole call (DeviceEncoder.encode)", n, timed(torch, lambda: enc.encode(d_in), a.repeats))
        _, offs, _, summ = enc.encode(d_in)
        torch.cuda.synchronize()
        assert summ.tolist() == [0, 0]
        est = float(bits.sum().item()) / 8 + 2.5 * (n // B)
        print(f"  k_block_cost / k_byte_hist = {cost / hist:.2f}; estimated streams {est:.0f} bytes, coded {int(offs[-1])} bytes"
              f" (difference {int(offs[-1]) - est:+.0f} over {n // B} blocks)")
        if name == "zipf":
            zipf_head = d_in[: a.zipf_mib << 20].cpu().numpy().tobytes()
    del enc, d_in, bits
    torch.cuda.empty_cache()

    print(f"part 2: estimated / actual container bytes per model, blocks of {B} bytes; * = the smallest actual; auto = the model"
          " `auto` chose")
    inputs = [(f"zipf {a.zipf_mib} MiB", zipf_head)]
    top = os.path.join(ROOT, "tests", "golden", "corpora")
    for d in sorted(os.listdir(top)):
        for f in sorted(os.listdir(os.path.join(top, d))):
            inputs.append((f"{d}/{f}", open(os.path.join(top, d, f), "rb").read()))
    hits, worst = 0, 0
    for name, data in inputs:
        est = container.estimate_bytes(data, B, P)
        actual = {m: len(container.compress_bytes(data, B, P, model=m)) for m in est}
        chosen = container.choose_model(est)
        auto = container.compress_bytes(data, B, P, model="auto")
        assert len(auto) == actual[chosen] and container.decompress_bytes(auto) == data
        best = min(actual.values())
        hit = actual[chosen] == best
        hits += hit
        worst = max(worst, max(abs(actual[m] - est[m]) for m in est))
        cells = "  ".join(f"{m} {est[m]}/{actual[m]}{'*' if actual[m] == best else ''}" for m in est)
        print(f"  {name:28s} {len(data):9d} B  {cells}  auto {chosen}{'' if hit else f' (+{actual[chosen] - best} B over the smallest)'}")
    print(f"auto wrote the smallest container on {hits} of {len(inputs)} inputs; largest |actual - estimate| of any model on any input:"
          f" {worst} bytes")
    print("not measured: profiler counters; element sizes above 1; block sizes other than 64 KiB")


if __name__ == "__main__":
    main()
