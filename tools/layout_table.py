"""Layout estimates on an MI355X: what k_layout_cost costs next to the composed path it replaces, and how close the
estimates of the eight layouts come to the containers the layouts really write.

    python tools/layout_table.py [--gib 4] [--repeats 5] > profiles/layout_cost.txt

Part 1, on --gib GiB of int64 timestamps generated in HBM, blocks of 64 KiB at (8, 30, 32), in one run on one buffer:
redux_layout_cost_dev for all eight layouts (and for each element size's two alone), and the composed path -- for each layout
k, redux_planes_dev / redux_delta_planes_dev into a scratch buffer (nothing for k = 0), then redux_block_cost_dev on it.  Each
figure is the median of --repeats timed calls after one untimed call, with the range, from HIP events around the C calls.
The two paths' results are compared before they are timed.
Part 2, for the five inputs of the layout table (tests/test_layout_auto_cpu.py) and every file under tests/golden/corpora:
container.estimate_layout_bytes beside the length of container.compress_bytes for each layout, the layout `auto` chose, and
|actual - estimate|.  No rate or pick is fixed in advance: the lines say what was measured.  profiles/layout_cost.txt is
this output."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    print(f"  {what:64s} {med:8.3f} ms  (range {lo:.3f} .. {hi:.3f}; {nbytes / med / 1e6:7.1f} GB/s of input)")
    return med


def name_of(key):
    return f"{key[0]}{'d' if key[1] else 'p'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    import redux_amd as rx
    from redux_amd import _lib, container
    from test_layout_auto_cpu import TABLE, table_input
    L = _lib.lib()
    B, P = 65536, (8, 30, 32)
    cp = _lib.Params(*P)
    n = a.gib << 30
    nb = n // B
    print(f"{rx.version()}  source {L.redux_source_hash().decode()}  {torch.cuda.get_device_name(0)}")
    print(f"part 1: {a.gib} GiB of int64 timestamps in HBM, blocks of {B} bytes, parameters {P}, median of {a.repeats} after one"
          " warm-up call")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    step = torch.randint(900, 1100, (n // 8,), dtype=torch.int64, device="cuda:0", generator=g)
    d_in = (1_700_000_000_000 + torch.cumsum(step, 0)).view(torch.uint8)
    del step
    scratch = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    bits = torch.full((8, nb), float("nan"), dtype=torch.float64, device="cuda:0")
    ref = torch.full((8, nb), float("nan"), dtype=torch.float64, device="cuda:0")
    ptr, tmp = C.c_void_p(d_in.data_ptr()), C.c_void_p(scratch.data_ptr())

    def fused(mask):
        assert L.redux_layout_cost_dev(C.byref(cp), ptr, n, B, mask, C.c_void_p(bits.data_ptr()), s) == _lib.OK

    def composed(ks):
        for k in ks:
            E, row = 1 << (k & 3), C.c_void_p(ref.data_ptr() + 8 * k * nb)
            if k == 0:
                assert L.redux_block_cost_dev(C.byref(cp), ptr, n, B, row, s) == _lib.OK
                continue
            call = L.redux_delta_planes_dev if k >= 4 else L.redux_planes_dev
            assert call(ptr, tmp, n, B, E, 0, s) == _lib.OK
            assert L.redux_block_cost_dev(C.byref(cp), tmp, n, B, row, s) == _lib.OK

    fused(0xFF)
    composed(range(8))
    torch.cuda.synchronize()
    print(f"  largest |k_layout_cost - composed| over 8 x {nb} blocks: {float((bits - ref).abs().max().item()):.3g} bits;"
          f" kernels: {', '.join(L.redux_layout_cost_kernel_name_at(ptr, n, B, k).decode() for k in range(4))}")
    all8 = line("k_layout_cost, all eight layouts (redux_layout_cost_dev 0xff)", n, timed(torch, lambda: fused(0xFF), a.repeats))
    for e in range(4):
        line(f"  element size {1 << e} alone, plain and delta (mask {0x11 << e:#04x})", n,
             timed(torch, lambda: fused(0x11 << e), a.repeats))
    line("  layout 0 alone (mask 0x01)", n, timed(torch, lambda: fused(1), a.repeats))
    comp = line("composed: 7 transforms into scratch + 8 x redux_block_cost_dev", n,
                timed(torch, lambda: composed(range(8)), a.repeats))
    line("  of which: redux_block_cost_dev on the input (layout 0)", n, timed(torch, lambda: composed([0]), a.repeats))
    line("  of which: redux_delta_planes_dev E = 8 + redux_block_cost_dev (layout 7)", n,
         timed(torch, lambda: composed([7]), a.repeats))
    print(f"  k_layout_cost / composed = {all8 / comp:.3f}")
    del d_in, scratch, bits, ref
    torch.cuda.empty_cache()

    print(f"part 2: estimated / actual container bytes per layout (element size, p = plain, d = delta), blocks of {B} bytes;"
          " * = the smallest actual; auto = the layout `auto` chose")
    inputs = [(name, table_input(name).tobytes()) for name in TABLE]
    top = os.path.join(ROOT, "tests", "golden", "corpora")
    for d in sorted(os.listdir(top)):
        for f in sorted(os.listdir(os.path.join(top, d))):
            inputs.append((f"{d}/{f}", open(os.path.join(top, d, f), "rb").read()))
    hits, worst, worst_rel = 0, 0, 0.0
    for name, data in inputs:
        est = container.estimate_layout_bytes(data, B, P)
        actual = {k: len(container.compress_bytes(data, B, P, k[0], filter=k[1])) for k in est}
        chosen = container.choose_layout(est)
        auto = container.compress_bytes(data, B, P, None, layout="auto")
        assert len(auto) == actual[chosen] and container.decompress_bytes(auto) == data
        best = min(actual.values())
        hit = actual[chosen] == best
        hits += hit
        err = max(abs(actual[k] - est[k]) for k in est)
        blocks = max(1, -(-len(data) // B))
        worst, worst_rel = max(worst, err), max(worst_rel, err / (2 * blocks + 1))
        cells = "  ".join(f"{name_of(k)} {est[k]}/{actual[k]}{'*' if actual[k] == best else ''}" for k in est)
        print(f"  {name:24s} {len(data):8d} B  {cells}  auto {name_of(chosen)}  max |actual - estimate| {err}"
              f"{'' if hit else f'  (+{actual[chosen] - best} B over the smallest)'}")
    print(f"auto wrote the smallest container on {hits} of {len(inputs)} inputs; largest |actual - estimate| of any layout on any"
          f" input: {worst} bytes, {worst_rel:.2f} of its bound 2 nblocks + 1")
    print("not measured: profiler counters (whether the delta wave's loads hit the CU's cache); block sizes other than 64 KiB")


if __name__ == "__main__":
    main()
