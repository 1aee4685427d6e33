"""Mixed layouts on an MI355X: what a layout per unit of 8 blocks saves on files of several element types, from written
containers, and what the transform and the choice cost next to the whole-buffer transforms.

    python tools/mixed_table.py [--gib 4] [--repeats 5] > profiles/mixed_layout.txt

Part 1, for the inputs of the mixed-layout table (tests/test_mixed_cpu.py: the concatenation timestamps + bf16 + fp32 + text,
the same behind 100,000 bytes of text, and the four parts alone), blocks of 64 KiB at (8, 30, 32): the container every single
layout writes, the one `--layout auto` writes, the one `--layout mixed` writes with its estimate and its unit table, and the
ratio mixed / auto.  Every mixed container is decoded and compared.
Part 2, on --gib GiB of int64 timestamps generated in HBM, in one run on one pair of buffers, each figure the median of
--repeats timed calls after one untimed call, with the range, from HIP events around the C calls, the two alternating layout
by layout: k_mixed_planes on a uniform table of k against the whole-buffer transform of layout k, in both directions; both
directions on the table arange % 8; and cost + choose + transform end to end (redux_layout_cost_dev, redux_mixed_choose_dev,
redux_mixed_layout_dev on one stream, no host synchronisation between them).  The outputs of the two paths are compared before
they are timed.  No figure is fixed in advance: the lines say what was measured.  profiles/mixed_layout.txt is this output."""
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


def cell(t):
    return f"{t[0]:7.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-containers", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import redux_amd as rx
    from redux_amd import _lib, container
    from test_mixed_cpu import PARTS, mixed_input
    L = _lib.lib()
    B, P = 65536, (8, 30, 32)
    cp = _lib.Params(*P)
    print(f"{rx.version()}  source {L.redux_source_hash().decode()}  {torch.cuda.get_device_name(0)}")

    if not a.skip_containers:
        print(f"part 1: written containers, blocks of {B} bytes, parameters {P}; best single = the smallest of the eight layouts'"
              " containers")
        for name in ("concat", "shifted") + PARTS:
            data = mixed_input(name).tobytes()
            nb = max(1, -(-len(data) // B))
            single = {k: len(container.compress_bytes(data, B, P, k[0], filter=k[1])) for k in rx.LAYOUTS}
            best = min(single, key=lambda k: single[k])
            auto = container.compress_bytes(data, B, P, None, layout="auto")
            est = container.estimate_layout_bytes(data, B, P, None, mixed=True)["mixed"]
            mixed = container.compress_bytes(data, B, P, None, layout="mixed")
            assert container.decompress_bytes(mixed) == data
            table = container.unit_layouts(mixed)
            print(f"  {name:10s} {len(data):8d} B {nb:3d} blocks {len(table):2d} units  best single {single[best]:8d} {best}  auto"
                  f" {len(auto):8d}  mixed {len(mixed):8d} (estimate {est}, off by {len(mixed) - est}; bound {2 * nb + 1})  mixed / auto"
                  f" {len(mixed) / len(auto):.4f}  table {''.join(str(int(k)) for k in table)}")

    n = a.gib << 30
    nunits = n // (8 * B)
    nb = n // B
    print(f"part 2: {a.gib} GiB of int64 timestamps in HBM, blocks of {B} bytes, {nunits} units, median of {a.repeats} after one"
          " warm-up call (range)")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    step = torch.randint(900, 1100, (n // 8,), dtype=torch.int64, device="cuda:0", generator=g)
    d_in = (1_700_000_000_000 + torch.cumsum(step, 0)).view(torch.uint8)
    del step
    d_a = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    d_b = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    src, pa, pb = C.c_void_p(d_in.data_ptr()), C.c_void_p(d_a.data_ptr()), C.c_void_p(d_b.data_ptr())
    d_table = torch.zeros(nunits, dtype=torch.uint8, device="cuda:0")
    ptab = C.c_void_p(d_table.data_ptr())

    def mixed(x, y, inverse):
        assert L.redux_mixed_layout_dev(x, y, n, B, ptab, inverse, s) == _lib.OK

    def single(k, x, y, inverse):
        if k == 0:
            d_a.copy_(d_in) if y is pa else d_b.copy_(d_a)
            return
        call = L.redux_delta_planes_dev if k >= 4 else L.redux_planes_dev
        assert call(x, y, n, B, 1 << (k & 3), inverse, s) == _lib.OK

    print(f"  kernels: {L.redux_mixed_kernel_name_at(src, pa, n, B, 0).decode()}, {L.redux_mixed_kernel_name_at(pa, pb, n, B, 1).decode()}")
    print("  layout k, forward: k_mixed_planes on a uniform table | the whole-buffer transform; then the two inverses")
    for k in range(8):
        d_table.fill_(k)
        single(k, src, pa, 0)
        mixed(src, pb, 0)
        torch.cuda.synchronize()
        assert torch.equal(d_a, d_b), k
        mixed(pa, pb, 1)
        torch.cuda.synchronize()
        assert torch.equal(d_b, d_in), k
        f_single = timed(torch, lambda: single(k, src, pa, 0), a.repeats)
        f_mixed = timed(torch, lambda: mixed(src, pa, 0), a.repeats)
        i_single = timed(torch, lambda: single(k, pa, pb, 1), a.repeats)
        i_mixed = timed(torch, lambda: mixed(pa, pb, 1), a.repeats)
        print(f"  k = {k}  forward {cell(f_mixed)} | {cell(f_single)}   inverse {cell(i_mixed)} | {cell(i_single)}")
    d_table.copy_(torch.arange(nunits, device="cuda:0") % 8)
    mixed(src, pa, 0)
    mixed(pa, pb, 1)
    torch.cuda.synchronize()
    assert torch.equal(d_b, d_in)
    print(f"  table arange % 8: forward {cell(timed(torch, lambda: mixed(src, pa, 0), a.repeats))}   inverse"
          f" {cell(timed(torch, lambda: mixed(pa, pb, 1), a.repeats))}")
    bits = torch.empty((8, nb), dtype=torch.float64, device="cuda:0")
    pbits = C.c_void_p(bits.data_ptr())

    def end_to_end():
        assert L.redux_layout_cost_dev(C.byref(cp), src, n, B, 0xFF, pbits, s) == _lib.OK
        assert L.redux_mixed_choose_dev(pbits, nb, 0xFF, ptab, None, s) == _lib.OK
        mixed(src, pa, 0)

    def cost_only():
        assert L.redux_layout_cost_dev(C.byref(cp), src, n, B, 0xFF, pbits, s) == _lib.OK

    def choose_only():
        assert L.redux_mixed_choose_dev(pbits, nb, 0xFF, ptab, None, s) == _lib.OK

    print(f"  cost + choose + transform end to end {cell(timed(torch, end_to_end, a.repeats))}; of which the costs"
          f" {cell(timed(torch, cost_only, a.repeats))}, the choice {cell(timed(torch, choose_only, a.repeats))}")
    print(f"  the chosen table holds layouts {sorted(set(d_table.cpu().numpy().tolist()))}")
    print("not measured: profiler counters; block sizes other than 64 KiB; the coder behind the transform (unchanged code)")


if __name__ == "__main__":
    main()
