"""Context-static coding on an MI355X: throughput and ratio against the static and adaptive coders on the same buffer.

    python tools/measure_context_static.py [--blocks 65536] [--repeats 5] [--only-context]

The buffer is tests/golden/corpora/large/bible.txt tiled to --blocks blocks of 64 KiB, device-resident.  Every figure is the
median of --repeats timed calls after one untimed call, with the range, from HIP events around the C call (table check and
compaction included).  Prints one line per figure; profiles/r12_context_static.txt is this output.
The library picks the coders' waves per workgroup from the launch size.  To time the values it does not pick, build variant
libraries with -DREDUX_CTX_WAVES=4 / 8 / 16 and run this tool with REDUX_LIB=<variant> --only-context: the first line
shows which library answered.
Not measured here: profiler counters, and launches smaller than the chip."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

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
    print(f"{what:58s} {nbytes / med / 1e6:8.1f} GB/s  (median of {med:.3f} ms; range {nbytes / hi / 1e6:.1f} .. {nbytes / lo / 1e6:.1f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only-context", action="store_true", help="the context-static coder alone (variant libraries)")
    a = ap.parse_args()
    import torch
    import redux_amd as rx
    from redux_amd import _lib
    L = _lib.lib()
    B, P = 65536, (8, 30, 32)
    n = a.blocks * B
    text = np.fromfile(os.path.join(ROOT, "tests", "golden", "corpora", "large", "bible.txt"), dtype=np.uint8)
    d_text = torch.from_numpy(text).cuda()
    d_in = d_text.repeat(-(-n // len(text)))[:n].contiguous()
    del d_text
    print(f"{rx.version()}  source {L.redux_source_hash().decode()}  {torch.cuda.get_device_name(0)}")
    print(f"buffer: bible.txt tiled, {a.blocks} x {B} bytes, repeats {a.repeats}")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    adaptive_bytes = static_bytes = 0
    if not a.only_context:
        # histograms
        c1 = torch.zeros(256, dtype=torch.int64, device="cuda:0")
        c2 = torch.zeros(65536, dtype=torch.int64, device="cuda:0")
        line("k_byte_hist (redux_histogram_dev)", n, timed(torch, lambda: L.redux_histogram_dev(C.c_void_p(d_in.data_ptr()), n, C.c_void_p(c1.data_ptr()), None, 0, s), a.repeats))
        line("k_context_hist (redux_context_histogram_dev)", n, timed(torch, lambda: L.redux_context_histogram_dev(C.c_void_p(d_in.data_ptr()), n, B, C.c_void_p(c2.data_ptr()), s), a.repeats))

        # static coder on the same buffer
        cp = _lib.Params(*P)
        st = rx.DeviceStaticCoder.from_data(d_in, P, B, n)
        print("static encode kernel:", L.redux_static_encode_kernel_name(C.byref(cp), st.cum, n, B).decode())
        print("static decode kernel:", L.redux_static_decode_kernel_name(C.byref(cp), st.cum, a.blocks).decode(), "(the dispatch's choice, not forced)")
        out, offs, _, summ = st.encode(d_in)
        torch.cuda.synchronize()
        assert summ.tolist() == [0, 0]
        static_bytes = int(offs[-1])
        line("static encode (redux_static_encode_blocks_dev)", n, timed(torch, lambda: st.encode(d_in), a.repeats))
        line("static decode (redux_static_decode_blocks_dev)", n, timed(torch, lambda: st.decode(out[:static_bytes], offs), a.repeats))
        del st, out

        # adaptive, for the ratio
        enc = rx.DeviceEncoder(P, B, n)
        _, aoffs, _, summ = enc.encode(d_in)
        torch.cuda.synchronize()
        adaptive_bytes = int(aoffs[-1])
        line("adaptive encode (DeviceEncoder)", n, timed(torch, lambda: enc.encode(d_in), a.repeats))
        del enc

    # context-static
    cs = rx.DeviceContextStaticCoder.from_data(d_in, P, B, n)
    out, offs, _, summ = cs.encode(d_in)
    torch.cuda.synchronize()
    assert summ.tolist() == [0, 0]
    ctx_bytes = int(offs[-1])
    back, _, _, dsum = cs.decode(out[:ctx_bytes], offs)
    torch.cuda.synchronize()
    assert dsum.tolist() == [0, 0] and torch.equal(back, d_in)
    line("context-static encode (redux_context_static_encode_dev)", n, timed(torch, lambda: cs.encode(d_in), a.repeats))
    line("context-static decode (redux_context_static_decode_dev)", n, timed(torch, lambda: cs.decode(out[:ctx_bytes], offs), a.repeats))
    if a.only_context:
        print(f"ratio (streams / input): context-static {ctx_bytes / n:.4f}")
        return
    print(f"ratio (streams / input): adaptive {adaptive_bytes / n:.4f}  static {static_bytes / n:.4f}  context-static {ctx_bytes / n:.4f}"
          f"  (context-static / adaptive {ctx_bytes / adaptive_bytes:.4f}, / static {ctx_bytes / static_bytes:.4f})")
    print("not measured: profiler counters; launches smaller than the chip; a forced k_decode_static")


if __name__ == "__main__":
    main()
