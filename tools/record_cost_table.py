#!/usr/bin/env python3
"""Record estimates, measured in one GPU run (results: profiles/record_cost.txt).

On `--gib` GiB (default 4) at 64 KiB blocks of imu23 repeated and of ticks20 repeated, the two GENERATED tables of packed
structs of tests/test_record_cpu.py, every entry warmed up once and then taken in turn in every round (device events; per
entry the median, the fastest and the slowest; the clocks are not touched):

  (a) per candidate  for R = 3, 12, 20, 23, 64, 255, 256: redux_record_cost_dev over {(R, plain), (R, delta)} on every frame
                     (k_record_cost, no transformed copy) next to what it replaces: two redux_record_planes_dev into a scratch
                     buffer, each followed by redux_block_cost_dev.  THE CONDITION: the fused call takes less time than the
                     composed one in every row; a row that misses it says MISS.  The two results are compared block by block.
  (b) stages         stage 1 of api.choose_record (all 510 candidates on about 64 blocks each), stage 2 (the four finalists
                     on every frame, and the plain bytes) and the whole choice with its sums and read-backs, next to the
                     adaptive encoder's coder kernel on the chosen layout of the same bytes (DeviceEncoder.encode_slots).
                     Reported, not gated.
  (c) one counter    the rows of (a) on a buffer of zeros: every lane of the fast kernel adds to the same few counters.

  (d) choices        what api.choose_record picks, its estimate, and the container compress_bytes(record_size="auto") writes,
                     for the two tables at `--records` records (default 4,000,000) and for kennedy.xls, alice29.txt and geo of
                     tests/golden/corpora.  The tables are generated; the three files are the only recorded inputs.

usage: python tools/record_cost_table.py [--gib N] [--records N] [--rounds R] [--out FILE]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import redux_amd as rx  # noqa: E402
from redux_amd import _lib, api, container  # noqa: E402
from tools.record_table import B, PARAMS, SIZES, generated_tables, measure  # noqa: E402

CORPORA = os.path.join(ROOT, "tests", "golden", "corpora")
FILES = (("kennedy.xls", "canterbury"), ("alice29.txt", "canterbury"), ("geo", "calgary"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=int, default=4)
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = a.gib << 30
    nb = n // B
    L = _lib.lib()
    cp = _lib.Params(*PARAMS)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    say(f"# {rx.version()}  source hash {L.redux_source_hash().decode()}  device {torch.cuda.get_device_name(0)}")
    say(f"# timings: {a.gib} GiB = {nb} blocks of 64 KiB; one warm-up, then {a.rounds} rounds of every entry in turn; "
        "ms: median [fastest .. slowest]; the clocks were not touched")
    tables = generated_tables(a.records)
    scratch = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    fused_bits = {R: torch.empty((2, nb), dtype=torch.float64, device="cuda:0") for R in SIZES}
    composed_bits = {R: torch.empty((2, nb), dtype=torch.float64, device="cuda:0") for R in SIZES}
    h_deltas = np.array([0, 1], dtype=np.uint8)
    misses = []

    def pair_rows(tag, src):
        """(a) / (c): fused against composed for every R of SIZES on src"""
        def fused(R):
            h = np.array([R, R], dtype=np.uint32)
            api._raise(L.redux_record_cost_dev(C.byref(cp), C.c_void_p(src.data_ptr()), n, B, h.ctypes.data, h_deltas.ctypes.data, 2, 0,
                                               C.c_void_p(fused_bits[R].data_ptr()), stream))

        def composed(R):
            for F in (0, 1):
                api.record_planes(src, R, B, delta=bool(F), out=scratch)
                api._raise(L.redux_block_cost_dev(C.byref(cp), C.c_void_p(scratch.data_ptr()), n, B,
                                                  C.c_void_p(composed_bits[R][F].data_ptr()), stream))
        runs = {}
        for R in SIZES:
            runs[f"R={R} fused"] = lambda R=R: fused(R)
            runs[f"R={R} composed"] = lambda R=R: composed(R)
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        for R in SIZES:
            f, c = ms[f"R={R} fused"], ms[f"R={R} composed"]
            ratio = med[f"R={R} fused"] / med[f"R={R} composed"]
            diff = float((fused_bits[R] - composed_bits[R]).abs().max().item())
            if ratio >= 1.0:
                misses.append(f"{tag} R={R}")
            say(f"{tag} R={R}: fused {med[f'R={R} fused']:.3f} ms [{f[0]:.3f} .. {f[-1]:.3f}]  composed {med[f'R={R} composed']:.3f} ms "
                f"[{c[0]:.3f} .. {c[-1]:.3f}]  {ratio:.2f} x composed  {'ok' if ratio < 1.0 else 'MISS'}  max |difference| = {diff:.3g} bits")

    for name, (x, R0) in tables.items():
        piece = torch.from_numpy(x).cuda()
        src = piece.repeat((n + piece.numel() - 1) // piece.numel())[:n].contiguous()
        del piece
        say(f"# (a) {name} repeated: redux_record_cost_dev over (R, plain) and (R, delta), every frame, against 2 x (record_planes + block_cost)")
        pair_rows(f"(a) {name}", src)
        # ---- (b) ----
        cands = api.record_candidates()
        costed = {c: api.record_cost_sample(n, B, c[0], api.RECORD_SAMPLE_BLOCKS)[2] for c in cands}
        state, chosen = {}, []

        def stage1():
            with torch.cuda.device(src.device):
                state["est"] = api._record_estimates(torch, L, cp, src, B, cands, api.RECORD_SAMPLE_BLOCKS)

        def stage2():
            with torch.cuda.device(src.device):
                fin = api.record_finalists(state["est"], costed)
                state["exact"] = api._record_estimates(torch, L, cp, src, B, fin, 0)
                bits = api._device_block_cost(torch, L, cp, src, B)
                state["plain"] = float(bits.sum().cpu())
        choice, est = api.choose_record(src, B, PARAMS)
        t = src if choice is None else api.record_planes(src, choice[0], B, delta=choice[1] is not None)  # what the coder sees
        enc = rx.DeviceEncoder(PARAMS, B, n)
        runs = {"stage 1 (510 candidates, 64 blocks each)": stage1, "stage 2 (4 finalists, every frame; the plain bytes)": stage2,
                "choose_record": lambda: chosen.append(api.choose_record(src, B, PARAMS)[0]), "coder forward": lambda: enc.encode_slots(t)}
        ms = measure(runs, a.rounds)
        med = {k: v[len(v) // 2] for k, v in ms.items()}
        for k, v in ms.items():
            tail = "" if k == "coder forward" else f"  {med[k] / med['coder forward']:.2f} x coder"
            say(f"(b) {name} {k}: {med[k]:.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]{tail}")
        say(f"(b) {name}: choose_record picked {sorted(set(chosen), key=str)} among {sorted((k for k in est if k is not None))} and the plain bytes; "
            f"stage 1 costed {sum(costed.values()) / 2 ** 30:.2f} GiB of input over the 510 candidates")
        del enc, t, src
        torch.cuda.empty_cache()
    src = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    say("# (c) a buffer of zeros: the rows of (a)")
    pair_rows("(c) zeros", src)
    del src, scratch
    torch.cuda.empty_cache()
    say("# the condition (fused < composed in every row of (a) and (c)): " + ("met by every row" if not misses else "MISSED by " + ", ".join(misses)))
    # ---- (d) ----
    say(f"# (d) choices at 64 KiB blocks: GENERATED tables of {a.records} records; kennedy.xls, alice29.txt and geo as recorded")
    inputs = [(name, x.tobytes()) for name, (x, _) in tables.items()]
    inputs += [(f, open(os.path.join(CORPORA, d, f), "rb").read()) for f, d in FILES]
    for name, data in inputs:
        choice, est = api.choose_record(data, B, PARAMS)
        blob = container.compress_bytes(data, B, PARAMS, record_size="auto")
        plain = container.compress_bytes(data, B, PARAMS)
        nbk = max(1, -(-len(data) // B))
        over = container.overhead_bytes("adaptive", nbk)
        assert container.decompress_bytes(blob) == data
        say(f"(d) {name} ({len(data)} bytes): choice {choice}, estimated container {est[choice] + over}, written {len(blob)}; "
            f"plain estimated {est[None] + over}, written {len(plain)}; {len(blob) / len(plain):.3f} of plain")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
