"""The host contract of the layered calls, as data: every workspace and bound value, every kernel-name string and the return
code of every refusal that is decided before any HIP call, for the planes, delta, stored, static, plane-static,
segment-static and context-static families, and for the adaptive coder's own entry points under them: the plain, split,
`_v`, base and const calls, over every parameter class (8-bit, the lock-step widths, general parameters).

    python tools/record_layer_contract.py [--lib PATH] > tests/golden/layer_contract.json
    python tools/record_layer_contract.py [--lib PATH] --part adaptive > tests/golden/adaptive_contract.json

record the two parts (the layered families; the adaptive coder's own calls) from a library (the product's by default); tests/test_layer_contract_cpu.py runs the same collection on the
library under test and compares.  Record the fixture from the library of the commit whose behaviour is to be kept, never
from the change that is being checked against it.

The refusal rows pass dummy device pointers, so every row must be one the library refuses before it touches the runtime:
collect() asserts that no row returns OK or IO_ERROR (what a HIP call gives on a machine without a GPU), and main() hides
the GPUs from the process, so that a row that does reach the runtime fails there instead of launching on a dummy pointer.
"""
import ctypes as C
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(path=None):
    """The library with the signatures of redux_amd/_lib.py, without importing the package (and torch with it)."""
    spec = importlib.util.spec_from_file_location("_redux_lib_decl", os.path.join(ROOT, "redux_amd", "_lib.py"))
    decl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(decl)
    L = C.CDLL(path or decl.LIB_PATH)
    for name, (res, args) in decl.SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L, decl


PARAMS = [(8, 30, 32), (8, 14, 16), (8, 20, 24)]
BLOCKS = [512, 1040, 4096, 65536]
ES = [1, 2, 4, 8]
TOTALS = [4096, 60000, 200000]            # a lookup-decoder total, one above 2^15, one that needs the quotient fix-up
OK, IO_ERROR = 0, 3


def lengths(bs):
    return [0, 1, bs, 67 * bs + 5, 4096 * bs]


# the adaptive coder's own grid ("adaptive/..." rows): the 8-bit triples, a lock-step width below 8 and one above, general
# parameters (code_bits > 32); a block above 64 KiB and one of 3 MiB, which the small-grid encoder codes in windows; lengths
# on both sides of its limit of 2048 blocks
APARAMS = PARAMS + [(4, 20, 24), (12, 20, 32), (8, 24, 40)]
ABLOCKS = BLOCKS + [1 << 17, 3 << 20]
AES = [1, 4]


def alengths(bs):
    return [0, 1, 67 * bs + 5, 2048 * bs, 2049 * bs, 4096 * bs]


def table(total):
    return (C.c_uint32 * 258)(*(list(range(257)) + [total]))


def sizes(L, decl, part):
    """name -> values over PARAMS x BLOCKS x [ES] x lengths, in that nesting order ("adaptive/" rows: the adaptive grid)."""
    return adaptive_sizes(L, decl) if part == "adaptive" else layered_sizes(L, decl)


def layered_sizes(L, decl):
    out = {}
    plain = ["redux_encode_bound", "redux_encode_workspace_bytes", "redux_static_encode_bound", "redux_static_encode_workspace_bytes",
             "redux_plane_static_encode_bound", "redux_segment_static_encode_bound", "redux_context_static_encode_bound",
             "redux_context_static_encode_workspace_bytes"]
    by_e = ["redux_encode_planes_workspace_bytes", "redux_decode_planes_workspace_bytes", "redux_encode_delta_workspace_bytes",
            "redux_decode_delta_workspace_bytes", "redux_encode_stored_workspace_bytes", "redux_decode_stored_workspace_bytes",
            "redux_plane_static_encode_workspace_bytes", "redux_plane_static_decode_workspace_bytes",
            "redux_segment_static_encode_workspace_bytes", "redux_segment_static_decode_workspace_bytes"]
    grid = [(decl.Params(*w), bs) for w in PARAMS for bs in BLOCKS]
    for n in plain:
        out[n] = [getattr(L, n)(C.byref(p), ln, bs) for p, bs in grid for ln in lengths(bs)]
    for n in ("redux_decode_workspace_bytes", "redux_context_static_decode_workspace_bytes"):   # by block count
        out[n] = [getattr(L, n)(C.byref(p), L.redux_block_count(ln, bs), bs) for p, bs in grid for ln in lengths(bs)]
    for n in by_e:
        out[n] = [getattr(L, n)(C.byref(p), ln, bs, E) for p, bs in grid for E in ES for ln in lengths(bs)]
    for k in (1, 2):                                                                               # segments of 64 E k blocks
        out["redux_segment_static_build_encode_workspace_bytes/k%d" % k] = [
            L.redux_segment_static_build_encode_workspace_bytes(C.byref(p), ln, bs, E, 64 * E * k)
            for p, bs in grid for E in ES for ln in lengths(bs)]
    out["redux_segment_static_table_count/k1"] = [L.redux_segment_static_table_count(L.redux_block_count(ln, bs), E, 64 * E)
                                                  for bs in BLOCKS for E in ES for ln in lengths(bs)]
    return out


def adaptive_sizes(L, decl):
    out = {}
    agrid = [(decl.Params(*w), bs) for w in APARAMS for bs in ABLOCKS]
    for n in ("redux_encode_bound", "redux_encode_workspace_bytes"):
        out["adaptive/" + n] = [getattr(L, n)(C.byref(p), ln, bs) for p, bs in agrid for ln in alengths(bs)]
    out["adaptive/redux_encode_slot_bytes"] = [L.redux_encode_slot_bytes(C.byref(p), bs) for p, bs in agrid]
    out["adaptive/redux_decode_workspace_bytes"] = [L.redux_decode_workspace_bytes(C.byref(p), nb, bs) for p, bs in agrid
                                                    for nb in [0] + [L.redux_block_count(ln, bs) for ln in alengths(bs)]]
    for n in ("redux_encode_const_workspace_bytes", "redux_decode_const_workspace_bytes", "redux_encode_base_workspace_bytes",
              "redux_decode_base_workspace_bytes"):
        out["adaptive/" + n] = [getattr(L, n)(C.byref(p), ln, bs, E) for p, bs in agrid for E in AES for ln in alengths(bs)]
    return out


def names(L, decl, part):
    """name -> indices into `strings`, over PARAMS x TOTALS x BLOCKS x [ES] x lengths ("adaptive/" rows: the adaptive grid)."""
    strings, out = [], {}

    def idx(b):
        s = b.decode()
        if s not in strings:
            strings.append(s)
        return strings.index(s)

    (adaptive_names if part == "adaptive" else layered_names)(L, decl, idx, out)
    return {"strings": strings, "rows": out}


def layered_names(L, decl, idx, out):
    grid = [(decl.Params(*w), t, bs) for w in PARAMS for t in TOTALS for bs in BLOCKS]
    out["redux_static_encode_kernel_name"] = [idx(L.redux_static_encode_kernel_name(C.byref(p), table(t), ln, bs))
                                              for p, t, bs in grid for ln in lengths(bs)]
    out["redux_static_decode_kernel_name"] = [idx(L.redux_static_decode_kernel_name(C.byref(p), table(t), L.redux_block_count(ln, bs)))
                                              for p, t, bs in grid for ln in lengths(bs)]
    out["redux_plane_static_encode_kernel_name"] = [idx(L.redux_plane_static_encode_kernel_name(C.byref(p), t, ln, bs, E))
                                                    for p, t, bs in grid for E in ES for ln in lengths(bs)]
    out["redux_plane_static_decode_kernel_name"] = [idx(L.redux_plane_static_decode_kernel_name(C.byref(p), t, L.redux_block_count(ln, bs), E))
                                                    for p, t, bs in grid for E in ES for ln in lengths(bs)]
    for k in (1, 4, 8):
        out["redux_segment_static_encode_kernel_name/k%d" % k] = [
            idx(L.redux_segment_static_encode_kernel_name(C.byref(p), t, ln, bs, E, 64 * E * k))
            for p, t, bs in grid for E in ES for ln in lengths(bs)]
        out["redux_segment_static_decode_kernel_name/k%d" % k] = [
            idx(L.redux_segment_static_decode_kernel_name(C.byref(p), t, L.redux_block_count(ln, bs), E, 64 * E * k))
            for p, t, bs in grid for E in ES for ln in lengths(bs)]
    # the lane-offset refusal of the encoders: blocks of 2^26 bytes and more
    out["giant blocks"] = [idx(L.redux_static_encode_kernel_name(C.byref(decl.Params(8, 30, 32)), table(4096), 1, bs)) for bs in (1 << 25, 1 << 26)] + \
                          [idx(L.redux_plane_static_encode_kernel_name(C.byref(decl.Params(8, 30, 32)), 4096, 1, bs, E))
                           for bs in (1 << 23, 1 << 24, 1 << 25, 1 << 26) for E in ES]


def adaptive_names(L, decl, idx, out):
    # input 16-byte aligned and not; a workspace that holds the small-grid pairs area and one a byte short
    agrid = [(decl.Params(*w), bs) for w in APARAMS for bs in ABLOCKS]
    for tag, d_in in (("", ptr(1)), ("/unaligned", ptr(1) + 4)):
        out["adaptive/redux_encode_kernel_name" + tag] = [idx(L.redux_encode_kernel_name(C.byref(p), d_in, ln, bs))
                                                          for p, bs in agrid for ln in alengths(bs)]
    for tag, short in (("/fits", 0), ("/short", 1)):
        out["adaptive/redux_encode_kernel_name_ws" + tag] = [
            idx(L.redux_encode_kernel_name_ws(C.byref(p), ptr(1), ln, bs, L.redux_encode_workspace_bytes(C.byref(p), ln, bs) - short))
            for p, bs in agrid for ln in alengths(bs)]
    counts = lambda bs: [0] + [L.redux_block_count(ln, bs) for ln in alengths(bs)]
    out["adaptive/redux_decode_kernel_name_n"] = [idx(L.redux_decode_kernel_name_n(C.byref(p), ptr(2), bs, nb))
                                                  for p, bs in agrid for nb in counts(bs)]
    out["adaptive/redux_decode_kernel_name_table"] = [idx(L.redux_decode_kernel_name_table(C.byref(p), bs, nb))
                                                      for p, bs in agrid for nb in counts(bs)]


# ---- refusals ---------------------------------------------------------------------------------------------------------------
BS, E0 = 1040, 4
LEN = 67 * BS + 5                      # 68 blocks: more than one 64-block wave, no multiple of any E > 1, a ragged last block
NB = 68
COPY = (LEN + 16 + 255) // 256 * 256            # planes_copy_bytes of the input ...
DCOPY = (NB * BS + 16 + 255) // 256 * 256       # ... and of the decoders' plane buffer
BIG = 1 << 60
CTX_HEAD = 256 * 256 * 2 + 256


def ptr(i):
    return (1 << 40) + (i << 32)       # dummy device pointers: 256-aligned, far apart


def refusals(L, decl, part):
    good, bad, anyp, wide = decl.Params(8, 30, 32), decl.Params(8, 9, 16), decl.Params(12, 20, 32), decl.Params(8, 24, 40)
    P = {"good": C.byref(good), "bad": C.byref(bad), "any": C.byref(anyp), "wide": C.byref(wide), "null": None}
    tab, badtab = table(4096), (C.c_uint32 * 258)(*([1] + list(range(1, 257)) + [4096]))
    T = {"good": tab, "bad": badtab, "null": None}
    dec_ws = L.redux_decode_planes_workspace_bytes(P["good"], LEN, BS, E0)
    sto_dec_ws = lambda E: L.redux_decode_stored_workspace_bytes(P["good"], LEN, BS, E)
    st_ws = L.redux_static_encode_workspace_bytes(P["good"], LEN, BS)
    seg_cb = (L.redux_segment_static_table_count(NB, E0, 64 * E0) * 256 * 8 + 255) // 256 * 256

    # entry point -> (argument names in order, the values of a call that would run, the faults).  A fault is a dict of
    # overrides; `p` and `cum` name an entry of P / T.
    transform = (["src", "dst", "len", "bs", "E", "inverse", "stream"],
                 dict(src=ptr(1), dst=ptr(2), len=LEN, bs=BS, E=E0, inverse=0, stream=None),
                 {"null src": dict(src=None), "null dst": dict(dst=None), "block_size 0": dict(bs=0), "E 3": dict(E=3), "E 16": dict(E=16),
                  "in place": dict(dst=ptr(1)), "overlap": dict(dst=ptr(1) + 16), "inverse in place": dict(dst=ptr(1), inverse=1),
                  "E 3 and len 0": dict(E=3, len=0), "block_size 0 and len 0": dict(bs=0, len=0)})
    enc_layout = (["p", "d_in", "len", "bs", "E", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
                  dict(p="good", d_in=ptr(1), len=LEN, bs=BS, E=E0, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4), d_sum=ptr(5),
                       d_ws=ptr(6), ws_bytes=BIG, stream=None),
                  {"bad params": dict(p="bad"), "null params": dict(p="null"), "null workspace": dict(d_ws=None), "null input": dict(d_in=None),
                   "block_size 0": dict(bs=0), "E 3": dict(E=3), "E 16": dict(E=16), "below the copy": dict(ws_bytes=COPY - 1),
                   "no workspace bytes": dict(ws_bytes=0),
                   "E 1: null status": dict(E=1, d_st=None),
                   "E 1: no workspace bytes": dict(E=1, ws_bytes=0), "E 1: workspace not 256-aligned": dict(E=1, d_ws=ptr(6) + 16),
                   "E 3 and no workspace bytes": dict(E=3, ws_bytes=0), "null workspace and no workspace bytes": dict(d_ws=None, ws_bytes=0),
                   "bad params and E 3": dict(p="bad", E=3)})
    dec_layout = (["p", "d_in", "d_off", "out_len", "bs", "E", "d_out", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
                  dict(p="good", d_in=ptr(1), d_off=ptr(3), out_len=LEN, bs=BS, E=E0, d_out=ptr(2), d_sz=ptr(7), d_st=ptr(4), d_sum=ptr(5),
                       d_ws=ptr(6), ws_bytes=BIG, stream=None),
                  {"bad params": dict(p="bad"), "null params": dict(p="null"), "null workspace": dict(d_ws=None), "null offsets": dict(d_off=None),
                   "null sizes": dict(d_sz=None), "null status": dict(d_st=None), "null output": dict(d_out=None), "block_size 0": dict(bs=0),
                   "E 3": dict(E=3), "E 16": dict(E=16), "below the copy": dict(ws_bytes=DCOPY - 1), "below the full size": dict(ws_bytes=dec_ws - 1),
                   "E 1: below the full size": dict(E=1, ws_bytes=L.redux_decode_planes_workspace_bytes(P["good"], LEN, BS, 1) - 1),
                   "E 3 and no workspace bytes": dict(E=3, ws_bytes=0), "null status and no workspace bytes": dict(d_st=None, ws_bytes=0),
                   "bad params and null sizes": dict(p="bad", d_sz=None)})
    tables_enc_faults = {
        "bad params": dict(p="bad"), "general params": dict(p="any"), "total 100": dict(total=100), "total 2^31": dict(total=1 << 31),
        "E 3": dict(E=3), "E 16": dict(E=16), "block_size 0": dict(bs=0), "null tables": dict(d_cum=None), "null input": dict(d_in=None),
        "null status": dict(d_st=None), "null workspace": dict(d_ws=None), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
        "below the copy": dict(ws_bytes=COPY - 1), "no workspace bytes": dict(ws_bytes=0),
        "E 1: below the full size": dict(E=1, ws_bytes=st_ws - 1), "E 1: blocks of 2^26": dict(E=1, bs=1 << 26, len=1),
        "E 1: blocks of 2^26 and no workspace bytes": dict(E=1, bs=1 << 26, len=1, ws_bytes=0),
        "workspace not 256-aligned and below the copy": dict(d_ws=ptr(6) + 16, ws_bytes=COPY - 1),
        "general params and total 100": dict(p="any", total=100), "total 100 and E 3": dict(total=100, E=3)}
    tables_dec_faults = {
        "bad params": dict(p="bad"), "general params": dict(p="any"), "total 100": dict(total=100), "total 2^31": dict(total=1 << 31),
        "E 3": dict(E=3), "E 16": dict(E=16), "block_size 0": dict(bs=0), "null tables": dict(d_cum=None), "null workspace": dict(d_ws=None),
        "null offsets": dict(d_off=None), "null sizes": dict(d_sz=None), "null status": dict(d_st=None), "null output": dict(d_out=None),
        "below the copy": dict(ws_bytes=DCOPY - 1), "no workspace bytes": dict(ws_bytes=0),
        "null status and no workspace bytes": dict(d_st=None, ws_bytes=0), "general params and E 3": dict(p="any", E=3)}
    seg_faults = {"segment_blocks 0": dict(G=0), "segment_blocks 64": dict(G=64), "segment_blocks 64 E + 64": dict(G=64 * E0 + 64),
                  "segment_blocks 64 and null status": dict(G=64, d_st=None), "segment_blocks 64 and total 100": dict(G=64, total=100)}
    calls = {
        "redux_planes_dev": transform,
        "redux_delta_planes_dev": transform,
        "redux_encode_planes_dev": enc_layout,
        "redux_encode_delta_dev": (enc_layout[0], enc_layout[1], {k: v for k, v in enc_layout[2].items() if not k.startswith("E 1:")}),
        "redux_decode_planes_dev": dec_layout,
        "redux_decode_delta_dev": dec_layout,
        "redux_encode_stored_dev": (
            ["p", "d_in", "len", "bs", "E", "ratio", "d_out", "out_cap", "d_off", "d_stored", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), len=LEN, bs=BS, E=E0, ratio=65536, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_stored=ptr(8),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "E 3": dict(E=3), "E 16": dict(E=16), "block_size 0": dict(bs=0),
             "store_ratio above one": dict(ratio=65537), "null workspace": dict(d_ws=None), "null flags": dict(d_stored=None),
             "null status": dict(d_st=None), "null input": dict(d_in=None), "below the copy": dict(ws_bytes=COPY - 1),
             "no workspace bytes": dict(ws_bytes=0), "E 1: no workspace bytes": dict(E=1, ws_bytes=0),
             "E 1: workspace not 256-aligned": dict(E=1, d_ws=ptr(6) + 16),
             "general params and E 3": dict(p="any", E=3), "store_ratio above one and no workspace bytes": dict(ratio=65537, ws_bytes=0),
             "general params and store_ratio above one": dict(p="any", ratio=65537)}),
        "redux_decode_stored_dev": (
            ["p", "d_in", "d_off", "d_stored", "out_len", "bs", "E", "d_out", "out_cap", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), d_off=ptr(3), d_stored=ptr(8), out_len=LEN, bs=BS, E=E0, d_out=ptr(2), out_cap=LEN, d_sz=ptr(7),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "E 3": dict(E=3), "E 16": dict(E=16), "block_size 0": dict(bs=0),
             "null workspace": dict(d_ws=None), "null offsets": dict(d_off=None), "null flags": dict(d_stored=None), "null sizes": dict(d_sz=None),
             "null status": dict(d_st=None), "null output": dict(d_out=None), "out_cap below out_len": dict(out_cap=LEN - 1),
             "below the copy": dict(ws_bytes=DCOPY - 1), "below the full size": dict(ws_bytes=sto_dec_ws(E0) - 1),
             "E 1: below the full size": dict(E=1, ws_bytes=sto_dec_ws(1) - 1), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
             "out_cap below out_len and workspace not 256-aligned": dict(out_cap=LEN - 1, d_ws=ptr(6) + 16),
             "null flags and out_cap below out_len": dict(d_stored=None, out_cap=LEN - 1)}),
        "redux_static_encode_blocks_dev": (
            ["p", "cum", "d_in", "len", "bs", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", cum="good", d_in=ptr(1), len=LEN, bs=BS, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4), d_sum=ptr(5),
                 d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "bad table": dict(cum="bad"), "null table": dict(cum="null"),
             "block_size 0": dict(bs=0), "null input": dict(d_in=None), "null status": dict(d_st=None), "null workspace": dict(d_ws=None),
             "workspace not 256-aligned": dict(d_ws=ptr(6) + 16), "below the full size": dict(ws_bytes=st_ws - 1),
             "blocks of 2^26": dict(bs=1 << 26, len=1), "blocks of 2^26 and no workspace bytes": dict(bs=1 << 26, len=1, ws_bytes=0),
             "workspace not 256-aligned and no workspace bytes": dict(d_ws=ptr(6) + 16, ws_bytes=0),
             "general params and bad table": dict(p="any", cum="bad")}),
        "redux_static_decode_blocks_dev": (
            ["p", "cum", "d_in", "d_off", "nblocks", "bs", "d_out", "out_cap", "d_sz", "d_st", "d_sum", "stream"],
            dict(p="good", cum="good", d_in=ptr(1), d_off=ptr(3), nblocks=NB, bs=BS, d_out=ptr(2), out_cap=NB * BS, d_sz=ptr(7), d_st=ptr(4),
                 d_sum=ptr(5), stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "bad table": dict(cum="bad"), "null table": dict(cum="null"),
             "block_size 0": dict(bs=0), "null offsets": dict(d_off=None), "null sizes": dict(d_sz=None), "null status": dict(d_st=None),
             "out_cap below out_len": dict(out_cap=NB * BS - 1), "null offsets and out_cap below out_len": dict(d_off=None, out_cap=0),
             "bad table and block_size 0": dict(cum="bad", bs=0)}),
        "redux_plane_static_encode_dev": (
            ["p", "d_cum", "total", "d_in", "len", "bs", "E", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), len=LEN, bs=BS, E=E0, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4),
                 d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            tables_enc_faults),
        "redux_plane_static_decode_dev": (
            ["p", "d_cum", "total", "d_in", "d_off", "out_len", "bs", "E", "d_out", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), d_off=ptr(3), out_len=LEN, bs=BS, E=E0, d_out=ptr(2), d_sz=ptr(7),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            tables_dec_faults),
        "redux_segment_static_encode_dev": (
            ["p", "d_cum", "total", "d_in", "len", "bs", "E", "G", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), len=LEN, bs=BS, E=E0, G=64 * E0, d_out=ptr(2), out_cap=BIG, d_off=ptr(3),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {**{k: (dict(v, G=64) if v.get("E") == 1 else v) for k, v in tables_enc_faults.items()}, **seg_faults}),
        "redux_segment_static_build_encode_dev": (
            ["p", "total", "d_in", "len", "bs", "E", "G", "d_cum", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", total=4096, d_in=ptr(1), len=LEN, bs=BS, E=E0, G=64 * E0, d_cum=ptr(9), d_out=ptr(2), out_cap=BIG, d_off=ptr(3),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {**{k: v for k, v in tables_enc_faults.items() if not k.startswith("E 1:") and "below the copy" not in k}, **seg_faults,
             "below the counts": dict(ws_bytes=seg_cb - 1), "below the counts and the copy": dict(ws_bytes=seg_cb + COPY - 1),
             "E 1: below the counts": dict(E=1, G=64, ws_bytes=(L.redux_segment_static_table_count(NB, 1, 64) * 2048 + 255) // 256 * 256 - 1),
             "workspace not 256-aligned and below the counts": dict(d_ws=ptr(6) + 16, ws_bytes=seg_cb - 1)}),
        "redux_segment_static_decode_dev": (
            ["p", "d_cum", "total", "d_in", "d_off", "out_len", "bs", "E", "G", "d_out", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), d_off=ptr(3), out_len=LEN, bs=BS, E=E0, G=64 * E0, d_out=ptr(2), d_sz=ptr(7),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {**tables_dec_faults, **seg_faults}),
        "redux_context_static_encode_dev": (
            ["p", "d_cum", "total", "d_in", "len", "bs", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), len=LEN, bs=BS, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4),
                 d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "total 100": dict(total=100), "total 65537": dict(total=65537),
             "block_size 0": dict(bs=0), "null tables": dict(d_cum=None), "null input": dict(d_in=None), "null status": dict(d_st=None),
             "null workspace": dict(d_ws=None), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
             "below the image": dict(ws_bytes=CTX_HEAD - 1), "below the full size": dict(ws_bytes=CTX_HEAD + st_ws - 1),
             "blocks of 2^26": dict(bs=1 << 26, len=1), "blocks of 2^26 and no workspace bytes": dict(bs=1 << 26, len=1, ws_bytes=0),
             "workspace not 256-aligned and no workspace bytes": dict(d_ws=ptr(6) + 16, ws_bytes=0),
             "total 65537 and null status": dict(total=65537, d_st=None)}),
        "redux_context_static_decode_dev": (
            ["p", "d_cum", "total", "d_in", "d_off", "nblocks", "bs", "d_out", "out_cap", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_cum=ptr(9), total=4096, d_in=ptr(1), d_off=ptr(3), nblocks=NB, bs=BS, d_out=ptr(2), out_cap=NB * BS, d_sz=ptr(7),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "general params": dict(p="any"), "total 100": dict(total=100), "total 65537": dict(total=65537),
             "block_size 0": dict(bs=0), "null tables": dict(d_cum=None), "null offsets": dict(d_off=None), "null sizes": dict(d_sz=None),
             "null status": dict(d_st=None), "null workspace": dict(d_ws=None), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
             "out_cap below out_len": dict(out_cap=NB * BS - 1), "below the image": dict(ws_bytes=CTX_HEAD - 1),
             "workspace not 256-aligned and below the image": dict(d_ws=ptr(6) + 16, ws_bytes=CTX_HEAD - 1),
             "total 65537 and out_cap below out_len": dict(total=65537, out_cap=0)}),
    }
    if part == "adaptive":
        calls = adaptive_calls(L, P)
    out = {}
    for fn, (order, base, faults) in calls.items():
        out[fn] = {}
        for label, over in faults.items():
            a = dict(base, **over)
            if "p" in a:
                a["p"] = P[a["p"]]
            if "cum" in a:
                a["cum"] = T[a["cum"]]
            rc = getattr(L, fn)(*[a[k] for k in order])
            assert rc not in (OK, IO_ERROR), "%s, %s: returned %d: the row is not refused before the runtime" % (fn, label, rc)
            out[fn][label] = rc
    return out


def adaptive_calls(L, P):
    """The adaptive coder's own entry points, in the form of refusals()'s `calls`.  `any` is a lock-step width (12-bit symbols),
    `wide` general parameters (code_bits 40): the plain calls take both, the table forms and the const calls neither."""
    dec_ws = L.redux_decode_workspace_bytes(P["good"], NB, BS)
    const_front = COPY + (NB * 16 + 255) // 256 * 256           # x', then the table of the blocks that are left
    const_dec_ws = L.redux_decode_const_workspace_bytes(P["good"], LEN, BS, E0)
    base_dec_ws = L.redux_decode_base_workspace_bytes(P["good"], LEN, BS, E0)
    slots = (["p", "d_in", "len", "bs", "d_st", "d_ws", "ws_bytes", "stream"],
             dict(p="good", d_in=ptr(1), len=LEN, bs=BS, d_st=ptr(4), d_ws=ptr(6), ws_bytes=BIG, stream=None),
             {"bad params": dict(p="bad"), "null params": dict(p="null"), "block_size 0": dict(bs=0), "null workspace": dict(d_ws=None),
              "null status": dict(d_st=None), "null input": dict(d_in=None), "no workspace bytes": dict(ws_bytes=0),
              "4 KiB of workspace": dict(ws_bytes=4096), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
              "lock-step width: no workspace bytes": dict(p="any", ws_bytes=0), "general params: no workspace bytes": dict(p="wide", ws_bytes=0),
              "bad params and null workspace": dict(p="bad", d_ws=None),
              "no workspace bytes and workspace not 256-aligned": dict(ws_bytes=0, d_ws=ptr(6) + 16),
              "null status and no workspace bytes": dict(d_st=None, ws_bytes=0)})
    blocks = (["p", "d_in", "len", "bs", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
              dict(p="good", d_in=ptr(1), len=LEN, bs=BS, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6),
                   ws_bytes=BIG, stream=None),
              slots[2])
    v_faults = {"null table": dict(d_tab=None), "no blocks": dict(nblocks=0, nentries=0), "fewer entries than blocks": dict(nentries=NB - 1),
                "2^32 entries": dict(nentries=1 << 32), "null status": dict(d_st=None), "null workspace": dict(d_ws=None),
                "bad params": dict(p="bad"), "null params": dict(p="null"), "block_size 0": dict(bs=0),
                "lock-step width": dict(p="any"), "general params": dict(p="wide"), "no workspace bytes": dict(ws_bytes=0),
                "general params and no workspace bytes": dict(p="wide", ws_bytes=0), "null table and bad params": dict(d_tab=None, p="bad")}
    return {
        "redux_encode_slots_dev": slots,
        "redux_compact_slots_dev": (
            ["p", "len", "bs", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", len=LEN, bs=BS, d_out=ptr(2), out_cap=BIG, d_off=ptr(3), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG,
                 stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "block_size 0": dict(bs=0), "null workspace": dict(d_ws=None),
             "null status": dict(d_st=None), "null offsets": dict(d_off=None), "null output": dict(d_out=None),
             "no workspace bytes": dict(ws_bytes=0), "general params: no workspace bytes": dict(p="wide", ws_bytes=0),
             "bad params and null output": dict(p="bad", d_out=None), "null output and no workspace bytes": dict(d_out=None, ws_bytes=0)}),
        "redux_encode_blocks_dev": blocks,
        "redux_encode_blocks_v_dev": (
            ["p", "d_in", "in_bytes", "d_tab", "nentries", "nblocks", "bs", "flags", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws",
             "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), in_bytes=LEN, d_tab=ptr(9), nentries=2 * NB, nblocks=NB, bs=BS, flags=0, d_out=ptr(2), out_cap=BIG,
                 d_off=ptr(3), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {**v_faults, "null input": dict(d_in=None), "input of 2^32 bytes": dict(in_bytes=1 << 32),
             "workspace not 256-aligned": dict(d_ws=ptr(6) + 16), "input of 2^32 bytes and no workspace bytes": dict(in_bytes=1 << 32, ws_bytes=0),
             "no workspace bytes and workspace not 256-aligned": dict(ws_bytes=0, d_ws=ptr(6) + 16)}),
        "redux_decode_blocks_dev": (
            ["p", "d_in", "d_off", "nblocks", "bs", "d_out", "out_cap", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), d_off=ptr(3), nblocks=NB, bs=BS, d_out=ptr(2), out_cap=NB * BS, d_sz=ptr(7), d_st=ptr(4), d_sum=ptr(5),
                 d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "block_size 0": dict(bs=0), "null offsets": dict(d_off=None),
             "null sizes": dict(d_sz=None), "null status": dict(d_st=None), "null workspace": dict(d_ws=None),
             "out_cap below the blocks": dict(out_cap=NB * BS - 1), "below the full size": dict(ws_bytes=dec_ws - 1),
             "lock-step width: no workspace bytes": dict(p="any", ws_bytes=0), "general params: no workspace bytes": dict(p="wide", ws_bytes=0),
             "bad params and out_cap below the blocks": dict(p="bad", out_cap=0), "null sizes and out_cap below the blocks": dict(d_sz=None, out_cap=0),
             "out_cap below the blocks and no workspace bytes": dict(out_cap=0, ws_bytes=0)}),
        "redux_decode_blocks_v_dev": (
            ["p", "d_in", "d_off", "d_tab", "nentries", "nblocks", "bs", "flags", "d_out", "out_bytes", "d_sz", "d_st", "d_sum", "d_ws",
             "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), d_off=ptr(3), d_tab=ptr(9), nentries=2 * NB, nblocks=NB, bs=BS, flags=0, d_out=ptr(2), out_bytes=LEN,
                 d_sz=ptr(7), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {**v_faults, "null output": dict(d_out=None), "null offsets": dict(d_off=None), "null sizes": dict(d_sz=None),
             "below the full size": dict(ws_bytes=L.redux_decode_workspace_bytes(P["good"], 2 * NB, BS) - 1),
             "null output and bad params": dict(d_out=None, p="bad")}),
        "redux_encode_const_dev": (
            ["p", "d_in", "len", "d_base", "base_len", "bs", "E", "d_out", "out_cap", "d_off", "d_const", "d_st", "d_sum", "d_ws", "ws_bytes",
             "stream"],
            dict(p="good", d_in=ptr(1), len=LEN, d_base=ptr(10), base_len=LEN, bs=BS, E=E0, d_out=ptr(2), out_cap=BIG, d_off=ptr(3),
                 d_const=ptr(8), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "lock-step width": dict(p="any"), "general params": dict(p="wide"),
             "E 3": dict(E=3), "block_size 0": dict(bs=0), "null workspace": dict(d_ws=None), "null flags": dict(d_const=None),
             "null status": dict(d_st=None), "null output": dict(d_out=None), "null offsets": dict(d_off=None), "null input": dict(d_in=None),
             "null base": dict(d_base=None), "input of 2^32 bytes": dict(len=1 << 32), "below the table": dict(ws_bytes=const_front - 1),
             "no workspace bytes": dict(ws_bytes=0), "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
             "input of 2^32 bytes and no workspace bytes": dict(len=1 << 32, ws_bytes=0),
             "no workspace bytes and workspace not 256-aligned": dict(ws_bytes=0, d_ws=ptr(6) + 16),
             "general params and E 3": dict(p="wide", E=3)}),
        "redux_decode_const_dev": (
            ["p", "d_in", "d_off", "d_const", "d_base", "base_len", "out_len", "bs", "E", "d_out", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes",
             "stream"],
            dict(p="good", d_in=ptr(1), d_off=ptr(3), d_const=ptr(8), d_base=ptr(10), base_len=LEN, out_len=LEN, bs=BS, E=E0, d_out=ptr(2),
                 d_sz=ptr(7), d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "lock-step width": dict(p="any"), "general params": dict(p="wide"),
             "E 3": dict(E=3), "block_size 0": dict(bs=0), "null workspace": dict(d_ws=None), "null offsets": dict(d_off=None),
             "null flags": dict(d_const=None), "null sizes": dict(d_sz=None), "null status": dict(d_st=None), "null output": dict(d_out=None),
             "null base": dict(d_base=None), "below the full size": dict(ws_bytes=const_dec_ws - 1), "no workspace bytes": dict(ws_bytes=0),
             "workspace not 256-aligned": dict(d_ws=ptr(6) + 16),
             "no workspace bytes and workspace not 256-aligned": dict(ws_bytes=0, d_ws=ptr(6) + 16),
             "null flags and no workspace bytes": dict(d_const=None, ws_bytes=0)}),
        "redux_base_planes_dev": (
            ["src", "d_base", "base_len", "dst", "len", "bs", "E", "inverse", "stream"],
            dict(src=ptr(1), d_base=ptr(10), base_len=LEN, dst=ptr(2), len=LEN, bs=BS, E=E0, inverse=0, stream=None),
            {"null src": dict(src=None), "null dst": dict(dst=None), "null base": dict(d_base=None), "block_size 0": dict(bs=0),
             "E 3": dict(E=3), "E 16": dict(E=16), "in place": dict(dst=ptr(1)), "overlap": dict(dst=ptr(1) + 16),
             "destination over the base": dict(dst=ptr(10) + 16), "inverse in place": dict(dst=ptr(1), inverse=1),
             "E 3 and len 0": dict(E=3, len=0), "null base and len 0": dict(d_base=None, len=0)}),
        "redux_encode_base_dev": (
            ["p", "d_in", "len", "d_base", "base_len", "bs", "E", "d_out", "out_cap", "d_off", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), len=LEN, d_base=ptr(10), base_len=LEN, bs=BS, E=E0, d_out=ptr(2), out_cap=BIG, d_off=ptr(3),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "null workspace": dict(d_ws=None), "null input": dict(d_in=None),
             "null base": dict(d_base=None), "block_size 0": dict(bs=0), "E 3": dict(E=3), "E 16": dict(E=16),
             "below the copy": dict(ws_bytes=COPY - 1), "E 1: below the copy": dict(E=1, ws_bytes=COPY - 1),
             "no workspace bytes": dict(ws_bytes=0), "E 3 and no workspace bytes": dict(E=3, ws_bytes=0),
             "null base and no workspace bytes": dict(d_base=None, ws_bytes=0), "bad params and E 3": dict(p="bad", E=3)}),
        "redux_decode_base_dev": (
            ["p", "d_in", "d_off", "d_base", "base_len", "out_len", "bs", "E", "d_out", "d_sz", "d_st", "d_sum", "d_ws", "ws_bytes", "stream"],
            dict(p="good", d_in=ptr(1), d_off=ptr(3), d_base=ptr(10), base_len=LEN, out_len=LEN, bs=BS, E=E0, d_out=ptr(2), d_sz=ptr(7),
                 d_st=ptr(4), d_sum=ptr(5), d_ws=ptr(6), ws_bytes=BIG, stream=None),
            {"bad params": dict(p="bad"), "null params": dict(p="null"), "null workspace": dict(d_ws=None), "null offsets": dict(d_off=None),
             "null sizes": dict(d_sz=None), "null status": dict(d_st=None), "null output": dict(d_out=None), "null base": dict(d_base=None),
             "block_size 0": dict(bs=0), "E 3": dict(E=3), "E 16": dict(E=16), "below the copy": dict(ws_bytes=DCOPY - 1),
             "below the full size": dict(ws_bytes=base_dec_ws - 1), "E 3 and no workspace bytes": dict(E=3, ws_bytes=0),
             "null base and no workspace bytes": dict(d_base=None, ws_bytes=0), "bad params and null sizes": dict(p="bad", d_sz=None)}),
    }


def collect(L, decl, part):
    return {"sizes": sizes(L, decl, part), "names": names(L, decl, part), "refusals": refusals(L, decl, part)}


def main():
    os.environ["HIP_VISIBLE_DEVICES"] = "-1"     # before the library's first HIP call: no row may reach a GPU
    os.environ["ROCR_VISIBLE_DEVICES"] = "-1"
    path = sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else None
    L, decl = load(path)
    part = sys.argv[sys.argv.index("--part") + 1] if "--part" in sys.argv else "layered"
    assert part in ("layered", "adaptive"), part
    json.dump(collect(L, decl, part), sys.stdout, separators=(",", ":"), sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
