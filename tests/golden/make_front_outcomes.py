#!/usr/bin/env python3
"""Records which combinations of the options in front of the coder the Python layer accepts: front_outcomes.json.

The cross product of AXES (model kind, element_size, filter, base, base_op, constant, stored, unit_layouts) is given to
each call of CALLS with `_lib.lib` and `api._torch` replaced by functions that raise a sentinel, so that a call either
refuses its arguments first (InvalidInput), reaches the library or torch (the sentinel), or, where it needs neither,
returns.  No GPU is needed, and a check that moved behind the first library call shows as a changed outcome.

The file holds, for every combination in itertools.product order of AXES, one string with a letter per call of CALLS:
I (InvalidInput), L (the library or torch was reached), K (the call returned), X (any other exception).

    python tests/golden/make_front_outcomes.py            rewrite front_outcomes.json
    python tests/golden/make_front_outcomes.py --check    exit 1 unless the code reproduces it
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "front_outcomes.json")

AXES = (("model", ("adaptive", "static", "context", "plane", "segment")),
        ("element_size", (1, 2)),
        ("filter", (None, "delta", "zigzag", "xor")),
        ("base", (None, "bytes")),
        ("base_op", ("xor", "sub", "and")),
        ("constant", (None, True, "flags")),
        ("stored", (None, "flags")),
        ("unit_layouts", (None, "table")))
CALLS = ("compress_blocks", "decompress_blocks", "decompress_blocks_length", "DeviceEncoder", "DeviceDecoder", "pack")
B = 4  # block size; the input is one block


class Reached(Exception):
    """the library or torch was asked for"""


def _reached(*args, **kwargs):
    raise Reached()


def setup():
    """-> (api, container, models by kind), the models made before the library is taken away by patch()"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from redux_amd import api, container
    P = (8, 30, 32)
    models = {"adaptive": P,
              "static": api.StaticModel(P, np.arange(258)),
              "context": api.ContextStaticModel(P, np.tile(np.arange(258), (256, 1))),
              "plane": api.PlaneStaticModel(P, np.tile(np.arange(258), (2, 1))),
              "segment": api.SegmentStaticModel.template(P, 2)}
    return api, container, models


def patch(setattr_):
    """replaces `_lib.lib` and `api._torch` through setattr_(object, name, value) (a test passes monkeypatch.setattr)"""
    from redux_amd import _lib, api
    setattr_(_lib, "lib", _reached)
    setattr_(api, "_torch", _reached)


def combinations():
    return itertools.product(*(values for _, values in AXES))


def outcomes(api, container, models, combo):
    """the letters of CALLS for one combination; patch() must be in force"""
    model, E, filt, base, base_op, constant, stored, units = combo
    m = models[model]
    flags = lambda: np.zeros(1, dtype=np.uint8)
    base = None if base is None else b"abcd"
    constant = flags() if constant == "flags" else constant
    stored = None if stored is None else flags()
    units = None if units is None else flags()
    offs = np.array([0, 1], dtype=np.uint64)
    opts = dict(element_size=E, filter=filt, base=base, constant=constant, base_op=base_op)
    host = dict(opts, stored=stored, unit_layouts=units)
    dev = dict(opts, mixed=units is not None)
    calls = (lambda: api.compress_blocks(b"abcd", B, m, **host),
             lambda: api.decompress_blocks(b"\0", offs, B, m, **host),
             lambda: api.decompress_blocks(b"\0", offs, B, m, length=4, **host),
             lambda: api.DeviceEncoder(m, B, B, **dev),
             lambda: api.DeviceDecoder(m, B, 1, **dev),
             lambda: container.pack(np.zeros(1, dtype=np.uint8), offs, m, B, 4,
                                    **dict(host, base=None if base is None else (4, 0))))
    got = ""
    for call in calls:
        try:
            call()
            got += "K"
        except api.InvalidInput:
            got += "I"
        except Reached:
            got += "L"
        except Exception:  # noqa: BLE001 (whatever else: recorded as such)
            got += "X"
    return got


def record():
    api, container, models = setup()
    from redux_amd import _lib
    saved = (_lib.lib, api._torch)
    patch(setattr)
    try:
        rows = [outcomes(api, container, models, c) for c in combinations()]
    finally:
        _lib.lib, api._torch = saved
    return {"axes": [[name, list(values)] for name, values in AXES], "calls": list(CALLS), "outcomes": rows}


if __name__ == "__main__":
    rec = record()
    if "--check" in sys.argv:
        same = rec == json.load(open(OUT))
        print("front_outcomes.json: " + ("reproduced" if same else "DIFFERS"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    n = {k: sum(r.count(k) for r in rec["outcomes"]) for k in "ILKX"}
    print("front_outcomes.json: %d combinations x %d calls, %s" % (len(rec["outcomes"]), len(CALLS), n))
