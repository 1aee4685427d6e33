#!/usr/bin/env python3
"""Records what the container's accessors make of valid and damaged containers: container_outcomes.json.

Inputs are containers written by container.pack() from made-up streams (no GPU): versions 1, 2 (E = 2, 4, 8) and 3,
with and without CRC tables and stored-block bitmaps, for 1, 3 and 11 blocks.  Each input is then varied: cut at, and
one byte either side of, every section boundary; cut at every byte inside the header; given every version byte; and
given selected values in the parameter bytes, block size, reserved word, block count, total and body.

For every variation the file holds the outcome of each accessor in ACCESSORS: the exception's class name, or the first
16 hex digits of a sha256 over the result.  Per input and accessor, the outcomes of all variations (in variations()
order) are one run-length string of tokens: E (Eof), I (InvalidInput), N (None), T (True), F (False), any other
exception's class name, or the index of a digest in "results"; `x*n` repeats x n times.

    python tests/golden/make_container_outcomes.py            rewrite container_outcomes.json
    python tests/golden/make_container_outcomes.py --check    exit 1 unless the code reproduces it
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "container_outcomes.json")
ACCESSORS = ("unpack", "block_crcs", "block_stored", "element_size", "static_table", "header_is_wellformed")
B = 100  # block size of every input
NAMED = {"Eof": "E", "InvalidInput": "I", None: "N", True: "T", False: "F"}

# (name, version, E, crc, stored, nblocks); total = (nblocks - 1) * B + 37, or 0 for the "empty" input
INPUTS = [
    ("v1_nb1", 1, 1, False, False, 1), ("v1_nb11", 1, 1, False, False, 11), ("v1_crc_nb3", 1, 1, True, False, 3),
    ("v1_stored_nb1", 1, 1, False, True, 1), ("v1_stored_nb11", 1, 1, False, True, 11),
    ("v1_crc_stored_nb11", 1, 1, True, True, 11), ("v1_stored_empty", 1, 1, False, True, 0),
    ("v2e2_nb11", 2, 2, False, False, 11), ("v2e2_crc_nb1", 2, 2, True, False, 1),
    ("v2e2_stored_nb3", 2, 2, False, True, 3), ("v2e2_crc_stored_nb11", 2, 2, True, True, 11),
    ("v2e4_nb3", 2, 4, False, False, 3), ("v2e4_crc_stored_nb11", 2, 4, True, True, 11),
    ("v2e8_crc_nb11", 2, 8, True, False, 11), ("v2e8_stored_nb1", 2, 8, False, True, 1),
    ("v3_nb1", 3, 1, False, False, 1), ("v3_nb11", 3, 1, False, False, 11), ("v3_crc_nb3", 3, 1, True, False, 3),
    ("v3_crc_nb11", 3, 1, True, False, 11),
]


def _container():
    sys.path.insert(0, ROOT)
    from redux_amd import api, container
    return api, container


def make_input(version, E, crc, stored, nblocks):
    """-> (blob, section ends): a container of made-up streams, every third block stored when `stored`"""
    api, container = _container()
    nb = max(nblocks, 1)
    total = (nblocks - 1) * B + 37 if nblocks else 0
    raw = np.clip(total - np.arange(nb, dtype=np.int64) * B, 0, B)
    flags = (np.arange(nb) % 3 == 0).astype(np.uint8) if stored else None
    sizes = np.arange(1, nb + 1, dtype=np.int64) * 3
    if stored:
        sizes[flags == 1] = raw[flags == 1]
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    streams = (np.arange(int(offs[-1]), dtype=np.uint64) * 7 + 1).astype(np.uint8)
    crcs = (np.arange(nb, dtype=np.uint64) * 0x9E3779B1 + 5).astype(np.uint32) if crc else None
    params = (8, 30, 32)
    if version == 3:
        params = api.StaticModel(api.Parameters(8, 30, 32), np.arange(258, dtype=np.uint32) * 4)
    blob = container.pack(streams, offs, params, B, total, E, block_crc=crcs, stored=flags)
    ends = [container.HEADER.size]
    if version == 3:
        ends.append(ends[-1] + container.TABLE)
    ends.append(ends[-1] + 4 * nb)
    if crc:
        ends.append(ends[-1] + 4 * nb)
    if stored:
        ends.append(ends[-1] + (nb + 7) // 8)
    ends.append(ends[-1] + int(offs[-1]))
    assert ends[-1] == len(blob)
    return blob, ends


def _put(blob, at, value, width):
    return blob[:at] + int(value).to_bytes(width, "little") + blob[at + width:]


def variations(blob, ends):
    """-> [(label, bytes)], in a fixed order"""
    out = [("whole", blob)]
    out += [(f"cut{k}", blob[:k]) for k in range(32)]
    cuts = sorted({k for e in ends for k in (e - 1, e, e + 1) if 32 <= k < len(blob)})
    out += [(f"cut{k}", blob[:k]) for k in cuts]
    out += [(f"ver{v:#04x}", blob[:4] + bytes([v]) + blob[5:]) for v in range(256)]
    nb = int.from_bytes(blob[16:24], "little")
    total = int.from_bytes(blob[24:32], "little")
    out += [(f"sym{v}", _put(blob, 5, v, 1)) for v in (0, 7, 12)]
    out += [("params_12_20_32", blob[:5] + bytes([12, 20, 32]) + blob[8:])]
    out += [(f"bs{v}", _put(blob, 8, v, 4)) for v in (0, 1, B - 1, B + 1, 1 << 30, (1 << 30) + 1, 0xFFFFFFFF)]
    out += [(f"res{v:#x}", _put(blob, 12, v, 4)) for v in (0, 1, 2, 4, 8, 16, 0x80000000)]
    out += [(f"nb{v}", _put(blob, 16, v, 8)) for v in (0, nb - 1, nb + 1, 1 << 63)]
    out += [(f"total{v}", _put(blob, 24, v, 8))
            for v in (0, max(total - 1, 0), total + 1, nb * B, nb * B + 1, (nb - 1) * B, (1 << 64) - 1)]
    at = 32 + (1032 if blob[4] & 0x0F == 3 else 0)  # the first size entry
    out += [("size0+1", _put(blob, at, int.from_bytes(blob[at:at + 4], "little") + 1, 4))]
    if blob[4] & 0x40:
        at = ends[-2] - 1  # last bitmap byte
        out += [("bitmap_ff", blob[:at] + b"\xff" + blob[at + 1:]), ("bitmap_00", blob[:at] + b"\x00" + blob[at + 1:])]
    if blob[4] & 0x0F == 3:
        out += [("cum1_0", _put(blob, 36, 0, 4)), ("cum257_big", _put(blob, 32 + 4 * 257, 1 << 31, 4))]
    return out


def _digest(value):
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, np.ndarray):
            h.update(f"nd{v.dtype.str}{v.shape}".encode() + v.tobytes())
        elif isinstance(v, tuple):
            h.update(b"(")
            for x in v:
                feed(x)
            h.update(b")")
        elif hasattr(v, "triple"):
            h.update(b"P" + repr(v.triple()).encode())
        else:
            h.update(f"{type(v).__name__}:{v!r}".encode())
    feed(value)
    return h.hexdigest()[:16]


def outcome(fn, buf):
    """the exception's class name, or NAMED's entry for None / True / False, or a digest"""
    try:
        r = fn(buf)
    except Exception as e:  # noqa: BLE001  (every exception class is part of the record)
        return type(e).__name__
    if r is None or r is True or r is False:
        return r
    return "#" + _digest(r)


def _rle(codes):
    toks, i = [], 0
    while i < len(codes):
        j = i
        while j < len(codes) and codes[j] == codes[i]:
            j += 1
        toks.append(codes[i] if j - i == 1 else f"{codes[i]}*{j - i}")
        i = j
    return " ".join(toks)


def unrle(s):
    out = []
    for t in s.split():
        code, _, n = t.partition("*")
        out += [code] * int(n or 1)
    return out


def decode(code, results):
    """a token of the file -> the outcome() value it stands for"""
    back = {v: k for k, v in NAMED.items()}
    if code in back:
        return back[code]
    if code.isdigit():
        return "#" + results[int(code)]
    return code


def record():
    _, container = _container()
    results, index, cases = [], {}, {}
    for name, *spec in INPUTS:
        blob, ends = make_input(*spec)
        var = variations(blob, ends)
        row = {"variations": len(var)}
        for acc in ACCESSORS:
            codes = []
            for _, buf in var:
                o = outcome(getattr(container, acc), buf)
                if isinstance(o, str) and o.startswith("#"):
                    if o not in index:
                        index[o] = len(results)
                        results.append(o[1:])
                    codes.append(str(index[o]))
                else:
                    codes.append(NAMED.get(o, o))
            row[acc] = _rle(codes)
        cases[name] = row
    return {"accessors": list(ACCESSORS), "results": results, "cases": cases}


def main():
    text = json.dumps(record(), indent=1) + "\n"
    if "--check" in sys.argv:
        same = open(OUT).read() == text
        print("container_outcomes.json: " + ("reproduced" if same else "DIFFERS"))
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
