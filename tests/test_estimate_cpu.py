"""Size estimates (include/redux_hip.h, "size estimates") without a GPU: the library's host calls against the oracle's
streams and against a math.lgamma / numpy.log2 restatement of the two rules, the container's overhead arithmetic against
pack(), and the command line's `--model auto`."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import cbind as ox
from redux_amd import _lib, api, cli, container

P = (8, 30, 32)
FILES = ("canterbury/alice29.txt", "canterbury/kennedy.xls", "calgary/geo", "calgary/pic", "artificial/random.txt")


def _read(name):
    return open(os.path.join(GOLDEN, "corpora", *name.split("/")), "rb").read()


def _blocks(data, bs, most=None):
    out = [data[o: o + bs] for o in range(0, max(len(data), 1), bs)]
    return out if most is None else out[:most]


def _counts(blocks):
    return np.stack([np.bincount(np.frombuffer(b, dtype=np.uint8), minlength=256) for b in blocks]).astype(np.uint64)


def _synthetic():
    rng = np.random.default_rng(0xE571)
    n = 65536
    zipf = 1.0 / np.arange(1, 257) ** 1.2
    skew = rng.integers(1, 256, n).astype(np.uint8)
    skew[rng.random(n) >= 0.001] = 0                                   # 0.1 % of the bytes are not zero
    return {
        "zeros": bytes(n), "ff": b"\xff" * n, "iid": rng.integers(0, 256, n).astype(np.uint8).tobytes(),
        "two-value": rng.choice(np.array([3, 250], dtype=np.uint8), n).tobytes(), "skewed": skew.tobytes(),
        "zipf": rng.choice(256, n, p=zipf / zipf.sum()).astype(np.uint8).tobytes(),
        "empty": b"", "one byte": b"x", "63 bytes": rng.integers(0, 256, 63).astype(np.uint8).tobytes(),
    }


@pytest.fixture(scope="module")
def cases():
    """name -> list of blocks: the corpus files at 64 KiB, their first 64 blocks at 4 KiB and 256 B, the synthetic blocks,
    and long blocks of bible.txt"""
    out = {}
    for f in FILES:
        data = _read(f)
        out[f + " 64K"] = _blocks(data, 65536)
        out[f + " 4K"] = _blocks(data, 4096, 64)
        out[f + " 256"] = _blocks(data, 256, 64)
    out.update((k, [v]) for k, v in _synthetic().items())
    bible = _read("large/bible.txt")
    out["bible long"] = [bible[: 128 << 10], bible[: 1 << 20], bible[: 4 << 20]]
    return out


def _restate_adaptive(c):
    n = int(c.sum())
    return (math.lgamma(n + 258) - math.lgamma(257) - sum(math.lgamma(int(h) + 1) for h in c)) / math.log(2)


def _restate_table(c, cum):
    T = int(cum[257])
    f = np.diff(cum[:257].astype(np.int64))
    nz = c > 0
    if T == 0 or bool((f[nz] <= 0).any()):
        return math.inf
    return float((c[nz].astype(np.float64) * (np.log2(float(T)) - np.log2(f[nz].astype(np.float64)))).sum())


def test_adaptive_cost_against_the_oracle(cases):
    worst = [0, 0]
    for name, blocks in cases.items():
        bits = api.adaptive_cost_from_counts(_counts(blocks), P)
        for b, blk in enumerate(blocks):
            stream, _ = ox.compress(blk, P)
            d = len(stream) - (math.ceil(bits[b] / 8) + 2)
            worst = [min(worst[0], d), max(worst[1], d)]
            assert abs(d) <= 2, (name, b, len(stream), bits[b])
    print("adaptive: len(stream) - (ceil(bits / 8) + 2) in", worst)


def test_table_cost_against_the_oracle():
    worst = [0, 0]
    for f in FILES:
        data = _read(f)
        cum = api.static_table_from_counts(_counts([data])[0], P)       # the default total
        blocks = _blocks(data, 65536)
        bits = api.table_cost_from_counts(_counts(blocks), np.tile(cum, (len(blocks), 1))) + math.log2(int(cum[257]))
        for b, blk in enumerate(blocks):
            stream, _ = ox.compress_static(blk, cum, P)
            d = len(stream) - (math.ceil(bits[b] / 8) + 2)
            worst = [min(worst[0], d), max(worst[1], d)]
            assert abs(d) <= 2, (f, b, len(stream), bits[b])
    print("static: len(stream) - (ceil(bits / 8) + 2) in", worst)


def test_both_calls_equal_their_definition(cases):
    """within 2^-10 bit for blocks up to 1 MiB: at most 258 terms, each below 2^25 bits (ulp 2^-27), a few ulp each"""
    tol = 2.0 ** -10
    cum = api.static_table_from_counts(_counts([_read(FILES[0])])[0], P)
    for name, blocks in cases.items():
        blocks = [b for b in blocks if len(b) <= 1 << 20]
        c = _counts(blocks)
        got_a = api.adaptive_cost_from_counts(c, P)
        got_t = api.table_cost_from_counts(c, np.tile(cum, (len(c), 1)))
        for b in range(len(c)):
            assert abs(got_a[b] - _restate_adaptive(c[b])) <= tol, (name, b)
            assert abs(got_t[b] - _restate_table(c[b], cum)) <= tol, (name, b)


def test_status_and_edge_cases():
    row = np.zeros(256, dtype=np.uint64)
    row[7] = 65536
    with pytest.raises(api.Unsupported):
        api.adaptive_cost_from_counts(row, (8, 14, 16))                 # a 64 KiB block freezes the 14-bit model
    with pytest.raises(api.Unsupported):
        api.adaptive_cost_from_counts(row, (7, 14, 16))
    with pytest.raises(api.Unsupported):
        api.adaptive_cost_from_counts(row, (8, 24, 40))
    short = np.zeros(256, dtype=np.uint64)
    short[7] = 16383 - 257                                              # 256 + n < freq_max: the longest block that cannot freeze
    assert api.adaptive_cost_from_counts(short, (8, 14, 16))[0] > 0
    short[8] = 1
    with pytest.raises(api.Unsupported):
        api.adaptive_cost_from_counts(short, (8, 14, 16))
    # the device call's refusals are decided before any launch (dummy pointers: nothing is read)
    L = _lib.lib()
    import ctypes as C
    for triple, bs, want in (((8, 14, 16), 65536, _lib.UNSUPPORTED), ((7, 14, 16), 64, _lib.UNSUPPORTED),
                             ((8, 24, 40), 64, _lib.UNSUPPORTED), ((8, 30, 32), 0, _lib.INVALID_INPUT),
                             ((8, 30, 32), (1 << 30) + 1, _lib.INVALID_INPUT)):
        cp = _lib.Params(*triple)
        assert L.redux_block_cost_dev(C.byref(cp), C.c_void_p(256), 1 << 20, bs, C.c_void_p(256), None) == want, (triple, bs)
    ones = np.arange(258, dtype=np.uint32)                              # every frequency 1, total 257
    zeros = np.zeros(256, dtype=np.uint64)
    assert api.table_cost_from_counts(zeros, ones)[0] == 0.0            # a row of zeros costs nothing
    assert api.adaptive_cost_from_counts(zeros, P)[0] == pytest.approx(math.log2(257), abs=2.0 ** -10)   # the EOF alone
    hole = ones.copy()
    hole[8:] -= 1                                                       # byte 7 has frequency 0
    assert api.table_cost_from_counts(row, hole)[0] == math.inf
    assert api.table_cost_from_counts(zeros, hole)[0] == 0.0            # ... which costs nothing where it is not used
    back = ones.copy()
    back[8] = 3                                                         # a negative frequency
    assert api.table_cost_from_counts(row, back)[0] == math.inf
    assert api.table_cost_from_counts(zeros, np.zeros(258, dtype=np.uint32))[0] == math.inf   # T == 0
    assert api.table_cost_from_counts(row, ones)[0] == pytest.approx(65536 * math.log2(257), rel=1e-12)


def _made_up(nb, rng):
    sizes = rng.integers(1, 40, nb)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    return rng.integers(0, 256, int(offs[-1])).astype(np.uint8), offs


@pytest.mark.parametrize("nb", [1, 5, 256, 257, 600])
def test_overhead_equals_what_pack_writes(nb):
    rng = np.random.default_rng(nb)
    B = 4096
    streams, offs = _made_up(nb, rng)
    payload = int(offs[-1])
    text = np.frombuffer(_read(FILES[0]), dtype=np.uint8)
    cum = api.static_table_from_counts(np.bincount(text, minlength=256), P)
    pair = np.zeros((256, 256), dtype=np.uint64)
    np.add.at(pair, (text[:-1], text[1:]), 1)
    ctx = api.ContextStaticModel(P, api.context_static_tables_from_counts(pair, P))
    models = {"adaptive": (P, 1), "static": (api.StaticModel(P, cum), 1), "context-static": (ctx, 1)}
    for E in (2, 4, 8):
        models["plane-static %d" % E] = (api.PlaneStaticModel(P, np.tile(cum, (E, 1))), E)
    for E, G in ((1, None), (1, 64), (2, None), (4, 512)):
        g = api.default_segment_blocks(E) if G is None else G
        nseg = max(1, -(-nb // g))
        models["segment-static %d %s" % (E, G)] = (api.SegmentStaticModel(P, np.tile(cum, (nseg * E, 1)), E, g), E, G)
    for name, (m, E, *G) in models.items():
        model = name.split()[0]
        kw = dict(element_size=E, segment_blocks=G[0] if G else None, context_cums=ctx.cums if model == "context-static" else None)
        for checksum in (False, True):
            crc = np.zeros(nb, dtype=np.uint32) if checksum else None
            blob = container.pack(streams, offs, m, B, nb * B, E, block_crc=crc)
            assert container.overhead_bytes(model, nb, checksum=checksum, **kw) == len(blob) - payload, (name, checksum)
    flags = np.zeros(nb, dtype=np.uint8)                                # the stored-block bitmap (adaptive model only)
    blob = container.pack(streams, offs, P, B, nb * B, stored=flags)
    assert container.overhead_bytes("adaptive", nb, stored=True) == len(blob) - payload
    with pytest.raises(api.InvalidInput):
        container.overhead_bytes("context-static", nb)                  # the tables decide which contexts are recorded
    with pytest.raises(api.InvalidInput):
        container.overhead_bytes("auto", nb)


def test_choose_model_breaks_ties_by_order():
    assert container.choose_model({"context-static": 10, "static": 10, "adaptive": 11}) == "static"
    assert container.choose_model({"segment-static": 7, "adaptive": 7}) == "adaptive"
    assert container.choose_model({"adaptive": 9, "plane-static": 8, "segment-static": 8}) == "plane-static"
    assert api.estimate_candidates(1) == ("adaptive", "static", "segment-static", "context-static")
    assert api.estimate_candidates(4) == ("adaptive", "plane-static", "segment-static")


def test_cli_model_auto():
    ok = cli.parse(["-c", "--block-size", "65536", "--model", "auto"])
    assert ok is not None and ok["model"] == "auto"
    assert cli.parse(["-c", "--block-size", "65536", "--model", "auto", "--element-size", "4", "--checksum"])["element_size"] == 4
    assert cli.parse(["-c", "--model", "auto"]) is None                                                  # --block-size 0
    assert cli.parse(["-c", "--block-size", "0", "--model", "auto"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "auto", "--stored"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "auto", "--filter", "delta"]) is None
    assert cli.parse(["-c", "--block-size", "65536", "--model", "auto", "--segment-blocks", "256"]) is None
    assert "auto" in cli.USAGE and "--model auto" in cli.__doc__
    for m in ("adaptive", "static", "segment-static", "context-static"):
        assert cli.parse(["-c", "--block-size", "65536", "--model", m])["model"] == m
    assert cli.parse(["-c", "--block-size", "65536", "--model", "plane-static", "--element-size", "2"])["model"] == "plane-static"
    assert cli.parse(["-c", "--block-size", "65536", "--model", "automatic"]) is None


def test_auto_refuses_what_it_does_not_choose():
    for kw in (dict(stored=True), dict(filter="delta"), dict(segment_blocks=256), dict(block_size=0), dict(element_size=3)):
        with pytest.raises(api.InvalidInput):                           # (decided before the GPU is touched)
            container.compress_bytes(b"abc", **{"block_size": 4096, "model": "auto", **kw})
