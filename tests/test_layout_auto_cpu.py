"""`--layout auto` without a GPU: the CLI's flag rules, the pure choice function, the Python argument checks, and the value
claim -- which of the eight layouts (include/redux_hip.h, "layout estimates") is smallest on typed data -- on the numpy
restatement of the layouts and the library's host cost rule.  The restatement and the inputs are shared with the GPU tests."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_delta_cpu import delta_planes_ref
from test_planes_cpu import planes_ref

P = (8, 30, 32)
LAYOUTS = [(E, f) for f in (None, "delta") for E in (1, 2, 4, 8)]  # layout k = 4 F + log2 E


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def transform_ref(x, k, B):
    """transform_k(x): the byte-plane layout for E = 2^(k mod 4), behind the delta filter for k >= 4 (the rule of the header)"""
    E = 1 << (k & 3)
    return delta_planes_ref(x, E, B) if k >= 4 else planes_ref(x, E, B)


def block_counts(a, B):
    nb = max(1, -(-len(a) // B))
    return np.stack([np.bincount(a[b * B: (b + 1) * B], minlength=256) for b in range(nb)]).astype(np.uint64)


@functools.lru_cache(maxsize=None)
def table_input(name):
    """the inputs of the layout table, each from np.random.default_rng(1) -> uint8 array"""
    rng = np.random.default_rng(1)
    if name == "timestamps":
        return (1.7e12 + np.cumsum(rng.integers(900, 1100, 262144))).astype("<i8").view(np.uint8)
    if name == "sorted-u32":
        return np.sort(rng.integers(0, 2 ** 30, 524288)).astype("<u4").view(np.uint8)
    if name == "bf16":
        f = rng.normal(0, 0.02, 524288).astype(np.float32)
        return (f.view(np.uint32) >> 16).astype("<u2").view(np.uint8)     # bf16 by truncation: the high half of fp32
    if name == "fp32":
        return rng.normal(0, 1, 524288).astype("<f4").view(np.uint8)
    assert name == "bible"
    return np.frombuffer(open(os.path.join(GOLDEN, "corpora", "large", "bible.txt"), "rb").read()[: 1 << 20], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def host_estimates(name, B=65536):
    """{(E, filter): ceil(sum bits / 8 + 2.5 nblocks)} by the host rule on the restatement: what api.estimate_layouts computes"""
    import redux_amd as rx
    x = table_input(name)
    out = {}
    for k, key in enumerate(LAYOUTS):
        bits = rx.adaptive_cost_from_counts(block_counts(transform_ref(x, k, B), B), P)
        out[key] = int(np.ceil(bits.sum() / 8 + rx.api.TERMINATION_BYTES * len(bits)))
    return out


# per input byte, plain E = 1 / 2 / 4 / 8 then delta E = 1 / 2 / 4 / 8 (ideal cost + 2.5 bytes per block, B = 65536); how
# closely the row is held; the pick: the filter and the element sizes that tie.  The series and the text reproduce the
# recorded figures to the last place.  The other three rows were recorded from draws whose exact call is not on record
# (integer dtype, rounding to bf16): every variant of them lands within 0.0005 of the row, far inside the gaps that decide
# the picks (0.026 and more), so they are held to 0.0006.
TABLE = {
    "timestamps": ((0.6426, 0.6044, 0.5226, 0.4126, 0.7476, 0.7756, 0.8273, 0.1388), 0.00006, "delta", {8}),
    "sorted-u32": ((0.8813, 0.8742, 0.8467, 0.8777, 1.0017, 1.0017, 0.3926, 0.4186), 0.0006, "delta", {4}),
    "bf16": ((0.7786, 0.6687, 0.6687, 0.6687, 1.0013, 0.7055, 0.7056, 0.7055), 0.0006, None, {2, 4, 8}),
    "fp32": ((0.9202, 0.8888, 0.8334, 0.8334, 1.0015, 1.0017, 0.8537, 0.8536), 0.0006, None, {4, 8}),
    "bible": ((0.5438, 0.5441, 0.5444, 0.5449, None, None, None, None), 0.00006, None, {1}),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_the_layout_table(rx, name):
    from redux_amd import container
    ratios, tol, want_filter, want_E = TABLE[name]
    est = host_estimates(name)
    n = len(table_input(name))
    got = [est[key] / n for key in LAYOUTS]
    print(name, " ".join("%.4f" % g for g in got))
    for g, w in zip(got, ratios):
        assert w is None or abs(g - w) <= tol, (name, got)
    if name == "bible":
        assert all(0.7775 <= g <= 0.8324 for g in got[4:])
    E, filt = container.choose_layout(est)
    assert filt == want_filter and E in want_E, (name, E, filt)
    if name == "bf16":  # the caller who knows the dtype
        assert container.choose_layout({k: v for k, v in est.items() if k[0] == 2}) == (2, None)


def test_choose_layout_on_hand_made_estimates(rx):
    from redux_amd import container
    base = {key: 1000 + i for i, key in enumerate(LAYOUTS)}
    assert container.LAYOUT_ORDER == tuple(LAYOUTS) == rx.LAYOUTS
    assert container.choose_layout(base) == (1, None)
    assert container.choose_layout({**base, (8, "delta"): 999}) == (8, "delta")
    assert container.choose_layout({**base, (4, None): 7, (2, "delta"): 8}) == (4, None)
    # exact ties go to the earlier of the order: plain before delta, small elements before large
    assert container.choose_layout({key: 5 for key in LAYOUTS}) == (1, None)
    assert container.choose_layout({**base, (2, None): 3, (4, None): 3, (8, None): 3}) == (2, None)
    assert container.choose_layout({**base, (8, None): 3, (1, "delta"): 3}) == (8, None)
    assert container.choose_layout({**base, (4, "delta"): 3, (8, "delta"): 3}) == (4, "delta")
    assert container.choose_layout({(8, "delta"): 3, (2, None): 3}) == (2, None)      # (the order, not the dict's)
    assert container.choose_layout({(2, None): 10, (2, "delta"): 10}) == (2, None)
    assert container.choose_layout({(2, None): 10, (2, "delta"): 9}) == (2, "delta")
    assert [rx.layout_index(*key) for key in LAYOUTS] == list(range(8))
    with pytest.raises(rx.InvalidInput):
        rx.layout_index(3, None)


def test_overhead_of_the_delta_container(rx):
    from redux_amd import container
    for E in (1, 2, 4, 8):
        for checksum in (False, True):
            want = container.overhead_bytes("adaptive", 7, E, checksum=checksum)
            assert container.overhead_bytes("adaptive", 7, E, checksum=checksum, filter="delta") == want
            sizes = np.arange(8, dtype=np.uint64) * 3
            crc = np.zeros(7, dtype=np.uint32) if checksum else None
            blob = container.pack(np.zeros(21, dtype=np.uint8), sizes, P, 64, 7 * 64, E, block_crc=crc, filter="delta")
            assert len(blob) == want + 21 and blob[4] == (6 | (0x10 if checksum else 0))
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("static", 7, 1, filter="delta")
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("adaptive", 7, 1, stored=True, filter="delta")
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("adaptive", 7, 1, filter="xor")


def test_compress_bytes_refuses_before_the_library_is_touched(rx, monkeypatch):
    from redux_amd import _lib, container

    def no_library():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "lib", no_library)
    data = bytes(1000)
    for kw in ({"model": "auto"}, {"model": "static"}, {"model": "plane-static", "element_size": 2}, {"model": "segment-static"},
               {"model": "context-static"}, {"stored": True}, {"base": bytes(1000)}, {"skip_constant": True},
               {"filter": "delta"}, {"segment_blocks": 256}, {"element_size": 3}, {"block_size": 0},
               {"block_size": (1 << 30) + 1}):
        with pytest.raises(rx.InvalidInput):
            container.compress_bytes(data, **{"block_size": 256, "layout": "auto", **kw})
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(data, 256, layout="delta")
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(data, 256, layout=True)


GOOD = [
    ["-c", "--block-size", "65536", "--layout", "auto"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--checksum"],
    ["-c", "--block-size", "4096", "--layout", "auto", "--element-size", "1"],
    ["-c", "--block-size", "4096", "--layout", "auto", "--element-size", "2"],
    ["-c", "--block-size", "4096", "--layout", "auto", "--element-size", "8", "--checksum"],
    ["-c", "--block-size", "4096", "--layout", "auto", "--model", "adaptive"],
    ["--layout", "auto", "-i", "a", "-o", "b", "--block-size", "1", "-c"],
]
BAD = [
    ["-c", "--layout", "auto"],                                                  # no block size
    ["-c", "--block-size", "0", "--layout", "auto"],
    ["-c", "--block-size", "65536", "--layout"],
    ["-c", "--block-size", "65536", "--layout", "delta"],
    ["-c", "--block-size", "65536", "--layout", "none"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--stored"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--filter", "delta"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--base", "b"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--skip-constant"],
    ["-d", "--block-size", "65536", "--layout", "auto"],
    ["-d", "--layout", "auto"],
    ["--block-size", "65536", "--layout", "auto"],                               # neither -c nor -d
    ["-c", "--block-size", "65536", "--layout", "auto", "--model", "auto"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--model", "static"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--model", "segment-static"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--model", "context-static"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--model", "plane-static", "--element-size", "2"],
    ["-c", "--block-size", "65536", "--layout", "auto", "--element-size", "3"],
]


def test_cli_parse_accepts_and_refuses():
    from redux_amd import cli
    for argv in GOOD:
        opts = cli.parse(argv)
        assert opts is not None and opts["layout"] == "auto" and opts["compress"] is True, argv
    assert "element_size" not in cli.parse(GOOD[0]) and cli.parse(GOOD[3])["element_size"] == 2
    for argv in BAD:
        assert cli.parse(argv) is None, argv
    assert "--layout" in cli.USAGE and "--layout auto" in cli.__doc__
    assert "layout" not in cli.parse(["-c", "--block-size", "65536"])            # nothing changes without the flag


def test_cli_usage_error_exit_code(capsys):
    from redux_amd import cli
    assert cli.main(["-c", "--block-size", "0", "--layout", "auto"]) == 1
    assert "Usage" in capsys.readouterr().err
