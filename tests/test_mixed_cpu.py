"""`--layout mixed` without a GPU: the CLI's flag rules, container version 10 through pack / _parse with made-up streams, the
choice rule (include/redux_hip.h, "mixed layouts") restated in numpy on hand-made bits, the Python argument checks, and the
value claim -- a layout per unit of 8 blocks against the best single layout on files of several element types -- on the numpy
restatement of the layouts and the library's host cost rule.  The restatement is shared with the GPU tests."""
import functools

import numpy as np
import pytest

from test_layout_auto_cpu import block_counts, table_input, transform_ref

P = (8, 30, 32)
B = 65536
UNIT = 8
PARTS = ("timestamps", "bf16", "fp32", "bible")


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


# ---- the restatements --------------------------------------------------------------------------------------------------
def choose_ref(bits, mask=0xFF):
    """The choice rule: S[k][u] = the unit's bits[k][b] added in f64 one after the other, in ascending block order from 0.0
    (np.sum over 8 values adds in another order); table[u] = the lowest selected k with the smallest S[k][u].
    -> (np.uint8[nunits], S float64[8, nunits] with inf in the rows that are not selected)"""
    bits = np.asarray(bits, dtype=np.float64)
    nb = bits.shape[1]
    nunits = -(-nb // UNIT)
    S = np.full((8, nunits), np.inf)
    for k in range(8):
        if mask >> k & 1:
            s = np.zeros(nunits)
            for j in range(UNIT):  # column j of every unit, one after the other
                col = bits[k, j::UNIT]
                s[: len(col)] = s[: len(col)] + col
            S[k] = s
    return np.argmin(S, axis=0).astype(np.uint8), S  # (argmin: the first of equal minima)


def mixed_ref(x, table, Bs, inverse=False):
    """the mixed transform: unit u of the result is unit u of the whole-buffer transform under layout table[u] & 7"""
    from test_delta_cpu import delta_planes_ref
    from test_planes_cpu import planes_ref
    x = np.ascontiguousarray(x, dtype=np.uint8)
    out = x.copy()
    U = UNIT * Bs
    whole = {}
    for u in range(-(-len(x) // U)):
        k = int(table[u]) & 7
        if k not in whole:
            E = 1 << (k & 3)
            whole[k] = (delta_planes_ref if k >= 4 else planes_ref)(x, E, Bs, inverse=inverse)
        out[u * U: (u + 1) * U] = whole[k][u * U: (u + 1) * U]
    return out


@functools.lru_cache(maxsize=None)
def mixed_input(name):
    """a table_input row, "concat" = timestamps + bf16 + fp32 + bible[:1 MiB] (6,291,456 bytes, 96 blocks, 12 units), or
    "shifted" = the same behind bible[:100000] (tensor boundaries inside units)"""
    if name == "concat":
        return np.concatenate([table_input(p) for p in PARTS])
    if name == "shifted":
        return np.concatenate([table_input("bible")[:100000], mixed_input("concat")])
    return table_input(name)


@functools.lru_cache(maxsize=None)
def host_bits(name):
    """float64[8, nblocks]: the host cost rule on the restatement of each layout of mixed_input(name)"""
    import redux_amd as rx
    x = mixed_input(name)
    return np.stack([rx.adaptive_cost_from_counts(block_counts(transform_ref(x, k, B), B), P) for k in range(8)])


def estimate(bits_sum, nblocks):
    import redux_amd as rx
    return int(np.ceil(bits_sum / 8 + rx.api.TERMINATION_BYTES * nblocks))


@functools.lru_cache(maxsize=None)
def host_mixed(name):
    """(best single layout's estimate, its k, the mixed estimate, the table, S) of mixed_input(name)"""
    bits = host_bits(name)
    nb = bits.shape[1]
    single = [estimate(bits[k].sum(), nb) for k in range(8)]
    table, S = choose_ref(bits)
    chosen = float(sum(S[table[u], u] for u in range(len(table))))
    return min(single), int(np.argmin(single)), estimate(chosen, nb), table, S


# ---- the choice rule on hand-made bits -----------------------------------------------------------------------------
def test_choice_rule_on_hand_made_bits():
    nb = 19  # two full units and a short one of 3 blocks
    bits = np.full((8, nb), 100.0)
    bits[3, 0:8] = 99.0                      # unit 0: layout 3 wins by 8 bits
    bits[6, 8:16] = 50.0                     # unit 1: 6 and 2 tie exactly -> the lower k
    bits[2, 8:16] = 50.0
    bits[7, 16:19] = 1.0                     # the short unit: 3 blocks
    bits[5, 16:19] = [0.5, 0.5, 2.0]         # 3.0, the same sum as layout 7 -> 5
    table, S = choose_ref(bits)
    assert table.tolist() == [3, 2, 5]
    assert S[3, 0] == 792.0 and S[0, 0] == 800.0 and S[7, 2] == 3.0 and S[5, 2] == 3.0 and S[0, 2] == 300.0
    # a mask leaves the other rows out, whatever they hold
    table, S = choose_ref(bits, 0x81)
    assert table.tolist() == [0, 0, 7] and np.isinf(S[3]).all()
    table, _ = choose_ref(bits, 0x22)
    assert table.tolist() == [1, 1, 5]
    # one after the other: sums that differ in the last place by the order of the additions
    v = np.array([1e16, 1.0, -1e16, 1.0, 1.0, 1.0, 1.0, 1.0])
    want = 0.0
    for t in v:
        want += t
    b2 = np.zeros((8, 8))
    b2[:] = 1e300
    b2[4] = v
    _, S = choose_ref(b2, 0x10)
    assert S[4, 0] == want == 5.0


def test_mixed_ref_is_the_splice_of_the_whole_buffer_transforms():
    rng = np.random.default_rng(5)
    Bs = 16
    x = rng.integers(0, 256, 3 * 8 * Bs + 5 * Bs + 7, dtype=np.uint8)
    table = np.array([7, 0, 2 | 0xF8, 5], dtype=np.uint8)  # (high bits are ignored)
    y = mixed_ref(x, table, Bs)
    U = 8 * Bs
    for u, k in enumerate([7, 0, 2, 5]):
        assert np.array_equal(y[u * U: (u + 1) * U], transform_ref(x, k, Bs)[u * U: (u + 1) * U])
    assert np.array_equal(mixed_ref(y, table, Bs, inverse=True), x)
    assert np.array_equal(mixed_ref(x, np.zeros(4, np.uint8), Bs), x)


# ---- the value claim -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["concat", "shifted"])  # (computed when the feature was proposed: 0.896 and 0.905)
def test_mixed_beats_the_best_single_layout_on_mixed_files(rx, name):
    best, k, mixed, table, S = host_mixed(name)
    nunits = len(table)
    x = mixed_input(name)
    assert len(table) == -(-len(x) // (8 * B)) == {"concat": 12, "shifted": 13}[name]
    print(name, "best single", best, "layout", k, "mixed + table", mixed + nunits, "ratio %.4f" % ((mixed + nunits) / best))
    assert k == 7
    assert mixed + nunits <= 0.91 * best
    if name == "concat":  # every tensor is whole units: what coding each part on its own would give
        parts = sum(host_mixed(p)[0] for p in PARTS)
        assert abs(mixed + nunits - parts) <= nunits + 1, (mixed, parts)
        # the picks, where the runner-up is more than a bit away (bf16 at E = 2 / 4 / 8 ties to rounding)
        want = [{7}] * 4 + [{1, 2, 3}] * 2 + [{2, 3}] * 4 + [{0}] * 2
        for u in range(nunits):
            order = np.sort(S[:, u])
            if order[1] - order[0] > 1.0:
                assert int(table[u]) in want[u], (u, table.tolist())
        assert table[:4].tolist() == [7] * 4 and table[10:].tolist() == [0, 0]


@pytest.mark.parametrize("name", PARTS)
def test_a_single_dtype_file_pays_the_table_and_no_more(rx, name):
    best, _, mixed, table, _ = host_mixed(name)
    print(name, "best single", best, "mixed + table", mixed + len(table))
    assert mixed <= best and mixed + len(table) <= best + len(table)


# ---- container version 10 -------------------------------------------------------------------------------------------
def _made_up(nb, seed=0):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 9, nb)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(sizes)
    return rng.integers(0, 256, int(offs[-1]), dtype=np.uint8), offs


@pytest.mark.parametrize("checksum", [False, True])
def test_container_round_trip_of_version_10(rx, checksum):
    from redux_amd import container
    nb, Bs = 19, 64
    total = 18 * Bs + 5
    streams, offs = _made_up(nb)
    table = np.array([7, 0, 5], dtype=np.uint8)
    crc = np.arange(nb, dtype=np.uint32) * 0x01010101 if checksum else None
    blob = container.pack(streams, offs, P, Bs, total, block_crc=crc, unit_layouts=table)
    assert blob[4] == (0x1A if checksum else 0x0A) and blob[12:16] == bytes([0, 0, 0, 0xA0])
    assert len(blob) == container.overhead_bytes("adaptive", nb, checksum=checksum, mixed=True) + len(streams)
    assert container.overhead_bytes("adaptive", nb, checksum=checksum, mixed=True) == \
        container.overhead_bytes("adaptive", nb, checksum=checksum) + 3
    c = container._parse(blob)
    assert c.unit_layouts.tolist() == [7, 0, 5] and c.element_size is None and c.filter is None
    assert c.total == total and c.block_size == Bs and np.array_equal(c.offsets, offs) and np.array_equal(c.payload, streams)
    assert (c.crcs is None) if not checksum else np.array_equal(c.crcs, crc)
    assert container.unit_layouts(blob).tolist() == [7, 0, 5]
    assert container.element_size(blob) is None and container.filter(blob) is None
    assert container.header_is_wellformed(blob)
    at = container.HEADER.size + 4 * nb * (2 if checksum else 1)  # where the unit table lies
    assert blob[at: at + 3] == bytes([7, 0, 5])
    # a table byte of 8
    bad = bytearray(blob)
    bad[at + 1] = 8
    with pytest.raises(rx.InvalidInput):
        container._parse(bytes(bad))
    # a truncated table, and a truncated payload
    for cut in (at, at + 2):
        with pytest.raises(rx.Eof):
            container._parse(blob[:cut])
    with pytest.raises(rx.Eof):
        container._parse(blob[:-1])
    # a missing marker nibble, and other words
    for word in (0, 1, 0xA0000001, 0x60000001, 0x90000001):
        bad = bytearray(blob)
        bad[12:16] = int(word).to_bytes(4, "little")
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
        assert not container.header_is_wellformed(bytes(bad))
    # stored blocks: 0x4A / 0x5A; other high bits
    for ver in (0x4A, 0x5A, 0x2A, 0x8A):
        bad = bytearray(blob)
        bad[4] = ver
        with pytest.raises(rx.InvalidInput):
            container._parse(bytes(bad))
    # the other versions have no unit table
    plain = container.pack(streams, offs, P, Bs, total)
    assert plain[4] == 1 and container.unit_layouts(plain) is None and container._parse(plain).unit_layouts is None


def test_pack_refuses_bad_unit_tables_and_combinations(rx):
    from redux_amd import container
    nb, Bs = 19, 64
    total = 18 * Bs + 5
    streams, offs = _made_up(nb)
    ok = np.array([1, 2, 3], dtype=np.uint8)
    for table in (np.array([1, 2], np.uint8), np.array([1, 2, 3, 4], np.uint8), np.array([1, 8, 3], np.uint8),
                  np.array([[1, 2, 3]], np.uint8), np.array([1.0, 2.0, 3.0])):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, P, Bs, total, unit_layouts=table)
    for kw in ({"element_size": 2}, {"filter": "delta"}, {"stored": np.zeros(nb, np.uint8)}, {"base": (0, 0)},
               {"constant": np.zeros(nb, np.uint8)}):
        with pytest.raises(rx.InvalidInput):
            container.pack(streams, offs, P, Bs, total, unit_layouts=ok, **kw)
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("static", nb, mixed=True)
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("adaptive", nb, 2, mixed=True)
    with pytest.raises(rx.InvalidInput):
        container.overhead_bytes("adaptive", nb, stored=True, mixed=True)


# ---- refusals before the library is touched --------------------------------------------------------------------------
def test_refusals_before_the_library_is_touched(rx, monkeypatch):
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
            container.compress_bytes(data, **{"block_size": 256, "layout": "mixed", **kw})
    with pytest.raises(rx.InvalidInput):
        container.compress_bytes(data, 256, layout="Mixed")
    table = np.zeros(1, dtype=np.uint8)
    static = object.__new__(rx.StaticModel)
    for kw in ({"element_size": 2}, {"filter": "delta"}, {"stored": np.zeros(4, np.uint8)}, {"base": b"x"},
               {"constant": True}, {"params": static}):
        for ul in (True, table):
            with pytest.raises(rx.InvalidInput):
                rx.compress_blocks(data, 256, **{"unit_layouts": ul, **kw})
        with pytest.raises(rx.InvalidInput):
            rx.decompress_blocks(b"abcd", [0, 1, 2, 3, 4], 256, **{"unit_layouts": table, "length": 1000, **kw})
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(data, 256, layouts=[0, 1])  # (layouts without unit_layouts)


# ---- the CLI's flag rules --------------------------------------------------------------------------------------------
GOOD = [
    ["-c", "--block-size", "65536", "--layout", "mixed"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--checksum"],
    ["-c", "--block-size", "4096", "--layout", "mixed", "--element-size", "1"],
    ["-c", "--block-size", "4096", "--layout", "mixed", "--element-size", "2"],
    ["-c", "--block-size", "4096", "--layout", "mixed", "--element-size", "8", "--checksum"],
    ["-c", "--block-size", "4096", "--layout", "mixed", "--model", "adaptive"],
    ["--layout", "mixed", "-i", "a", "-o", "b", "--block-size", "1", "-c"],
]
BAD = [
    ["-c", "--layout", "mixed"],                                                 # no block size
    ["-c", "--block-size", "0", "--layout", "mixed"],
    ["-c", "--block-size", "65536", "--layout", "Mixed"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--stored"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--filter", "delta"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--base", "b"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--skip-constant"],
    ["-d", "--block-size", "65536", "--layout", "mixed"],
    ["-d", "--layout", "mixed"],
    ["--block-size", "65536", "--layout", "mixed"],                              # neither -c nor -d
    ["-c", "--block-size", "65536", "--layout", "mixed", "--model", "auto"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--model", "static"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--model", "segment-static"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--model", "context-static"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--model", "plane-static", "--element-size", "2"],
    ["-c", "--block-size", "65536", "--layout", "mixed", "--element-size", "3"],
]


def test_cli_parse_accepts_and_refuses(capsys):
    from redux_amd import cli
    for argv in GOOD:
        opts = cli.parse(argv)
        assert opts is not None and opts["layout"] == "mixed" and opts["compress"] is True, argv
    assert "element_size" not in cli.parse(GOOD[0]) and cli.parse(GOOD[3])["element_size"] == 2
    for argv in BAD:
        assert cli.parse(argv) is None, argv
    assert "auto|mixed" in cli.USAGE and "--layout mixed" in cli.__doc__
    assert cli.main(["-c", "--block-size", "65536", "--layout", "mixed", "--filter", "delta"]) == 1
    assert "Usage" in capsys.readouterr().err
