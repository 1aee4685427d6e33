"""`layout="auto"` on the GPU: every layout's estimate against the container that layout really writes, the choice made from
the estimates, its round trip, and the CLI flag end to end."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_layout_auto_cpu import LAYOUTS, TABLE, host_estimates, table_input

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
B = 65536
INPUTS = list(TABLE) + ["canterbury/kennedy.xls", "calgary/geo"]


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def _input(name):
    if name in TABLE:
        return table_input(name).tobytes()
    return open(os.path.join(GOLDEN, "corpora", *name.split("/")), "rb").read()


@functools.lru_cache(maxsize=None)
def _measured(name):
    """(estimates, written lengths) of the eight layouts, each coded once"""
    from redux_amd import container
    data = _input(name)
    est = container.estimate_layout_bytes(data, B, P)
    written = {(E, f): len(container.compress_bytes(data, B, P, E, filter=f)) for E, f in LAYOUTS}
    return est, written


@pytest.mark.parametrize("name", INPUTS)
def test_estimates_against_written_containers_and_the_choice(rx, name):
    from redux_amd import container
    data = _input(name)
    nb = max(1, -(-len(data) // B))
    bound = 2 * nb + 1
    est, written = _measured(name)
    assert list(est) == LAYOUTS
    for key in LAYOUTS:
        print("%s %s: estimate %d, written %d" % (name, key, est[key], written[key]))
    for key in LAYOUTS:
        assert abs(written[key] - est[key]) <= bound, (name, key)
    if name in TABLE:  # the device counts give what the host rule gives on the restatement
        hdr = container.overhead_bytes("adaptive", nb)
        assert {k: v - hdr for k, v in est.items()} == host_estimates(name)
    pick = container.choose_layout(est)
    auto = container.compress_bytes(data, B, P, None, layout="auto")
    assert len(auto) == written[pick]
    assert (container.element_size(auto), container.filter(auto)) == pick
    assert auto[4] == (6 if pick[1] else 1 if pick[0] == 1 else 2)
    assert container.decompress_bytes(auto) == data
    assert len(auto) <= min(written.values()) + 2 * bound
    if name in TABLE:
        _, _, want_filter, want_E = TABLE[name]
        assert pick[1] == want_filter and pick[0] in want_E, (name, pick)


def test_element_size_restricts_the_choice_and_checksum(rx):
    from redux_amd import container
    data = _input("bf16")
    est = container.estimate_layout_bytes(data, B, P, element_size=2)
    assert list(est) == [(2, None), (2, "delta")] and est == {k: _measured("bf16")[0][k] for k in est}
    blob = container.compress_bytes(data, B, P, 2, layout="auto")
    assert (container.element_size(blob), container.filter(blob)) == (2, None) and blob[4] == 2
    ts = _input("timestamps")
    blob = container.compress_bytes(ts, B, P, 4, checksum=True, layout="auto")   # delta at E = 4 loses to plain E = 4
    assert (container.element_size(blob), container.filter(blob)) == (4, None) and blob[4] == 0x12
    assert container.decompress_bytes(blob) == ts
    blob = container.compress_bytes(ts, B, P, None, checksum=True, layout="auto")
    assert (container.element_size(blob), container.filter(blob)) == (8, "delta") and blob[4] == 0x16
    assert container.decompress_bytes(blob) == ts
    empty = container.compress_bytes(b"", B, P, None, layout="auto")     # all eight tie on an empty input
    assert empty[4] == 1 and container.decompress_bytes(empty) == b""


def test_cli_end_to_end(rx, tmp_path):
    from redux_amd import cli, container
    ts = _input("timestamps")
    src, packed, back = tmp_path / "ts.bin", tmp_path / "ts.rdx", tmp_path / "ts.out"
    src.write_bytes(ts)
    assert cli.main(["-c", "--block-size", "65536", "--layout", "auto", "-i", str(src), "-o", str(packed)]) == 0
    buf = packed.read_bytes()
    assert buf[4] == 6 and container.filter(buf) == "delta" and container.element_size(buf) == 8
    assert len(buf) == _measured("timestamps")[1][(8, "delta")]
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0
    assert back.read_bytes() == ts
    assert cli.main(["-c", "--block-size", "65536", "--layout", "auto", "--element-size", "2", "--checksum", "-i", str(src),
                     "-o", str(packed)]) == 0
    buf = packed.read_bytes()
    assert buf[4] == 0x12 and container.filter(buf) is None and container.element_size(buf) == 2
    assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0 and back.read_bytes() == ts
    assert cli.main(["-c", "--block-size", "65536", "--layout", "auto", "--filter", "delta", "-i", str(src), "-o", str(packed)]) == 1
