"""order="auto" on the GPU (redux_amd/container.py: compress_bytes; redux_amd/api.py: choose_lag_order): the container it
writes is, byte for byte, the container of the order the estimates favour -- order 3 (version 14) on generated tones, order 1
(version 13) on generated walks -- with a given lag and with lag="auto", it decodes with nothing new, and the estimate stays
within a byte per block of what is written.  Small inputs: B = 4096 and a few frames, and one input above 64 frames at B = 256
for the sampled first stage.

The inputs are GENERATED (tests/test_lag_order_cpu.py: tones; tests/test_lag_cpu.py: channels): no recorded signal."""
import functools

import numpy as np
import pytest

from test_lag_cpu import channels
from test_lag_order_cpu import tones

pytestmark = pytest.mark.gpu

P = (8, 30, 32)
B = 4096
C_, E = 2, 2  # two interleaved int16 channels: the lag is 2


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


@functools.lru_cache(maxsize=None)
def _input(kind):
    return (tones(C_, E, 7) if kind == "tones" else channels(C_, E, 7)).tobytes()


@functools.lru_cache(maxsize=None)
def _fixed(kind, Bk, K, checksum=False):
    """the container of a given order at the known lag: what order="auto" has to reproduce"""
    from redux_amd import container
    return container.compress_bytes(_input(kind), Bk, P, E, filter="lag", lag=C_, order=K, checksum=checksum)


@pytest.mark.parametrize("kind,K,version", [("tones", 3, 14), ("walks", 1, 13)])
@pytest.mark.parametrize("lag", [C_, "auto"])
def test_order_auto_writes_the_container_of_the_favoured_order(rx, kind, K, version, lag):
    from redux_amd import container
    x = _input(kind)
    blob = container.compress_bytes(x, B, P, E, filter="lag", lag=lag, order="auto")
    assert blob == _fixed(kind, B, K), (kind, lag, container.lag(blob), container.order(blob))
    assert blob[4] == version and container.lag(blob) == C_ and container.order(blob) == K
    assert container.decompress_bytes(blob) == x
    sizes = [len(_fixed(kind, B, k)) for k in (1, 2, 3)]
    print("%s, lag %s: order auto wrote order %d; orders 1, 2, 3 write %s bytes" % (kind, lag, K, sizes))
    assert len(blob) == min(sizes)
    checked = container.compress_bytes(x, B, P, E, filter="lag", lag=lag, order="auto", checksum=True)
    assert checked == _fixed(kind, B, K, True) and container.decompress_bytes(checked) == x


@pytest.mark.parametrize("kind,K", [("tones", 3), ("walks", 1)])
def test_choice_and_estimates_against_the_written_containers(rx, kind, K):
    from redux_amd import api, container
    x = _input(kind)
    nb = -(-len(x) // B)
    choice, table = rx.choose_lag_order(x, E, B)
    lag, every = rx.choose_lag(x, E, B)
    assert choice == (C_, K) and lag == C_
    assert sorted({S for S, _ in table}) == api.lag_finalists(every) and 1 in {S for S, _ in table} and len(table) <= 12
    assert all(table[(S, 1)] == every[S] for S in {S for S, _ in table})   # order 1 is the lag estimate
    assert table[choice] <= every[lag] and table[choice] <= table[(1, 1)]  # never above lag="auto" alone, nor above zigzag
    assert rx.choose_lag_order(x, E, B, C_) == (choice, {(C_, k): table[(C_, k)] for k in (1, 2, 3)})
    est = container.estimate_lag_order_bytes(x, E, B, [(C_, 1), (C_, 2), (C_, 3)])
    for k in (1, 2, 3):
        wrote = len(_fixed(kind, B, k))
        print("%s, order %d: estimated %d, written %d bytes (%d blocks)" % (kind, k, est[(C_, k)], wrote, nb))
        assert abs(est[(C_, k)] - wrote) <= nb  # a byte per block
    assert min(est, key=lambda c: (est[c], c[1])) == choice


@pytest.mark.parametrize("kind,K", [("tones", 3), ("walks", 1)])
def test_the_sampled_first_stage_on_more_than_64_frames(rx, kind, K):
    from redux_amd import api, container
    Bk = 256
    x = _input(kind)
    frames = -(-len(x) // (E * Bk))
    assert frames > api.LAG_SAMPLE_FRAMES and api.lag_frame_step(frames) == 2
    blob = container.compress_bytes(x, Bk, P, E, filter="lag", lag="auto", order="auto")
    assert blob == _fixed(kind, Bk, K) and container.lag(blob) == C_ and container.order(blob) == K
    assert container.decompress_bytes(blob) == x
    choice, table = rx.choose_lag_order(x, E, Bk)
    sampled = rx.estimate_lags(x, E, Bk, None, P, frame_step=2)
    assert choice == (C_, K) and sorted({S for S, _ in table}) == api.lag_finalists(sampled)
    assert table == rx.estimate_lag_orders(x, E, Bk, api.lag_order_candidates(api.lag_finalists(sampled)), P)  # exact, every frame


def test_cli_order_auto_round_trip(rx, tmp_path):
    from redux_amd import cli, container
    x = _input("tones")
    src, packed, back = tmp_path / "in.bin", tmp_path / "out.rdx", tmp_path / "back.bin"
    src.write_bytes(x)
    head = ["-c", "-i", str(src), "-o", str(packed), "--block-size", str(B), "--element-size", str(E), "--filter", "lag"]
    for lag, extra in ((str(C_), []), ("auto", []), ("auto", ["--checksum"])):
        assert cli.main(head + ["--lag", lag, "--order-auto"] + extra) == 0
        blob = packed.read_bytes()
        assert blob == _fixed("tones", B, 3, bool(extra))
        assert cli.main(["-d", "-i", str(packed), "-o", str(back)]) == 0
        assert back.read_bytes() == x
    assert container.order(packed.read_bytes()) == 3
