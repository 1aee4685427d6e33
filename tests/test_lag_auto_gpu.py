"""lag="auto" on the GPU (redux_amd/api.py: choose_lag; container.compress_bytes(filter="lag", lag="auto"); `--filter lag
--lag auto`): the picks on the inputs of the value claim, the two-pass path against an exact pass over all lags, the
estimate against what is written, an input with no lag structure, and the CLI end to end."""
import numpy as np
import pytest

from test_lag_auto_cpu import B, CLAIMS, channels, records

pytestmark = pytest.mark.gpu

P = (8, 30, 32)


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def bound(nblocks):
    """what a container may differ from its estimate by: TERMINATION_BYTES is the midpoint of a stream's
    0.5 .. 4.5 bytes beyond its ideal length, so 2 bytes per block, and 1 for the ceiling"""
    return 2 * nblocks + 1


@pytest.mark.parametrize("C_,E", CLAIMS)
def test_the_picks(rx, C_, E):
    from redux_amd import container
    x = records(1) if C_ == "records" else channels(C_, E, 100 + 10 * C_ + E)
    want = 4 if C_ == "records" else C_
    S, est = rx.choose_lag(x, E, B)
    assert S == want and len(est) == 256 and est[S] == min(est.values())  # (3 E-frames and a short one: one exact pass)
    buf = container.compress_bytes(x.tobytes(), B, P, E, filter="lag", lag="auto")
    assert container.lag(buf) == want and container.filter(buf) == "lag" and buf[4] == 13
    assert buf == container.compress_bytes(x.tobytes(), B, P, E, filter="lag", lag=want)  # the existing path, byte for byte
    assert container.decompress_bytes(buf) == x.tobytes()
    # the estimate against what is written, for the chosen lag and for lag 1; never above zigzag's by more than the bound
    nb = -(-len(x) // B)
    full = container.estimate_lag_bytes(x, E, B, [want, 1])
    one = container.compress_bytes(x.tobytes(), B, P, E, filter="lag", lag=1)
    zz = container.compress_bytes(x.tobytes(), B, P, E, filter="zigzag")
    print("%s, E = %d: lag %d: %d bytes (estimate %d), lag 1: %d (estimate %d), zigzag %d"
          % (C_, E, want, len(buf), full[want], len(one), full[1], len(zz)))
    assert abs(len(buf) - full[want]) <= bound(nb) and abs(len(one) - full[1]) <= bound(nb)
    assert len(one) == len(zz) and len(buf) <= len(zz) + bound(nb)


def test_two_pass_path_agrees_with_an_exact_pass(rx):
    from redux_amd import api, container
    E, Bk = 2, 256
    rng = np.random.default_rng(7)
    n = 130 * Bk - 37                                                   # elements: 130 frames, the last a short one
    w = np.stack([np.cumsum(np.round(rng.normal(0, 50, n // 3 + 1))) + 5000 * c * (-1) ** c for c in range(3)], 1)
    x = w.reshape(-1)[:n].astype(np.int64).astype("<i2").view(np.uint8)
    frames = -(-len(x) // (E * Bk))
    assert frames == 130 and api.lag_frame_step(frames) == 3
    S, est = rx.choose_lag(x, E, Bk)
    exact = rx.estimate_lags(x, E, Bk)
    sampled = rx.estimate_lags(x, E, Bk, frame_step=3)
    assert S == 3 and S == api.best_lag(exact)
    assert sorted(est) == api.lag_finalists(sampled) and 1 in est and 2 <= len(est) <= 4
    assert all(est[k] == exact[k] for k in est)                          # the second pass is exact on every frame
    buf = container.compress_bytes(x.tobytes(), Bk, P, E, filter="lag", lag="auto", checksum=True)
    assert container.lag(buf) == 3 and buf[4] == 0x1D and container.decompress_bytes(buf) == x.tobytes()
    nb = -(-len(x) // Bk)
    assert abs(len(buf) - container.estimate_lag_bytes(x, E, Bk, [3], checksum=True)[3]) <= bound(nb)


def test_no_false_structure(rx):
    from redux_amd import container
    x = np.random.default_rng(11).integers(0, 256, 70 * 1024 + 3, dtype=np.uint8)  # iid bytes, 71 frames of 1 KiB: two passes
    S, est = rx.choose_lag(x, 1, 1024)
    assert 1 in est and est[S] <= est[1]
    buf = container.compress_bytes(x.tobytes(), 1024, P, 1, filter="lag", lag="auto")
    assert container.lag(buf) == S and container.decompress_bytes(buf) == x.tobytes()
    nb = -(-len(x) // 1024)
    zz = container.compress_bytes(x.tobytes(), 1024, P, 1, filter="zigzag")
    assert len(buf) <= len(zz) + bound(nb)
    empty = container.compress_bytes(b"", 1024, P, 2, filter="lag", lag="auto")    # no bytes: every estimate ties, lag 1
    assert container.lag(empty) == 1 and container.decompress_bytes(empty) == b""


def test_cli_end_to_end(rx, tmp_path):
    from redux_amd import cli, container
    x = channels(3, 2, 132).tobytes()
    src, out, back, part = tmp_path / "pcm.i16", tmp_path / "auto.rdxb", tmp_path / "back.i16", tmp_path / "part.i16"
    src.write_bytes(x)
    common = ["-c", "-i", str(src), "--filter", "lag", "--lag", "auto", "--element-size", "2", "--block-size", "4096"]
    assert cli.main(common + ["-o", str(out)]) == 0
    buf = out.read_bytes()
    assert buf[4] == 13 and container.lag(buf) == 3
    assert cli.main(["-d", "-i", str(out), "-o", str(back)]) == 0 and back.read_bytes() == x
    F = 2 * 4096                                                         # a range across the first frame boundary
    assert cli.main(["-d", "-i", str(out), "-o", str(part), "--range", "%d:%d" % (F - 50, 120)]) == 0
    assert part.read_bytes() == x[F - 50: F + 70]
    assert cli.main(common + ["-o", str(out), "--checksum"]) == 0
    buf = out.read_bytes()
    assert buf[4] == 0x1D and container.lag(buf) == 3 and container.decompress_bytes(buf) == x
    assert cli.main(["-c", "-i", str(src), "-o", str(out), "--filter", "lag", "--lag", "auto"]) == 1  # no block size
