"""compress_blocks / decompress_blocks over every legal combination of model, element size, block_crc, stored and
length: the streams equal those of the un-suffixed C call (through ctypes) or, for stored blocks, the CPU oracle's, the
CRCs equal zlib's, and every combination round-trips."""
import ctypes as C
import zlib

import numpy as np
import pytest

from oracle import cbind as ox
from test_planes_cpu import planes_ref
from test_stored_cpu import rule

pytestmark = pytest.mark.gpu

P3 = (8, 30, 32)
B = 4096


def _data():
    """incompressible, skewed and constant blocks and a ragged tail: stored and coded blocks side by side"""
    rng = np.random.default_rng(5)
    skew = np.minimum(rng.geometric(0.2, 2 * B), 255).astype(np.uint8)
    return np.concatenate([rng.integers(0, 256, B, dtype=np.uint8), skew, np.full(B, 9, np.uint8),
                           rng.integers(0, 256, B + 123, dtype=np.uint8)])


# (model, element_size, block_crc, stored, length): every combination decompress_blocks takes
COMBOS = [("static", 1, crc, False, False) for crc in (False, True)] + \
         [("adaptive", E, crc, stored, length) for E in (1, 2, 4, 8) for crc in (False, True) for stored in (False, True)
          for length in (False, True) if length or (E == 1 and not stored)]


def _plain(rx, x, model, E):
    """the streams of the un-suffixed C call: redux_encode_blocks, redux_encode_blocks_planes, redux_static_encode_blocks"""
    from redux_amd import _lib
    L = _lib.lib()
    cp = _lib.Params(*P3)
    nb = L.redux_block_count(len(x), B)
    cap = (L.redux_static_encode_bound if model is not None else L.redux_encode_bound)(C.byref(cp), len(x), B)
    out = np.empty(cap, np.uint8)
    offs = np.zeros(nb + 1, np.uint64)
    st = np.zeros(nb, np.int32)
    if model is not None:
        r = L.redux_static_encode_blocks(C.byref(cp), model._cum_ptr(), x.ctypes.data, len(x), B, out.ctypes.data, cap,
                                         offs.ctypes.data, st.ctypes.data)
    elif E == 1:
        r = L.redux_encode_blocks(C.byref(cp), x.ctypes.data, len(x), B, out.ctypes.data, cap, offs.ctypes.data,
                                  st.ctypes.data)
    else:
        r = L.redux_encode_blocks_planes(C.byref(cp), x.ctypes.data, len(x), B, E, out.ctypes.data, cap, offs.ctypes.data,
                                         st.ctypes.data)
    assert r == 0 and (st == 0).all()
    return [out[int(offs[b]): int(offs[b + 1])].tobytes() for b in range(nb)]


@pytest.mark.parametrize("kind,E,crc,stored,length", COMBOS)
def test_every_legal_combination(kind, E, crc, stored, length):
    import redux_amd as rx
    x = _data()
    nb = -(-len(x) // B)
    L = [min(B, len(x) - o) for o in range(0, len(x), B)]
    want_crc = [zlib.crc32(x[o: o + B].tobytes()) for o in range(0, len(x), B)]
    model = rx.StaticModel.from_data(x, P3) if kind == "static" else None
    params = model or P3
    ekw = {"element_size": E}
    if crc:
        ekw["block_crc"] = np.zeros(nb, np.uint32)
    if stored:
        ekw["stored"] = np.full(nb, 0xEE, np.uint8)
    out, offs, st = rx.compress_blocks(x, B, params, **ekw)
    assert (st == 0).all() and len(offs) == nb + 1
    got = [out[int(offs[b]): int(offs[b + 1])].tobytes() for b in range(nb)]
    if stored:  # stored blocks: the rule on the oracle's streams; a stored payload is the block's (plane) bytes
        xp = planes_ref(x, E, B) if E > 1 else x
        streams, ost = ox.compress_blocks(xp, B, P3)
        flags = rule(ost, [len(s) for s in streams], L, rx.STORE_RATIO).astype(np.uint8)
        assert ekw["stored"].tolist() == flags.tolist() and 0 < flags.sum() < nb
        assert got == [xp[b * B: b * B + L[b]].tobytes() if flags[b] else streams[b] for b in range(nb)]
    else:
        assert got == _plain(rx, x, model, E)
    if crc:
        assert ekw["block_crc"].tolist() == want_crc

    dkw = {"element_size": E}
    if length:
        dkw["length"] = len(x)
    if crc:
        dkw["block_crc"] = np.zeros(nb, np.uint32)
    if stored:
        dkw["stored"] = ekw["stored"]
    back, sizes, dst = rx.decompress_blocks(out, offs, B, params, **dkw)
    assert (dst == 0).all() and sizes.tolist() == L
    if length:
        assert back.tobytes() == x.tobytes()
    else:
        assert len(back) == nb * B and b"".join(back[b * B: b * B + L[b]].tobytes() for b in range(nb)) == x.tobytes()
    if crc:
        assert dkw["block_crc"].tolist() == want_crc
