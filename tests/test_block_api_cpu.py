"""compress_blocks / decompress_blocks reject every invalid argument combination with InvalidInput before any device
call, so the whole table runs without a GPU."""
import numpy as np
import pytest

P3 = (8, 30, 32)
B = 100
N = 1000  # 10 blocks
NB = 10


def _static():
    import redux_amd as rx
    return rx.StaticModel(rx.Parameters(*P3), np.arange(258, dtype=np.uint32) * 4)


def _ro(a):
    a.flags.writeable = False
    return a


def u32(n=NB):
    return np.zeros(n, np.uint32)


def u8(n=NB):
    return np.zeros(n, np.uint8)


# (label, keyword arguments of compress_blocks(x, B, ...)); "static" stands for a StaticModel
ENCODE = [
    ("static_stored", dict(params="static", stored=u8())),
    ("static_E2", dict(params="static", element_size=2)),
    ("static_E8_crc", dict(params="static", element_size=8, block_crc=u32())),
    ("E3", dict(element_size=3)),
    ("E0", dict(element_size=0)),
    ("block_size_0", dict(block_size=0)),
    ("block_size_neg", dict(block_size=-1)),
    ("static_block_size_0", dict(params="static", block_size=0)),
    ("crc_dtype", dict(block_crc=np.zeros(NB, np.int32))),
    ("crc_shape", dict(block_crc=u32(NB - 1))),
    ("crc_2d", dict(block_crc=np.zeros((NB, 1), np.uint32))),
    ("crc_readonly", dict(block_crc=_ro(u32()))),
    ("crc_strided", dict(block_crc=u32(2 * NB)[::2])),
    ("crc_list", dict(block_crc=[0] * NB)),
    ("static_crc_shape", dict(params="static", block_crc=u32(NB + 1))),
    ("stored_dtype", dict(stored=np.zeros(NB, np.bool_))),
    ("stored_shape", dict(stored=u8(NB + 1))),
    ("stored_readonly", dict(stored=_ro(u8()))),
    ("stored_E4_dtype", dict(element_size=4, stored=np.zeros(NB, np.uint16))),
    ("stored_crc_shape", dict(stored=u8(), block_crc=u32(1))),
    ("store_ratio_neg", dict(stored=u8(), store_ratio=-1)),
    ("store_ratio_65537", dict(stored=u8(), store_ratio=65537)),
    ("store_ratio_2_32", dict(stored=u8(), store_ratio=1 << 32)),
    ("store_ratio_float", dict(stored=u8(), store_ratio=0.5)),
]

OFFS = np.arange(NB + 1, dtype=np.uint64) * 3
STREAMS = np.zeros(3 * NB, np.uint8)

# (label, keyword arguments of decompress_blocks(STREAMS, OFFS, B, ...))
DECODE = [
    ("static_stored", dict(params="static", stored=u8(), length=N)),
    ("static_E2", dict(params="static", element_size=2, length=N)),
    ("static_E2_no_length", dict(params="static", element_size=2)),
    ("static_length", dict(params="static", length=N)),
    ("stored_no_length", dict(stored=u8())),
    ("E2_no_length", dict(element_size=2)),
    ("E8_crc_no_length", dict(element_size=8, block_crc=u32())),
    ("E3", dict(element_size=3, length=N)),
    ("block_size_0", dict(block_size=0)),
    ("block_size_neg", dict(block_size=-1)),
    ("block_size_0_length", dict(block_size=0, length=N)),
    ("block_size_neg_E2", dict(block_size=-5, element_size=2, length=N)),
    ("block_size_0_stored", dict(block_size=0, stored=u8(), length=N)),
    ("static_block_size_0", dict(params="static", block_size=0)),
    ("static_block_size_neg", dict(params="static", block_size=-1)),
    ("offsets_empty", dict(offsets=np.zeros(0, np.uint64))),
    ("offsets_decreasing", dict(offsets=OFFS[::-1].copy())),
    ("offsets_past_streams", dict(offsets=OFFS + 1)),
    ("static_offsets_past_streams", dict(params="static", offsets=OFFS * 2)),
    ("length_count_mismatch", dict(length=N + B)),
    ("length_count_mismatch_E2", dict(element_size=2, length=N - B)),
    ("length_count_mismatch_stored", dict(stored=u8(), length=N + 1)),
    ("length_negative", dict(length=-1)),
    ("crc_dtype", dict(block_crc=np.zeros(NB, np.uint64))),
    ("crc_shape", dict(block_crc=u32(NB + 1))),
    ("crc_readonly", dict(block_crc=_ro(u32()))),
    ("crc_readonly_length", dict(block_crc=_ro(u32()), length=N)),
    ("static_crc_dtype", dict(params="static", block_crc=np.zeros(NB, np.int64))),
    ("stored_dtype", dict(stored=np.zeros(NB, np.int8), length=N)),
    ("stored_shape", dict(stored=u8(NB - 1), length=N)),
    ("stored_strided", dict(stored=u8(2 * NB)[::2], length=N)),
    ("stored_crc_readonly", dict(stored=u8(), block_crc=_ro(u32()), length=N)),
]


def _model(kw):
    kw = dict(kw)
    if kw.get("params") == "static":
        kw["params"] = _static()
    return kw


@pytest.mark.parametrize("label,kw", ENCODE, ids=[e[0] for e in ENCODE])
def test_compress_blocks_rejects(label, kw):
    import redux_amd as rx
    kw = _model(kw)
    bs = kw.pop("block_size", B)
    with pytest.raises(rx.InvalidInput):
        rx.compress_blocks(np.arange(N, dtype=np.uint64).astype(np.uint8), bs, **kw)


@pytest.mark.parametrize("label,kw", DECODE, ids=[d[0] for d in DECODE])
def test_decompress_blocks_rejects(label, kw):
    import redux_amd as rx
    kw = _model(kw)
    bs = kw.pop("block_size", B)
    offs = kw.pop("offsets", OFFS)
    with pytest.raises(rx.InvalidInput):
        rx.decompress_blocks(STREAMS, offs, bs, **kw)
