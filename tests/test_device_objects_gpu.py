"""The device coder objects, reused: every configuration of DeviceEncoder / DeviceDecoder and the four static coder objects
code a 4-block ragged input, then 1 byte, then 0 bytes on the SAME object, so the later calls return shorter views of
buffers that still hold the earlier calls' data.  Every call is held against the host call compress_blocks on the same bytes
and options, and decoded back."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PARAMS = (8, 30, 32)
B = 4096
LENS = (3 * B + 5, 1, 0)
E_STATIC = 4  # the element size of the plane-static and segment-static coders


@pytest.fixture(scope="module")
def rx():
    import redux_amd
    return redux_amd


def with_constant_blocks(a, value, block):
    """a with an all-equal block, and with the bytes that make block 1 of its 4-byte plane layout all-equal as well: plane p
    of the N elements lies at p * N, so that block is the end of plane 1 and the start of plane 2"""
    a[block * B: (block + 1) * B] = value
    N = len(a) // 4
    elements = a[: 4 * N].reshape(N, 4)
    elements[B - N:, 1] = value
    elements[: 2 * B - 2 * N, 2] = value
    return a


class Inputs:
    """the three inputs (host bytes, read-only, and device tensors), the base, and compress_blocks of them, once per options"""

    def __init__(self, rx):
        import torch
        rng = np.random.default_rng(0x0B1EC75)
        first = with_constant_blocks(rng.integers(0, 256, LENS[0], dtype=np.uint8), 0x5A, 1)
        self.base = first ^ with_constant_blocks(rng.integers(0, 256, LENS[0], dtype=np.uint8), 0x11, 2)  # (the same of the XOR)
        self.x = (first, rng.integers(0, 256, LENS[1], dtype=np.uint8), np.zeros(LENS[2], dtype=np.uint8))
        for a in self.x + (self.base,):
            a.setflags(write=False)
        self.d_x = tuple(torch.from_numpy(a.copy()).cuda() for a in self.x)
        self.d_base = torch.from_numpy(self.base.copy()).cuda()
        self.rx = rx
        self.refs = {}

    def ref(self, i, key, model=PARAMS, **options):
        """compress_blocks(x[i], B, model, **options); key names the model and options"""
        if (i, key) not in self.refs:
            self.refs[i, key] = self.rx.compress_blocks(self.x[i], B, model, **options)
        return self.refs[i, key]


@pytest.fixture(scope="module")
def inputs(rx):
    return Inputs(rx)


def check_encode(res, ref):
    """a device encode call against compress_blocks' (streams, offsets, status) -> the streams on the device"""
    import torch
    out, offs, status, summary = res[:4]
    torch.cuda.synchronize()
    assert summary.tolist() == [0, 0]
    assert np.array_equal(offs.cpu().numpy().astype(np.uint64), ref[1])
    assert np.array_equal(status.cpu().numpy(), ref[2])
    total = int(ref[1][-1])
    assert np.array_equal(out[:total].cpu().numpy(), ref[0])
    return out[:total]


def check_decode(res, x, nbytes):
    """a device decode call: nbytes of output that begin with x, one size and one status per block"""
    import torch
    d_out, sizes, status, summary = res
    torch.cuda.synchronize()
    nb = max(1, -(-len(x) // B))
    assert summary.tolist() == [0, 0]
    assert sizes.numel() == nb and status.numel() == nb and status.tolist() == [0] * nb
    assert int(sizes.sum()) == len(x) and d_out.numel() == nbytes
    assert np.array_equal(d_out[: len(x)].cpu().numpy(), x)


OPTIONS = {"none": {}, "delta": {"filter": "delta"}, "base": {"base": True}, "constant": {"constant": True},
           "constant+base": {"constant": True, "base": True}}


@pytest.mark.parametrize("name", list(OPTIONS))
@pytest.mark.parametrize("E", [1, 4])
def test_encoder_and_decoder_reused(rx, inputs, E, name):
    """(E = 1, "none") is the plain coder, (E = 4, "none") the layout alone"""
    opts = OPTIONS[name]
    dev, host = dict(opts), dict(opts)
    if "base" in opts:
        dev["base"], host["base"] = inputs.d_base, inputs.base
    enc = rx.DeviceEncoder(PARAMS, B, LENS[0], element_size=E, **dev)
    dec = rx.DeviceDecoder(PARAMS, B, 4, element_size=E, **dev)
    plain = E == 1 and not opts
    for i, x in enumerate(inputs.x):
        ref = inputs.ref(i, (E, name), element_size=E, **host)
        res = enc.encode(inputs.d_x[i])
        streams = check_encode(res, ref)
        flags = {}
        if "constant" in opts:
            assert len(res) == 5 and np.array_equal(res[4].cpu().numpy(), ref[3])
            assert int(ref[3].sum()) >= (1 if len(x) else 0)   # (the option had a block to skip)
            flags = {"constant": res[4]}
        else:
            assert len(res) == 4
        if plain:
            check_decode(dec.decode(streams, res[1]), x, (res[1].numel() - 1) * B)
        check_decode(dec.decode(streams, res[1], length=len(x), **flags), x, len(x))


def test_plain_decoder_takes_a_length_after_a_call_without(rx, inputs):
    """element size 1 and no options: the object is made with the workspace of decode() without a length, and the first
    call with one grows it"""
    import torch
    x = inputs.x[0]
    ref = inputs.ref(0, (1, "none"), element_size=1)
    streams = torch.from_numpy(np.ascontiguousarray(ref[0])).cuda()
    offs = torch.from_numpy(ref[1].astype(np.int64)).cuda()
    dec = rx.DeviceDecoder(PARAMS, B, 4)
    check_decode(dec.decode(streams, offs), x, 4 * B)
    check_decode(dec.decode(streams, offs, length=len(x)), x, len(x))
    check_decode(dec.decode(streams, offs), x, 4 * B)


def test_static_coder_reused(rx, inputs):
    model = rx.StaticModel.from_data(inputs.x[0], PARAMS)
    c = rx.DeviceStaticCoder.from_data(inputs.d_x[0], PARAMS, B, LENS[0])
    assert np.array_equal(np.array(c.cum[:], dtype=np.uint32), model.cum)
    for i, x in enumerate(inputs.x):
        res = c.encode(inputs.d_x[i])
        streams = check_encode(res, inputs.ref(i, "static", model))
        check_decode(c.decode(streams, res[1]), x, (res[1].numel() - 1) * B)


def test_context_static_coder_reused(rx, inputs):
    model = rx.ContextStaticModel.from_data(inputs.x[0], B, PARAMS)
    c = rx.DeviceContextStaticCoder.from_data(inputs.d_x[0], PARAMS, B, LENS[0])
    assert np.array_equal(c.tables(), model.cums)
    for i, x in enumerate(inputs.x):
        res = c.encode(inputs.d_x[i])
        streams = check_encode(res, inputs.ref(i, "context", model))
        check_decode(c.decode(streams, res[1]), x, (res[1].numel() - 1) * B)


def test_plane_static_coder_reused(rx, inputs):
    model = rx.PlaneStaticModel.from_data(inputs.x[0], E_STATIC, B, PARAMS)
    c = rx.DevicePlaneStaticCoder.from_data(inputs.d_x[0], PARAMS, E_STATIC, B, LENS[0])
    assert np.array_equal(c.tables(), model.cums)
    for i, x in enumerate(inputs.x):
        res = c.encode(inputs.d_x[i])
        streams = check_encode(res, inputs.ref(i, "plane", model))
        check_decode(c.decode(streams, res[1], len(x)), x, len(x))


def test_segment_static_coder_reused(rx, inputs):
    """compress_blocks under a SegmentStaticModel builds the tables from the bytes it codes, so every input goes through
    encode_build first; encode then runs under the tables that call left behind"""
    c = rx.DeviceSegmentStaticCoder.from_data(inputs.d_x[0], PARAMS, E_STATIC, B, LENS[0])
    for i, x in enumerate(inputs.x):
        model = rx.SegmentStaticModel.template(PARAMS, E_STATIC, c.G)
        ref = inputs.ref(i, "segment", model)
        if i == 0:
            check_encode((c.out, c.offsets, c.status, c.summary), ref)   # what from_data left behind
        check_encode(c.encode_build(inputs.d_x[i]), ref)
        assert np.array_equal(c.tables(len(x)), model.cums)
        res = c.encode(inputs.d_x[i])
        streams = check_encode(res, ref)
        check_decode(c.decode(streams, res[1], len(x)), x, len(x))
