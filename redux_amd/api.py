"""Host-side mirror of the reference's public interface for the block-coding path.

Reference surface (file:line under the reference checkout) and what stands for it here:
  redux::Error / Result            src/lib.rs:57-98      -> Error, Eof, InvalidInput, IoError
  model::Parameters::new           src/model/mod.rs:63   -> Parameters(symbol, frequency, code)
  model::AdaptiveTreeModel::new    adaptive_tree.rs:36   -> AdaptiveTreeModel(params)
  redux::compress / decompress     src/lib.rs:102,113    -> compress / decompress (file-like in, file-like out)
  (new) block API                  SURVEY.md 8(b)        -> compress_blocks / decompress_blocks,
                                                            DeviceEncoder / DeviceDecoder (HBM-resident)

Every byte of every stream is produced by the gfx950 kernels behind include/redux_hip.h.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import Params as _CParams


# ---- src/lib.rs:57-98 -------------------------------------------------------------------
class Error(Exception):
    """redux::Error"""
    status = None


class Eof(Error):
    """Error::Eof -- "Unexpected end of file" (src/lib.rs:69)"""
    status = _lib.EOF

    def __str__(self):
        return "Unexpected end of file"


class InvalidInput(Error):
    """Error::InvalidInput (src/lib.rs:70)"""
    status = _lib.INVALID_INPUT

    def __str__(self):
        return "Invalid data found while processing input"


class IoError(Error):
    """Error::IoError -- on this path: a HIP runtime failure"""
    status = _lib.IO_ERROR


class OutputTooSmall(IoError):
    status = _lib.OUTPUT_TOO_SMALL


class Unsupported(Error):
    """Valid Parameters that the device path does not implement (no CPU fallback exists)."""
    status = _lib.UNSUPPORTED


_BY_STATUS = {c.status: c for c in (Eof, InvalidInput, IoError, OutputTooSmall, Unsupported)}


def _raise(status, what=""):
    if status != _lib.OK:
        raise _BY_STATUS.get(status, Error)(what or f"status {status}")


# ---- src/model/mod.rs:32-81 -------------------------------------------------------------
class Parameters:
    """model::Parameters: same eleven fields, same validation rule (mod.rs:64)."""

    def __init__(self, symbol, frequency, code):
        if _lib.lib().redux_params_check(symbol, frequency, code) != _lib.OK:
            raise InvalidInput()
        self.symbol_bits = symbol
        self.symbol_eof = 1 << symbol
        self.symbol_count = (1 << symbol) + 1
        self.freq_bits = frequency
        self.freq_max = (1 << frequency) - 1
        self.code_bits = code
        self.code_min = 0
        self.code_one_fourth = 1 << (code - 2)
        self.code_half = 2 << (code - 2)
        self.code_three_fourths = 3 << (code - 2)
        self.code_max = (1 << code) - 1

    @classmethod
    def new(cls, symbol, frequency, code):
        return cls(symbol, frequency, code)

    def _c(self):
        return _CParams(self.symbol_bits, self.freq_bits, self.code_bits)

    def triple(self):
        return (self.symbol_bits, self.freq_bits, self.code_bits)


class AdaptiveTreeModel:
    """model::AdaptiveTreeModel::new(Parameters) -- the model the device implements.  The
    object only carries the parameters: the tree itself lives in LDS, one per block."""

    def __init__(self, params):
        self.params = params

    @classmethod
    def new(cls, params):
        return cls(params)

    def parameters(self):
        return self.params


class StaticModel:
    """The static-table model (include/redux_hip.h, "static-table model"): Parameters plus a fixed table cum[0..=257].
    StaticModel.from_data builds the table from the data by the rule of "semi-static coding".  compress_blocks and
    decompress_blocks take it where they take Parameters."""

    def __init__(self, params, cum):
        self.params = _params_of(params)
        c = np.ascontiguousarray(cum, dtype=np.int64)
        if c.shape != (258,) or (c < 0).any() or (c > 0xFFFFFFFF).any():
            raise InvalidInput()
        self.cum = c.astype(np.uint32)
        cp = self.params._c()
        _raise(_lib.lib().redux_static_table_check(C.byref(cp), self.cum.ctypes.data_as(C.POINTER(C.c_uint32))))

    @classmethod
    def from_data(cls, data, params=(8, 30, 32), total=None):
        return cls(params, static_table(data, params, total))

    def parameters(self):
        return self.params

    def total(self):
        return int(self.cum[-1])

    def _cum_ptr(self):
        return self.cum.ctypes.data_as(C.POINTER(C.c_uint32))


class PlaneStaticModel:
    """Plane-static coding (include/redux_hip.h, "plane-static coding"): Parameters plus one static table per byte plane,
    cums of shape (E, 258), E = element_size in 2 / 4 / 8; block b of the byte-plane layout is coded under table b mod E.
    PlaneStaticModel.from_data builds the tables from the data.  compress_blocks and decompress_blocks take it where they
    take Parameters; the layout's element size is the model's."""

    def __init__(self, params, cums):
        self.params = _params_of(params)
        c = np.ascontiguousarray(cums, dtype=np.int64)
        if c.ndim != 2 or c.shape[0] not in (2, 4, 8) or c.shape[1] != 258 or (c < 0).any() or (c > 0xFFFFFFFF).any():
            raise InvalidInput()
        self.cums = c.astype(np.uint32)
        self.element_size = int(c.shape[0])
        cp = self.params._c()
        _raise(_lib.lib().redux_plane_static_table_check(C.byref(cp), self.cums.ctypes.data, self.element_size))

    @classmethod
    def from_data(cls, data, element_size, block_size, params=(8, 30, 32), total=None):
        return cls(params, plane_static_tables(data, element_size, block_size, params, total))

    def parameters(self):
        return self.params

    def total(self):
        """the tables' common total (a table without bytes keeps 257)"""
        return int(self.cums[:, -1].max())

    def _cum_ptr(self):
        return self.cums.ctypes.data


SEGMENT_K0 = 4  # default segment: G = 64 * E * SEGMENT_K0 blocks


class ContextStaticModel:
    """Context-static coding (include/redux_hip.h, "context-static coding"): Parameters plus one static table per preceding
    byte, cums of shape (256, 258), all of one total <= 2^16; a byte is coded under the table of the byte before it in
    its block (0 at a block's start).  ContextStaticModel.from_data builds the tables from the data.  compress_blocks and
    decompress_blocks take it where they take Parameters: element size 1, no filter, no stored blocks."""

    def __init__(self, params, cums):
        self.params = _params_of(params)
        c = np.ascontiguousarray(cums, dtype=np.int64)
        if c.shape != (256, 258) or (c < 0).any() or (c > 0xFFFFFFFF).any():
            raise InvalidInput()
        self.cums = c.astype(np.uint32)
        cp = self.params._c()
        _raise(_lib.lib().redux_context_static_table_check(C.byref(cp), self.cums.ctypes.data))

    @classmethod
    def from_data(cls, data, block_size, params=(8, 30, 32), total=None):
        return cls(params, context_static_tables(data, block_size, params, total))

    def parameters(self):
        return self.params

    def total(self):
        return int(self.cums[0, -1])

    def _cum_ptr(self):
        return self.cums.ctypes.data


def default_segment_blocks(element_size):
    """The segment length used when none is given: 64 * E * 4 blocks."""
    return 64 * int(element_size) * SEGMENT_K0


class SegmentStaticModel:
    """Segment-static coding (include/redux_hip.h, "segment-static coding"): Parameters plus static tables per range of
    segment_blocks = 64 * E * k blocks of the byte-plane layout, cums of shape (nseg * E, 258), E = element_size in
    1 / 2 / 4 / 8; block b is coded under table (b // segment_blocks) * E + b % E.  The tables belong to one input: nseg is
    checked against its block count when the model is used.  SegmentStaticModel.from_data codes the data while it builds
    the tables, so compress_blocks(data, block_size, SegmentStaticModel.template(...)) is the one-pass way to get both."""

    def __init__(self, params, cums, element_size, segment_blocks):
        self.params = _params_of(params)
        self.element_size = _check_element_size(element_size)
        G = segment_blocks
        if not isinstance(G, (int, np.integer)) or not 0 < G < 1 << 32 or G % (64 * self.element_size):
            raise InvalidInput()
        self.segment_blocks = int(G)
        self._total = _total_of(self.params, None)  # what compress_blocks builds tables with while the model has none
        self.cums = None
        if cums is not None:
            c = np.ascontiguousarray(cums, dtype=np.int64)
            if c.ndim != 2 or c.shape[0] == 0 or c.shape[0] % self.element_size or c.shape[1] != 258 or (c < 0).any() \
                    or (c > 0xFFFFFFFF).any():
                raise InvalidInput()
            self.cums = c.astype(np.uint32)
            # (every count of blocks that gives this many tables passes the same check: the first of them)
            nb = (c.shape[0] // self.element_size - 1) * self.segment_blocks + 1
            self.check(nb)

    @classmethod
    def template(cls, params=(8, 30, 32), element_size=1, segment_blocks=None, total=None):
        """A model without tables: compress_blocks builds them from the data it codes and returns them in the model."""
        E = _check_element_size(element_size)
        m = cls(params, None, E, default_segment_blocks(E) if segment_blocks is None else segment_blocks)
        m._total = _total_of(m.params, total)
        return m

    @classmethod
    def from_data(cls, data, element_size, block_size, params=(8, 30, 32), segment_blocks=None, total=None):
        E = _check_element_size(element_size)
        G = default_segment_blocks(E) if segment_blocks is None else segment_blocks
        return cls(params, segment_static_tables(data, E, block_size, G, params, total), E, G)

    def check(self, nblocks):
        """redux_segment_static_table_check for an input of nblocks blocks"""
        if self.cums is None:
            raise InvalidInput()
        cp = self.params._c()
        _raise(_lib.lib().redux_segment_static_table_check(C.byref(cp), self.cums.ctypes.data, len(self.cums), int(nblocks),
                                                            self.element_size, self.segment_blocks))

    def parameters(self):
        return self.params

    def total(self):
        """the tables' common total (a table without bytes keeps 257); a template's: the total it will build with"""
        return int(self.cums[:, -1].max()) if self.cums is not None else self._total

    def _cum_ptr(self):
        return self.cums.ctypes.data


def _params_of(model_or_params):
    if isinstance(model_or_params, (AdaptiveTreeModel, StaticModel, PlaneStaticModel, SegmentStaticModel, ContextStaticModel)):
        return model_or_params.params
    if isinstance(model_or_params, Parameters):
        return model_or_params
    if isinstance(model_or_params, (tuple, list)):
        return Parameters(*model_or_params)
    raise TypeError("expected Parameters, AdaptiveTreeModel or a (symbol, frequency, code) triple")


def _adaptive_only(model_or_params):
    """the `_v` calls and compress / decompress code under the adaptive model: a ContextStaticModel there is InvalidInput
    (its tables would be ignored), before the library is touched"""
    if isinstance(model_or_params, ContextStaticModel):
        raise InvalidInput()


MAX_BLOCK_BYTES = 0xFFFFFF00  # largest single block / whole stream the C ABI takes (redux_compress)


def version():
    return _lib.lib().redux_version().decode()


def _u8(data):
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data, dtype=np.uint8)
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _ptr(a):
    return a.ctypes.data if a.size else None


# ---- semi-static coding: the static table built from the data ------------------------------
def default_total(params):
    """The table total used when none is given: min(2^16, freq_max), so the table decodes on the lookup decoder."""
    return min(1 << 16, _params_of(params).freq_max)


def _total_of(params, total):
    T = default_total(params) if total is None else total
    if not isinstance(T, (int, np.integer)) or not 0 <= T < 1 << 32:
        raise InvalidInput()
    return int(T)


def static_table_from_counts(counts, params=(8, 30, 32), total=None):
    """redux_static_table_from_counts: the rule (include/redux_hip.h, "semi-static coding") on u64[256] counts, on the
    host.  Returns np.uint32[258]."""
    P = _params_of(params)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if c.shape != (256,):
        raise InvalidInput()
    cum = np.zeros(258, dtype=np.uint32)
    cp = P._c()
    _raise(_lib.lib().redux_static_table_from_counts(C.byref(cp), c.ctypes.data, _total_of(P, total), cum.ctypes.data))
    return cum


def static_table(data, params=(8, 30, 32), total=None):
    """The static table of `data`: np.uint32[258].  Host data (bytes-like, numpy) goes through redux_static_table; a torch
    uint8 device tensor is counted where it lies (redux_histogram_dev + redux_static_table_dev, one read-back)."""
    P = _params_of(params)
    T = _total_of(P, total)
    cp = P._c()
    L = _lib.lib()
    if not _is_device_tensor(data):
        a = _u8(data)
        cum = np.zeros(258, dtype=np.uint32)
        _raise(L.redux_static_table(C.byref(cp), _ptr(a), len(a), T, cum.ctypes.data))
        return cum
    torch = _torch()
    assert data.dtype == torch.uint8 and data.is_contiguous()
    with torch.cuda.device(data.device):
        counts = torch.zeros(256, dtype=torch.int64, device=data.device)
        d_cum = torch.zeros(258, dtype=torch.int32, device=data.device)
        s = _stream_ptr(torch)
        _raise(L.redux_histogram_dev(C.c_void_p(data.data_ptr()) if data.numel() else None, data.numel(),
                                     C.c_void_p(counts.data_ptr()), None, 0, s))
        _raise(L.redux_static_table_dev(C.byref(cp), C.c_void_p(counts.data_ptr()), T, C.c_void_p(d_cum.data_ptr()), s))
        cum = d_cum.cpu().numpy().view(np.uint32).copy()
    if not cum.any():  # the kernel's mark for N * R >= 2^64
        raise Unsupported()
    return cum


def context_static_tables_from_counts(counts, params=(8, 30, 32), total=None):
    """redux_context_static_tables_from_counts: the rule (include/redux_hip.h, "context-static coding") on u64[256][256]
    pair counts, on the host.  Returns np.uint32[256, 258]."""
    P = _params_of(params)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if c.shape != (256, 256):
        raise InvalidInput()
    cums = np.zeros((256, 258), dtype=np.uint32)
    cp = P._c()
    _raise(_lib.lib().redux_context_static_tables_from_counts(C.byref(cp), c.ctypes.data, _total_of(P, total), cums.ctypes.data))
    return cums


def context_static_tables(data, block_size, params=(8, 30, 32), total=None):
    """The tables of context-static coding for `data` cut into blocks of block_size: np.uint32[256, 258].  Host data goes
    through redux_context_static_tables; a torch uint8 device tensor is counted where it lies
    (redux_context_histogram_dev, redux_context_static_tables_dev, one read-back)."""
    P = _params_of(params)
    T = _total_of(P, total)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    cp = P._c()
    L = _lib.lib()
    if not _is_device_tensor(data):
        a = _u8(data)
        cums = np.zeros((256, 258), dtype=np.uint32)
        _raise(L.redux_context_static_tables(C.byref(cp), _ptr(a), len(a), int(block_size), T, cums.ctypes.data))
        return cums
    torch = _torch()
    with torch.cuda.device(data.device):
        d_cum = _device_context_tables(torch, L, cp, data, int(block_size), T)
        cums = d_cum.cpu().numpy().view(np.uint32).reshape(256, 258).copy()
    if not cums.any(axis=1).all():  # the kernel's mark for N * R >= 2^64
        raise Unsupported()
    return cums


def _device_context_tables(torch, L, cp, d_in, block_size, total):
    """a uint8 device tensor -> its 256 tables as an int32[256 * 258] device tensor"""
    assert d_in.dtype == torch.uint8 and d_in.is_contiguous()
    counts = torch.zeros(256 * 256, dtype=torch.int64, device=d_in.device)
    d_cum = torch.zeros(256 * 258, dtype=torch.int32, device=d_in.device)
    s = _stream_ptr(torch)
    _raise(L.redux_context_histogram_dev(C.c_void_p(d_in.data_ptr()) if d_in.numel() else None, d_in.numel(), block_size,
                                         C.c_void_p(counts.data_ptr()), s))
    _raise(L.redux_context_static_tables_dev(C.byref(cp), C.c_void_p(counts.data_ptr()), total, C.c_void_p(d_cum.data_ptr()), s))
    return d_cum


def plane_static_tables(data, element_size, block_size, params=(8, 30, 32), total=None):
    """The tables of plane-static coding for `data` in ORIGINAL byte order: np.uint32[E, 258].  Host data goes through
    redux_plane_static_tables; a torch uint8 device tensor is laid out and counted where it lies (redux_planes_dev,
    redux_plane_histogram_dev, redux_plane_static_tables_dev, one read-back)."""
    P = _params_of(params)
    T = _total_of(P, total)
    E = _check_element_size(element_size)
    if E == 1 or not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    cp = P._c()
    L = _lib.lib()
    if not _is_device_tensor(data):
        a = _u8(data)
        cums = np.zeros((E, 258), dtype=np.uint32)
        _raise(L.redux_plane_static_tables(C.byref(cp), _ptr(a), len(a), int(block_size), E, T, cums.ctypes.data))
        return cums
    torch = _torch()
    with torch.cuda.device(data.device):
        d_cum = _device_plane_tables(torch, L, cp, planes(data, E, block_size), E, int(block_size), T)
        cums = d_cum.cpu().numpy().view(np.uint32).reshape(E, 258).copy()
    if not cums.any(axis=1).all():  # the kernel's mark for N * R >= 2^64
        raise Unsupported()
    return cums


def _device_plane_tables(torch, L, cp, d_x, E, block_size, total):
    """x' (a uint8 device tensor already in the byte-plane layout) -> its E tables as an int32[E * 258] device tensor"""
    counts = torch.zeros(E * 256, dtype=torch.int64, device=d_x.device)
    d_cum = torch.zeros(E * 258, dtype=torch.int32, device=d_x.device)
    s = _stream_ptr(torch)
    _raise(L.redux_plane_histogram_dev(C.c_void_p(d_x.data_ptr()) if d_x.numel() else None, d_x.numel(), block_size, E,
                                       C.c_void_p(counts.data_ptr()), None, 0, s))
    _raise(L.redux_plane_static_tables_dev(C.byref(cp), C.c_void_p(counts.data_ptr()), E, total, C.c_void_p(d_cum.data_ptr()), s))
    return d_cum


def segment_static_tables_from_counts(counts, nblocks, element_size, segment_blocks, params=(8, 30, 32), total=None):
    """redux_segment_static_tables_from_counts: the rule on u64[nseg * E, 256] counts, on the host -> np.uint32[nseg * E, 258]."""
    P = _params_of(params)
    E = _check_element_size(element_size)
    L = _lib.lib()
    if not isinstance(segment_blocks, (int, np.integer)) or not 0 <= segment_blocks < 1 << 32:
        raise InvalidInput()
    n = L.redux_segment_static_table_count(int(nblocks), E, int(segment_blocks))
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    if n == 0 or c.shape != (n, 256):
        raise InvalidInput()
    cums = np.zeros((n, 258), dtype=np.uint32)
    cp = P._c()
    _raise(L.redux_segment_static_tables_from_counts(C.byref(cp), c.ctypes.data, int(nblocks), E, int(segment_blocks),
                                                     _total_of(P, total), cums.ctypes.data))
    return cums


def segment_static_tables(data, element_size, block_size, segment_blocks=None, params=(8, 30, 32), total=None):
    """The tables of segment-static coding for `data` in ORIGINAL byte order: np.uint32[nseg * E, 258].  A torch uint8
    device tensor is laid out and counted where it lies (redux_planes_dev, redux_segment_histogram_dev,
    redux_segment_static_tables_dev, one read-back).  Host data: the tables are those the one-pass encode builds
    (redux_segment_static_encode_blocks_crc), whose streams are dropped."""
    P = _params_of(params)
    T = _total_of(P, total)
    E = _check_element_size(element_size)
    G = default_segment_blocks(E) if segment_blocks is None else segment_blocks
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    m = SegmentStaticModel(P, None, E, G)  # (checks G)
    m._total = T
    if not _is_device_tensor(data):
        compress_blocks(data, int(block_size), m)
        return m.cums
    torch = _torch()
    L = _lib.lib()
    cp = P._c()
    with torch.cuda.device(data.device):
        d_x = planes(data, E, block_size) if E > 1 else data
        n = L.redux_segment_static_table_count(L.redux_block_count(d_x.numel(), int(block_size)), E, m.segment_blocks)
        counts = torch.zeros(n * 256, dtype=torch.int64, device=d_x.device)
        d_cum = torch.zeros(n * 258, dtype=torch.int32, device=d_x.device)
        s = _stream_ptr(torch)
        _raise(L.redux_segment_histogram_dev(C.c_void_p(d_x.data_ptr()) if d_x.numel() else None, d_x.numel(), int(block_size), E,
                                             m.segment_blocks, C.c_void_p(counts.data_ptr()), s))
        _raise(L.redux_segment_static_tables_dev(C.byref(cp), C.c_void_p(counts.data_ptr()),
                                                 L.redux_block_count(d_x.numel(), int(block_size)), E, m.segment_blocks, T,
                                                 C.c_void_p(d_cum.data_ptr()), s))
        cums = d_cum.cpu().numpy().view(np.uint32).reshape(n, 258).copy()
    if not cums.any(axis=1).all():  # the kernel's mark for N * R >= 2^64
        raise Unsupported()
    return cums


def _is_device_tensor(x):
    try:
        import torch
    except ImportError:
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda


# ---- block API, host buffers ------------------------------------------------------------
def _check_element_size(element_size):
    """1 (no layout), 2, 4 or 8; anything else is InvalidInput (redux_planes_check)."""
    if not isinstance(element_size, (int, np.integer)) or not 0 < element_size < 1 << 32 \
            or _lib.lib().redux_planes_check(int(element_size)) != _lib.OK:
        raise InvalidInput()
    return int(element_size)


# The filter in front of the byte-plane layout, as the C entry points name it (include/redux_hip.h): the infix of
# redux_{encode,decode}_{infix}_{dev,workspace_bytes}, redux_{encode,decode}_blocks_{infix} and redux_{infix}_planes_dev,
# whether those take a (base, base_len) pair, and whether decoding needs the length for every element size.  A new filter
# is a new row here (and a Filter value in redux_hip.hip, and a version row in container.py).  lag: the lag of the lagged
# delta filter, which its entry points take behind the element size; None for every other front.  order: the order of
# higher-order lagged differences, which their entry points take behind the lag; None for every other front.  record: the
# (record size, delta flag) of the record layout, which its entry points take in place of the element size; None elsewhere.
# stride: the stride of the snapshot-stride filter, which its entry points take where the lag filter's take the lag (and its
# decode workspace size and its transform take more: _ws_tail, stride_planes); None for every other front.
_Front = namedtuple("_Front", "infix takes_base needs_length lag order record stride", defaults=(None, None, None, None))
_PLANES = _Front("planes", False, False)                                 # no filter: the layout alone (none for element size 1)
_FILTERS = {"delta": _Front("delta", False, True),                       # filter="delta": the delta filter for integer series
            "zigzag": _Front("zigzag", False, True),                     # filter="zigzag": the same with folded differences
            "lag": _Front("lag", False, True)}                           # filter="lag", lag=S: the predecessor S elements back
_LAG_ORDER = _Front("lag_order", False, True)                            # filter="lag", lag=S, order=2 or 3: the lag filter K times
LAG_MAX = 256  # REDUX_LAG_MAX
LAG_ORDER_MAX = 3  # REDUX_LAG_ORDER_MAX
_RECORD = _Front("record", False, True)                                  # record_size=R: the record layout; filter="delta": its byte delta
RECORD_MAX = 256  # REDUX_RECORD_MAX
_STRIDE = _Front("stride", False, True)                                  # filter="stride", stride=S: the same element one snapshot back
_BASE_OPS = {"xor": _Front("base", True, True),                          # base=: the XOR against the base
             "sub": _Front("base_sub", True, True)}                      # base=, base_op="sub": the folded difference

# what _resolve_front makes of a call's options: the _Front, and whether the constant-block option / the mixed layouts are on
_Resolved = namedtuple("_Resolved", "front constant mixed")

_STATIC_MODELS = (StaticModel, PlaneStaticModel, SegmentStaticModel, ContextStaticModel)


def _resolve_front(params, element_size=1, filter=None, base=None, base_op="xor", constant=None, stored=None, unit_layouts=None,
                   device=False, stride=None, record_size=None, lag=None, order=None):
    """The one place that says which of filter=, base=, base_op=, constant=, stored=, unit_layouts= and the model's kind go
    together; anything else is InvalidInput.  A check on the arguments alone: it touches neither the library nor torch,
    so it comes before any call into either.  -> _Resolved.
    filter: None, "delta", "zigzag" or "lag"; with the adaptive model only, and not with stored blocks.
    lag: with filter="lag" and only with it, an int in 1 .. LAG_MAX; the _Front returned carries it.
    order: None, or with filter="lag" an int in 1 .. LAG_ORDER_MAX.  None and 1 are the lag front itself; 2 and 3 the
    lag_order front, which carries lag and order.
    base: None or a base; as a filter, and not together with one.  base_op: "xor" or "sub", "sub" only with a base and
    without the constant-block option.
    constant: None / False, or the option (True, or the flags); adaptive model only, with or without a base, not with a
    filter or stored blocks.
    unit_layouts: None, or the mixed layouts (any other value); adaptive model only, element size 1 and none of the above.
    device: the device coder objects take a model for its parameters alone and have no stored blocks: only the
    constant-block option and the mixed layouts look at the model's kind there.
    record_size: None, or the record layout (include/redux_hip.h, "record layout"): an int in 2 .. RECORD_MAX; adaptive
    model only, element size 1, filter None or "delta" (the byte delta against the record before), and none of lag=,
    order=, base=, constant=, stored= or unit_layouts=; the _Front returned carries (record size, delta flag).
    stride: with filter="stride" and only with it (include/redux_hip.h, "snapshot-stride filter"): an int of at least 1 (and
    below 2^64); adaptive model only, any element size, and none of stored=, base=, constant=, unit_layouts=, record_size=,
    lag= or order=; the _Front returned carries it."""
    static = isinstance(params, _STATIC_MODELS)
    if stride is not None or (isinstance(filter, str) and filter == "stride"):
        if stride is None or not (isinstance(filter, str) and filter == "stride") or isinstance(stride, bool) \
                or not isinstance(stride, (int, np.integer)) or not 1 <= stride < 1 << 64 or static \
                or any(x is not None for x in (stored, base, unit_layouts, record_size, lag, order)) \
                or not (constant is None or constant is False):
            raise InvalidInput()
        return _Resolved(_STRIDE._replace(stride=int(stride)), False, False)
    if record_size is not None:
        if isinstance(record_size, bool) or not isinstance(record_size, (int, np.integer)) or not 2 <= record_size <= RECORD_MAX \
                or static or not isinstance(element_size, (int, np.integer)) or isinstance(element_size, bool) or element_size != 1 \
                or not (filter is None or (isinstance(filter, str) and filter == "delta")) \
                or any(x is not None for x in (lag, order, base, stored, unit_layouts)) \
                or not (constant is None or constant is False):
            raise InvalidInput()
        return _Resolved(_RECORD._replace(record=(int(record_size), 1 if filter is not None else 0)), False, False)
    const = not (constant is None or constant is False)
    mixed = unit_layouts is not None
    if (lag is not None) != (isinstance(filter, str) and filter == "lag") or (lag is not None and (
            isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag <= LAG_MAX)):
        raise InvalidInput()
    if order is not None and (lag is None or isinstance(order, bool) or not isinstance(order, (int, np.integer))
                              or not 1 <= order <= LAG_ORDER_MAX):
        raise InvalidInput()
    if not isinstance(base_op, str) or base_op not in _BASE_OPS or (base_op == "sub" and (base is None or const)):
        raise InvalidInput()
    if mixed and (static or not isinstance(element_size, (int, np.integer)) or element_size != 1 or filter is not None
                  or stored is not None or base is not None or const):
        raise InvalidInput()
    filtered = stored is None and not (static and not device)  # where a filter or a base may stand
    if const and (static or stored is not None or filter is not None):
        raise InvalidInput()
    if base is not None and (not filtered or filter is not None):
        raise InvalidInput()
    if filter is not None and (not filtered or not isinstance(filter, str) or filter not in _FILTERS):
        raise InvalidInput()
    front = _FILTERS[filter] if filter is not None else _BASE_OPS[base_op] if base is not None else _PLANES
    if lag is not None:
        front = front._replace(lag=int(lag))
        if order is not None and order > 1:
            front = _LAG_ORDER._replace(lag=int(lag), order=int(order))
    return _Resolved(front, const, mixed)


def _no_front(filter=None, constant=None):
    """the calls that take no filter and no constant-block option at all: either is InvalidInput"""
    r = _resolve_front(None, filter=filter, constant=constant)
    if r.front is not _PLANES or r.constant:
        raise InvalidInput()


def _lag_arg(front):
    """what a _Front's entry points take behind the element size: the lag of the lagged delta filter, the lag and the order
    of higher-order lagged differences, or nothing"""
    if front.stride is not None:  # (the snapshot-stride filter's stride stands where the lag does)
        return (front.stride,)
    return () if front.lag is None else (front.lag,) if front.order is None else (front.lag, front.order)


def _elem_args(front, E):
    """what a _Front's entry points take behind the block size: the element size and the lag arguments, or the record
    layout's record size and delta flag"""
    return front.record if front.record is not None else (E, *_lag_arg(front))


def _blocks_entry(L, direction, front):
    """the host-pointer entry point of a _Front, redux_{direction}_blocks_{infix} (the layout's own family got its checksum
    argument later, under a name of its own)"""
    return getattr(L, "redux_%s_blocks_%s" % (direction, "planes_crc" if front is _PLANES else front.infix))


STORE_RATIO = 65536  # stored blocks: store a block whose stream is >= 65536/65536 of its bytes (include/redux_hip.h)


def _array_arg(a, dtype, nb, writable=True):
    """the caller's block_crc= (np.uint32[nblocks], filled in place) or stored= array (np.uint8[nblocks]; filled in
    place on encode) -> its pointer; None -> NULL"""
    if a is None:
        return None
    if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != (nb,) or not a.flags.c_contiguous \
            or (writable and not a.flags.writeable):
        raise InvalidInput()
    return _ptr(a)


MIXED_UNIT_BLOCKS = 8  # REDUX_MIXED_UNIT_BLOCKS: blocks of a unit of the mixed layouts


def _unit_table_arg(table, nunits):
    """a caller's unit table -> a contiguous np.uint8[nunits] with every entry 0 .. 7 (else InvalidInput)"""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint8 or table.shape != (nunits,) or bool((table > 7).any()):
        raise InvalidInput()
    return np.ascontiguousarray(table)


def mixed_units(nbytes, block_size):
    """units of 8 blocks (include/redux_hip.h, "mixed layouts") of an input of nbytes: ceil(nblocks / 8)"""
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30 or nbytes < 0:
        raise InvalidInput()
    return int(_lib.lib().redux_mixed_unit_count(int(nbytes), int(block_size)))


def _compress_blocks_mixed(data, block_size, params, unit_layouts, layouts, block_crc):
    P = _params_of(params)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30:
        raise InvalidInput()
    choose = unit_layouts is True
    mask = _layout_mask(layouts) if choose else 0
    if not choose and layouts is not None:
        raise InvalidInput()
    a = _u8(data)
    L = _lib.lib()
    cp = P._c()
    nunits = L.redux_mixed_unit_count(len(a), block_size)
    table = np.zeros(nunits, dtype=np.uint8) if choose else _unit_table_arg(unit_layouts, nunits).copy()
    _raise(L.redux_device_supports(C.byref(cp)))
    nb = L.redux_block_count(len(a), block_size)
    crc = _array_arg(block_crc, np.uint32, nb)
    cap = L.redux_encode_bound(C.byref(cp), len(a), block_size)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    status = np.zeros(nb, dtype=np.int32)
    _raise(L.redux_encode_blocks_mixed(C.byref(cp), _ptr(a), len(a), block_size, mask, table.ctypes.data, out.ctypes.data, cap,
                                       offs.ctypes.data, status.ctypes.data, crc))
    res = (out[: int(offs[-1])], offs, status)
    return res + (table,) if choose else res


def _decompress_blocks_mixed(streams, offsets, block_size, params, check, length, unit_layouts, block_crc):
    P = _params_of(params)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30 or length is None or int(length) < 0:
        raise InvalidInput()
    length = int(length)
    a = _u8(streams)
    offs = _offsets_in(offsets, len(a))
    nb = len(offs) - 1
    L = _lib.lib()
    if nb != L.redux_block_count(length, block_size):
        raise InvalidInput()
    table = _unit_table_arg(unit_layouts, L.redux_mixed_unit_count(length, block_size))
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    crc = _array_arg(block_crc, np.uint32, nb)
    out = np.empty(max(length, 1), dtype=np.uint8)
    sizes = np.zeros(nb, dtype=np.uint32)
    status = np.zeros(nb, dtype=np.int32)
    st = L.redux_decode_blocks_mixed(C.byref(cp), _ptr(a), offs.ctypes.data, table.ctypes.data, length, block_size, out.ctypes.data,
                                     sizes.ctypes.data, status.ctypes.data, crc)
    if check:
        _raise(st)
    return out[:length], sizes, status


def compress_blocks(data, block_size, params=(8, 30, 32), element_size=1, block_crc=None, stored=None,
                    store_ratio=STORE_RATIO, filter=None, base=None, constant=None, unit_layouts=None, layouts=None,
                    stride=None, record_size=None, lag=None, order=None, base_op="xor"):
    """Per-block redux::compress on the GPU.  Returns (dense streams as uint8 array,
    offsets uint64[nblocks+1], status int32[nblocks]); raises on the first non-OK block.
    element_size 2, 4 or 8: the byte-plane layout of typed data is applied first (include/redux_hip.h, "byte-plane
    layout"): the streams are those of the transformed bytes, which decompress_blocks(..., element_size, length) undoes.
    params may be a StaticModel: the blocks are then coded under its table (redux_static_encode_blocks_crc); no element_size.
    params may be a ContextStaticModel: every byte is coded under the table of the byte before it
    (redux_context_static_encode_blocks_crc); no element_size, no stored=, no filter.
    params may be a PlaneStaticModel: the layout of the model's element size, block b under table b mod E
    (redux_plane_static_encode_blocks_crc); element_size must be 1 (the default: the model's is used) or the model's.
    params may be a SegmentStaticModel (redux_segment_static_encode_blocks_crc): its tables are built from `data` as it is
    coded, with the model's total, and the model holds them afterwards (tables it held before are replaced).
    block_crc: a np.uint32[nblocks] the same call fills with the CRC-32 (zlib.crc32) of every input block, in original
    byte order for every layout (the `_crc` calls of include/redux_hip.h).
    stored: a np.uint8[nblocks] the same call fills with the stored-block flags (include/redux_hip.h, "stored blocks"):
    passing it turns stored blocks on, and block b's payload is then its raw (planes: plane) bytes wherever its stream
    is >= store_ratio / 65536 of them.  decompress_blocks(..., stored=flags, length=...) undoes it.
    filter="delta": the delta filter for integer series in front of the layout, for any element_size (include/redux_hip.h,
    "delta filter": redux_encode_blocks_delta); decompress_blocks(..., element_size, length, filter="delta") undoes it.
    Adaptive model only, and not with stored=.
    filter="zigzag": the delta filter with its differences folded, for series that move both ways (include/redux_hip.h,
    "zigzag-folded delta filter": redux_encode_blocks_zigzag); accepted and refused exactly where "delta" is.
    filter="lag", lag=S (1 .. 256): the zigzag filter with the predecessor S elements back, for S interleaved channels or
    records of S columns (include/redux_hip.h, "lagged delta filter": redux_encode_blocks_lag); accepted and refused where
    "zigzag" is.  A lag without filter="lag", or filter="lag" without one, is InvalidInput.
    order=K (1 .. 3, with filter="lag" only): the lag-S difference applied K times, for sampled signals that are locally
    polynomial (include/redux_hip.h, "higher-order lagged differences": redux_encode_blocks_lag_order).  None and 1 are the
    lagged delta filter itself; on random walks a higher order costs bytes, so nothing chooses it for the caller.
    base: bytes-like of any length, an earlier snapshot of the same data; the XOR against it is coded, for any element_size
    (include/redux_hip.h, "XOR-against-base filter": redux_encode_blocks_base); decompress_blocks(..., element_size, length,
    base=the same bytes) undoes it.  Adaptive model only, and not with stored= or filter=.
    constant: a np.uint8[nblocks] the same call fills with the constant-block flags (include/redux_hip.h, "constant
    blocks": redux_encode_blocks_const), or True: the flags are then allocated here and returned as a fourth value.  A block
    of the coder's input whose bytes are all equal has that one byte as its payload and skips the coder;
    decompress_blocks(..., element_size, length, constant=flags) undoes it.  With or without base=; adaptive model only, and
    not with stored= or filter=.
    unit_layouts: the mixed layouts (include/redux_hip.h, "mixed layouts": redux_encode_blocks_mixed), a layout per unit of 8
    blocks.  True: every unit's layout is chosen on the device among `layouts` (None: all eight; else as layout_cost's) and the
    table, np.uint8[nunits], is returned as a fourth value.  A np.uint8[nunits]: the table is dictated; an entry above 7 is
    InvalidInput.  decompress_blocks(..., unit_layouts=table, length=) undoes it.  Adaptive model only, and with none of
    element_size, filter=, stored=, base= or constant=.
    base_op: "xor" (the default), or "sub" with base=: the folded difference of the elements against the base in place of
    the XOR (include/redux_hip.h, "folded difference against a base": redux_encode_blocks_base_sub);
    decompress_blocks(..., base=, base_op="sub") undoes it.  Not with constant=.
    record_size=R (2 .. 256): the record layout for fixed-width structs (include/redux_hip.h, "record layout":
    redux_encode_blocks_record): every block then holds one byte column of B records of R bytes.  filter="delta" with it is
    the byte delta against the record before (not the integer delta filter).  Adaptive model only, element_size 1, and with
    none of lag=, order=, base=, constant=, stored= or unit_layouts=; decompress_blocks(..., length, record_size=R, filter=)
    undoes it.
    filter="stride", stride=S (1 or more): the snapshot-stride filter for one buffer of T snapshots of the same S elements
    (include/redux_hip.h, "snapshot-stride filter": redux_encode_blocks_stride): every element is predicted by the one S
    elements back, however far that is.  Adaptive model only, any element_size, and with none of the other options; the
    whole input is staged on one device.  decompress_blocks(..., element_size, length, filter="stride", stride=S) undoes it."""
    front, const, mixed = _resolve_front(params, element_size, filter, base, base_op, constant, stored, unit_layouts, lag=lag,
                                         order=order, record_size=record_size, stride=stride)
    if mixed:
        return _compress_blocks_mixed(data, block_size, params, unit_layouts, layouts, block_crc)
    if layouts is not None:
        raise InvalidInput()
    static, plane = isinstance(params, StaticModel), isinstance(params, PlaneStaticModel)
    segment = isinstance(params, SegmentStaticModel)
    context = isinstance(params, ContextStaticModel)
    static = static or context  # (the same checks: element size 1, no stored blocks, no filter)
    plane = plane or segment  # (the checks of a model that brings its own element size)
    P = _params_of(params)
    a = _u8(data)
    L = _lib.lib()
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    E = _check_element_size(element_size)
    # (a static model has one table for all byte planes, and its decoder has no table form for stored blocks; a
    # plane-static model brings its own element size)
    if block_size <= 0 or (static and (E != 1 or stored is not None)) \
            or (plane and (E not in (1, params.element_size) or stored is not None)) or (stored is not None and (
            not isinstance(store_ratio, (int, np.integer)) or not 0 <= store_ratio < 1 << 32)):
        raise InvalidInput()
    nb = L.redux_block_count(len(a), block_size)
    crc = _array_arg(block_crc, np.uint32, nb)
    flags = _array_arg(stored, np.uint8, nb)
    if const:
        cflags = np.zeros(nb, dtype=np.uint8) if constant is True else constant
        cptr = _array_arg(cflags, np.uint8, nb)
    cap = (L.redux_static_encode_bound if static or plane else L.redux_encode_bound)(C.byref(cp), len(a), block_size)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    status = np.zeros(nb, dtype=np.int32)
    if segment:  # the tables are built from the data as it is coded, and left in the model
        n = L.redux_segment_static_table_count(nb, params.element_size, params.segment_blocks)
        cums = np.zeros((n, 258), dtype=np.uint32)
        st = L.redux_segment_static_encode_blocks_crc(C.byref(cp), params.total(), _ptr(a), len(a), block_size, params.element_size,
                                                      params.segment_blocks, cums.ctypes.data, out.ctypes.data, cap,
                                                      offs.ctypes.data, status.ctypes.data, crc)
        if st == _lib.OK or cums.any():
            params.cums = cums
    elif const:
        y = _u8(base) if front.takes_base else _u8(b"")
        st = L.redux_encode_blocks_const(C.byref(cp), _ptr(a), len(a), _ptr(y) if len(y) else None, len(y), block_size, E,
                                         out.ctypes.data, cap, offs.ctypes.data, cptr, status.ctypes.data, crc)
    elif stored is not None:
        st = L.redux_encode_blocks_stored(C.byref(cp), _ptr(a), len(a), block_size, E, int(store_ratio), out.ctypes.data, cap,
                                          offs.ctypes.data, flags, status.ctypes.data, crc)
    elif context:
        st = L.redux_context_static_encode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), len(a), block_size, out.ctypes.data,
                                                      cap, offs.ctypes.data, status.ctypes.data, crc)
    elif static:
        st = L.redux_static_encode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), len(a), block_size, out.ctypes.data,
                                              cap, offs.ctypes.data, status.ctypes.data, crc)
    elif plane:
        st = L.redux_plane_static_encode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), len(a), block_size,
                                                    params.element_size, out.ctypes.data, cap, offs.ctypes.data,
                                                    status.ctypes.data, crc)
    else:  # the adaptive coder behind the front's filter (none, and element size 1, included: the coder without a layout)
        y = _u8(base) if front.takes_base else None
        st = _blocks_entry(L, "encode", front)(C.byref(cp), _ptr(a), len(a), *((_ptr(y), len(y)) if front.takes_base else ()),
                                               block_size, *_elem_args(front, E), out.ctypes.data, cap, offs.ctypes.data,
                                               status.ctypes.data, crc)
    _raise(st)
    if constant is True:
        return out[: int(offs[-1])], offs, status, cflags
    return out[: int(offs[-1])], offs, status


def _offsets_in(offsets, nbytes):
    """the caller's offsets -> np.uint64[nblocks+1]; InvalidInput unless there is at least one entry and every stream
    lies inside the nbytes of the streams, in order (the C calls read streams[offsets[b] .. offsets[b + 1]) from caller
    memory)"""
    offs = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(offs) == 0 or int(offs[-1]) > nbytes or bool((offs[1:] < offs[:-1]).any()):
        raise InvalidInput()
    return offs


def decompress_blocks(streams, offsets, block_size, params=(8, 30, 32), check=True, element_size=1, length=None,
                      block_crc=None, stored=None, filter=None, base=None, constant=None, unit_layouts=None, stride=None, record_size=None, lag=None,
                      order=None, base_op="xor"):
    """Per-block redux::decompress on the GPU.  Returns (out uint8[nblocks*block_size],
    sizes uint32[nblocks], status int32[nblocks]); block b occupies out[b*block_size:][:sizes[b]].
    With element_size > 1 (or a length given) the byte-plane layout is undone: length, the original byte count, is then
    required, there must be redux_block_count(length, block_size) streams, and out is the original bytes, uint8[length]
    (frames with a damaged block hold undefined bytes; their blocks' status says which).
    params may be a StaticModel: the streams are then decoded under its table (redux_static_decode_blocks_crc).
    params may be a ContextStaticModel (redux_context_static_decode_blocks_crc): as a StaticModel.
    params may be a PlaneStaticModel (redux_plane_static_decode_blocks_crc): length is required, element_size is 1 (the
    model's is used) or the model's, and out is the original bytes as with element_size > 1.
    params may be a SegmentStaticModel (redux_segment_static_decode_blocks_crc): as a PlaneStaticModel; its tables must be
    those of an input of this many blocks.
    block_crc: a np.uint32[nblocks] the same call fills with the CRC-32 of what each block decoded to (in original byte
    order: after the inverse byte-plane layout); unspecified for blocks whose status is not OK.
    stored: the np.uint8[nblocks] flags compress_blocks(..., stored=) wrote; length is then required and out is
    uint8[length] in original order, as with element_size > 1.
    filter="delta": the streams are compress_blocks(..., filter="delta")'s (redux_decode_blocks_delta); length is required
    for every element_size, and out is the original bytes.  Adaptive model only, and not with stored=.  filter="zigzag":
    the same for compress_blocks(..., filter="zigzag")'s streams (redux_decode_blocks_zigzag).  filter="lag", lag=S: the
    same for compress_blocks(..., filter="lag", lag=S)'s (redux_decode_blocks_lag); with order=K the same for
    compress_blocks(..., filter="lag", lag=S, order=K)'s (redux_decode_blocks_lag_order for K above 1).
    base: the bytes compress_blocks(..., base=) was given (redux_decode_blocks_base); length is required for every
    element_size, and out is the original bytes.  Adaptive model only, and not with stored= or filter=.
    constant: the np.uint8[nblocks] flags compress_blocks(..., constant=) wrote (redux_decode_blocks_const), with the
    same base= if one was given; length is required for every element_size, and out is the original bytes.  Adaptive model
    only, and not with stored= or filter=.
    unit_layouts: the np.uint8[nunits] table of compress_blocks(..., unit_layouts=) (redux_decode_blocks_mixed); length is
    required, and out is the original bytes.  Adaptive model only, and with none of the options above but block_crc.
    base_op: "sub" for the streams of compress_blocks(..., base=, base_op="sub") (redux_decode_blocks_base_sub).
    record_size=R, with the filter= the streams were made with: the streams are compress_blocks(..., record_size=R)'s
    (redux_decode_blocks_record); length is required, and out is the original bytes.
    filter="stride", stride=S: the streams are compress_blocks(..., filter="stride", stride=S)'s
    (redux_decode_blocks_stride); length is required.  A block that does not decode leaves the bytes at and after it in its
    columns undefined, not only its frame's."""
    front, const, mixed = _resolve_front(params, element_size, filter, base, base_op, constant, stored, unit_layouts, lag=lag,
                                         order=order, record_size=record_size, stride=stride)
    if mixed:
        return _decompress_blocks_mixed(streams, offsets, block_size, params, check, length, unit_layouts, block_crc)
    static, plane = isinstance(params, StaticModel), isinstance(params, PlaneStaticModel)
    segment = isinstance(params, SegmentStaticModel)
    context = isinstance(params, ContextStaticModel)
    static = static or context
    if (front.needs_length or const) and length is None:
        raise InvalidInput()
    plane = plane or segment
    E = _check_element_size(element_size)
    if block_size <= 0 or (static and (E != 1 or length is not None or stored is not None)) \
            or (plane and (E not in (1, params.element_size) or length is None or stored is not None)) \
            or (length is None and (E > 1 or stored is not None)):
        raise InvalidInput()
    P = _params_of(params)
    a = _u8(streams)
    offs = _offsets_in(offsets, len(a))
    nb = len(offs) - 1
    L = _lib.lib()
    length = None if length is None else int(length)
    if length is not None and (length < 0 or nb != L.redux_block_count(length, block_size)):
        raise InvalidInput()
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    crc = _array_arg(block_crc, np.uint32, nb)
    flags = _array_arg(stored, np.uint8, nb, writable=False)
    cptr = _array_arg(constant, np.uint8, nb, writable=False) if const else None
    out = np.empty(nb * block_size if length is None else max(length, 1), dtype=np.uint8)
    sizes = np.zeros(nb, dtype=np.uint32)
    status = np.zeros(nb, dtype=np.int32)
    if segment:
        if params.cums is None:
            raise InvalidInput()
        st = L.redux_segment_static_decode_blocks_crc(C.byref(cp), params._cum_ptr(), len(params.cums), _ptr(a), offs.ctypes.data,
                                                      length, block_size, params.element_size, params.segment_blocks,
                                                      out.ctypes.data, sizes.ctypes.data, status.ctypes.data, crc)
    elif const:
        y = _u8(base) if front.takes_base else _u8(b"")
        st = L.redux_decode_blocks_const(C.byref(cp), _ptr(a), offs.ctypes.data, cptr, _ptr(y) if len(y) else None, len(y),
                                         length, block_size, E, out.ctypes.data, sizes.ctypes.data, status.ctypes.data, crc)
    elif stored is not None:
        st = L.redux_decode_blocks_stored(C.byref(cp), _ptr(a), offs.ctypes.data, flags, length, block_size, E, out.ctypes.data,
                                          out.size, sizes.ctypes.data, status.ctypes.data, crc)
    elif context:
        st = L.redux_context_static_decode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), offs.ctypes.data, nb, block_size,
                                                      out.ctypes.data, out.size, sizes.ctypes.data, status.ctypes.data, crc)
    elif static:
        st = L.redux_static_decode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), offs.ctypes.data, nb, block_size,
                                              out.ctypes.data, out.size, sizes.ctypes.data, status.ctypes.data, crc)
    elif plane:
        st = L.redux_plane_static_decode_blocks_crc(C.byref(cp), params._cum_ptr(), _ptr(a), offs.ctypes.data, length, block_size,
                                                    params.element_size, out.ctypes.data, sizes.ctypes.data, status.ctypes.data,
                                                    crc)
    elif length is not None:  # the adaptive coder behind the front's filter, or behind the layout alone
        y = _u8(base) if front.takes_base else None
        st = _blocks_entry(L, "decode", front)(C.byref(cp), _ptr(a), offs.ctypes.data, *((_ptr(y), len(y)) if front.takes_base else ()),
                                               length, block_size, *_elem_args(front, E), out.ctypes.data, sizes.ctypes.data,
                                               status.ctypes.data, crc)
    else:
        st = L.redux_decode_blocks_crc(C.byref(cp), _ptr(a), offs.ctypes.data, nb, block_size, out.ctypes.data, out.size,
                                       sizes.ctypes.data, status.ctypes.data, crc)
    if check:
        _raise(st)
    return (out if length is None else out[:length]), sizes, status


# ---- several GPUs behind the host-pointer calls ------------------------------------------------
def host_set_devices(device_ids):
    """redux_host_set_devices: later compress_blocks / decompress_blocks calls deal their chunks round-robin over one
    context per entry of device_ids (an id may repeat); [] = back to HIP's current device."""
    ids = np.ascontiguousarray(device_ids, dtype=np.int32)
    _raise(_lib.lib().redux_host_set_devices(ids.ctypes.data if ids.size else None, int(ids.size)))


def host_chunk_plan(nblocks, block_size, ncontexts=1, decode=False, record_size=None):
    """(blocks per chunk, number of chunks) a host-pointer call uses; chunk k runs on context k % ncontexts.  record_size:
    the plan of the record layout's calls, whose chunks are whole frames of record_size blocks."""
    cb, nc = C.c_uint64(), C.c_uint64()
    if record_size is None:
        _raise(_lib.lib().redux_host_chunk_plan(nblocks, block_size, ncontexts, 1 if decode else 0, C.byref(cb), C.byref(nc)))
    else:
        _raise(_lib.lib().redux_host_chunk_plan_record(nblocks, block_size, record_size, ncontexts, 1 if decode else 0,
                                                       C.byref(cb), C.byref(nc)))
    return cb.value, nc.value


def host_set_chunk_bytes(min_bytes=0, max_bytes=0):
    """Test hook: chunk size limits of the host-pointer pipeline (0, 0 = the defaults)."""
    _raise(_lib.lib().redux_host_set_chunk_bytes(min_bytes, max_bytes))


# ---- many independent inputs in one call (tests/corpora.rs:32-85 codes file by file) --------
BLOCK_DTYPE = np.dtype([("offset", "<u8"), ("length", "<u4"), ("index", "<u4")])  # redux_block
BLOCK_IDLE = 0xFFFFFFFF  # REDUX_BLOCK_IDLE


def block_table_v(offsets, lengths, block_size):
    """redux_block_table_v: the block table (launch order) of inputs at `offsets` with `lengths`."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    ln = np.ascontiguousarray(lengths, dtype=np.uint64)
    L = _lib.lib()
    ne = L.redux_block_table_v(off.ctypes.data, ln.ctypes.data, len(ln), block_size, None)  # entries: blocks + idle lanes
    tab = np.zeros(ne, dtype=BLOCK_DTYPE)
    L.redux_block_table_v(off.ctypes.data, ln.ctypes.data, len(ln), block_size, tab.ctypes.data)
    return tab


def compress_blocks_v(inputs, block_size, params=(8, 30, 32), filter=None, constant=None):
    """redux::compress of every block of every input (a list of bytes-like objects), ONE launch for all of
    them; each input is cut into blocks on its own.  Returns (dense streams uint8, offsets
    uint64[nblocks+1], status int32[nblocks], first_block int64[len(inputs)+1]): input i owns blocks
    first_block[i] .. first_block[i+1]-1.  filter: None (the `_v` calls have no delta filter: "delta" is InvalidInput)."""
    _adaptive_only(params)
    _no_front(filter, constant)  # (no filter and no constant blocks in the `_v` calls: InvalidInput)
    P = _params_of(params)
    L = _lib.lib()
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    if block_size <= 0 or len(inputs) == 0:
        raise InvalidInput()
    arrs = [_u8(x) for x in inputs]
    lens = np.array([len(a) for a in arrs], dtype=np.uint64)
    offs_in = np.zeros(len(arrs), dtype=np.uint64)
    offs_in[1:] = np.cumsum(lens)[:-1]
    flat = np.concatenate(arrs) if int(lens.sum()) else np.zeros(0, dtype=np.uint8)
    counts = np.array([L.redux_block_count(int(n), block_size) for n in lens], dtype=np.int64)
    first = np.zeros(len(arrs) + 1, dtype=np.int64)
    first[1:] = np.cumsum(counts)
    nb = int(first[-1])
    cap = nb * L.redux_encode_slot_bytes(C.byref(cp), block_size)
    out = np.empty(cap, dtype=np.uint8)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    status = np.zeros(nb, dtype=np.int32)
    _raise(L.redux_encode_blocks_v(C.byref(cp), _ptr(flat), offs_in.ctypes.data, lens.ctypes.data, len(arrs), block_size,
                                   out.ctypes.data, cap, offs.ctypes.data, status.ctypes.data))
    return out[: int(offs[-1])], offs, status, first


def decompress_blocks_v(streams, offsets, lengths, block_size, params=(8, 30, 32), check=True, filter=None, constant=None):
    """The inverse of compress_blocks_v: `lengths[i]` is the decoded size of input i.  Returns (list of
    uint8 arrays, sizes uint32[nblocks], status int32[nblocks]).  filter: None ("delta" is InvalidInput)."""
    _adaptive_only(params)
    _no_front(filter, constant)  # (no filter and no constant blocks in the `_v` calls: InvalidInput)
    P = _params_of(params)
    L = _lib.lib()
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    a = _u8(streams)
    lens = np.ascontiguousarray(lengths, dtype=np.uint64)
    if block_size <= 0 or len(lens) == 0:
        raise InvalidInput()
    nb = L.redux_block_count_v(lens.ctypes.data, len(lens), block_size)
    offs = _offsets_in(offsets, len(a))
    if nb != len(offs) - 1 or int(offs[0]) != 0:  # (the C call copies streams[offsets[0] .. offsets[nb]) in one piece)
        raise InvalidInput()
    out_off = np.zeros(len(lens), dtype=np.uint64)
    out_off[1:] = np.cumsum(lens)[:-1]
    out = np.zeros(max(1, int(lens.sum())), dtype=np.uint8)
    sizes = np.zeros(nb, dtype=np.uint32)
    status = np.zeros(nb, dtype=np.int32)
    st = L.redux_decode_blocks_v(C.byref(cp), _ptr(a), offs.ctypes.data, out.ctypes.data, out_off.ctypes.data, lens.ctypes.data,
                                 len(lens), block_size, sizes.ctypes.data, status.ctypes.data)
    if check:
        _raise(st)
    return [out[int(o): int(o) + int(n)] for o, n in zip(out_off, lens)], sizes, status


# ---- src/lib.rs:102-120: whole-stream drop-ins --------------------------------------------
def compress(istream, ostream, model, filter=None):
    """redux::compress(istream, ostream, model) -> (bytes_in, bytes_out).  The whole input is
    one block, so the stream equals the reference's; it is coded by one GPU lane.  filter: None (a raw reference stream
    has no delta filter: "delta" is InvalidInput)."""
    _adaptive_only(model)
    _no_front(filter)
    P = _params_of(model)
    a = _u8(istream.read())
    L = _lib.lib()
    cp = P._c()
    cap = L.redux_encode_bound(C.byref(cp), len(a), max(len(a), 1))
    _raise(L.redux_device_supports(C.byref(cp)))
    out = np.empty(cap, dtype=np.uint8)
    bi, bo = C.c_uint64(), C.c_uint64()
    _raise(L.redux_compress(C.byref(cp), _ptr(a), len(a), out.ctypes.data, cap, C.byref(bi), C.byref(bo)))
    ostream.write(out[: bo.value].tobytes())
    return (bi.value, bo.value)


def decompress(istream, ostream, model, max_output=None, filter=None):
    """redux::decompress(istream, ostream, model) -> (bytes_in, bytes_out).  filter: None ("delta" is InvalidInput)."""
    _adaptive_only(model)
    _no_front(filter)
    P = _params_of(model)
    a = _u8(istream.read())
    L = _lib.lib()
    cp = P._c()
    _raise(L.redux_device_supports(C.byref(cp)))
    # The reference writes to an unbounded io::Write (src/lib.rs:113); the C ABI wants a capacity.
    # With no explicit max_output the capacity grows until the stream fits (or the ABI's one-block
    # limit of 0xFFFFFF00 bytes is reached): a highly compressible stream (2 MiB of zeros is
    # ~500 bytes) must not fail because of a guess.
    cap = max_output if max_output is not None else max(64 * len(a), 1 << 20)
    while True:
        cap = min(cap, MAX_BLOCK_BYTES)
        out = np.empty(cap, dtype=np.uint8)
        bi, bo = C.c_uint64(), C.c_uint64()
        st = L.redux_decompress(C.byref(cp), _ptr(a), len(a), out.ctypes.data, cap, C.byref(bi), C.byref(bo))
        if st == _lib.OUTPUT_TOO_SMALL and max_output is None and cap < MAX_BLOCK_BYTES:
            cap *= 8
            continue
        _raise(st)
        break
    ostream.write(out[: bo.value].tobytes())
    return (bi.value, bo.value)


# ---- block API, HBM-resident (torch only provides memory + streams) ------------------------
def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("redux_amd device API needs a GPU (torch.cuda.is_available() is False)")
    return torch


def _stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dptr(t):
    """a device tensor's address for a void* parameter (ctypes converts the int); NULL for a tensor without bytes"""
    return t.data_ptr() if t.numel() else None


def _on_device(method):
    """The C ABI launches on HIP's CURRENT device and on the stream it is handed.  A coder object
    built for cuda:1 while cuda:0 is current would run its kernels on GPU 0 against GPU 1's memory,
    so every launching method makes the object's device current first (torch's current stream of
    that device is then the one passed down)."""
    import functools

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with _torch().cuda.device(self.device):
            return method(self, *args, **kwargs)
    return wrapper


# ---- range reads: the plan and the segmented copy (include/redux_hip.h, "range reads") -------
SEGMENT_DTYPE = np.dtype([("src", "<u8"), ("dst", "<u8"), ("len", "<u8")])  # redux_segment


def _ranges_arg(ranges):
    """the caller's (start, length) pairs -> (starts, lens) as np.uint64; InvalidInput for anything but pairs of integers
    in [0, 2^64)"""
    try:
        pairs = [(int(s), int(n)) for s, n in ranges]
    except (TypeError, ValueError):
        raise InvalidInput()
    if any(not 0 <= v < 1 << 64 for p in pairs for v in p):
        raise InvalidInput()
    a = np.array(pairs, dtype=np.uint64).reshape(-1, 2)
    return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])


def range_plan(total, block_size, granule_blocks, ranges):
    """redux_range_plan: the granules of granule_blocks blocks that the byte ranges (start, length) of an input of `total`
    bytes cover.  -> (runs, virt_off, virt_len): runs the covered granules as ascending disjoint (first granule, count)
    pairs, virt_len the bytes of their concatenation (the virtual input), virt_off[i] where range i begins in it (0 for a
    range without bytes).  A range that leaves [0, total] is InvalidInput.  Host arithmetic: no GPU call."""
    if not 0 <= total < 1 << 64 or not 0 < block_size < 1 << 32 or not 0 < granule_blocks < 1 << 64:
        raise InvalidInput()
    starts, lens = _ranges_arg(ranges)
    n = len(starts)
    first, count, off = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
    nruns, vlen = C.c_uint64(), C.c_uint64()
    _raise(_lib.lib().redux_range_plan(total, block_size, granule_blocks, starts.ctypes.data, lens.ctypes.data, n, first.ctypes.data,
                                       count.ctypes.data, C.byref(nruns), off.ctypes.data, C.byref(vlen)))
    return ([(int(first[r]), int(count[r])) for r in range(nruns.value)], [int(v) for v in off[:n]], vlen.value)


def _segments_arg(segments):
    """(src, dst, len) triples, or an array of SEGMENT_DTYPE -> a contiguous array of SEGMENT_DTYPE"""
    if isinstance(segments, np.ndarray) and segments.dtype == SEGMENT_DTYPE:
        return np.ascontiguousarray(segments)
    try:
        rows = [(int(s), int(d), int(n)) for s, d, n in segments]
    except (TypeError, ValueError):
        raise InvalidInput()
    if any(not 0 <= v < 1 << 64 for r in rows for v in r):
        raise InvalidInput()
    return np.array(rows, dtype=SEGMENT_DTYPE)


def segment_tiles(segments):
    """redux_segment_tiles: the tiles (an array of SEGMENT_DTYPE) the segmented copy cuts the segments into.  No GPU call."""
    segs = _segments_arg(segments)
    L = _lib.lib()
    tiles = np.zeros(L.redux_segment_tiles(segs.ctypes.data, len(segs), None), dtype=SEGMENT_DTYPE)
    L.redux_segment_tiles(segs.ctypes.data, len(segs), tiles.ctypes.data)
    return tiles


def _segment_copy(torch, d_src, d_dst, segs, ws=None):
    """redux_segment_copy_dev on the current stream; ws: a uint8 device tensor to take the workspace from if it is large
    enough (a new one otherwise)"""
    L = _lib.lib()
    need = L.redux_segment_copy_workspace_bytes(segs.ctypes.data, len(segs))
    if ws is None or ws.numel() < need + 8:
        ws = torch.empty(need + 8, dtype=torch.uint8, device=d_dst.device)
    at = ws.data_ptr() + (-ws.data_ptr()) % 8
    _raise(L.redux_segment_copy_dev(_dptr(d_src), d_src.numel(), _dptr(d_dst), d_dst.numel(), segs.ctypes.data, len(segs), at, need,
                                    _stream_ptr(torch)))
    return ws


def segment_copy(d_src, d_dst, segments):
    """d_dst[dst : dst + len] = d_src[src : src + len] for every (src, dst, len) of `segments`, in one launch of
    k_segment_copy on torch's current stream.  d_src, d_dst: contiguous uint8 tensors on one device, at any byte alignment,
    that do not overlap; the destination segments must not overlap each other (InvalidInput, before any GPU call).
    Returns d_dst."""
    torch = _torch()
    for t in (d_src, d_dst):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
            raise InvalidInput()
    if d_src.device != d_dst.device:
        raise InvalidInput()
    with torch.cuda.device(d_dst.device):
        _segment_copy(torch, d_src, d_dst, _segments_arg(segments))
    return d_dst


def _device_base(torch, base, device):
    """base= of the device coder objects: None, or a contiguous uint8 tensor on the coder's device (else InvalidInput)"""
    if base is None:
        return None
    if not isinstance(base, torch.Tensor) or not base.is_cuda or base.dtype != torch.uint8 or not base.is_contiguous() \
            or torch.device(device).index not in (None, base.device.index):
        raise InvalidInput()
    return base


def _base_pair(base):
    """the (base, base_len) arguments of the `_dev` entry points that take a base; (NULL, 0) without one or for an empty one"""
    return (base.data_ptr(), base.numel()) if base is not None and base.numel() else (None, 0)


class _DeviceCoder:
    """What the device coder objects below share: the parameters and sizes, the workspace, the encode-side buffers (out,
    offsets, status, summary), the decode-side buffers (dec_out, dec_sizes, dec_status, dec_summary, made on first use;
    a subclass that decodes sets dec_out_bytes), and the trailing arguments every `_dev` entry point takes.  A subclass
    adds its tables and its C entry points.  Every buffer is read when a call is made, so a caller may swap one."""

    dec_out = None  # (until the first call that decodes)

    def __init__(self, params, block_size, max_in_len, device, nblocks_max=None):
        self.P = _params_of(params)
        self.cp = self.P._c()
        self.block_size = int(block_size)
        self.max_in_len = int(max_in_len)
        self.nblocks_max = _lib.lib().redux_block_count(self.max_in_len, self.block_size) if nblocks_max is None else nblocks_max
        self.device = _torch().device(device)

    def _alloc_workspace(self, nbytes):
        """ws_bytes of room from the 256-byte boundary ws.data_ptr() + ws_off on"""
        torch = _torch()
        self.ws_bytes = nbytes
        self.ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self.ws_off = (-self.ws.data_ptr()) % 256

    def _ws_ptr(self):
        return self.ws.data_ptr() + self.ws_off

    def _alloc_encode(self, out_cap):
        torch = _torch()
        self.out_cap = out_cap
        self.out = torch.empty(max(out_cap, 1), dtype=torch.uint8, device=self.device)
        self.offsets = torch.zeros(self.nblocks_max + 1, dtype=torch.int64, device=self.device)
        self.status = torch.zeros(self.nblocks_max, dtype=torch.int32, device=self.device)
        self.summary = torch.zeros(2, dtype=torch.int32, device=self.device)

    def _new_dec_buffers(self, out_bytes):
        torch = _torch()
        return (torch.empty(out_bytes, dtype=torch.uint8, device=self.device),
                torch.zeros(self.nblocks_max, dtype=torch.int32, device=self.device),
                torch.zeros(self.nblocks_max, dtype=torch.int32, device=self.device),
                torch.zeros(2, dtype=torch.int32, device=self.device))

    def _dec_buffers(self):
        """(out, sizes, status, summary) of the decode side"""
        if self.dec_out is None:
            self.dec_out, self.dec_sizes, self.dec_status, self.dec_summary = self._new_dec_buffers(self.dec_out_bytes)
        return self.dec_out, self.dec_sizes, self.dec_status, self.dec_summary

    def _enc_tail(self):
        """out, out_cap, offsets, status, summary, ws, ws_bytes, stream: how every encode entry point ends"""
        return (self.out.data_ptr(), self.out_cap, self.offsets.data_ptr(), self.status.data_ptr(), self.summary.data_ptr(),
                self._ws_ptr(), self.ws_bytes, _stream_ptr(_torch()))

    def _dec_tail(self):
        """sizes, status, summary, ws, ws_bytes, stream: how every decode entry point ends, after its output"""
        _, sizes, status, summary = self._dec_buffers()
        return (sizes.data_ptr(), status.data_ptr(), summary.data_ptr(), self._ws_ptr(), self.ws_bytes, _stream_ptr(_torch()))

    def _check_input(self, d_in):
        """-> the input's byte count"""
        n = d_in.numel()
        assert d_in.dtype == _torch().uint8 and d_in.is_contiguous() and n <= self.max_in_len
        return n

    def _check_streams(self, d_streams, d_offsets, length=None):
        """-> the number of streams; with a length, InvalidInput unless it is that of an input of `length` bytes"""
        torch = _torch()
        nb = d_offsets.numel() - 1
        assert d_offsets.dtype == torch.int64 and d_streams.dtype == torch.uint8
        if length is None:
            assert 0 <= nb <= self.nblocks_max
        else:
            assert 0 <= length <= self.max_in_len
            if nb != _lib.lib().redux_block_count(length, self.block_size):
                raise InvalidInput()
        return nb

    def _enc_result(self, n):
        """what encoding n bytes returns: views of this object's buffers (valid until the next call)"""
        nb = _lib.lib().redux_block_count(n, self.block_size)
        return self.out, self.offsets[: nb + 1], self.status[:nb], self.summary

    def _dec_result(self, nbytes, nb, out=None):
        d_out, sizes, status, summary = self._dec_buffers()
        return (d_out if out is None else out)[:nbytes], sizes[:nb], status[:nb], summary


class DeviceEncoder(_DeviceCoder):
    """Reusable encoder for inputs of up to max_in_len bytes already resident in HBM.
    Allocates once (workspace, dense output, offsets, status); encode() only enqueues kernels
    on torch's current stream.  base: a uint8 device tensor of any length, an earlier snapshot of the data: encode() codes the
    XOR against it (include/redux_hip.h, "XOR-against-base filter"); not together with filter=.  constant=True: blocks of
    the coder's input whose bytes are all equal skip the coder (include/redux_hip.h, "constant blocks"), with or without
    base=, not together with filter=; encode() then returns the u8 flags as a fifth value.  base_op="sub" with base=: the
    folded difference of the elements against the base in place of the XOR (include/redux_hip.h, "folded difference against a
    base"); not together with constant=True.  filter="lag", lag=S: the lagged delta filter (include/redux_hip.h, "lagged delta
    filter"), where filter="zigzag" may stand; order=K (1 .. 3) with it: the difference applied K times (include/redux_hip.h,
    "higher-order lagged differences").  record_size=R: the record layout for fixed-width structs (include/redux_hip.h, "record
    layout"), with filter=None or "delta", its byte delta; element size 1 and none of the other options.  filter="stride",
    stride=S: the snapshot-stride filter (include/redux_hip.h, "snapshot-stride filter"), with none of the other options."""

    def __init__(self, params, block_size, max_in_len, device="cuda:0", element_size=1, filter=None, base=None, constant=False,
                 mixed=False, layouts=None, stride=None, record_size=None, lag=None, order=None, base_op="xor"):
        # (mixed: with the adaptive model and nothing else; `layouts`: what encode() chooses among, None = all eight)
        self.front, self.constant, self.mixed = _resolve_front(params, element_size, filter, base, base_op, constant,
                                                               unit_layouts=True if mixed else None, device=True, lag=lag,
                                                               order=order, record_size=record_size, stride=stride)
        if self.mixed:
            self.mixed_mask = _layout_mask(layouts)
        elif layouts is not None:
            raise InvalidInput()
        torch = _torch()
        self.base = _device_base(torch, base, device)  # the XOR-against-base filter in front of the layout (encode() only)
        P = _params_of(params)
        L = _lib.lib()
        _raise(L.redux_device_supports(C.byref(P._c())))
        E = self.element_size = _check_element_size(element_size)  # > 1: the byte-plane layout in front of the coder
        super().__init__(P, block_size, max_in_len, device)
        B = self.block_size
        # what encode() runs: the workspace size of the entry point, the entry point, and its arguments between
        # (cp, d_in, n) and the tail
        if self.mixed:  # (encode() fills in the mask and the table)
            if not 0 < B <= 1 << 30:
                raise InvalidInput()
            ws_bytes, self._encode_dev, self._lead = (lambda cp, n, b, e: L.redux_encode_mixed_workspace_bytes(cp, n, b)), \
                L.redux_encode_mixed_dev, (B,)
            self.unit_table = torch.zeros(max(L.redux_mixed_unit_count(self.max_in_len, B), 1), dtype=torch.uint8, device=self.device)
        elif self.constant:  # (the tail then holds the flags as well)
            ws_bytes, self._encode_dev = L.redux_encode_const_workspace_bytes, L.redux_encode_const_dev
            self._lead = (*_base_pair(self.base), B, E)
        elif self.front is _PLANES and E == 1:  # (the coder without a layout)
            ws_bytes, self._encode_dev, self._lead = L.redux_encode_planes_workspace_bytes, L.redux_encode_blocks_dev, (B,)
        else:  # the layered entry points of the front's family
            ws_bytes = getattr(L, "redux_encode_%s_workspace_bytes" % self.front.infix)
            self._encode_dev = getattr(L, "redux_encode_%s_dev" % self.front.infix)
            self._lead = (*(_base_pair(self.base) if self.front.takes_base else ()), B, *_elem_args(self.front, E))
        ws_bytes = ws_bytes(C.byref(self.cp), self.max_in_len, B, _elem_args(self.front, E)[0])
        if (self.constant or self.mixed) and ws_bytes == 0:
            raise Unsupported()  # (the adaptive model with 8-bit symbols and code_bits <= 32 only)
        out_cap = L.redux_encode_bound(C.byref(self.cp), self.max_in_len, B)
        self._alloc_workspace(ws_bytes)
        self._alloc_encode(out_cap)
        self.const_flags = torch.zeros(self.nblocks_max, dtype=torch.uint8, device=self.device) if self.constant else None

    def _plain_only(self):
        """the two phases are the plain coder's; encode() applies the layout and the filter"""
        if self.element_size != 1 or self.front is not _PLANES or self.constant or self.mixed:
            raise Unsupported()

    @_on_device
    def encode_slots(self, d_in):
        """Phase 1 only: the coder kernel (padded slots + sizes inside the workspace)."""
        self._plain_only()
        n = self._check_input(d_in)
        _raise(_lib.lib().redux_encode_slots_dev(C.byref(self.cp), d_in.data_ptr(), n, self.block_size, self.status.data_ptr(),
                                                 self._ws_ptr(), self.ws_bytes, _stream_ptr(_torch())))

    @_on_device
    def compact(self, n):
        """Phase 2 only: scan + gather into the dense output."""
        self._plain_only()
        self.summary.zero_()
        _raise(_lib.lib().redux_compact_slots_dev(C.byref(self.cp), n, self.block_size, *self._enc_tail()))

    @_on_device
    def encode(self, d_in, unit_layouts=None):
        """Full pass, stream-ordered: returns (out, offsets[nblocks+1], status, summary) views
        of this encoder's buffers (valid until the next call).  An encoder made with mixed=True chooses a layout per unit of
        8 blocks on the device (include/redux_hip.h, "mixed layouts") and returns the device table, uint8[nunits], as a fifth
        value; unit_layouts: a uint8 device tensor of nunits entries that dictates the table instead (taken & 7)."""
        n = self._check_input(d_in)
        if self.mixed:
            L = _lib.lib()
            nunits = L.redux_mixed_unit_count(n, self.block_size)
            mask = self.mixed_mask
            if unit_layouts is not None:
                torch = _torch()
                if not isinstance(unit_layouts, torch.Tensor) or not unit_layouts.is_cuda or unit_layouts.dtype != torch.uint8 \
                        or not unit_layouts.is_contiguous() or unit_layouts.numel() != nunits:
                    raise InvalidInput()
                self.unit_table[:nunits].copy_(unit_layouts)
                mask = 0
            self.summary.zero_()
            _raise(self._encode_dev(C.byref(self.cp), _dptr(d_in), n, self.block_size, mask, self.unit_table.data_ptr(),
                                    *self._enc_tail()))
            return self._enc_result(n) + (self.unit_table[:nunits],)
        if unit_layouts is not None:
            raise InvalidInput()
        self.summary.zero_()
        tail = self._enc_tail()
        if self.constant:  # (the flags go between the offsets and the status)
            tail = tail[:3] + (self.const_flags.data_ptr(),) + tail[3:]
        _raise(self._encode_dev(C.byref(self.cp), d_in.data_ptr(), n, *self._lead, *tail))
        res = self._enc_result(n)
        return res + (self.const_flags[: res[2].numel()],) if self.constant else res


class DeviceDecoder(_DeviceCoder):
    """Reusable decoder for up to max_blocks blocks resident in HBM.  element_size > 1: the streams are of the byte-plane
    layout (DeviceEncoder(..., element_size)) and decode(..., length) gives back the original bytes.  filter="delta": the
    streams are DeviceEncoder(..., filter="delta")'s; decode needs the length for every element size; filter="zigzag": the same
    for the delta filter with folded differences (include/redux_hip.h, "zigzag-folded delta filter").  base: the uint8 device
    tensor DeviceEncoder(..., base=) was given; decode needs the length; not together with filter=.  constant=True: the
    streams are DeviceEncoder(..., constant=True)'s; decode needs the length and the flags (decode(..., constant=flags)).
    base_op="sub": the streams are DeviceEncoder(..., base=, base_op="sub")'s.  filter="lag", lag=S: the streams are
    DeviceEncoder(..., filter="lag", lag=S)'s; as filter="zigzag"; order=K: the encoder's order.  record_size=R (with the
    encoder's filter=): the streams are DeviceEncoder(..., record_size=R)'s; decode needs the length, and decode_ranges reads
    whole frames of R blocks.  filter="stride", stride=S: the streams are DeviceEncoder(..., filter="stride", stride=S)'s;
    decode needs the length, and decode_ranges raises Unsupported."""

    def __init__(self, params, block_size, max_blocks, device="cuda:0", element_size=1, filter=None, base=None, constant=False,
                 mixed=False, stride=None, record_size=None, lag=None, order=None, base_op="xor"):
        # (mixed: the streams are DeviceEncoder(..., mixed=True)'s: decode(..., length, unit_layouts=table))
        self.front, self.constant, self.mixed = _resolve_front(params, element_size, filter, base, base_op, constant,
                                                               unit_layouts=True if mixed else None, device=True, lag=lag,
                                                               order=order, record_size=record_size, stride=stride)
        torch = _torch()
        self.base = _device_base(torch, base, device)
        P = _params_of(params)
        L = _lib.lib()
        _raise(L.redux_device_supports(C.byref(P._c())))
        self.element_size = _check_element_size(element_size)
        self.max_blocks = int(max_blocks)
        super().__init__(P, block_size, self.max_blocks * int(block_size), device, nblocks_max=self.max_blocks)
        # what decode(..., length) runs: the entry point and its arguments between the offsets and the length
        if self.mixed:
            if not 0 < self.block_size <= 1 << 30:
                raise InvalidInput()
            self._decode_dev, self._lead, ws_bytes = L.redux_decode_mixed_dev, (), self._layout_ws_bytes(self.max_in_len)
        elif self.constant:  # (the flags of the call come in front of the base pair, which is the call's: _takes_base)
            self._decode_dev, self._lead, self._takes_base = L.redux_decode_const_dev, (), True
            ws_bytes = L.redux_decode_const_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size, self.element_size)
            if ws_bytes == 0:
                raise Unsupported()
        else:  # the front's family (element size 1 without a filter: decode() without a length needs less, and the first
            # one with a length regrows it)
            self._decode_dev = getattr(L, "redux_decode_%s_dev" % self.front.infix)
            self._lead, self._takes_base = (), self.front.takes_base
            ws_bytes = L.redux_decode_workspace_bytes(C.byref(self.cp), self.max_blocks, self.block_size) \
                if self.front is _PLANES and self.element_size == 1 else self._layout_ws_bytes(self.max_in_len)
        self._alloc_workspace(ws_bytes)
        self.out, self.sizes, self.status, self.summary = self._new_dec_buffers(self.max_in_len)

    def _dec_buffers(self):
        """a decoder's buffers go by their plain names and are there from the start"""
        return self.out, self.sizes, self.status, self.summary

    def _layout_ws_bytes(self, nbytes):
        """the workspace of the entry points that undo the layout, for an input of nbytes (the snapshot-stride filter's second
        stage has a share of its own, which never falls as nbytes grows)"""
        if self.front.stride is not None:
            return _lib.lib().redux_decode_stride_workspace_bytes(C.byref(self.cp), nbytes, self.block_size, self.element_size,
                                                                  self.front.stride)
        return _lib.lib().redux_decode_planes_workspace_bytes(C.byref(self.cp), nbytes, self.block_size, self.element_size)

    _takes_base = False  # (the entry points of base= and constant=True take a (base, base_len) pair, whole or gathered)
    _range_bufs = None   # (decode_ranges' buffers, made on its first call)

    @_on_device
    def decode(self, d_streams, d_offsets, length=None, constant=None, unit_layouts=None):
        """length: bytes of the original input; required with element_size > 1 (d_offsets then holds
        redux_block_count(length, block_size) + 1 entries), and the result is out[:length].  constant: the uint8 device
        tensor of nblocks flags the encoder returned, for a decoder made with constant=True (and only for one).
        unit_layouts: the uint8 device tensor of nunits entries the encoder returned, for a decoder made with mixed=True (and
        only for one); the length is then required."""
        return self._decode(d_streams, d_offsets, length, constant, unit_layouts, self.base)

    def _decode(self, d_streams, d_offsets, length, constant, unit_layouts, base):
        """decode()'s body; base: the uint8 device tensor the XOR is undone against, the decoder's own or a gathered one"""
        torch = _torch()
        L = _lib.lib()
        nb = d_offsets.numel() - 1
        assert nb <= self.max_blocks and d_offsets.dtype == torch.int64 and d_streams.dtype == torch.uint8
        if (unit_layouts is None) == self.mixed:
            raise InvalidInput()
        if self.mixed:
            if length is None or length < 0 or L.redux_block_count(int(length), self.block_size) != nb \
                    or not isinstance(unit_layouts, torch.Tensor) or not unit_layouts.is_cuda or unit_layouts.dtype != torch.uint8 \
                    or not unit_layouts.is_contiguous() \
                    or unit_layouts.numel() != L.redux_mixed_unit_count(int(length), self.block_size):
                raise InvalidInput()
            self.summary.zero_()
            _raise(self._decode_dev(C.byref(self.cp), _dptr(d_streams), d_offsets.data_ptr(), unit_layouts.data_ptr(), int(length),
                                    self.block_size, self.out.data_ptr(), *self._dec_tail()))
            return self._dec_result(int(length), nb)
        if (length is None and (self.element_size > 1 or self.front.needs_length or self.constant)) \
                or (length is not None and (length < 0 or L.redux_block_count(int(length), self.block_size) != nb)) \
                or (constant is None) == self.constant:
            raise InvalidInput()
        flags = ()
        if self.constant:
            if not isinstance(constant, torch.Tensor) or not constant.is_cuda or constant.dtype != torch.uint8 \
                    or not constant.is_contiguous() or constant.numel() != nb:
                raise InvalidInput()
            flags = (constant.data_ptr(),)
        if length is None:
            nbytes = nb * self.block_size
            decode_dev, args = L.redux_decode_blocks_dev, (nb, self.block_size, self.out.data_ptr(), self.out.numel())
        else:
            nbytes = int(length)
            if self.element_size == 1 and not self.constant and self.ws_bytes < self._layout_ws_bytes(nbytes):
                self._alloc_workspace(self._layout_ws_bytes(self.max_in_len))
            decode_dev = self._decode_dev
            lead = _base_pair(base) if self._takes_base else self._lead
            args = (*flags, *lead, nbytes, self.block_size, *_elem_args(self.front, self.element_size), self.out.data_ptr())
        self.summary.zero_()
        _raise(decode_dev(C.byref(self.cp), d_streams.data_ptr(), d_offsets.data_ptr(), *args, *self._dec_tail()))
        return self._dec_result(nbytes, nb)

    def _range_buffer(self, name, nbytes):
        """a uint8 device buffer of at least nbytes that decode_ranges keeps between calls, next to the workspace"""
        torch = _torch()
        if self._range_bufs is None:
            self._range_bufs = {}
        t = self._range_bufs.get(name)
        if t is None or t.numel() < nbytes:
            t = self._range_bufs[name] = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        return t

    def _range_copy(self, d_src, d_dst, segs):
        """the segmented copy with its tile table in the buffer decode_ranges keeps (the copies of a call follow each other on
        one stream, so they can share it)"""
        ws = _segment_copy(_torch(), d_src, d_dst, _segments_arg(segs), self._range_buffer("tiles", 0))
        self._range_bufs["tiles"] = ws

    @_on_device
    def decode_ranges(self, d_streams, offsets, length, ranges, out=None, constant=None, unit_layouts=None):
        """The bytes [start, start + n) of every (start, n) of `ranges` of the original input, from streams resident in
        device memory, decoding only the granules the ranges cover (include/redux_hip.h, "range reads"): element_size blocks,
        record_size blocks for a decoder made with one, or 8 for a decoder made with mixed=True.  ONE decode launch whatever the number of ranges: the covered streams are
        gathered into a compact buffer (k_segment_copy), with their entries of `constant` / `unit_layouts` and their bytes
        of the base, decoded by the entry point decode() uses, and the requested bytes scattered into `out`
        (k_segment_copy).
        offsets: the nblocks + 1 stream offsets as a host array of integers, or the int64 device tensor the encoder returned,
        which is copied to the host ONCE per call (a synchronisation: a caller who reads often keeps the host copy).
        length: bytes of the original input.  constant / unit_layouts: as for decode(), for the WHOLE input.
        out: a contiguous uint8 device tensor of sum(n) bytes at any alignment (a view into a larger one is fine); None: a
        new one.  Returns (out, [where each range begins in out]).  A covered block that does not decode raises its status
        (the decoder's summary is read: a synchronisation); ranges that leave [0, length], and covered granules of more than
        max_blocks * block_size bytes, are InvalidInput.  Ranges without bytes make no GPU call.  A decoder made with
        filter="stride" raises Unsupported: an element of that filter needs every snapshot before it."""
        if self.front.stride is not None:
            raise Unsupported()
        torch = _torch()
        L = _lib.lib()
        B = self.block_size
        length = int(length)
        offs = offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
        if offs.ndim != 1 or offs.dtype.kind not in "ui" or length < 0 or len(offs) != L.redux_block_count(length, B) + 1 \
                or d_streams.dtype != torch.uint8 or not d_streams.is_contiguous():
            raise InvalidInput()
        offs = _offsets_in(offs, d_streams.numel())
        nb = len(offs) - 1
        if (unit_layouts is None) == self.mixed or (constant is None) == self.constant:
            raise InvalidInput()
        g = MIXED_UNIT_BLOCKS if self.mixed else self.front.record[0] if self.front.record else self.element_size
        ranges = list(ranges)
        runs, virt_off, virt_len = range_plan(length, B, g, ranges)
        lens = [int(n) for _, n in ranges]
        out_off = [int(v) for v in np.cumsum([0] + lens)[:-1]]
        nout = sum(lens)
        if out is None:
            out = torch.empty(nout, dtype=torch.uint8, device=self.device)
        elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous() \
                or out.numel() != nout or out.device != self.out.device:
            raise InvalidInput()
        if virt_len == 0:
            return out, out_off
        if virt_len > self.max_in_len:
            raise InvalidInput()
        for name, t, n in (("constant", constant, nb), ("unit_layouts", unit_layouts, L.redux_mixed_unit_count(length, B))):
            if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8
                                  or not t.is_contiguous() or t.numel() != n):
                raise InvalidInput()
        # the covered blocks, run by run: their streams as segments, their sizes, their bytes of the base
        blocks = [(f * g, min((f + c) * g, nb)) for f, c in runs]
        sel = np.concatenate([np.arange(b0, b1, dtype=np.int64) for b0, b1 in blocks])
        v_offs = np.zeros(len(sel) + 1, dtype=np.int64)
        v_offs[1:] = np.cumsum((offs[sel + 1] - offs[sel]).astype(np.int64))
        segs, at = [], 0
        for b0, b1 in blocks:
            segs.append((int(offs[b0]), at, int(offs[b1] - offs[b0])))
            at += segs[-1][2]
        d_v = self._range_buffer("streams", at)[:at]
        self._range_copy(d_streams, d_v, segs)
        d_voffs = torch.from_numpy(v_offs).to(self.device)
        v_const = None if constant is None else constant[torch.from_numpy(sel).to(self.device)]
        v_units = None if unit_layouts is None else unit_layouts[torch.from_numpy(np.unique(sel // MIXED_UNIT_BLOCKS)).to(self.device)]
        v_base = self.base
        if self._takes_base and self.base is not None and self.base.numel():
            segs, at = [], 0
            for b0, b1 in blocks:  # (what the base holds of each run: in ascending order a prefix of the virtual input)
                lo, hi = min(b0 * B, self.base.numel()), min(b1 * B, length, self.base.numel())
                segs.append((lo, at, hi - lo))
                at += hi - lo
            v_base = self._range_buffer("base", at)[:at]
            self._range_copy(self.base, v_base, segs)
        res = self._decode(d_v, d_voffs, virt_len, v_const, v_units, v_base)
        st, _ = self.summary.tolist()
        _raise(st)
        self._range_copy(res[0], out, list(zip(virt_off, out_off, lens)))
        return out, out_off


class DeviceStaticCoder(_DeviceCoder):
    """The coder core under a fixed frequency table (include/redux_hip.h
    "static-table model").  cum: 258 cumulative frequencies, cum[0] = 0, strictly increasing,
    cum[257] = total <= freq_max; symbol 256 is EOF.  Same buffers as DeviceEncoder/DeviceDecoder."""

    def __init__(self, params, cum, block_size, max_in_len, device="cuda:0"):
        _torch()
        P = _params_of(params)
        L = _lib.lib()
        self.cum = (C.c_uint32 * 258)(*[int(x) for x in cum])
        _raise(L.redux_static_table_check(C.byref(P._c()), self.cum))
        super().__init__(P, block_size, max_in_len, device)
        ws_bytes = L.redux_static_encode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size)
        out_cap = L.redux_static_encode_bound(C.byref(self.cp), self.max_in_len, self.block_size)
        self._alloc_workspace(ws_bytes)
        self._alloc_encode(out_cap)
        self.dec_out_bytes = self.nblocks_max * self.block_size

    @classmethod
    def from_data(cls, d_in, params, block_size, max_in_len, total=None):
        """A coder whose table is built from d_in (a uint8 device tensor) on the device (static_table)."""
        return cls(params, static_table(d_in, params, total), block_size, max_in_len, device=d_in.device)

    @_on_device
    def encode(self, d_in):
        n = self._check_input(d_in)
        self.summary.zero_()
        _raise(_lib.lib().redux_static_encode_blocks_dev(C.byref(self.cp), self.cum, d_in.data_ptr(), n, self.block_size,
                                                         *self._enc_tail()))
        return self._enc_result(n)

    @_on_device
    def decode(self, d_streams, d_offsets):
        nb = self._check_streams(d_streams, d_offsets)
        d_out, _, _, summary = self._dec_buffers()
        summary.zero_()
        tail = self._dec_tail()  # (this entry point takes no workspace)
        _raise(_lib.lib().redux_static_decode_blocks_dev(C.byref(self.cp), self.cum, d_streams.data_ptr(), d_offsets.data_ptr(), nb,
                                                         self.block_size, d_out.data_ptr(), d_out.numel(), *tail[:3], tail[-1]))
        return self._dec_result(nb * self.block_size, nb)


class DeviceContextStaticCoder(_DeviceCoder):
    """Context-static coding on device tensors (include/redux_hip.h, "context-static coding"): d_cum, an int32[256 * 258]
    device tensor of 256 tables with the common total `total`, stays on the device; every call checks it there."""

    def __init__(self, params, d_cum, total, block_size, max_in_len):
        torch = _torch()
        P = _params_of(params)
        L = _lib.lib()
        assert d_cum.is_cuda and d_cum.dtype == torch.int32 and d_cum.is_contiguous() and d_cum.numel() == 256 * 258
        self.d_cum = d_cum
        self.total = int(total)
        super().__init__(P, block_size, max_in_len, d_cum.device)
        ws_bytes = max(L.redux_context_static_encode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size),
                       L.redux_context_static_decode_workspace_bytes(C.byref(self.cp), self.nblocks_max, self.block_size))
        if ws_bytes == 0:
            raise InvalidInput()
        out_cap = L.redux_context_static_encode_bound(C.byref(self.cp), self.max_in_len, self.block_size)
        self._alloc_workspace(ws_bytes)
        self._alloc_encode(out_cap)
        self.dec_out_bytes = max(self.nblocks_max * self.block_size, 1)

    @classmethod
    def from_data(cls, d_in, params, block_size, max_in_len, total=None):
        """A coder whose tables are built from d_in (a uint8 device tensor) on the device; nothing is read back."""
        torch = _torch()
        P = _params_of(params)
        T = _total_of(P, total)
        with torch.cuda.device(d_in.device):
            d_cum = _device_context_tables(torch, _lib.lib(), P._c(), d_in, int(block_size), T)
        return cls(P, d_cum, T, block_size, max_in_len)

    def tables(self):
        """the tables on the host: np.uint32[256, 258]"""
        return self.d_cum.cpu().numpy().view(np.uint32).reshape(256, 258).copy()

    @_on_device
    def encode(self, d_in):
        n = self._check_input(d_in)
        self.summary.zero_()
        _raise(_lib.lib().redux_context_static_encode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, _dptr(d_in), n,
                                                          self.block_size, *self._enc_tail()))
        return self._enc_result(n)

    @_on_device
    def decode(self, d_streams, d_offsets, out=None):
        """-> (out uint8[nblocks * block_size], sizes, status, summary); block b occupies out[b * block_size:][:sizes[b]].
        out: a uint8 device tensor of at least nblocks * block_size bytes to decode into (default: the coder's own)."""
        nb = self._check_streams(d_streams, d_offsets)
        d_out, _, _, summary = self._dec_buffers()
        if out is not None:
            d_out = out
        assert d_out.dtype == _torch().uint8 and d_out.is_contiguous() and d_out.numel() >= nb * self.block_size
        summary.zero_()
        _raise(_lib.lib().redux_context_static_decode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, d_streams.data_ptr(),
                                                          d_offsets.data_ptr(), nb, self.block_size, d_out.data_ptr(),
                                                          nb * self.block_size, *self._dec_tail()))
        return self._dec_result(nb * self.block_size, nb, out)


class DevicePlaneStaticCoder(_DeviceCoder):
    """Plane-static coding on device tensors (include/redux_hip.h, "plane-static coding"): d_cum, an int32[E * 258] device
    tensor of E tables with the common total `total`, stays on the device.  Input and output are in original byte order."""

    def __init__(self, params, d_cum, total, element_size, block_size, max_in_len):
        torch = _torch()
        P = _params_of(params)
        L = _lib.lib()
        self.E = _check_element_size(element_size)
        assert d_cum.is_cuda and d_cum.dtype == torch.int32 and d_cum.is_contiguous() and d_cum.numel() == self.E * 258
        self.d_cum = d_cum
        self.total = int(total)
        super().__init__(P, block_size, max_in_len, d_cum.device)
        ws_bytes = max(L.redux_plane_static_encode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size, self.E),
                       L.redux_plane_static_decode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size, self.E))
        if ws_bytes == 0:
            raise InvalidInput()
        out_cap = L.redux_plane_static_encode_bound(C.byref(self.cp), self.max_in_len, self.block_size)
        self._alloc_workspace(ws_bytes)
        self._alloc_encode(out_cap)
        self.dec_out_bytes = max(self.max_in_len, 1)

    @classmethod
    def from_data(cls, d_in, params, element_size, block_size, max_in_len, total=None):
        """A coder whose tables are built from d_in (a uint8 device tensor, original order) on the device; nothing is
        read back."""
        torch = _torch()
        P = _params_of(params)
        T = _total_of(P, total)
        E = _check_element_size(element_size)
        with torch.cuda.device(d_in.device):
            d_x = planes(d_in, E, block_size) if E > 1 else d_in
            d_cum = _device_plane_tables(torch, _lib.lib(), P._c(), d_x, E, int(block_size), T)
        return cls(P, d_cum, T, E, block_size, max_in_len)

    def tables(self):
        """the tables on the host: np.uint32[E, 258]"""
        return self.d_cum.cpu().numpy().view(np.uint32).reshape(self.E, 258).copy()

    @_on_device
    def encode(self, d_in):
        n = self._check_input(d_in)
        self.summary.zero_()
        _raise(_lib.lib().redux_plane_static_encode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, _dptr(d_in), n,
                                                        self.block_size, self.E, *self._enc_tail()))
        return self._enc_result(n)

    @_on_device
    def decode(self, d_streams, d_offsets, length):
        """-> (the original bytes uint8[length], sizes, status, summary)"""
        nb = self._check_streams(d_streams, d_offsets, length)
        d_out, _, _, summary = self._dec_buffers()
        summary.zero_()
        _raise(_lib.lib().redux_plane_static_decode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, d_streams.data_ptr(),
                                                        d_offsets.data_ptr(), length, self.block_size, self.E, d_out.data_ptr(),
                                                        *self._dec_tail()))
        return self._dec_result(length, nb)


class DeviceSegmentStaticCoder(_DeviceCoder):
    """Segment-static coding on device tensors (include/redux_hip.h, "segment-static coding").  encode_build(d_in) builds
    the tables from d_in while it codes it (redux_segment_static_build_encode_dev: one layout pass) and leaves them in
    d_cum, an int32[nseg * E * 258] device tensor; encode / decode run under the tables d_cum holds.  Input and output are
    in original byte order."""

    def __init__(self, params, element_size, block_size, max_in_len, segment_blocks=None, total=None, device="cuda:0"):
        torch = _torch()
        P = _params_of(params)
        L = _lib.lib()
        self.E = _check_element_size(element_size)
        self.G = SegmentStaticModel(P, None, self.E,
                                    default_segment_blocks(self.E) if segment_blocks is None else segment_blocks).segment_blocks
        self.total = _total_of(P, total)
        super().__init__(P, block_size, max_in_len, device)
        self.ntables_max = L.redux_segment_static_table_count(self.nblocks_max, self.E, self.G)
        ws_bytes = max(L.redux_segment_static_build_encode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size,
                                                                           self.E, self.G),
                       L.redux_segment_static_decode_workspace_bytes(C.byref(self.cp), self.max_in_len, self.block_size, self.E))
        if ws_bytes == 0:
            raise InvalidInput()
        out_cap = L.redux_segment_static_encode_bound(C.byref(self.cp), self.max_in_len, self.block_size)
        self._alloc_workspace(ws_bytes)
        self.d_cum = torch.zeros(self.ntables_max * 258, dtype=torch.int32, device=self.device)
        self._alloc_encode(out_cap)
        self.dec_out_bytes = max(self.max_in_len, 1)

    @classmethod
    def from_data(cls, d_in, params, element_size, block_size, max_in_len, segment_blocks=None, total=None):
        """A coder whose tables are those of d_in (a uint8 device tensor, original order), built by encode_build: the
        streams of d_in are in .out / .offsets, nothing is read back."""
        c = cls(params, element_size, block_size, max_in_len, segment_blocks, total, d_in.device)
        c.encode_build(d_in)
        return c

    def ntables(self, n):
        L = _lib.lib()
        return L.redux_segment_static_table_count(L.redux_block_count(n, self.block_size), self.E, self.G)

    def tables(self, n):
        """the tables of an n-byte input on the host: np.uint32[nseg * E, 258]"""
        k = self.ntables(n)
        return self.d_cum[: k * 258].cpu().numpy().view(np.uint32).reshape(k, 258).copy()

    def set_tables(self, cums):
        torch = _torch()
        c = np.ascontiguousarray(cums, dtype=np.uint32).reshape(-1)
        assert c.size <= self.d_cum.numel()
        self.d_cum[: c.size] = torch.from_numpy(c.view(np.int32)).to(self.device)

    def _encode(self, d_in, build):
        n = self._check_input(d_in)
        self.summary.zero_()
        L = _lib.lib()
        data = (_dptr(d_in), n, self.block_size, self.E, self.G)
        if build:
            st = L.redux_segment_static_build_encode_dev(C.byref(self.cp), self.total, *data, self.d_cum.data_ptr(), *self._enc_tail())
        else:
            st = L.redux_segment_static_encode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, *data, *self._enc_tail())
        _raise(st)
        return self._enc_result(n)

    @_on_device
    def encode_build(self, d_in):
        return self._encode(d_in, True)

    @_on_device
    def encode(self, d_in):
        return self._encode(d_in, False)

    @_on_device
    def decode(self, d_streams, d_offsets, length):
        """-> (the original bytes uint8[length], sizes, status, summary)"""
        nb = self._check_streams(d_streams, d_offsets, length)
        d_out, _, _, summary = self._dec_buffers()
        summary.zero_()
        _raise(_lib.lib().redux_segment_static_decode_dev(C.byref(self.cp), self.d_cum.data_ptr(), self.total, d_streams.data_ptr(),
                                                          d_offsets.data_ptr(), length, self.block_size, self.E, self.G,
                                                          d_out.data_ptr(), *self._dec_tail()))
        return self._dec_result(length, nb)


# ---- byte-plane layout of typed data ----------------------------------------------------------
def _transform(front, d_src, element_size, block_size, inverse, out, d_base=None):
    """planes / delta_planes / base_planes ...: the transform of a _Front (redux_planes_dev, redux_{infix}_planes_dev) from
    d_src into `out`, on torch's current stream"""
    name = "redux_planes_dev" if front is _PLANES else "redux_%s_planes_dev" % front.infix
    torch = _torch()
    E = _check_element_size(element_size)
    assert d_src.dtype == torch.uint8 and d_src.is_contiguous()
    assert d_base is None or (d_base.dtype == torch.uint8 and d_base.is_contiguous() and d_base.device == d_src.device)
    if block_size <= 0:
        raise InvalidInput()
    n = d_src.numel()
    t = out if out is not None else torch.empty(n, dtype=torch.uint8, device=d_src.device)
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n and t.device == d_src.device
    base = _base_pair(d_base) if front.takes_base else ()
    ws = ()
    if front.stride is not None:  # (its inverse keeps the time segments' sums in a workspace, in front of the stream)
        need = _lib.lib().redux_stride_workspace_bytes(n, E, front.stride) if inverse else 0
        d_ws = torch.empty(need, dtype=torch.uint8, device=t.device) if need else None
        ws = (d_ws.data_ptr() if need else None, need)
    with torch.cuda.device(t.device):
        _raise(getattr(_lib.lib(), name)(d_src.data_ptr(), *base, t.data_ptr(), n, block_size, *_elem_args(front, E),
                                         1 if inverse else 0, *ws, _stream_ptr(torch)))
    return t


def planes(d_src, element_size, block_size, inverse=False, out=None):
    """The byte-plane layout (include/redux_hip.h) of a uint8 device tensor, or its inverse: redux_planes_dev on torch's
    current stream.  out: a uint8 tensor of the same length on the same device (allocated when None)."""
    return _transform(_PLANES, d_src, element_size, block_size, inverse, out)


def delta_planes(d_src, element_size, block_size, inverse=False, out=None):
    """The delta filter followed by the byte-plane layout (include/redux_hip.h, "delta filter") of a uint8 device tensor,
    or their inverse: redux_delta_planes_dev on torch's current stream.  out: as for planes()."""
    return _transform(_resolve_front(None, filter="delta").front, d_src, element_size, block_size, inverse, out)


def zigzag_planes(d_src, element_size, block_size, inverse=False, out=None):
    """The zigzag-folded delta filter followed by the byte-plane layout (include/redux_hip.h, "zigzag-folded delta filter")
    of a uint8 device tensor, or their inverse: redux_zigzag_planes_dev on torch's current stream.  out: as for planes()."""
    return _transform(_resolve_front(None, filter="zigzag").front, d_src, element_size, block_size, inverse, out)


def lag_planes(d_src, element_size, block_size, lag, inverse=False, out=None):
    """The lagged delta filter followed by the byte-plane layout (include/redux_hip.h, "lagged delta filter") of a uint8
    device tensor, or their inverse: redux_lag_planes_dev on torch's current stream.  lag: 1 .. 256.  out: as for planes()."""
    return _transform(_resolve_front(None, filter="lag", lag=lag).front, d_src, element_size, block_size, inverse, out)


def lag_order_planes(d_src, element_size, block_size, lag, order, inverse=False, out=None):
    """Higher-order lagged differences followed by the byte-plane layout (include/redux_hip.h, "higher-order lagged
    differences") of a uint8 device tensor, or their inverse: redux_lag_order_planes_dev on torch's current stream, for order
    1 too.  lag: 1 .. 256; order: 1 .. 3.  out: as for planes()."""
    if order is None:  # (the resolver's "no order" is the lag filter; this call names the order)
        raise InvalidInput()
    _resolve_front(None, filter="lag", lag=lag, order=order)
    return _transform(_LAG_ORDER._replace(lag=int(lag), order=int(order)), d_src, element_size, block_size, inverse, out)


def stride_planes(d_src, element_size, block_size, stride, inverse=False, out=None):
    """The snapshot-stride filter followed by the byte-plane layout (include/redux_hip.h, "snapshot-stride filter") of a uint8
    device tensor, or their inverse: redux_stride_planes_dev on torch's current stream.  stride: 1 or more, in elements.  The
    inverse's workspace (redux_stride_workspace_bytes) is allocated here; torch's allocator keeps it alive for the stream.
    out: as for planes()."""
    return _transform(_resolve_front(None, filter="stride", stride=stride).front, d_src, element_size, block_size, inverse, out)


def stride_kernel_name(nbytes, block_size, element_size, stride, inverse=False, d_src=None, d_dst=None):
    """The kernels stride_planes runs for nbytes bytes (redux_stride_kernel_name; d_src and d_dst, device tensors: their
    alignment counts; None: aligned), joined by " + "; "" for arguments the call refuses."""
    if isinstance(stride, bool) or not isinstance(stride, (int, np.integer)) or not 0 <= stride < 1 << 64 \
            or not isinstance(element_size, (int, np.integer)) or not 0 <= element_size < 1 << 32:
        return ""
    return _lib.lib().redux_stride_kernel_name(int(nbytes), int(block_size), int(element_size), int(stride), 1 if inverse else 0,
                                               None if d_src is None else d_src.data_ptr(),
                                               None if d_dst is None else d_dst.data_ptr()).decode()


def record_planes(d_src, record_size, block_size, delta=False, inverse=False, out=None):
    """The record layout for fixed-width structs (include/redux_hip.h, "record layout") of a uint8 device tensor, or its
    inverse: redux_record_planes_dev on torch's current stream.  record_size: 2 .. RECORD_MAX.  delta: the byte delta
    against the record before, in front of the layout.  out: as for planes()."""
    front = _resolve_front(None, filter="delta" if delta else None, record_size=record_size).front
    return _transform(front, d_src, 1, block_size, inverse, out)


def record_kernel_name(nbytes, block_size, record_size, inverse=False, d_src=None, d_dst=None):
    """The kernels record_planes runs for nbytes bytes (redux_record_kernel_name; with d_src and d_dst, device tensors,
    redux_record_kernel_name_at: their alignment counts), joined by " + "; "" for arguments the call refuses."""
    L = _lib.lib()
    if d_src is None and d_dst is None:
        return L.redux_record_kernel_name(nbytes, block_size, record_size, 1 if inverse else 0).decode()
    return L.redux_record_kernel_name_at(d_src.data_ptr(), d_dst.data_ptr(), nbytes, block_size, record_size,
                                         1 if inverse else 0).decode()


RecordPlan = namedtuple("RecordPlan", "lgT PC grid_fast grid_bytes")


def record_plan(nbytes, block_size, record_size, delta=False, inverse=False, cus=0):
    """The shape record_planes launches with for nbytes bytes on 16-byte aligned buffers (redux_record_plan; nothing is
    launched) -> RecordPlan(lgT, PC, grid_fast, grid_bytes): the fast kernel's tile is 1 << lgT records, PC the inverse's byte
    columns per workgroup, a grid of 0 a kernel that does not run.  cus: the CU count to plan for, 0: the current device's."""
    plan = (C.c_uint32 * 4)()
    _raise(_lib.lib().redux_record_plan(nbytes, block_size, record_size, 1 if delta else 0, 1 if inverse else 0, cus, plan))
    return RecordPlan(*plan)


def _device_unit_table(torch, table, nunits, device):
    """a unit table for a device call: a uint8 device tensor is taken as it is, host values (np.uint8, a list) are uploaded;
    InvalidInput unless it has nunits entries.  Entries are taken & 7 on the device."""
    if isinstance(table, torch.Tensor):
        if not table.is_cuda or table.dtype != torch.uint8 or not table.is_contiguous() or table.device != device:
            raise InvalidInput()
        t = table
    else:
        t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.uint8).copy()).to(device)
    if t.dim() != 1 or t.numel() != nunits:
        raise InvalidInput()
    return t


def mixed_layout(d_src, table, block_size, inverse=False, out=None):
    """The mixed transform (include/redux_hip.h, "mixed layouts") of a uint8 device tensor, or its inverse: unit u of 8 blocks
    under layout table[u] & 7, redux_mixed_layout_dev on torch's current stream.  table: nunits entries, a uint8 device tensor
    or host values.  out: as for planes()."""
    torch = _torch()
    assert d_src.dtype == torch.uint8 and d_src.is_contiguous()
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30:
        raise InvalidInput()
    n = d_src.numel()
    L = _lib.lib()
    d_table = _device_unit_table(torch, table, L.redux_mixed_unit_count(n, int(block_size)), d_src.device)
    t = out if out is not None else torch.empty(n, dtype=torch.uint8, device=d_src.device)
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n and t.device == d_src.device
    with torch.cuda.device(t.device):
        _raise(L.redux_mixed_layout_dev(_dptr(d_src), _dptr(t), n, int(block_size), d_table.data_ptr(), 1 if inverse else 0,
                                        _stream_ptr(torch)))
    return t


def mixed_kernel_name(d_src, d_dst, block_size, inverse=False):
    """what mixed_layout runs between these two tensors: "k_mixed_planes<I>", "k_mixed_bytes<I>" or both joined by " + " """
    return _lib.lib().redux_mixed_kernel_name_at(_dptr(d_src), _dptr(d_dst), d_src.numel(), int(block_size),
                                                 1 if inverse else 0).decode()


def base_planes(d_src, d_base, element_size, block_size, inverse=False, out=None):
    """The XOR against d_base followed by the byte-plane layout (include/redux_hip.h, "XOR-against-base filter") of a uint8
    device tensor, or their inverse: redux_base_planes_dev on torch's current stream.  d_base: a uint8 tensor of any length
    on the same device.  out: as for planes()."""
    return _transform(_resolve_front(None, base=d_base).front, d_src, element_size, block_size, inverse, out, d_base)


def base_sub_planes(d_src, d_base, element_size, block_size, inverse=False, out=None):
    """The folded difference against d_base followed by the byte-plane layout (include/redux_hip.h, "folded difference
    against a base") of a uint8 device tensor, or their inverse: redux_base_sub_planes_dev on torch's current stream.
    d_base and out: as for base_planes()."""
    return _transform(_resolve_front(None, base=d_base, base_op="sub").front, d_src, element_size, block_size, inverse, out, d_base)


def constant_blocks(data, block_size):
    """The constant-block flags (include/redux_hip.h, "constant blocks") of every block of block_size bytes of `data`:
    1 where the block has at least one byte and all its bytes are equal, else 0.  A uint8 device tensor: redux_const_blocks_dev
    on torch's current stream, -> a uint8 device tensor of nblocks flags.  Anything bytes-like: copied to cuda:0 first,
    -> np.uint8[nblocks]."""
    torch = _torch()
    if block_size <= 0:
        raise InvalidInput()
    host = not isinstance(data, torch.Tensor)
    d = torch.from_numpy(_u8(data).copy()).to("cuda:0") if host else data
    assert d.dtype == torch.uint8 and d.is_contiguous() and d.is_cuda
    nb = _lib.lib().redux_block_count(d.numel(), block_size)
    flags = torch.empty(nb, dtype=torch.uint8, device=d.device)
    with torch.cuda.device(d.device):
        _raise(_lib.lib().redux_const_blocks_dev(_dptr(d), d.numel(), block_size, flags.data_ptr(), _stream_ptr(torch)))
    return flags.cpu().numpy() if host else flags


# ---- per-block CRC-32 checksums -----------------------------------------------------------------
def crc32_blocks(data, block_size, sizes=None):
    """CRC-32 (zlib.crc32) of every block of block_size bytes of `data` (the last may be shorter; empty data: one block,
    CRC 0) -> np.uint32[nblocks].  Host data (bytes-like, numpy) goes through redux_crc32_blocks; a uint8 device tensor is
    checksummed where it lies (redux_crc32_blocks_dev, one read-back).  sizes (device tensors only: an int32 / uint32
    device tensor of nblocks entries, as DeviceDecoder.decode returns): block b is then data[b*B : b*B + min(sizes[b], B)),
    the layout of a decoder's output (redux_crc32_sizes_dev)."""
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    L = _lib.lib()
    if not _is_device_tensor(data):
        if sizes is not None:
            raise InvalidInput()
        a = _u8(data)
        crc = np.zeros(L.redux_block_count(len(a), block_size), dtype=np.uint32)
        _raise(L.redux_crc32_blocks(_ptr(a), len(a), block_size, crc.ctypes.data))
        return crc
    torch = _torch()
    assert data.dtype == torch.uint8 and data.is_contiguous()
    with torch.cuda.device(data.device):
        s = _stream_ptr(torch)
        if sizes is None:
            n = data.numel()
            d_crc = torch.empty(L.redux_block_count(n, block_size), dtype=torch.int32, device=data.device)
            _raise(L.redux_crc32_blocks_dev(_dptr(data), n, block_size, d_crc.data_ptr(), s))
        else:
            assert sizes.is_cuda and sizes.device == data.device and sizes.element_size() == 4 and sizes.is_contiguous()
            nb = sizes.numel()
            if nb * block_size > data.numel():  # (the kernel may read any byte of every block's room)
                raise InvalidInput()
            d_crc = torch.empty(max(nb, 1), dtype=torch.int32, device=data.device)
            _raise(L.redux_crc32_sizes_dev(data.data_ptr(), nb, block_size, sizes.data_ptr(), d_crc.data_ptr(), s))
            d_crc = d_crc[:nb]
        return d_crc.cpu().numpy().view(np.uint32).copy()


def crc32_combine(crc1, crc2, len2):
    """zlib's crc32_combine (redux_crc32_combine, on the host): the CRC of A || B from crc32(A), crc32(B) and len(B)."""
    return int(_lib.lib().redux_crc32_combine(int(crc1) & 0xFFFFFFFF, int(crc2) & 0xFFFFFFFF, int(len2)))


# ---- size estimates (include/redux_hip.h, "size estimates") ---------------------------------------
MODELS = ("adaptive", "static", "plane-static", "segment-static", "context-static")  # (ties in an estimate go to the earlier)
TERMINATION_BYTES = 2.5  # a stream's bytes beyond its ideal length: the midpoint of what DESIGN.md 6j measured


def adaptive_cost_from_counts(counts, params=(8, 30, 32)):
    """redux_adaptive_cost_from_counts: the adaptive model's ideal code length in bits, EOF included, of blocks with the
    byte counts `counts` (u64[n, 256], or [256] for one block), on the host -> np.float64[n].  Unsupported where a block
    could freeze the model."""
    P = _params_of(params)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    c = c.reshape(1, 256) if c.shape == (256,) else c
    if c.ndim != 2 or c.shape[1] != 256:
        raise InvalidInput()
    bits = np.zeros(len(c), dtype=np.float64)
    cp = P._c()
    _raise(_lib.lib().redux_adaptive_cost_from_counts(C.byref(cp), _ptr(c), len(c), bits.ctypes.data_as(C.POINTER(C.c_double))))
    return bits


def _cost_rows(counts, cums):
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    t = np.ascontiguousarray(cums, dtype=np.uint32)
    c = c.reshape(1, 256) if c.shape == (256,) else c
    t = t.reshape(1, 258) if t.shape == (258,) else t
    if c.ndim != 2 or c.shape[1] != 256 or t.shape != (len(c), 258):
        raise InvalidInput()
    return c, t


def table_cost_from_counts(counts, cums):
    """redux_table_cost_from_counts: sum_s c[s] (log2 T - log2 f[s]) in bits for n count rows (u64[n, 256]) under n
    static tables (u32[n, 258]), on the host -> np.float64[n].  EOF is not included (add log2 T per block); +inf for a
    table that cannot code its row."""
    c, t = _cost_rows(counts, cums)
    bits = np.zeros(len(c), dtype=np.float64)
    _raise(_lib.lib().redux_table_cost_from_counts(_ptr(c), _ptr(t), len(c), bits.ctypes.data_as(C.POINTER(C.c_double))))
    return bits


def _device_u8(torch, data):
    """a uint8 device tensor is taken in place; host data (bytes-like, numpy) is uploaded to the current device"""
    if _is_device_tensor(data):
        assert data.dtype == torch.uint8 and data.is_contiguous()
        return data
    return torch.from_numpy(_u8(data).copy()).cuda()


def block_cost(data, block_size, params=(8, 30, 32)):
    """The adaptive model's ideal code length in bits, EOF included, of every block of block_size bytes of `data`
    (redux_block_cost_dev: k_block_cost on torch's current stream, one read-back) -> np.float64[nblocks].  A uint8 device
    tensor is read where it lies; host data is uploaded first."""
    P = _params_of(params)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    torch = _torch()
    d = _device_u8(torch, data)
    L = _lib.lib()
    cp = P._c()
    with torch.cuda.device(d.device):
        return _device_block_cost(torch, L, cp, d, int(block_size)).cpu().numpy()


def _device_block_cost(torch, L, cp, d, block_size):
    n = d.numel()
    d_bits = torch.empty(L.redux_block_count(n, block_size), dtype=torch.float64, device=d.device)
    _raise(L.redux_block_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, block_size,
                                  C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits


def table_cost(counts, cums):
    """table_cost_from_counts on the device (redux_table_cost_dev: k_table_cost on torch's current stream, one read-back)
    -> np.float64[n].  counts: an int64 device tensor of n * 256 entries, as the `_dev` histogram calls leave it, with cums
    an int32 device tensor of n * 258; or host arrays of those shapes, which are uploaded first."""
    torch = _torch()
    if _is_device_tensor(counts) != _is_device_tensor(cums):
        raise InvalidInput()
    if _is_device_tensor(counts):
        assert counts.element_size() == 8 and cums.element_size() == 4 and counts.is_contiguous() and cums.is_contiguous()
        if counts.numel() % 256 or cums.numel() != counts.numel() // 256 * 258 or cums.device != counts.device:
            raise InvalidInput()
        d_c, d_t = counts, cums
    else:
        c, t = _cost_rows(counts, cums)
        d_c, d_t = torch.from_numpy(c.view(np.int64).copy()).cuda(), torch.from_numpy(t.view(np.int32).copy()).cuda()
    with torch.cuda.device(d_c.device):
        return _device_table_cost(torch, _lib.lib(), d_c, d_t).cpu().numpy()


def _device_table_cost(torch, L, d_counts, d_cum):
    n = d_counts.numel() // 256
    d_bits = torch.empty(n, dtype=torch.float64, device=d_counts.device)
    _raise(L.redux_table_cost_dev(C.c_void_p(d_counts.data_ptr()) if n else None, C.c_void_p(d_cum.data_ptr()) if n else None, n,
                                  C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits


def estimate_candidates(element_size=1):
    """The models an estimate covers for this element size, in MODELS order: adaptive and segment-static always, static and
    context-static for element size 1, plane-static above."""
    E = _check_element_size(element_size)
    return tuple(m for m in MODELS if m in ("adaptive", "segment-static") or (m == "plane-static") == (E > 1))


def estimate_payload(data, block_size, params=(8, 30, 32), element_size=1, segment_blocks=None, models=None):
    """-> {model: estimated payload bytes}: what the streams of compress_blocks would add up to under each model of
    `models` (None: estimate_candidates(element_size)), without coding anything.  One histogram pass per model on the device
    (k_block_cost; the `_dev` histogram and table calls with the default total, then k_table_cost), on the byte-plane layout
    for element_size > 1, as the coders run.  The estimate is ceil(sum bits / 8 + TERMINATION_BYTES * nblocks), every block's
    EOF symbol included.  A uint8 device tensor is read where it lies; host data is uploaded once."""
    return _estimate(data, block_size, params, element_size, segment_blocks, models)[0]


def _estimate(data, block_size, params, element_size, segment_blocks, models):
    """estimate_payload, and the context-static tables (np.uint32[256, 258]; None unless that model was estimated): the
    container's overhead for them depends on which contexts occur"""
    P = _params_of(params)
    E = _check_element_size(element_size)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    B = int(block_size)
    models = estimate_candidates(E) if models is None else tuple(models)
    if any(m not in estimate_candidates(E) for m in models):
        raise InvalidInput()
    G = default_segment_blocks(E) if segment_blocks is None else segment_blocks
    if "segment-static" in models:
        G = SegmentStaticModel(P, None, E, G).segment_blocks  # (checks G)
    T = _total_of(P, None)
    torch = _torch()
    L = _lib.lib()
    cp = P._c()
    d = _device_u8(torch, data)
    out, context_cums = {}, None
    with torch.cuda.device(d.device):
        d_x = planes(d, E, B) if E > 1 else d
        n = d_x.numel()
        nb = L.redux_block_count(n, B)
        x_ptr = C.c_void_p(d_x.data_ptr()) if n else None
        s = _stream_ptr(torch)

        def static_bits(nrows, table_of_block, histogram, tables):
            """counts -> tables -> the rows' cross-entropy, plus log2(total) of its table for every block's EOF"""
            counts = torch.zeros(nrows * 256, dtype=torch.int64, device=d_x.device)
            d_cum = torch.zeros(nrows * 258, dtype=torch.int32, device=d_x.device)
            _raise(histogram(C.c_void_p(counts.data_ptr())))
            _raise(tables(C.c_void_p(counts.data_ptr()), C.c_void_p(d_cum.data_ptr())))
            bits = _device_table_cost(torch, L, counts, d_cum).cpu().numpy()
            cums = d_cum.cpu().numpy().view(np.uint32).reshape(nrows, 258)
            if not cums.any(axis=1).all():  # the table kernel's mark for N * R >= 2^64
                raise Unsupported()
            eof = np.log2(cums[table_of_block(np.arange(nb, dtype=np.int64)), 257].astype(np.float64))
            return float(bits.sum()) + float(eof.sum()), cums

        for m in models:
            if m == "adaptive":
                total = float(_device_block_cost(torch, L, cp, d_x, B).sum().item())
            elif m == "static":
                total, _ = static_bits(1, lambda b: 0 * b,
                                       lambda c: L.redux_histogram_dev(x_ptr, n, c, None, 0, s),
                                       lambda c, t: L.redux_static_table_dev(C.byref(cp), c, T, t, s))
            elif m == "plane-static":
                total, _ = static_bits(E, lambda b: b % E,
                                       lambda c: L.redux_plane_histogram_dev(x_ptr, n, B, E, c, None, 0, s),
                                       lambda c, t: L.redux_plane_static_tables_dev(C.byref(cp), c, E, T, t, s))
            elif m == "segment-static":
                total, _ = static_bits(L.redux_segment_static_table_count(nb, E, G), lambda b: b // G * E + b % E,
                                       lambda c: L.redux_segment_histogram_dev(x_ptr, n, B, E, G, c, s),
                                       lambda c, t: L.redux_segment_static_tables_dev(C.byref(cp), c, nb, E, G, T, t, s))
            else:  # context-static: a block's EOF is coded under its last byte's table; all 256 have one total
                total, context_cums = static_bits(256, lambda b: 0 * b,
                                                  lambda c: L.redux_context_histogram_dev(x_ptr, n, B, c, s),
                                                  lambda c, t: L.redux_context_static_tables_dev(C.byref(cp), c, T, t, s))
            out[m] = int(np.ceil(total / 8 + TERMINATION_BYTES * nb))
    return out, context_cums


BASE_OPS = ("xor", "sub")  # what the base filter does with the base; ties go to the earlier


def estimate_base_ops(data, base, block_size, params=(8, 30, 32), element_size=1):
    """-> {"xor": bytes, "sub": bytes}: the estimated payload of the adaptive coder behind each operation of the base filter
    (include/redux_hip.h, "XOR-against-base filter" and "folded difference against a base").  Each transform runs into one
    scratch tensor (base_planes, base_sub_planes) and block_cost's kernel reads it; nothing is coded."""
    P = _params_of(params)
    E = _check_element_size(element_size)
    if base is None or not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    B = int(block_size)
    torch = _torch()
    L = _lib.lib()
    cp = P._c()
    d = _device_u8(torch, data)
    out = {}
    with torch.cuda.device(d.device):
        d_y = _device_u8(torch, base).to(d.device)
        t = torch.empty_like(d)
        nb = L.redux_block_count(d.numel(), B)
        for op, transform in zip(BASE_OPS, (base_planes, base_sub_planes)):
            if d.numel():
                transform(d, d_y, E, B, out=t)
            out[op] = int(np.ceil(float(_device_block_cost(torch, L, cp, t, B).sum().item()) / 8 + TERMINATION_BYTES * nb))
    return out


# ---- layout estimates (include/redux_hip.h, "layout estimates") -----------------------------------
LAYOUTS =tuple((E, f) for f in (None, "delta") for E in (1, 2, 4, 8))  # layout k = 4 F + log2 E; ties go to the earlier


def layout_index(element_size, filter=None):
    """k of (element_size, filter): 4 F + log2 E"""
    try:
        return LAYOUTS.index((element_size, filter))
    except ValueError:
        raise InvalidInput()


def _layout_mask(layouts):
    """None: all eight; an int: the bit mask itself; else an iterable of (element_size, filter) pairs or indices"""
    if layouts is None:
        return 0xFF
    if isinstance(layouts, (int, np.integer)):
        mask = int(layouts)
    else:
        mask = 0
        for k in layouts:
            k = layout_index(*k) if isinstance(k, tuple) else k
            if not isinstance(k, (int, np.integer)) or not 0 <= k < 8:
                raise InvalidInput()
            mask |= 1 << int(k)
    if not 0 < mask <= 0xFF:
        raise InvalidInput()
    return mask


def layout_cost(data, block_size, params=(8, 30, 32), layouts=None):
    """The adaptive model's ideal code length in bits, EOF included, of every block of each of the eight layouts of `data`
    -- LAYOUTS[k]: the byte-plane layout for element size 1 / 2 / 4 / 8, then the same behind the delta filter -- counted
    from the bytes as they are, with no transformed copy (redux_layout_cost_dev: k_layout_cost on torch's current stream, one
    read-back) -> np.float64[8, nblocks].  layouts: None for all eight, or a bit mask, or (element_size, filter) pairs / layout
    indices; rows that were not asked for are NaN.  A uint8 device tensor is read where it lies; host data is uploaded once."""
    P = _params_of(params)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    mask = _layout_mask(layouts)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _device_layout_cost(torch, _lib.lib(), P._c(), d, int(block_size), mask).cpu().numpy()


def _device_layout_cost(torch, L, cp, d, block_size, mask):
    n = d.numel()
    d_bits = torch.full((8, L.redux_block_count(n, block_size)), float("nan"), dtype=torch.float64, device=d.device)
    _raise(L.redux_layout_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, block_size, mask,
                                   C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits


MIXED_SUM_SCALE = 65536.0  # redux_mixed_choose_dev's sum counts 2^-16 bit (REDUX_MIXED_SUM_FRAC_BITS)


def _device_choose(torch, L, d_bits, mask):
    """d_bits f64[8][nblocks] on the device -> (device table uint8[nunits], device sum int64[1] in 2^-16 bit)"""
    nb = d_bits.shape[1]
    d_table = torch.zeros((nb + 7) // 8, dtype=torch.uint8, device=d_bits.device)
    d_sum = torch.zeros(1, dtype=torch.int64, device=d_bits.device)
    _raise(L.redux_mixed_choose_dev(d_bits.data_ptr(), nb, mask, d_table.data_ptr(), d_sum.data_ptr(), _stream_ptr(torch)))
    return d_table, d_sum


def choose_unit_layouts(bits, layouts=None):
    """The choice of the mixed layouts (include/redux_hip.h, "mixed layouts") on the device: bits, float64[8, nblocks] as
    layout_cost returns them (a numpy array is uploaded, a device tensor read where it lies) -> (np.uint8[nunits], the sum of
    the chosen units' bits as a float).  table[u] is the lowest layout of `layouts` (None: all eight; else as layout_cost's)
    with the smallest sum over the unit's blocks, added in ascending block order (redux_mixed_choose_dev: k_mixed_choose on
    torch's current stream, one read-back).  Only the rows of `layouts` are read."""
    mask = _layout_mask(layouts)
    torch = _torch()
    if isinstance(bits, torch.Tensor):
        d_bits = bits
        if not d_bits.is_cuda or d_bits.dtype != torch.float64 or not d_bits.is_contiguous():
            raise InvalidInput()
    else:
        d_bits = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.float64).copy()).cuda()
    if d_bits.dim() != 2 or d_bits.shape[0] != 8 or d_bits.shape[1] == 0:
        raise InvalidInput()
    with torch.cuda.device(d_bits.device):
        d_table, d_sum = _device_choose(torch, _lib.lib(), d_bits, mask)
        return d_table.cpu().numpy(), int(d_sum.cpu()[0]) / MIXED_SUM_SCALE


def estimate_layouts(data, block_size, params=(8, 30, 32), element_size=None, mixed=False):
    """-> {(element_size, filter): estimated payload bytes}: what the streams of compress_blocks(..., element_size=,
    filter=) would add up to under the adaptive model for each layout, without transforming or coding anything: one
    layout_cost call, then ceil(sum bits / 8 + TERMINATION_BYTES * nblocks) as estimate_payload.  element_size None: all
    eight layouts; 1 / 2 / 4 / 8: that element size's two, plain and delta.  mixed=True adds the key "mixed": the same for the
    streams of compress_blocks(..., unit_layouts=True, layouts=those layouts), from the bits of the layout chosen for each
    unit of 8 blocks (redux_mixed_choose_dev, on the cost rows where they lie)."""
    if element_size is not None:
        _check_element_size(element_size)
    want = [k for k in LAYOUTS if element_size is None or k[0] == element_size]
    if not mixed:
        bits = layout_cost(data, block_size, params, want)
        nb = bits.shape[1]
        return {k: int(np.ceil(float(bits[LAYOUTS.index(k)].sum()) / 8 + TERMINATION_BYTES * nb)) for k in want}
    P = _params_of(params)
    if not isinstance(block_size, (int, np.integer)) or not 0 < block_size < 1 << 32:
        raise InvalidInput()
    mask = _layout_mask(want)
    torch = _torch()
    d = _device_u8(torch, data)
    L = _lib.lib()
    with torch.cuda.device(d.device):
        d_bits = _device_layout_cost(torch, L, P._c(), d, int(block_size), mask)
        _, d_sum = _device_choose(torch, L, d_bits, mask)
        bits, chosen = d_bits.cpu().numpy(), int(d_sum.cpu()[0]) / MIXED_SUM_SCALE
    nb = bits.shape[1]
    est = {k: int(np.ceil(float(bits[LAYOUTS.index(k)].sum()) / 8 + TERMINATION_BYTES * nb)) for k in want}
    est["mixed"] = int(np.ceil(chosen / 8 + TERMINATION_BYTES * nb))
    return est


# ---- lag estimates (include/redux_hip.h, "lag estimates") ------------------------------------------
LAG_SAMPLE_FRAMES = 64  # choose_lag's first pass counts about this many frames of a longer input
LAG_FINALISTS = 3       # and its second pass the lags with the smallest sampled estimates, this many, plus lag 1


def _lag_list(lags):
    """None: 1 .. LAG_MAX; else 1 to LAG_MAX ints in 1 .. LAG_MAX, repeats allowed -> list of int"""
    if lags is None:
        return list(range(1, LAG_MAX + 1))
    try:
        lags = list(lags)
    except TypeError:
        raise InvalidInput()
    if not 1 <= len(lags) <= LAG_MAX or any(isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= LAG_MAX
                                            for S in lags):
        raise InvalidInput()
    return [int(S) for S in lags]


def _lag_cost_args(element_size, block_size, lags, frame_step):
    """the argument checks of the lag estimates, on the arguments alone -> (E, B, lag list, T)"""
    if not isinstance(element_size, (int, np.integer)) or isinstance(element_size, bool) or element_size not in (1, 2, 4, 8) \
            or not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30 \
            or isinstance(frame_step, bool) or not isinstance(frame_step, (int, np.integer)) or not 0 < frame_step < 1 << 32:
        raise InvalidInput()
    return int(element_size), int(block_size), _lag_list(lags), int(frame_step)


def _device_lag_cost(torch, L, cp, d, E, B, lags, T):
    """-> float64 device tensor [len(lags), redux_lag_cost_block_count]; the lag list is consumed by the call"""
    n = d.numel()
    d_bits = torch.empty((len(lags), L.redux_lag_cost_block_count(n, B, E, T)), dtype=torch.float64, device=d.device)
    h_lags = np.asarray(lags, dtype=np.uint32)
    _raise(L.redux_lag_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, E, h_lags.ctypes.data, len(lags), T,
                                C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits


def lag_cost(data, element_size, lags, block_size=65536, params=(8, 30, 32), frame_step=1):
    """The adaptive model's ideal code length in bits, EOF included, of every block of `data` behind the lagged delta filter
    (filter="lag") for each lag of `lags` (1 to 256 of them, each 1 .. LAG_MAX, repeats allowed), counted from the bytes as they
    are, with no transformed copy (redux_lag_cost_dev: k_lag_cost on torch's current stream, one read-back)
    -> np.float64[len(lags), block_count]: row j is block_cost(lag_planes(data, element_size, block_size, lags[j])).
    frame_step T > 1 costs only the frames 0, T, 2T, ... (of element_size * block_size bytes) and returns their blocks in
    order.  A uint8 device tensor is read where it lies; host data is uploaded once."""
    E, B, lags, T = _lag_cost_args(element_size, block_size, lags, frame_step)  # (before the library is touched)
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _device_lag_cost(torch, _lib.lib(), P._c(), d, E, B, lags, T).cpu().numpy()


def _lag_estimates(torch, L, cp, d, E, B, lags, T):
    bits = _device_lag_cost(torch, L, cp, d, E, B, lags, T)
    sums, nb = bits.sum(dim=1).cpu().numpy(), bits.shape[1]
    out = {}
    for j, S in enumerate(lags):
        out.setdefault(S, int(np.ceil(float(sums[j]) / 8 + TERMINATION_BYTES * nb)))
    return out


def estimate_lags(data, element_size, block_size, lags=None, params=(8, 30, 32), frame_step=1):
    """-> {S: estimated payload bytes}: what the streams of compress_blocks(..., element_size=, filter="lag", lag=S) would
    add up to for each lag of `lags` (None: 1 .. LAG_MAX), without transforming or coding anything: one lag_cost call, then
    ceil(sum bits / 8 + TERMINATION_BYTES * blocks) as estimate_payload, over the blocks of the selected frames (frame_step
    1: all of them; a repeated lag keeps its first row)."""
    E, B, lags, T = _lag_cost_args(element_size, block_size, lags, frame_step)  # (before the library is touched)
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _lag_estimates(torch, _lib.lib(), P._c(), d, E, B, lags, T)


def lag_frame_step(nframes):
    """the frame step of choose_lag's first pass: 1 up to LAG_SAMPLE_FRAMES frames (one exact pass), ceil(F / 64) above"""
    return 1 if nframes <= LAG_SAMPLE_FRAMES else -(-nframes // LAG_SAMPLE_FRAMES)


def lag_finalists(estimates):
    """the lags of choose_lag's second pass, ascending: the LAG_FINALISTS smallest estimates (ties go to the smaller S), and
    lag 1 always"""
    return sorted(set(sorted(estimates, key=lambda S: (estimates[S], S))[:LAG_FINALISTS]) | {1})


def best_lag(estimates):
    """The lag with the smallest estimate; ties go to the smaller S."""
    return min(estimates, key=lambda S: (estimates[S], S))


def choose_lag(data, element_size, block_size, params=(8, 30, 32), estimate=None):
    """-> (S, {S: estimated payload bytes}): the lag of the lagged delta filter with the smallest estimate_lags, counted on
    the GPU and never guessed.  Up to LAG_SAMPLE_FRAMES (64) frames: one exact pass over all 256 lags.  Above: a first pass
    over all 256 lags on every ceil(F / 64)-th frame, then an exact pass over every frame for the finalists alone -- the
    LAG_FINALISTS (3) smallest sampled estimates and S = 1, which is always among them, so the chosen lag's estimate is never
    above the zigzag filter's.  Ties go to the smaller S; there is no hysteresis.  The dict holds the estimates of the last
    pass.  estimate: the rule alone, for a caller with costs of its own: a function (lags or None, frame_step) -> {S: bytes}
    in place of the device."""
    E, B, _, _ = _lag_cost_args(element_size, block_size, None, 1)  # (before the library is touched)
    if estimate is None:
        P = _params_of(params)
        torch = _torch()
        d = _device_u8(torch, data)
        L, cp = _lib.lib(), P._c()
        nbytes = d.numel()

        def estimate(lags, T):
            with torch.cuda.device(d.device):
                return _lag_estimates(torch, L, cp, d, E, B, _lag_list(lags), T)
    else:
        nbytes = len(data)
    T = lag_frame_step(max(1, -(-nbytes // (E * B))))
    est = estimate(None, T)
    if T > 1:
        est = estimate(lag_finalists(est), 1)
    return best_lag(est), est


# ---- order estimates (include/redux_hip.h, "order estimates") --------------------------------------
LAG_ORDER_COST_MAX = 256  # REDUX_LAG_ORDER_COST_MAX: the candidates of one call


def _candidate_list(candidates):
    """1 to LAG_ORDER_COST_MAX (S, K) pairs of ints, S in 1 .. LAG_MAX, K in 1 .. LAG_ORDER_MAX, repeats allowed
    -> list of (int, int)"""
    try:
        cands = [tuple(c) for c in candidates]
    except TypeError:
        raise InvalidInput()
    if not 1 <= len(cands) <= LAG_ORDER_COST_MAX:
        raise InvalidInput()
    for c in cands:
        if len(c) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in c) \
                or not 1 <= c[0] <= LAG_MAX or not 1 <= c[1] <= LAG_ORDER_MAX:
            raise InvalidInput()
    return [(int(S), int(K)) for S, K in cands]


def _lag_order_cost_args(element_size, block_size, candidates, frame_step):
    """the argument checks of the order estimates, on the arguments alone -> (E, B, candidate list, T)"""
    E, B, _, T = _lag_cost_args(element_size, block_size, None, frame_step)
    return E, B, _candidate_list(candidates), T


def _device_lag_order_cost(torch, L, cp, d, E, B, cands, T):
    """-> float64 device tensor [len(cands), redux_lag_cost_block_count]; both lists are consumed by the call"""
    n = d.numel()
    d_bits = torch.empty((len(cands), L.redux_lag_cost_block_count(n, B, E, T)), dtype=torch.float64, device=d.device)
    h_lags = np.asarray([S for S, _ in cands], dtype=np.uint32)
    h_orders = np.asarray([K for _, K in cands], dtype=np.uint32)
    _raise(L.redux_lag_order_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, E, h_lags.ctypes.data,
                                      h_orders.ctypes.data, len(cands), T, C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits


def lag_order_cost(data, element_size, candidates, block_size=65536, params=(8, 30, 32), frame_step=1):
    """The adaptive model's ideal code length in bits, EOF included, of every block of `data` behind the lag filter at a
    higher order (filter="lag", lag=S, order=K) for each (S, K) of `candidates` (1 to 256 pairs, S in 1 .. LAG_MAX, K in 1 ..
    LAG_ORDER_MAX, repeats allowed), counted from the bytes as they are, with no transformed copy (redux_lag_order_cost_dev:
    k_lag_order_cost on torch's current stream, one read-back) -> np.float64[len(candidates), block_count]: row c is
    block_cost(lag_order_planes(data, element_size, block_size, S, K)), and lag_cost's row of S for K = 1.  Four consecutive
    candidates are counted side by side at the pace of the highest order among them: a list ordered by order first is the
    fastest.  frame_step as for lag_cost.
    A uint8 device tensor is read where it lies; host data is uploaded once."""
    E, B, cands, T = _lag_order_cost_args(element_size, block_size, candidates, frame_step)  # (before the library is touched)
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _device_lag_order_cost(torch, _lib.lib(), P._c(), d, E, B, cands, T).cpu().numpy()


def _lag_order_estimates(torch, L, cp, d, E, B, cands, T):
    bits = _device_lag_order_cost(torch, L, cp, d, E, B, cands, T)
    sums, nb = bits.sum(dim=1).cpu().numpy(), bits.shape[1]
    out = {}
    for j, c in enumerate(cands):
        out.setdefault(c, int(np.ceil(float(sums[j]) / 8 + TERMINATION_BYTES * nb)))
    return out


def estimate_lag_orders(data, element_size, block_size, candidates, params=(8, 30, 32), frame_step=1):
    """-> {(S, K): estimated payload bytes}: what the streams of compress_blocks(..., element_size=, filter="lag", lag=S,
    order=K) would add up to for each pair of `candidates`, without transforming or coding anything: one lag_order_cost call,
    then ceil(sum bits / 8 + TERMINATION_BYTES * blocks) as estimate_lags, over the blocks of the selected frames (frame_step
    1: all of them; a repeated candidate keeps its first row)."""
    E, B, cands, T = _lag_order_cost_args(element_size, block_size, candidates, frame_step)  # (before the library is touched)
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _lag_order_estimates(torch, _lib.lib(), P._c(), d, E, B, cands, T)


def lag_order_candidates(lags):
    """the candidates of choose_lag_order's exact pass: every order of every lag, by order first (the four waves of a
    workgroup take consecutive candidates and move at the pace of the highest order among them)"""
    return [(S, K) for K in range(1, LAG_ORDER_MAX + 1) for S in lags]


def best_lag_order(estimates):
    """The (S, K) with the smallest estimate; ties go to the smaller K, then to the smaller S."""
    return min(estimates, key=lambda c: (estimates[c], c[1], c[0]))


def choose_lag_order(data, element_size, block_size, lag=None, params=(8, 30, 32), estimate=None):
    """-> ((S, K), {(S, K): estimated payload bytes}): the lag and the order of the lag filter with the smallest
    estimate_lag_orders, counted on the GPU and never guessed.  With a lag S: one exact pass over (S, 1), (S, 2), (S, 3).
    With lag None: choose_lag's first stage as it stands -- the order-1 estimates of all 256 lags, on about LAG_SAMPLE_FRAMES
    frames of a longer input -- then lag_finalists (the LAG_FINALISTS smallest and S = 1), then one exact pass over every
    order of every finalist, at most 12 candidates, by order first.  Ties go to the smaller K, then to the smaller S; there is no hysteresis.
    (S, 1) of every finalist is among the candidates, so the chosen estimate is never above what choose_lag estimates for
    its choice, nor above the zigzag filter's.  The dict holds the estimates of the exact pass.  estimate: the rule alone,
    for a caller with costs of its own: a function (candidates or None, frame_step) in place of the device, which returns
    {S: bytes} at order 1 for None (all 256 lags) and {(S, K): bytes} for a list of pairs."""
    E, B, _, _ = _lag_cost_args(element_size, block_size, None, 1)  # (before the library is touched)
    if lag is not None and (isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag <= LAG_MAX):
        raise InvalidInput()
    if estimate is None:
        P = _params_of(params)
        torch = _torch()
        d = _device_u8(torch, data)
        L, cp = _lib.lib(), P._c()
        nbytes = d.numel()

        def estimate(cands, T):
            with torch.cuda.device(d.device):
                if cands is None:
                    return _lag_estimates(torch, L, cp, d, E, B, _lag_list(None), T)
                return _lag_order_estimates(torch, L, cp, d, E, B, _candidate_list(cands), T)
    else:
        nbytes = len(data)
    if lag is None:
        lags = lag_finalists(estimate(None, lag_frame_step(max(1, -(-nbytes // (E * B))))))
    else:
        lags = [int(lag)]
    est = estimate(lag_order_candidates(lags), 1)
    return best_lag_order(est), est


# ---- record estimates (include/redux_hip.h, "record estimates") ------------------------------------
RECORD_COST_MAX = 256      # REDUX_RECORD_COST_MAX: the candidates of one call
RECORD_SAMPLE_BLOCKS = 64  # choose_record's first stage costs about this many blocks of every candidate
RECORD_FINALISTS = 4       # and its second stage the candidates with the smallest sampled rates, this many


def record_candidates():
    """all 510 candidates (R, filter): R in 2 .. RECORD_MAX, filter None then "delta" """
    return [(R, f) for R in range(2, RECORD_MAX + 1) for f in (None, "delta")]


def _record_candidate_list(candidates, cap=RECORD_COST_MAX):
    """1 to cap (R, filter) pairs, R an int in 2 .. RECORD_MAX, filter None or "delta" (False / True and 0 / 1 are taken for
    them), repeats allowed -> list of (int, None or "delta")"""
    try:
        cands = [tuple(c) for c in candidates]
    except TypeError:
        raise InvalidInput()
    if not 1 <= len(cands) <= cap:
        raise InvalidInput()
    out = []
    for c in cands:
        if len(c) != 2 or isinstance(c[0], bool) or not isinstance(c[0], (int, np.integer)) or not 2 <= c[0] <= RECORD_MAX:
            raise InvalidInput()
        f = c[1]
        if f is None or (isinstance(f, (bool, int, np.integer)) and int(f) == 0):
            f = None
        elif (isinstance(f, str) and f == "delta") or (isinstance(f, (bool, int, np.integer)) and int(f) == 1):
            f = "delta"
        else:
            raise InvalidInput()
        out.append((int(c[0]), f))
    return out


def _record_cost_args(block_size, sample_blocks):
    """the argument checks of the record estimates, on the arguments alone -> (B, Q)"""
    if isinstance(block_size, bool) or not isinstance(block_size, (int, np.integer)) or not 0 < block_size <= 1 << 30 \
            or isinstance(sample_blocks, bool) or not isinstance(sample_blocks, (int, np.integer)) or not 0 <= sample_blocks < 1 << 32:
        raise InvalidInput()
    return int(block_size), int(sample_blocks)


def record_cost_sample(nbytes, block_size, record_size, sample_blocks=0):
    """The frame sampling of the record estimates (include/redux_hip.h, "record estimates"), in Python and on the arguments
    alone -> (T, blocks of the row, input bytes costed): frames 0, T, 2T, ... of record_size * block_size bytes."""
    frame = record_size * block_size
    nframes = max(1, -(-nbytes // frame))
    T = 1
    if sample_blocks:
        want = -(-sample_blocks // record_size)
        if nframes > want:
            T = -(-nframes // want)
    nsel = (nframes - 1) // T + 1
    last = (nsel - 1) * T  # the last selected frame
    nblocks = max(1, -(-nbytes // block_size))
    row = (nsel - 1) * record_size + min(record_size, nblocks - last * record_size)
    return T, row, (nsel - 1) * frame + min(frame, nbytes - last * frame)


def _device_record_cost(torch, L, cp, d, B, cands, Q, fill=None):
    """-> (float64 device tensor [len(cands), redux_block_count], the rows' own block counts); both lists are consumed by
    the call.  fill: what the entries past a row's count hold (None: nothing is written there)"""
    n = d.numel()
    shape = (len(cands), L.redux_block_count(n, B))
    d_bits = torch.empty(shape, dtype=torch.float64, device=d.device) if fill is None \
        else torch.full(shape, fill, dtype=torch.float64, device=d.device)
    h_records = np.asarray([R for R, _ in cands], dtype=np.uint32)
    h_deltas = np.asarray([f is not None for _, f in cands], dtype=np.uint8)
    _raise(L.redux_record_cost_dev(C.byref(cp), C.c_void_p(d.data_ptr()) if n else None, n, B, h_records.ctypes.data,
                                   h_deltas.ctypes.data, len(cands), Q, C.c_void_p(d_bits.data_ptr()), _stream_ptr(torch)))
    return d_bits, [int(L.redux_record_cost_block_count(n, B, R, Q)) for R, _ in cands]


def record_cost(data, candidates, block_size=65536, params=(8, 30, 32), sample_blocks=0):
    """The adaptive model's ideal code length in bits, EOF included, of every block of `data` behind the record layout
    (record_size=R, filter=) for each (R, filter) of `candidates` (1 to RECORD_COST_MAX pairs, R in 2 .. RECORD_MAX, filter
    None or "delta", repeats allowed), counted from the bytes as they are, with no transformed copy (redux_record_cost_dev:
    k_record_cost on torch's current stream, one read-back) -> np.float64[len(candidates), block_count]: row c is
    block_cost(record_planes(data, R, block_size, delta)).  sample_blocks Q > 0 costs about Q blocks of every candidate --
    every T-th frame of R * block_size bytes, T the candidate's own (record_cost_sample) -- and returns a list of rows, each
    the blocks of its candidate's selected frames in order.  A uint8 device tensor is read where it lies; host data is
    uploaded once."""
    B, Q = _record_cost_args(block_size, sample_blocks)  # (before the library is touched)
    cands = _record_candidate_list(candidates)
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        bits, counts = _device_record_cost(torch, _lib.lib(), P._c(), d, B, cands, Q)
        bits = bits.cpu().numpy()
    return bits if Q == 0 else [bits[c, :n].copy() for c, n in enumerate(counts)]


def _record_estimates(torch, L, cp, d, B, cands, Q):
    out = {}
    for at in range(0, len(cands), RECORD_COST_MAX):
        part = cands[at:at + RECORD_COST_MAX]
        bits, counts = _device_record_cost(torch, L, cp, d, B, part, Q, fill=0.0)
        sums = bits.sum(dim=1).cpu().numpy()
        for j, c in enumerate(part):
            out.setdefault(c, int(np.ceil(float(sums[j]) / 8 + TERMINATION_BYTES * counts[j])))
    return out


def estimate_records(data, block_size, candidates=None, params=(8, 30, 32), sample_blocks=0):
    """-> {(R, filter): estimated payload bytes}: what the streams of compress_blocks(..., record_size=R, filter=) would add
    up to for each pair of `candidates` (up to 510; None: all 510 of record_candidates(); in calls of at most RECORD_COST_MAX), without
    transforming or coding anything: record_cost, then ceil(sum bits / 8 + TERMINATION_BYTES * blocks) as estimate_payload,
    over the blocks of the selected frames (sample_blocks 0: all of them; a repeated candidate keeps its first row)."""
    B, Q = _record_cost_args(block_size, sample_blocks)  # (before the library is touched)
    cands = record_candidates() if candidates is None else _record_candidate_list(candidates, 2 * (RECORD_MAX - 1))
    P = _params_of(params)
    torch = _torch()
    d = _device_u8(torch, data)
    with torch.cuda.device(d.device):
        return _record_estimates(torch, _lib.lib(), P._c(), d, B, cands, Q)


def _record_rank(c):
    """ties among candidates: the smaller R, then no filter"""
    return (c[0], c[1] is not None)


def record_finalists(estimates, costed=None):
    """the candidates of choose_record's second stage: the RECORD_FINALISTS smallest of `estimates` {(R, filter): bytes}, by
    bytes per costed input byte where costed {(R, filter): bytes of the input} is given (candidates sample different
    amounts); ties go to the smaller R, then to no filter"""
    def rate(c):
        return estimates[c] / max(1, costed[c]) if costed is not None else estimates[c]
    return sorted((c for c in estimates if c is not None), key=lambda c: (rate(c), _record_rank(c)))[:RECORD_FINALISTS]


def best_record(estimates):
    """The key of {(R, filter) or None: bytes} with the smallest estimate.  None, the plain bytes, wins every tie; among
    candidates ties go to the smaller R, then to no filter."""
    return min(estimates, key=lambda c: (estimates[c], (0, 0, False) if c is None else (1,) + _record_rank(c)))


RECORD_NOISE_SIGMAS = 6.4  # choose_record: a layout must beat the plain bytes by this many standard deviations of the noise


def record_noise_bytes(bits, nfull=None):
    """The standard deviation, in bytes, that an estimate over these blocks shows on data WITHOUT record structure, from the
    plain bytes' own block costs `bits` (block_cost's).  On such data the blocks are draws of one source, the sample
    deviation s of their costs is the noise of one block, a sum of n independent blocks has s * sqrt(n), and a candidate of
    the record layout is the same bytes dealt into other blocks: another such sum.  Data that drifts from block to block
    makes it larger, which errs towards the plain bytes.  nfull: the leading blocks of full size (None: all); a short last
    block costs less for being short, which is no noise, so s is taken over the full ones.  0 for fewer than two of them."""
    bits = np.asarray(bits, dtype=np.float64).reshape(-1)
    full = bits if nfull is None else bits[:nfull]
    if len(full) < 2:
        return 0.0
    return float(np.std(full, ddof=1)) * float(np.sqrt(len(bits))) / 8


def choose_record(data, block_size, params=(8, 30, 32), estimate=None):
    """-> ((R, filter) or None, {key: estimated payload bytes}): the record size and the filter of the record layout with
    the smallest estimate, or None where the plain bytes are estimated no larger, counted on the GPU and never guessed.
    Stage 1: all 510 candidates on about RECORD_SAMPLE_BLOCKS (64) blocks each, ranked by sampled bytes per costed input
    byte.  Stage 2: one exact pass over the RECORD_FINALISTS (4) best, and block_cost of the plain bytes under the key None,
    which wins ties: the choice is never estimated above the plain container.  Where stage 1 was exact for every candidate
    (an input of few frames), its figures stand and only the plain cost is added.  The dict holds the exact estimates.
    The smallest of 510 estimates lies below the plain one on any data, by noise: on iid bytes every candidate is the same
    bytes in other blocks, the smallest of 510 such draws lies about 3.1 standard deviations below their mean with a spread
    of 0.4, and the plain estimate is one more draw, so a gain of 3.1 +- 1.1 deviations says nothing.  A candidate is chosen
    only where it beats the plain bytes by more than RECORD_NOISE_SIGMAS (6.4 = 3.1 + 3 * 1.1) times record_noise_bytes of
    the plain bytes' block costs; else None.
    estimate: the rule alone, for a caller with costs of its own: a function (candidates, sample_blocks) -> {key: bytes} in
    place of the device, where candidates is a list of (R, filter), or None for the plain bytes: {None: bytes}, and under
    the key "noise" the deviation in bytes (record_noise_bytes), without which it is 0 and only ties go to None."""
    B, _ = _record_cost_args(block_size, 0)  # (before the library is touched)
    if estimate is None:
        P = _params_of(params)
        torch = _torch()
        d = _device_u8(torch, data)
        L, cp = _lib.lib(), P._c()
        nbytes = d.numel()

        def estimate(cands, Q):
            with torch.cuda.device(d.device):
                if cands is None:
                    bits = _device_block_cost(torch, L, cp, d, B).cpu().numpy()
                    return {None: int(np.ceil(float(bits.sum()) / 8 + TERMINATION_BYTES * len(bits))), "noise": record_noise_bytes(bits, nbytes // B)}
                return _record_estimates(torch, L, cp, d, B, cands, Q)
    else:
        nbytes = len(data)
    cands = record_candidates()
    est = estimate(cands, RECORD_SAMPLE_BLOCKS)
    samples = {c: record_cost_sample(nbytes, B, c[0], RECORD_SAMPLE_BLOCKS) for c in cands}
    if any(samples[c][0] > 1 for c in cands):
        est = estimate(record_finalists(est, {c: samples[c][2] for c in cands}), 0)
    est = dict(est)
    plain = dict(estimate(None, 0))
    noise = plain.pop("noise", 0.0)
    est.update(plain)
    best = best_record(est)
    if best is not None and est[None] - est[best] <= RECORD_NOISE_SIGMAS * noise:
        best = None  # (a gain that the smallest of 510 draws of noise explains)
    return best, est


# ---- synthetic workloads (BASELINE.json configs 2 and 5) ------------------------------------
def gen_iid(nbytes, seed=0x5EED0001, first_byte=0, device="cuda:0", out=None):
    torch = _torch()
    t = out if out is not None else torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(t.device):
        _raise(_lib.lib().redux_gen_iid_dev(C.c_void_p(t.data_ptr()), nbytes, first_byte, seed, _stream_ptr(torch)))
    return t


def gen_zipf(nbytes, seed=0x5EED0005, first_byte=0, device="cuda:0", out=None):
    torch = _torch()
    t = out if out is not None else torch.empty(nbytes, dtype=torch.uint8, device=device)
    with torch.cuda.device(t.device):
        _raise(_lib.lib().redux_gen_zipf_dev(C.c_void_p(t.data_ptr()), nbytes, first_byte, seed, _stream_ptr(torch)))
    return t


def zipf_thresholds():
    p = _lib.lib().redux_zipf_thresholds()
    return np.ctypeslib.as_array(p, shape=(256,)).copy()
