"""Block container: makes the multi-block output of the GPU path a self-describing file.

The reference has no container (one stream per call, src/lib.rs:102); SURVEY.md 8(f).1 asks
for one so that blocked output can be decoded again.  Every payload stays byte-identical to
`redux::compress(block)`.

Layout (little-endian):
    0   4  magic  b"RDXB"
    4   1  version (1; 2 = byte-plane layout; 3 = static-table model; 4 = plane-static: a static table per byte plane;
           5 = segment-static: static tables per block range; 6 = delta filter in front of the byte-plane layout;
           7 = context-static: a static table per preceding byte; 8 = XOR-against-base filter in front of the byte-plane
           layout; 9 = constant blocks skipped, with or without the XOR-against-base filter; 10 = mixed layouts: a layout
           per unit of 8 blocks; 11 = zigzag-folded delta filter in front of the byte-plane layout; 12 = folded difference
           against a base in front of the byte-plane layout; 13 = lagged delta filter in front of the byte-plane layout;
           14 = higher-order lagged differences in front of the byte-plane layout; 15 = further layouts, told apart by a kind
           field in the word at offset 12: kind 1 = record layout for fixed-width structs; kind 2 = snapshot-stride filter
           in front of the byte-plane layout)
    5   3  symbol_bits, freq_bits, code_bits      (Parameters::new arguments, src/model/mod.rs:63)
    8   4  block_size
   12   4  versions 1 and 3: reserved (0); version 2: element size E, one of 2, 4, 8; version 4: E in the low 16 bits and
           the table count, which must equal E, in the high 16 bits (0x00020002, 0x00040004, 0x00080008); version 5:
           0x50000000 | k << 4 | E with E one of 1, 2, 4, 8 and 1 <= k < 2^24: segments of 64 E k blocks; version 6:
           0x60000000 | E with E one of 1, 2, 4, 8; version 7: 0x70000000; version 8: 0x80000000 | E with E one of 1, 2, 4, 8;
           version 9: 0x90000000 | F << 4 | E with E one of 1, 2, 4, 8 and F 1 if a base was used, else 0; version 10:
           0xA0000000; version 11: 0xB0000000 | E with E one of 1, 2, 4, 8; version 12: 0xC0000000 | E with E one of 1, 2, 4, 8;
           version 13: 0xD0000000 | S << 4 | E with E one of 1, 2, 4, 8 and the lag S, 1 <= S <= 256;
           version 14: 0xE0000000 | K << 16 | S << 4 | E with E and S as in version 13 and the order K, 2 <= K <= 3;
           version 15: 0xF0000000 | kind << 24 | F << 12 | R with kind 1, the record size R, 2 <= R <= 256, in bits 0 to 8 and
           F 1 for the byte delta, else 0; or 0xF0000000 | 2 << 24 | E with kind 2, E one of 1, 2, 4, 8 and every other bit 0
   16   8  nblocks
   24   8  total uncompressed length
   (versions 8 and 12, and version 9 with F = 1) 12  the base record: u64 base_used = min(len(base), total), u32 zlib.crc32(base[:base_used])
   (version 15 kind 2 only) 8  the stride record: u64 S, the stride in elements, at least 1
   (version 3 only) 4*258  the static table cum[0..=257], u32
   (version 4 only) E*4*258  the E static tables, table t (blocks b with b mod E == t) first to last
   (version 5 only) nseg*E*4*258  the static tables, u32[nseg][E][258], nseg = max(1, ceil(nblocks / (64 E k)))
   (version 7 only) 4  the tables' total; 32  presence mask, bit c % 8 of byte c // 8 (LSB first) = table c is recorded;
           then for each recorded table, in order of c, 256 u16 frequencies of the byte values (EOF = 1 is implied)
   ..  4*nblocks   compressed size of each block
   (flag 0x10 only) 4*nblocks  CRC-32 of each block's uncompressed bytes, u32
   (flag 0x40 only) ceil(nblocks/8)  stored-block bitmap: bit b % 8 of byte b // 8 (LSB first) = block b is stored
   (version 10 only) ceil(nblocks/8)  the unit table: the layout k = 4 F + log2 E, 0 .. 7, of each unit of 8 blocks, u8
   ..  payloads, concatenated in block order

Version 2 is the same layout for data coded with the byte-plane layout of typed data (include/redux_hip.h): the payloads
are the streams of the transformed bytes, and decoding undoes the layout.  Element size 1 (no layout) writes version 1,
byte for byte what this module wrote before version 2 existed.

Version 3 holds streams of the static-table model (include/redux_hip.h, "static-table model" and "semi-static coding"):
the header is followed by the table the blocks were coded under, and decoding uses it.  A table that
redux_static_table_check rejects is InvalidInput, a truncated one Eof.

Version 4 holds streams of plane-static coding (include/redux_hip.h, "plane-static coding"): the byte-plane layout of
version 2, block b coded by the static coder under table b mod E.  Tables that redux_plane_static_table_check rejects are
InvalidInput, truncated ones Eof.  It has no stored blocks (no 0x44).

Version 5 holds streams of segment-static coding (include/redux_hip.h, "segment-static coding"): the layout of version 2
(none for E = 1), block b coded by the static coder under table (b // G) E + b mod E, G = 64 E k.  The marker nibble 5 of
the word at offset 12 is required: no other version's word carries it.  Tables that redux_segment_static_table_check
rejects are InvalidInput, truncated ones Eof.  It has no stored blocks (no 0x45 / 0x55).

Version 6 holds streams of the adaptive coder behind the delta filter for integer series (include/redux_hip.h, "delta
filter"): the sections are version 2's, the payloads are the streams of the filtered bytes in the byte-plane layout (no
layout for E = 1), and decoding undoes both.  The marker nibble 6 of the word at offset 12 is required: no other version's
word carries it.  It has no stored blocks (no 0x46 / 0x56).  Without filter="delta" the writers emit exactly the bytes they
emitted before the version existed.

Version 7 holds streams of context-static coding (include/redux_hip.h, "context-static coding"): element size 1, a byte
coded under the table of the byte before it in its block.  The sections are version 3's with the table section in the
compact form above: a table equal to the one the rule gives a context without bytes (a count of one for every byte value)
is not recorded, and reading rebuilds it, so text pays for its 60 to 100 contexts and not for 256.  A total outside
257 .. min(2^16, freq_max), a frequency of 0, a row that does not sum to total - 1 and a section that ends early are
InvalidInput.  The marker nibble 7 of the word at offset 12 is required.  It has no stored blocks (no 0x47 / 0x57).

Version 8 holds streams of the adaptive coder behind the XOR-against-base filter for series of snapshots
(include/redux_hip.h, "XOR-against-base filter"): the header is followed by the base record, then come version 2's sections;
the payloads are the streams of input ^ base in the byte-plane layout (no layout for E = 1), and decoding needs the same
base: decompress_bytes(buf, base=...) refuses, before any GPU call, a missing base, one shorter than base_used and one whose
first base_used bytes have another CRC-32 (InvalidInput); a longer one is fine.  The record's base_used above the total is
InvalidInput, a truncated record Eof.  The marker nibble 8 of the word at offset 12 is required: no other version's word
carries it.  It has no stored blocks (no 0x48 / 0x58).  Without base= the writers emit exactly the bytes they emitted
before the version existed.

Version 9 holds streams of the adaptive coder with constant blocks skipped (include/redux_hip.h, "constant blocks"): a
block of the coder's input -- the bytes, their byte-plane layout, or the layout of input ^ base -- whose bytes are all equal
has that one byte as its payload.  The sections: header, version 8's base record if F is set, size table, CRC table (0x19),
the constant bitmap of ceil(nblocks / 8) bytes (LSB first, padding bits 0), payloads.  A constant block's size entry other
than 1 and set padding bits are InvalidInput, a truncated bitmap Eof; the base checks of version 8 apply when F = 1, and a
base given for F = 0 is InvalidInput.  The marker nibble 9 of the word at offset 12 is required: no other version's word
carries it.  It has no stored blocks (no 0x49 / 0x59), and 0x29 / 0x89 are InvalidInput as for every version.  Without
skip_constant=True the writers emit exactly the bytes they emitted before the version existed.

Version 10 holds streams of the adaptive coder behind the mixed layouts (include/redux_hip.h, "mixed layouts"): every unit
of 8 blocks has a layout of its own -- the byte-plane layout for elements of 1, 2, 4 or 8 bytes, with or without the delta
filter -- recorded in the unit table, one byte per unit, which follows the size table and the CRC table (0x1A).  A table
byte above 7 is InvalidInput, a truncated table Eof.  The marker nibble 0xA of the word at offset 12 is required: no other
version's word carries it.  It has no stored blocks (no 0x4A / 0x5A).  Without layout="mixed" the writers emit exactly the
bytes they emitted before the version existed.

Version 11 holds streams of the adaptive coder behind the zigzag-folded delta filter for signed series (include/redux_hip.h,
"zigzag-folded delta filter"): version 6 with every difference folded, the same sections, and decoding undoes layout, fold
and filter.  The word at offset 12 is 0xB0000000 | E: no other version takes that word, and version 11 takes no other.  It
has no stored blocks (no 0x4B / 0x5B).  Without filter="zigzag" the writers emit exactly the bytes they emitted before the
version existed.

Version 12 holds streams of the adaptive coder behind the folded difference against a base (include/redux_hip.h, "folded
difference against a base"): version 8 with the other operation of the base filter, the same sections, base record included,
and the same checks of the base before any GPU call.  The word at offset 12 is 0xC0000000 | E: no other version takes that
word, and version 12 takes no other.  It has no stored blocks (no 0x4C / 0x5C).  Without base_op="sub" (or "auto") the writers
emit exactly the bytes they emitted before the version existed.

Version 13 holds streams of the adaptive coder behind the lagged delta filter for interleaved channels and fixed-width
records (include/redux_hip.h, "lagged delta filter"): version 11 with the predecessor S elements back, the same sections, and
decoding undoes layout, fold and filter with the lag the word records.  The word at offset 12 is 0xD0000000 | S << 4 | E: no
other version takes that word, and version 13 takes no other; S = 0 and S > 256 are InvalidInput.  It has no stored blocks
(no 0x4D / 0x5D).  Without filter="lag" the writers emit exactly the bytes they emitted before the version existed.

Version 14 holds streams of the adaptive coder behind higher-order lagged differences (include/redux_hip.h, "higher-order
lagged differences"): version 13 with the lag-S difference applied K times, the same sections, and decoding undoes layout,
fold and filter with the lag and the order the word records.  The word at offset 12 is 0xE0000000 | K << 16 | S << 4 | E: no
other version takes that word, and version 14 takes no other; K outside 2 .. 3 and S outside 1 .. 256 are InvalidInput.  Order
1 is the lagged delta filter and is always written as version 13, so a version 14 word with K = 1 is malformed.  It has no
stored blocks (no 0x4E / 0x5E).  Without an order above 1 the writers emit exactly the bytes they emitted before the version
existed.

Version 15 is the last version number under the flag bits, so it is not spent on one layout: bits 24 .. 27 of its word at
offset 12 hold a KIND, and later layouts take kinds 2 .. 15 of version 15 rather than a version.  Kind 1 holds streams of
the adaptive coder behind the record layout for fixed-width structs (include/redux_hip.h, "record layout"): the sections are
version 2's, the payloads are the streams of the bytes in the layout of records of R bytes -- every block one byte column of
B records -- behind the byte delta against the record before when F is set, and decoding undoes both.  The word is
0xF0000000 | 1 << 24 | F << 12 | R: every other kind, any other set bit and R outside 2 .. 256 are InvalidInput; no other
version takes that word, and version 15 takes no other.  It has no stored blocks (no 0x4F / 0x5F).  Without a record size the
writers emit exactly the bytes they emitted before the version existed.

Kind 2 of version 15 holds streams of the adaptive coder behind the snapshot-stride filter for time series of fields
(include/redux_hip.h, "snapshot-stride filter"): every element against the element S back, counted over the whole buffer,
in front of the byte-plane layout of E.  The word is 0xF0000000 | 2 << 24 | E with E one of 1, 2, 4, 8 in bits 0 to 3 and
EVERY other bit zero; S does not fit a word and travels as a little-endian u64 record directly behind the header, where
version 8 keeps its base record; the remaining sections are version 2's.  Any other bit, E outside the set or S = 0 is
InvalidInput, a truncated record Eof; no other version takes the word.  It has no stored blocks, and no range reads: an
element needs every snapshot before it, and the container keeps no keyframes (Reader.read raises Unsupported).  Without
filter="stride" the writers emit exactly the bytes they emitted before the kind existed.

Bit 0x10 of the version byte (versions 0x11 to 0x1F: versions 1 to 15 with checksums) means a table of nblocks
CRC-32 values follows the size table: crc[b] = zlib.crc32 of block b's ORIGINAL bytes, x[b*B .. min((b+1)*B, total)), for
every layout (include/redux_hip.h, "per-block CRC-32 checksums").  decompress_bytes checks every block against it: a
block that is whole and correct but in the wrong place (swapped, duplicated, stitched in from another file) decodes to the
right length and is caught only here.  Any other high bit is InvalidInput, a truncated table Eof.  Without checksums the
writers emit exactly the bytes they emitted before the flag existed.

Bit 0x40 (versions 0x41 / 0x42, with checksums 0x51 / 0x52) means stored blocks (include/redux_hip.h, "stored blocks"): a
bitmap of the blocks whose payload is their raw coder input -- the bytes themselves, or for version 2 their plane -- follows
the size table and the CRC table.  A stored block's size entry must be its raw length min(B, total - b*B), and the bitmap's
padding bits must be 0 (else InvalidInput); a truncated bitmap is Eof.  The static-table model (version 3) has no stored
blocks.  Without stored=True the writers emit exactly the bytes they emitted before the flag existed.
"""
import struct
import zlib
from collections import namedtuple

import numpy as np

from . import api

MAGIC = b"RDXB"
VERSION = 1
VERSION_PLANES = 2
VERSION_STATIC = 3
VERSION_PLANE_STATIC = 4
VERSION_SEGMENT_STATIC = 5
VERSION_DELTA = 6
VERSION_CONTEXT_STATIC = 7
VERSION_BASE = 8
VERSION_CONST = 9
VERSION_MIXED = 10
VERSION_ZIGZAG = 11
VERSION_BASE_SUB = 12
VERSION_LAG = 13
VERSION_LAG_ORDER = 14
VERSION_KINDS = 15
KINDS_MARK = 0xF0000000  # version 15's word at offset 12: KINDS_MARK | kind << 24 | what the kind records
KIND_RECORD = 1  # the record layout: KINDS_MARK | KIND_RECORD << 24 | F << 12 | R
KIND_STRIDE = 2  # the snapshot-stride filter: KINDS_MARK | KIND_STRIDE << 24 | E, every other bit zero; S in STRIDE_RECORD
STRIDE_RECORD = struct.Struct("<Q")  # version 15 kind 2, after the header: the stride S in elements, at least 1
RECORD_MAX = api.RECORD_MAX  # the largest record size R (REDUX_RECORD_MAX)
LAG_ORDER_MARK = 0xE0000000  # version 14's word at offset 12: LAG_ORDER_MARK | K << 16 | S << 4 | E
LAG_ORDER_MAX = api.LAG_ORDER_MAX  # the largest order K (REDUX_LAG_ORDER_MAX); version 14 records 2 .. LAG_ORDER_MAX
LAG_MARK = 0xD0000000  # version 13's word at offset 12: LAG_MARK | S << 4 | E
LAG_MAX = api.LAG_MAX  # the largest lag S (REDUX_LAG_MAX)
BASE_SUB_MARK = 0xC0000000  # version 12's word at offset 12: BASE_SUB_MARK | E
ZIGZAG_MARK = 0xB0000000  # version 11's word at offset 12: ZIGZAG_MARK | E
MIXED_MARK = 0xA0000000  # version 10's word at offset 12
MIXED_UNIT_BLOCKS = 8  # blocks of a unit of the mixed layouts (REDUX_MIXED_UNIT_BLOCKS)
CONST_MARK = 0x90000000  # version 9's word at offset 12: CONST_MARK | F << 4 | E, F = 1 with a base record
BASE_MARK = 0x80000000  # version 8's word at offset 12: BASE_MARK | E
BASE_RECORD = struct.Struct("<QI")  # version 8, after the header: base_used, CRC-32 of base[:base_used]
CONTEXT_MARK = 0x70000000  # version 7's word at offset 12
DELTA_MARK = 0x60000000  # version 6's word at offset 12: DELTA_MARK | E
SEGMENT_MARK = 0x50000000  # version 5's word at offset 12: SEGMENT_MARK | k << 4 | E
TABLE = 258 * 4  # version 3: cum[0..=257] as u32 after the header
CRC_FLAG = 0x10  # version bit: a table of per-block CRC-32 values follows the size table
STORED_FLAG = 0x40  # version bit: a stored-block bitmap follows the size table (and the CRC table)
ELEMENT_SIZES = (2, 4, 8)  # what version 2 may record
HEADER = struct.Struct("<4sBBBBIIQQ")
# A header field, not a promise: a crafted 40-byte file must not make the decoder allocate
# gigabytes.  The container never holds blocks above 1 GiB (the CLI refuses larger ones), and
# the decode capacity is additionally capped by the total length the header declares.
MAX_BLOCK_SIZE = 1 << 30

# The versions that are version 2's sections behind a filter (version 2 itself: behind none): the marker nibble of the word
# at offset 12, which is mark << 28 | E; the filter and the operation of the base filter a reader reports; whether the base
# record follows the header; whether bits 4 .. 27 of the word hold the filter's lag (else they are 0); whether bits 16 .. 27
# hold the filter's order, which leaves the lag bits 4 .. 15.  pack, _version_ok, _header and _parse_index go by this table: a
# new filter is a new row.
_FilterVersion = namedtuple("_FilterVersion", "mark filter base_op has_base has_lag has_order", defaults=(False, False))
FILTER_VERSIONS = {VERSION_PLANES: _FilterVersion(0, None, None, False),
                   VERSION_DELTA: _FilterVersion(DELTA_MARK >> 28, "delta", None, False),
                   VERSION_BASE: _FilterVersion(BASE_MARK >> 28, None, "xor", True),
                   VERSION_ZIGZAG: _FilterVersion(ZIGZAG_MARK >> 28, "zigzag", None, False),
                   VERSION_BASE_SUB: _FilterVersion(BASE_SUB_MARK >> 28, None, "sub", True),
                   VERSION_LAG: _FilterVersion(LAG_MARK >> 28, "lag", None, False, True),
                   VERSION_LAG_ORDER: _FilterVersion(LAG_ORDER_MARK >> 28, "lag", None, False, True, True)}
# (the lag filter's version goes by its order: 13 for order 1, 14 above)
_VERSION_OF_FILTER = {(row.filter, row.base_op): ver for ver, row in FILTER_VERSIONS.items() if not row.has_order}


def _lag_word(row, res):
    """(S, K) of the word at offset 12 of a version whose row has a lag; K is None where the row has no order"""
    return (res >> 4 & 0xFFF, res >> 16 & 0xFFF) if row.has_order else (res >> 4 & 0xFFFFFF, None)


def _raw_lengths(nblocks, block_size, total):
    """L_b = min(B, total - b*B): the bytes of each block (0 for an empty input's one block)"""
    o = np.arange(nblocks, dtype=np.int64) * block_size
    return np.clip(total - o, 0, block_size)


def _record_word(res):
    """(R, delta flag) of a well-formed version 15 word of kind 1, else None"""
    R, F = res & 0x1FF, res >> 12 & 1
    if res != (KINDS_MARK | KIND_RECORD << 24 | F << 12 | R) or not 2 <= R <= RECORD_MAX:
        return None
    return R, bool(F)


def _stride_word(res):
    """E of a well-formed version 15 word of kind 2, else None"""
    E = res & 0xF
    if res != (KINDS_MARK | KIND_STRIDE << 24 | E) or E not in (1,) + ELEMENT_SIZES:
        return None
    return E


def pack(streams, offsets, params, block_size, total_len, element_size=1, block_crc=None, stored=None, filter=None, base=None,
         constant=None, unit_layouts=None, stride=None, record_size=None, lag=None, order=None, base_op="xor"):
    """streams: dense uint8 array; offsets: uint64[nblocks+1]; element_size: 1, or 2 / 4 / 8 for streams of the
    byte-plane layout (version 2).  params a StaticModel: streams of the static-table model (version 3, element size 1).
    params a PlaneStaticModel: streams of plane-static coding (version 4; element_size 1, the default, or the model's).
    params a SegmentStaticModel: streams of segment-static coding (version 5; element_size as for version 4).
    params a ContextStaticModel: streams of context-static coding (version 7, element size 1; tables equal to the rule's
    substitute for a context without bytes are dropped).
    block_crc: nblocks CRC-32 values of the uncompressed blocks (the version gets flag 0x10); None: no table.
    stored: nblocks 0 / 1 flags of compress_blocks(..., stored=) (the version gets flag 0x40); None: no bitmap.
    filter "delta": streams of compress_blocks(..., filter="delta") (version 6, any element_size; adaptive model, no stored).
    filter "zigzag": streams of compress_blocks(..., filter="zigzag") (version 11, as version 6).
    filter "lag" with lag S: streams of compress_blocks(..., filter="lag", lag=S) (version 13, as version 11).
    order K (with filter "lag"): streams of compress_blocks(..., filter="lag", lag=S, order=K) (version 14 for K = 2 or 3;
    None and 1: version 13).
    base (base_used, crc): streams of compress_blocks(..., base=y) with base_used = min(len(y), total_len) and crc =
    zlib.crc32(y[:base_used]) (version 8, any element_size; adaptive model, no stored, no filter).
    constant: nblocks 0 / 1 flags of compress_blocks(..., constant=) (version 9, any element_size, with or without base;
    adaptive model, no stored, no filter); None: no bitmap.
    unit_layouts: the ceil(nblocks / 8) layouts, 0 .. 7, of compress_blocks(..., unit_layouts=) (version 10; adaptive model,
    element_size 1 and none of stored, filter, base and constant); None: no unit table.
    base_op "sub" (with base, not with constant): streams of compress_blocks(..., base=y, base_op="sub") (version 12, as
    version 8).
    record_size R (with filter None or "delta" only): streams of compress_blocks(..., record_size=R, filter=) (version 15,
    kind 1; adaptive model, element_size 1 and none of the other options).
    filter "stride" with stride S: streams of compress_blocks(..., filter="stride", stride=S) (version 15, kind 2, any
    element_size, S as a u64 record behind the header; adaptive model and none of the other options)."""
    front, const, mixed = api._resolve_front(params, element_size, filter, base, base_op, constant, stored, unit_layouts, lag=lag,
                                             order=order, record_size=record_size, stride=stride)
    xbase = front.takes_base
    static, plane = isinstance(params, api.StaticModel), isinstance(params, api.PlaneStaticModel)
    segment = isinstance(params, api.SegmentStaticModel)
    context = isinstance(params, api.ContextStaticModel)
    if xbase:
        try:
            base_used, base_crc = (int(v) for v in base)
        except (TypeError, ValueError):
            raise api.InvalidInput()
        if not 0 <= base_used <= total_len or not 0 <= base_crc < 1 << 32:
            raise api.InvalidInput()
    if element_size not in (1,) + ELEMENT_SIZES or ((static or context) and element_size != 1) \
            or ((plane or segment) and element_size not in (1, params.element_size)):
        raise api.InvalidInput()
    if plane or segment:
        element_size = params.element_size
    P = api._params_of(params)
    offs = np.asarray(offsets, dtype=np.uint64)
    sizes = np.diff(offs.astype(np.int64))
    if (sizes < 0).any() or (sizes > 0xFFFFFFFF).any():
        raise api.InvalidInput()
    ver, res = (VERSION_STATIC, 0) if static else (VERSION_PLANE_STATIC, element_size << 16 | element_size) if plane \
        else (VERSION, 0) if element_size == 1 else (VERSION_PLANES, element_size)
    if segment:
        k = params.segment_blocks // (64 * element_size)
        if not 1 <= k < 1 << 24:
            raise api.InvalidInput()
        params.check(len(sizes))  # (the table count against this many blocks)
        ver, res = VERSION_SEGMENT_STATIC, SEGMENT_MARK | k << 4 | element_size
    if context:
        ver, res = VERSION_CONTEXT_STATIC, CONTEXT_MARK
    if front.record is not None:
        ver, res = VERSION_KINDS, KINDS_MARK | KIND_RECORD << 24 | front.record[1] << 12 | front.record[0]
    elif front.stride is not None:
        ver, res = VERSION_KINDS, KINDS_MARK | KIND_STRIDE << 24 | element_size
    elif filter is not None or xbase:
        ver = VERSION_LAG_ORDER if front.order else _VERSION_OF_FILTER[filter, base_op if xbase else None]
        res = FILTER_VERSIONS[ver].mark << 28 | (front.order or 0) << 16 | (front.lag or 0) << 4 | element_size
    if const:
        ver, res = VERSION_CONST, CONST_MARK | (1 if xbase else 0) << 4 | element_size
    crc = b""
    if block_crc is not None:
        c = np.asarray(block_crc)
        if c.shape != (len(sizes),):
            raise api.InvalidInput()
        ver |= CRC_FLAG
        crc = c.astype("<u4").tobytes()
    bitmap = b""
    if stored is not None:
        f = np.asarray(stored)
        if static or plane or segment or context or f.shape != (len(sizes),) or bool((f > 1).any()) \
                or bool((sizes[f == 1] != _raw_lengths(len(sizes), block_size, total_len)[f == 1]).any()):
            raise api.InvalidInput()
        ver |= STORED_FLAG
        bitmap = np.packbits(f.astype(np.uint8), bitorder="little").tobytes()
    if const:
        f = np.asarray(constant)
        if f.shape != (len(sizes),) or bool((f > 1).any()) or bool((sizes[f == 1] != 1).any()) \
                or bool((_raw_lengths(len(sizes), block_size, total_len)[f == 1] == 0).any()):
            raise api.InvalidInput()
        bitmap = np.packbits(f.astype(np.uint8), bitorder="little").tobytes()
    if mixed:
        t = np.asarray(unit_layouts)
        if t.shape != ((len(sizes) + MIXED_UNIT_BLOCKS - 1) // MIXED_UNIT_BLOCKS,) or t.dtype.kind not in "ui" \
                or bool((t > 7).any()) or bool((t < 0).any()):
            raise api.InvalidInput()
        ver, res = VERSION_MIXED | (ver & CRC_FLAG), MIXED_MARK
        bitmap = t.astype(np.uint8).tobytes()
    head = HEADER.pack(MAGIC, ver, P.symbol_bits, P.freq_bits, P.code_bits, block_size, res, len(sizes), total_len)
    if xbase:
        head += BASE_RECORD.pack(base_used, base_crc)
    if front.stride is not None:
        head += STRIDE_RECORD.pack(front.stride)
    if static:
        head += params.cum.astype("<u4").tobytes()
    if plane or segment:
        head += params.cums.astype("<u4").tobytes()
    if context:
        head += _pack_context_tables(params.cums)
    return head + sizes.astype("<u4").tobytes() + crc + bitmap + np.asarray(streams, dtype=np.uint8)[: int(offs[-1])].tobytes()


def _substitute_freqs(total):
    """the 256 byte frequencies of the table a context without bytes gets (include/redux_hip.h, "context-static coding",
    rule 3): the semi-static rule on a count of one for every byte value"""
    f = np.full(256, 1 + (total - 257) // 256, dtype=np.int64)
    f[: total - 1 - int(f.sum())] += 1
    return f


def _pack_context_tables(cums):
    """version 7's table section of np.uint32[256, 258] tables"""
    c = np.asarray(cums, dtype=np.int64)
    total = int(c[0, 257])
    freqs = np.diff(c[:, :257], axis=1)  # [256, 256]: the byte values' frequencies (all <= 65,535: the total is <= 2^16)
    present = (freqs != _substitute_freqs(total)).any(axis=1)
    return struct.pack("<I", total) + np.packbits(present, bitorder="little").tobytes() + freqs[present].astype("<u2").tobytes()


def _unpack_context_tables(b, at, P):
    """(np.uint32[256, 258], where the next section begins) of version 7's table section at b[at:]; InvalidInput for
    anything the rule cannot have written"""
    try:
        (total,), at = _take(b, at, "<u4", 1)
        mask, at = _take(b, at, np.uint8, 32)
        total = int(total)
        if not 257 <= total <= min(1 << 16, P.freq_max):
            raise api.InvalidInput()
        present = np.unpackbits(mask, bitorder="little").astype(bool)
        rows, at = _take(b, at, "<u2", 256 * int(present.sum()))
    except api.Eof:
        raise api.InvalidInput()
    freqs = np.tile(_substitute_freqs(total), (256, 1))
    freqs[present] = rows.reshape(-1, 256)
    if bool((freqs == 0).any()) or bool((freqs.sum(axis=1) != total - 1).any()):
        raise api.InvalidInput()
    cums = np.zeros((256, 258), dtype=np.int64)
    cums[:, 1:257] = np.cumsum(freqs, axis=1)
    cums[:, 257] = total
    return cums.astype(np.uint32), at


def _layout(ver):
    """the version without its checksum and stored-block flags"""
    return ver & ~(CRC_FLAG | STORED_FLAG)


def _version_ok(ver, res):
    """a known layout, its reserved word, and no stored blocks with a static table"""
    layout = _layout(ver)
    row = FILTER_VERSIONS.get(layout)
    if row is not None:  # (version 2 alone may have stored blocks, and has no element size 1: that is version 1)
        plain = layout == VERSION_PLANES
        if row.has_lag:
            S, K = _lag_word(row, res)
            if not 1 <= S <= LAG_MAX or (row.has_order and not 2 <= K <= LAG_ORDER_MAX):
                return False
        return res >> 28 == row.mark and res & (0xF if row.has_lag else 0x0FFFFFFF) in (() if plain else (1,)) + ELEMENT_SIZES \
            and (plain or not ver & STORED_FLAG)
    return (res == 0 and (layout == VERSION or (layout == VERSION_STATIC and not ver & STORED_FLAG))) \
        or (layout == VERSION_PLANE_STATIC and not ver & STORED_FLAG and res & 0xFFFF in ELEMENT_SIZES and res >> 16 == res & 0xFFFF) \
        or (layout == VERSION_SEGMENT_STATIC and not ver & STORED_FLAG and res >> 28 == 5 and res & 0xF in (1,) + ELEMENT_SIZES
            and res >> 4 & 0xFFFFFF >= 1) \
        or (layout == VERSION_CONTEXT_STATIC and not ver & STORED_FLAG and res == CONTEXT_MARK) \
        or (layout == VERSION_CONST and not ver & STORED_FLAG and res >> 28 == 9 and res & 0x0FFFFFEF in (1,) + ELEMENT_SIZES) \
        or (layout == VERSION_MIXED and not ver & STORED_FLAG and res == MIXED_MARK) \
        or (layout == VERSION_KINDS and not ver & STORED_FLAG and (_record_word(res) is not None or _stride_word(res) is not None))


def _has_base_record(ver, res):
    """of a checked header: does the base record follow it"""
    row = FILTER_VERSIONS.get(_layout(ver))
    return row.has_base if row is not None else _layout(ver) == VERSION_CONST and bool(res & 0x10)


# What _parse reads from a container: element_size 1, or E of versions 2 and 4; static the StaticModel of a version 3 table
# or the PlaneStaticModel of version 4's tables;
# offsets uint64[nblocks+1]; payload the uint8 streams; crcs (flag 0x10) uint32[nblocks]; stored (flag 0x40) uint8[nblocks]
# of 0 / 1.  static, crcs and stored are None where the container has no such section.  filter: "delta" for version 6, "zigzag"
# for version 11, else None.
# base: (base_used, crc) of the record of version 8 or 12, or of version 9 with F = 1, else None; base_op: "xor" or "sub" where
# there is a record, else None.  constant: uint8[nblocks] of 0 / 1
# for version 9, else None.  unit_layouts: uint8[ceil(nblocks / 8)] of 0 .. 7 for version 10, else None; element_size is then
# None, as the table holds it unit by unit.  lag: the lag S of version 13 or 14, else None.  order: the order K of version 14,
# else None.  record: (R, delta) of version 15's record layout, else None; element_size is then 1 and filter None.  stride: the
# stride S of version 15's snapshot-stride filter (kind 2), else None; filter is then "stride".
_Container = namedtuple("_Container", "params block_size total element_size static offsets payload crcs stored filter base constant"
                        " unit_layouts base_op lag order record stride", defaults=(None, None, None, None, None, None))


def _header(b):
    """-> (version, Parameters, block_size, element size, nblocks, total) of a consistent header; Eof if b is shorter
    than a header, InvalidInput if it is not consistent"""
    if len(b) < HEADER.size:
        raise api.Eof()
    magic, ver, sb, fb, cb, block_size, res, nblocks, total = HEADER.unpack_from(b, 0)
    if magic != MAGIC or not _version_ok(ver, res) or not 0 < block_size <= MAX_BLOCK_SIZE:
        raise api.InvalidInput()
    P = api.Parameters(sb, fb, cb)
    if nblocks != (1 if total == 0 else (total + block_size - 1) // block_size):
        raise api.InvalidInput()
    layout = _layout(ver)
    E = res & 0xF if layout in FILTER_VERSIONS or layout in (VERSION_SEGMENT_STATIC, VERSION_CONST) \
        else res & 0xFFFF if layout == VERSION_PLANE_STATIC else _stride_word(res) or 1 if layout == VERSION_KINDS else 1
    return ver, P, block_size, E, nblocks, total


def _segment_k(b):
    """k of a version 5 header (already checked by _header)"""
    return HEADER.unpack_from(b, 0)[6] >> 4 & 0xFFFFFF


def _take(b, at, dtype, count):
    """(count items of dtype at b[at:], where the next section begins); Eof if b ends first"""
    end = at + np.dtype(dtype).itemsize * count
    if len(b) < end:
        raise api.Eof()
    return np.frombuffer(b, dtype=dtype, count=count, offset=at), end


def _parse_index(b):
    """every check of the layout before the payload, section by section: header, table, sizes, CRCs, bitmap.  -> (the
    _Container without its payload, where the payload begins).  Malformed containers raise InvalidInput, truncated ones Eof
    (src/lib.rs:57-64)."""
    ver, P, block_size, E, nblocks, total = _header(b)
    static = crcs = stored = base = constant = units = stride = None
    at = HEADER.size
    if _layout(ver) == VERSION_KINDS and _stride_word(HEADER.unpack_from(b, 0)[6]) is not None:  # where version 8 keeps its record
        if len(b) < at + STRIDE_RECORD.size:
            raise api.Eof()
        stride, = STRIDE_RECORD.unpack_from(b, at)
        at += STRIDE_RECORD.size
        if stride == 0:
            raise api.InvalidInput()
    if _has_base_record(ver, HEADER.unpack_from(b, 0)[6]):
        if len(b) < at + BASE_RECORD.size:
            raise api.Eof()
        base = BASE_RECORD.unpack_from(b, at)
        at += BASE_RECORD.size
        if base[0] > total:
            raise api.InvalidInput()
    if _layout(ver) == VERSION_STATIC:
        cum, at = _take(b, at, "<u4", 258)
        try:
            static = api.StaticModel(P, cum)
        except api.Error:  # (redux_static_table_check: a bad table, or parameters the static coder does not take)
            raise api.InvalidInput()
    if _layout(ver) == VERSION_PLANE_STATIC:
        cums, at = _take(b, at, "<u4", 258 * E)
        try:
            static = api.PlaneStaticModel(P, cums.reshape(E, 258))
        except api.Error:  # (redux_plane_static_table_check)
            raise api.InvalidInput()
    if _layout(ver) == VERSION_SEGMENT_STATIC:
        G = 64 * E * _segment_k(b)
        nseg = max(1, -(-nblocks // G))  # (nseg follows from the header: a file with another table count reads as damaged)
        cums, at = _take(b, at, "<u4", 258 * E * nseg)
        try:
            static = api.SegmentStaticModel(P, cums.reshape(E * nseg, 258), E, G)
            static.check(nblocks)
        except api.Error:  # (redux_segment_static_table_check)
            raise api.InvalidInput()
    if _layout(ver) == VERSION_CONTEXT_STATIC:
        cums, at = _unpack_context_tables(b, at, P)
        try:
            static = api.ContextStaticModel(P, cums)
        except api.Error:  # (redux_context_static_table_check: parameters the static coder does not take)
            raise api.InvalidInput()
    sizes, at = _take(b, at, "<u4", nblocks)
    sizes = sizes.astype(np.uint64)
    offsets = np.zeros(nblocks + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(sizes)
    if ver & CRC_FLAG:
        crcs, at = _take(b, at, "<u4", nblocks)
        crcs = crcs.astype(np.uint32)
    if ver & STORED_FLAG:
        bits, at = _take(b, at, np.uint8, (nblocks + 7) // 8)
        flags = np.unpackbits(bits, bitorder="little")
        if bool(flags[nblocks:].any()):  # padding bits
            raise api.InvalidInput()
        stored = flags[:nblocks].astype(np.uint8)
        raw = stored == 1
        if bool((sizes[raw] != _raw_lengths(nblocks, block_size, total)[raw].astype(np.uint64)).any()):
            raise api.InvalidInput()
    if _layout(ver) == VERSION_CONST:
        bits, at = _take(b, at, np.uint8, (nblocks + 7) // 8)
        flags = np.unpackbits(bits, bitorder="little")
        if bool(flags[nblocks:].any()):  # padding bits
            raise api.InvalidInput()
        constant = flags[:nblocks].astype(np.uint8)
        if bool((sizes[constant == 1] != 1).any()):
            raise api.InvalidInput()
    if _layout(ver) == VERSION_MIXED:
        units, at = _take(b, at, np.uint8, (nblocks + MIXED_UNIT_BLOCKS - 1) // MIXED_UNIT_BLOCKS)
        units = units.copy()
        if bool((units > 7).any()):
            raise api.InvalidInput()
        E = None
    row = FILTER_VERSIONS.get(_layout(ver))  # (version 9's record, where it has one, is the XOR's)
    return _Container(P, block_size, total, E, static, offsets, None, crcs, stored,
                      row.filter if row else "stride" if stride is not None else None, base, constant,
                      units, row.base_op if row else None if base is None else "xor",
                      *(_lag_word(row, HEADER.unpack_from(b, 0)[6]) if row and row.has_lag else (None, None)),
                      _record_word(HEADER.unpack_from(b, 0)[6]) if _layout(ver) == VERSION_KINDS else None, stride), at


def _parse(buf):
    """_parse_index, then the payload: a payload shorter than the size table says is Eof"""
    b = memoryview(buf)
    c, at = _parse_index(b)
    payload, _ = _take(b, at, np.uint8, int(c.offsets[-1]))
    return c._replace(payload=payload)


def unpack(buf):
    """-> (Parameters, block_size, total_len, offsets uint64[nblocks+1], payload uint8 array).
    Malformed containers raise InvalidInput, truncated ones Eof (src/lib.rs:57-64)."""
    c = _parse(buf)
    return c.params, c.block_size, c.total, c.offsets, c.payload


def block_crcs(buf):
    """The per-block CRC-32 table (np.uint32[nblocks]) a flagged container (0x11 / 0x12 / 0x13) records; None without
    the flag.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).crcs


def block_stored(buf):
    """The stored-block flags (np.uint8[nblocks] of 0 / 1) a flagged container (0x41 / 0x42 / 0x51 / 0x52) records; None
    without the flag.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).stored


def element_size(buf):
    """Element size of the byte-plane layout a container records: 1 for versions 1 and 3, E for versions 2 and 4, None for
    version 10 (unit_layouts holds it unit by unit).  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).element_size


def filter(buf):
    """"delta" for a version 6 container (the delta filter for integer series), "zigzag" for a version 11 container (the same
    with folded differences), "lag" for a version 13 or 14 container (the lagged delta filter: lag(), order()), None for every other version (version 10 records the filter unit by unit: unit_layouts).  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).filter


def lag(buf):
    """The lag S of a version 13 or 14 container (the lagged delta filter, at order 1 or above); None for every other
    version.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).lag


def order(buf):
    """The order K of the lagged delta filter: 2 or 3 for a version 14 container (higher-order lagged differences), 1 for a
    version 13 container; None for every other version.  Malformed containers raise InvalidInput, truncated ones Eof."""
    c = _parse(buf)
    return c.order if c.order is not None else None if c.lag is None else 1


def record(buf):
    """(R, delta) of a version 15 container of kind 1 (the record layout for fixed-width structs): the record size and whether
    the byte delta against the record before was applied; None for every other container.  Malformed containers raise
    InvalidInput, truncated ones Eof."""
    return _parse(buf).record


def stride(buf):
    """(E, S) of a version 15 container of kind 2 (the snapshot-stride filter): the element size and the stride in elements;
    None for every other container.  Malformed containers raise InvalidInput, truncated ones Eof."""
    c = _parse(buf)
    return None if c.stride is None else (c.element_size, c.stride)


def base(buf):
    """(base_used, crc) of a version 8 container (the XOR-against-base filter), of a version 12 container (the folded
    difference against a base) and of a version 9 container with a base: the bytes of the base the coder used and the
    zlib.crc32 of them; None for every other container.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).base


def base_op(buf):
    """What the base filter of a container did with the base: "xor" for version 8 and for version 9 with a base, "sub" for
    version 12, None for every other container.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).base_op


def constant(buf):
    """The constant-block flags (np.uint8[nblocks] of 0 / 1) a version 9 container records; None for versions 1 to 8.
    Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).constant


def unit_layouts(buf):
    """The unit table (np.uint8[ceil(nblocks / 8)] of layouts 0 .. 7) a version 10 container records; None for versions 1 to
    9.  Malformed containers raise InvalidInput, truncated ones Eof."""
    return _parse(buf).unit_layouts


def static_table(buf):
    """The static table (np.uint32[258]) a version 3 container records; None for versions 1, 2 and 4.  Malformed
    containers raise InvalidInput, truncated ones Eof."""
    static = _parse(buf).static
    return static.cum if isinstance(static, api.StaticModel) else None


def plane_static_tables(buf):
    """The tables (np.uint32[E, 258]) a version 4 container records; None for versions 1, 2 and 3.  Malformed containers
    raise InvalidInput, truncated ones Eof."""
    static = _parse(buf).static
    return static.cums if isinstance(static, api.PlaneStaticModel) else None


def context_static_tables(buf):
    """The tables (np.uint32[256, 258]) a version 7 container records, the dropped ones rebuilt; None for versions 1 to 6.
    Malformed containers raise InvalidInput, truncated ones Eof."""
    static = _parse(buf).static
    return static.cums if isinstance(static, api.ContextStaticModel) else None


def segment_static_tables(buf):
    """(tables np.uint32[nseg * E, 258], segment_blocks) of a version 5 container; None for versions 1 to 4.  Malformed
    containers raise InvalidInput, truncated ones Eof."""
    static = _parse(buf).static
    return (static.cums, static.segment_blocks) if isinstance(static, api.SegmentStaticModel) else None


def header_is_wellformed(buf):
    """True when the first 32 bytes are a consistent container header: magic, version, a triple
    Parameters::new accepts, a block size in range and a block count that matches the declared
    length.  The CLI uses it to tell a container from a raw reference stream that happens to begin
    with the same four bytes: a well-formed header followed by a damaged or truncated body is a
    damaged CONTAINER (unpack's error is reported), not a raw stream."""
    try:
        _header(memoryview(buf))
    except api.Error:
        return False
    return True


def overhead_bytes(model, nblocks, element_size=1, segment_blocks=None, context_cums=None, checksum=False, stored=False,
                   filter=None, mixed=False, base=False, record_size=None):
    """The bytes pack() writes besides the payloads for `model` (one of api.MODELS) and nblocks blocks: header, tables, size
    table, and the CRC table / stored-block bitmap when asked for.  segment-static: segment_blocks None is
    api.default_segment_blocks(element_size).  context-static: context_cums, the np.uint32[256, 258] tables, is required,
    because only the tables of contexts that occur are recorded.  filter "delta", "zigzag" or "lag" (adaptive model, not stored):
    version 6, 11 or 13 (14 at an order above 1: the same size), which record the filter (and the lag and the order) in the header's reserved word and add no bytes.  mixed (adaptive model, element size 1, no
    filter, not stored): version 10, whose unit table adds a byte per 8 blocks.  base (adaptive model, no filter, not stored, not
    mixed): version 8 or 12, whose base record adds 12 bytes whatever the operation.  record_size (adaptive model, element size 1,
    filter None or "delta", not stored, not mixed, no base): version 15, which records the layout in the header's reserved word
    and adds no bytes.  filter "stride" (adaptive model, any element size, not stored, not mixed, no base, no record size):
    version 15 kind 2, whose stride record adds 8 bytes."""
    if isinstance(filter, str) and filter == "stride":
        if model != "adaptive" or stored or mixed or base or record_size is not None or nblocks < 1:
            raise api.InvalidInput()
        api._check_element_size(element_size)
        return HEADER.size + STRIDE_RECORD.size + 4 * nblocks + (4 * nblocks if checksum else 0)
    if record_size is not None:
        if model != "adaptive" or stored or mixed or base:
            raise api.InvalidInput()
        api._resolve_front(None, element_size, filter, record_size=record_size)
        if nblocks < 1:
            raise api.InvalidInput()
        return HEADER.size + 4 * nblocks + (4 * nblocks if checksum else 0)
    if model not in api.MODELS or nblocks < 1 or (mixed and (model != "adaptive" or element_size != 1 or stored or filter is not None)) \
            or (base and (model != "adaptive" or stored or filter is not None or mixed)):
        raise api.InvalidInput()
    if filter is not None and (model != "adaptive" or stored):
        raise api.InvalidInput()
    if filter is not None and (not isinstance(filter, str) or filter not in api._FILTERS):
        raise api.InvalidInput()
    E = api._check_element_size(element_size)
    n = HEADER.size + 4 * nblocks + (4 * nblocks if checksum else 0) + ((nblocks + 7) // 8 if stored else 0)
    if mixed:
        n += (nblocks + MIXED_UNIT_BLOCKS - 1) // MIXED_UNIT_BLOCKS
    if base:
        n += BASE_RECORD.size
    if model == "static":
        n += TABLE
    elif model == "plane-static":
        n += E * TABLE
    elif model == "segment-static":
        G = api.default_segment_blocks(E) if segment_blocks is None else segment_blocks
        n += max(1, -(-nblocks // G)) * E * TABLE
    elif model == "context-static":
        if context_cums is None:
            raise api.InvalidInput()
        n += len(_pack_context_tables(context_cums))
    return n


def estimate_bytes(data, block_size=65536, params=(8, 30, 32), element_size=1, segment_blocks=None, models=None, checksum=False,
                   record_size=None, filter=None):
    """-> {model: estimated container bytes}: api.estimate_payload's estimate of the payloads plus overhead_bytes, which is
    exact, for each model of `models` (None: api.estimate_candidates(element_size)).  Nothing is coded.  record_size (with
    filter None or "delta"; models None or ("adaptive",), no segment_blocks): the adaptive model behind the record layout,
    estimated on the transformed bytes (api.record_planes: one transform on the GPU, nothing coded)."""
    if record_size is not None or filter is not None:
        if record_size is None or segment_blocks is not None or (models is not None and tuple(models) != ("adaptive",)) \
                or not 0 < block_size <= MAX_BLOCK_SIZE:
            raise api.InvalidInput()
        front = api._resolve_front(None, element_size, filter, record_size=record_size).front
        torch = api._torch()
        a = api._u8(data)
        nb = max(1, -(-len(a) // block_size))
        over = overhead_bytes("adaptive", nb, checksum=checksum, filter=filter, record_size=record_size)
        if len(a) == 0:
            t = a
        else:
            t = api.record_planes(torch.from_numpy(a.copy()).cuda(), front.record[0], block_size, delta=bool(front.record[1])).cpu().numpy()
        payload, _ = api._estimate(t, block_size, params, 1, None, ["adaptive"])
        return {"adaptive": payload["adaptive"] + over}
    payload, context_cums = api._estimate(data, block_size, params, element_size, segment_blocks, models)
    nb = max(1, -(-len(data) // block_size))
    return {m: payload[m] + overhead_bytes(m, nb, element_size, segment_blocks, context_cums, checksum) for m in payload}


def choose_model(estimates):
    """The model with the smallest estimate; ties go to the earlier of api.MODELS."""
    return min(estimates, key=lambda m: (estimates[m], api.MODELS.index(m)))


LAYOUT_ORDER = api.LAYOUTS  # (1, None), (2, None), (4, None), (8, None), (1, "delta"), ... (8, "delta")


def estimate_layout_bytes(data, block_size=65536, params=(8, 30, 32), element_size=None, checksum=False, mixed=False):
    """-> {(element_size, filter): estimated container bytes} for the adaptive model behind each layout: api.estimate_layouts'
    estimate of the payloads (one pass over the bytes as they are on the GPU; nothing is transformed or coded) plus
    overhead_bytes, which is exact.  element_size None: all eight layouts; 1 / 2 / 4 / 8: plain and delta at that size.
    mixed=True adds the key "mixed": the version 10 container of compress_bytes(..., layout="mixed") among those layouts."""
    payload = api.estimate_layouts(data, block_size, params, element_size, mixed=mixed)
    nb = max(1, -(-len(data) // block_size))
    est = {k: payload[k] + overhead_bytes("adaptive", nb, k[0], checksum=checksum, filter=k[1]) for k in payload if k != "mixed"}
    if mixed:
        est["mixed"] = payload["mixed"] + overhead_bytes("adaptive", nb, checksum=checksum, mixed=True)
    return est


def estimate_lag_bytes(data, element_size, block_size=65536, lags=None, params=(8, 30, 32), checksum=False, frame_step=1):
    """-> {S: estimated container bytes} for the adaptive model behind the lagged delta filter with each lag of `lags` (None:
    1 .. LAG_MAX): api.estimate_lags' estimate of the payloads (counted from the bytes as they are on the GPU; nothing is
    transformed or coded) plus overhead_bytes(..., filter="lag"), which is exact: directly comparable with
    estimate_layout_bytes, for a caller who asks whether the filter pays at all.  frame_step above 1 estimates the selected
    frames' payload only, under the whole container's overhead."""
    payload = api.estimate_lags(data, element_size, block_size, lags, params, frame_step)
    over = overhead_bytes("adaptive", max(1, -(-len(data) // block_size)), element_size, checksum=checksum, filter="lag")
    return {S: payload[S] + over for S in payload}


def estimate_lag_order_bytes(data, element_size, block_size=65536, candidates=((1, 1), (1, 2), (1, 3)), params=(8, 30, 32), checksum=False,
                             frame_step=1):
    """-> {(S, K): estimated container bytes} for the adaptive model behind the lag filter at lag S and order K, for each pair
    of `candidates`: api.estimate_lag_orders' estimate of the payloads (counted from the bytes as they are on the GPU; nothing
    is transformed or coded) plus overhead_bytes(..., filter="lag"), which is exact for every order: version 13 (K = 1) and
    version 14 (K = 2, 3) record lag and order in the header's reserved word and have the same sections, so their overhead is
    the same size.  Directly comparable with estimate_lag_bytes and estimate_layout_bytes.  frame_step above 1 estimates the
    selected frames' payload only, under the whole container's overhead."""
    payload = api.estimate_lag_orders(data, element_size, block_size, candidates, params, frame_step)
    over = overhead_bytes("adaptive", max(1, -(-len(data) // block_size)), element_size, checksum=checksum, filter="lag")
    return {c: payload[c] + over for c in payload}


def estimate_record_bytes(data, block_size=65536, candidates=None, params=(8, 30, 32), checksum=False, sample_blocks=0):
    """-> {(R, filter): estimated container bytes} for the adaptive model behind the record layout for each pair of
    `candidates` (None: all 510): api.estimate_records' estimate of the payloads (counted from the bytes as they are on the
    GPU; nothing is transformed or coded) plus overhead_bytes(..., record_size=R), which is exact: version 15 records the layout in
    the header's reserved word, so it is the plain container's overhead and the figures compare directly with
    estimate_bytes(...)["adaptive"].  sample_blocks above 0 estimates the selected frames' payload only, under the whole
    container's overhead."""
    payload = api.estimate_records(data, block_size, candidates, params, sample_blocks)
    nb = max(1, -(-len(data) // block_size))
    return {c: payload[c] + overhead_bytes("adaptive", nb, checksum=checksum, filter=c[1], record_size=c[0]) for c in payload}


def choose_layout(estimates):
    """The (element_size, filter) with the smallest estimate; ties go to the earlier of LAYOUT_ORDER."""
    return min(estimates, key=lambda k: (estimates[k], LAYOUT_ORDER.index(k)))


def choose_base_op(estimates):
    """The operation of the base filter with the smaller estimate (api.estimate_base_ops); a tie goes to "xor"."""
    return min(estimates, key=lambda op: (estimates[op], api.BASE_OPS.index(op)))


def compress_bytes(data, block_size=65536, params=(8, 30, 32), element_size=1, model="adaptive", checksum=False,
                   stored=False, segment_blocks=None, filter=None, base=None, skip_constant=False, layout=None, stride=None, record_size=None, lag=None,
                   order=None, base_op="xor"):
    """bytes -> container bytes (every block coded on the GPU); element_size 2 / 4 / 8: byte-plane layout, version 2.
    model "static": the static table of the data (api.static_table, default total) codes every block, version 3.
    checksum: record the CRC-32 of every block (flag 0x10), taken by the same coding call.
    model "plane-static" (element_size 2 / 4 / 8): a static table per byte plane, built from the data
    (api.plane_static_tables, default total), version 4.
    stored: blocks whose stream does not shrink them travel raw (flag 0x40, api.STORE_RATIO); not with a static model.
    model "segment-static" (element_size 1 / 2 / 4 / 8): static tables per segment_blocks blocks (a multiple of
    64 * element_size; None: api.default_segment_blocks), built from each range as it is coded, version 5.
    filter "delta" (element_size 1 / 2 / 4 / 8, model "adaptive", not stored): the delta filter for integer series in front of
    the layout, version 6.
    filter "zigzag" (as "delta"): the delta filter with its differences folded, for series that move both ways, version 11.
    filter "lag" with lag S, 1 .. 256 (as "zigzag"; not with layout): the folded difference to the element S back, for S
    interleaved channels or records of S columns, version 13.  A lag without filter "lag" is InvalidInput, and so is the filter
    without one.  lag "auto" (with filter "lag"; here only, not in the block calls or the device coders): the lag with the
    smallest estimate codes the data (api.choose_lag: counted on the GPU from the bytes as they are, exact on every frame for
    the finalists, lag 1 always among them), and the container is that lag's, version 13, which records it: nothing new to
    decode.  The filter itself stays opt-in.
    order K, 1 .. 3 (with filter "lag" only): the lag-S difference applied K times, for sampled signals that are locally
    polynomial; version 14 for K = 2 or 3, which records K, and version 13, byte for byte, for K = 1.  On random walks a
    higher order costs bytes, so nothing chooses it unasked.  Not with lag "auto" above order 1: the lag estimates count order 1
    only.  order "auto" (with filter "lag" and a lag S or "auto"; here only, not in the block calls or the device coders): the
    order is counted too (api.choose_lag_order: one exact pass over orders 1, 2, 3 at lag S, or over the orders of every
    finalist of lag "auto"; ties go to the smaller order, then to the smaller lag), and the container is that choice's ordinary
    one, version 13 for order 1 and version 14 above: nothing new to decode.  Refused with everything order 2 is refused with.
    model "context-static" (element_size 1, not stored, no filter): a static table per preceding byte, built from the data
    (api.context_static_tables, default total), version 7.  It pays from about half a megabyte of text upward, and
    only model "auto" picks it for the caller.
    model "auto" (not stored, no filter, no segment_blocks): the model with the smallest estimate_bytes codes the data
    (choose_model), and the container is that model's: no version of its own, nothing new to decode.
    base (bytes-like of any length; any element_size, model "adaptive", not stored, no filter): an earlier snapshot of the
    data; the XOR against it is coded, version 8, and decompress_bytes needs the same base.
    skip_constant (any element_size, model "adaptive", not stored, no filter; with or without base): blocks of the coder's
    input whose bytes are all equal travel as one byte and skip the coder in both directions, version 9.
    layout "auto" (model "adaptive", not stored, no filter, no base, no skip_constant): the element size and the filter
    with the smallest estimate_layout_bytes code the data (choose_layout) -- of all eight layouts when element_size is None,
    of plain and delta at that size when element_size is 1 / 2 / 4 / 8 (the default, 1, included: a caller who knows the dtype
    says so, one who does not passes None) -- and the container is that layout's: version 1, 2 or 6, nothing new to
    decode.
    layout "mixed" (the exclusions of "auto"): a layout per unit of 8 blocks, chosen on the device by its estimated cost --
    among all eight when element_size is None, between plain and delta at that size when element_size is 1 / 2 / 4 / 8 --
    version 10.  For files that hold several element types.
    base_op (with base, not with skip_constant): "sub" codes the folded difference of the elements against the base in place
    of the XOR, version 12.  "auto": the operation with the smaller estimated payload codes the data (choose_base_op; a tie
    goes to "xor"), and the container is that operation's, version 8 or 12: nothing new to decode.  Related pairs favour
    "sub", unrelated ones "xor", and a caller cannot know in advance.
    record_size R, 2 .. 256 (element_size 1, model "adaptive", filter None or "delta", and none of stored, segment_blocks,
    base, skip_constant, layout, lag and order): the record layout for fixed-width structs, every block one byte column of
    block_size records of R bytes; filter "delta" is then the byte delta against the record before.  Version 15, kind 1.
    record_size "auto" (the exclusions of a record size, and no filter; here only, not in the block calls or the device
    coders): the record size and the filter with the smallest estimate code the data (api.choose_record: all 510 candidates
    counted on the GPU from the bytes as they are, on a sample first, then exactly for the finalists and for the plain bytes,
which also keep every gain that noise among 510 candidates explains),
    and the container is that choice's ordinary one, version 15 -- or version 1 where the plain bytes are estimated no
    larger: nothing new to decode.
    filter "stride" with stride S, 1 or more (any element_size, model "adaptive", and none of stored, segment_blocks, base,
    skip_constant, layout, record_size, lag and order): the snapshot-stride filter for one buffer of T snapshots of the same S
    elements, every element against the same element one snapshot back.  Version 15, kind 2, which records S; the container has
    no range reads.  A stride without the filter is InvalidInput, and so is the filter without one."""
    if stride is not None or (isinstance(filter, str) and filter == "stride"):
        if layout is not None or model != "adaptive" or stored or segment_blocks is not None or skip_constant or base_op != "xor" \
                or not 0 < block_size <= MAX_BLOCK_SIZE:
            raise api.InvalidInput()
        api._resolve_front(None, element_size, filter, base, lag=lag, order=order, record_size=record_size, stride=stride)
        crc = np.zeros(max(1, -(-len(data) // block_size)), dtype=np.uint32) if checksum else None
        out, offs, _ = api.compress_blocks(data, block_size, params, element_size=element_size, block_crc=crc, filter=filter,
                                           stride=stride)
        return pack(out, offs, params, block_size, len(data), element_size, block_crc=crc, filter=filter, stride=stride)
    auto_record = isinstance(record_size, str) and record_size == "auto"  # (the choice is made below, once nothing refuses the call)
    if auto_record:
        if filter is not None:
            raise api.InvalidInput()
        record_size = 2  # (until then it is refused where a record size is)
    if record_size is not None:
        if layout is not None or model != "adaptive" or stored or segment_blocks is not None or skip_constant or base_op != "xor" \
                or not 0 < block_size <= MAX_BLOCK_SIZE:
            raise api.InvalidInput()
        api._resolve_front(None, element_size, filter, base, lag=lag, order=order, record_size=record_size)
        if auto_record:
            choice = api.choose_record(data, block_size, params)[0]
            if choice is None:  # the layout is estimated to cost bytes: the plain container
                return compress_bytes(data, block_size, params, checksum=checksum)
            record_size, filter = choice
        crc = np.zeros(max(1, -(-len(data) // block_size)), dtype=np.uint32) if checksum else None
        out, offs, _ = api.compress_blocks(data, block_size, params, block_crc=crc, filter=filter, record_size=record_size)
        return pack(out, offs, params, block_size, len(data), block_crc=crc, filter=filter, record_size=record_size)
    api._resolve_front(None, base=base, base_op="sub" if base_op == "auto" else base_op,
                       constant=skip_constant or None)  # (base_op alone is judged here; "auto": the refusals of "sub")
    auto_lag = isinstance(lag, str) and lag == "auto"  # (the choice is made below, once nothing else refuses the call)
    if auto_lag:
        lag = 1
    auto_order = isinstance(order, str) and order == "auto"  # (the same: until then it is refused where order 2 is)
    if auto_order:
        order = 2
    if lag is not None or order is not None or (isinstance(filter, str) and filter == "lag"):  # (a lag, its order and their filter go together)
        if api._resolve_front(None, filter=filter, lag=lag, order=order).front.order and auto_lag and not auto_order:
            raise api.InvalidInput()  # (choose_lag counts order-1 costs only)
    if layout is not None:
        if layout not in ("auto", "mixed") or model != "adaptive" or stored or segment_blocks is not None or filter is not None \
                or base is not None or skip_constant or not 0 < block_size <= MAX_BLOCK_SIZE \
                or (element_size is not None and element_size != 1 and element_size not in ELEMENT_SIZES):
            raise api.InvalidInput()
        if layout == "mixed":
            want = [k for k in api.LAYOUTS if element_size is None or k[0] == element_size]
            nb = max(1, -(-len(data) // block_size))
            crc = np.zeros(nb, dtype=np.uint32) if checksum else None
            out, offs, _, table = api.compress_blocks(data, block_size, params, block_crc=crc, unit_layouts=True, layouts=want)
            return pack(out, offs, params, block_size, len(data), block_crc=crc, unit_layouts=table)
        element_size, filter = choose_layout(estimate_layout_bytes(data, block_size, params, element_size, checksum))
    if (skip_constant or base is not None or filter is not None) and (model != "adaptive" or stored):
        raise api.InvalidInput()
    api._resolve_front(None, filter=filter, base=base, constant=skip_constant or None, lag=lag, order=order)  # (the model is a name here)
    if model == "auto":
        if not 0 < block_size <= MAX_BLOCK_SIZE or (element_size != 1 and element_size not in ELEMENT_SIZES) or stored \
                or segment_blocks is not None:
            raise api.InvalidInput()
        model = choose_model(estimate_bytes(data, block_size, params, element_size, checksum=checksum))
    if not 0 < block_size <= MAX_BLOCK_SIZE or (element_size != 1 and element_size not in ELEMENT_SIZES) \
            or model not in ("adaptive", "static", "plane-static", "segment-static", "context-static") \
            or (model in ("static", "context-static") and (element_size != 1 or stored)) \
            or (model == "plane-static" and (element_size == 1 or stored)) or (model == "segment-static" and stored) \
            or (model != "segment-static" and segment_blocks is not None):
        raise api.InvalidInput()
    if auto_order:
        lag, order = api.choose_lag_order(data, element_size, block_size, None if auto_lag else lag, params)[0]
    elif auto_lag:
        lag = api.choose_lag(data, element_size, block_size, params)[0]
    nb = max(1, -(-len(data) // block_size))
    crc = np.zeros(nb, dtype=np.uint32) if checksum else None
    flags = np.zeros(nb, dtype=np.uint8) if stored else None
    m = api.StaticModel.from_data(data, params) if model == "static" \
        else api.PlaneStaticModel.from_data(data, element_size, block_size, params) if model == "plane-static" \
        else api.SegmentStaticModel.template(params, element_size, segment_blocks) if model == "segment-static" \
        else api.ContextStaticModel.from_data(data, block_size, params) if model == "context-static" else params
    record = None
    if base is not None:
        base = api._u8(base)[: len(data)]  # (what the coder uses of it)
        record = (len(base), zlib.crc32(base))
    if base_op == "auto":
        base_op = choose_base_op(api.estimate_base_ops(data, base, block_size, params, element_size))
    cflags = np.zeros(nb, dtype=np.uint8) if skip_constant else None
    out, offs, _ = api.compress_blocks(data, block_size, m, element_size=element_size, block_crc=crc, stored=flags, filter=filter,
                                       base=base, constant=cflags, base_op=base_op, lag=lag, order=order)
    return pack(out, offs, m, block_size, len(data), element_size, block_crc=crc, stored=flags, filter=filter, base=record,
                constant=cflags, base_op=base_op, lag=lag, order=order)


def decompress_bytes(buf, base=None):
    """container bytes -> original bytes.  base: the bytes a version 8 or 12 container, or a version 9 container with a base
    record, was written against (at least its base_used bytes of them; more is fine), and None for every other container: a
    missing, short or different base, and a base given for a container without a record, are InvalidInput before anything is
    decoded."""
    c = _parse(buf)
    return _decode_parsed(c, _checked_base(c, base))


def _checked_base(c, base):
    """the base a container's record asks for, cut to the bytes the coder used: InvalidInput for a missing, short or different
    base, and for a base given to a container without a record"""
    if (base is None) != (c.base is None):
        raise api.InvalidInput()
    if c.base is not None:
        base = api._u8(base)
        if len(base) < c.base[0] or zlib.crc32(base[: c.base[0]]) != c.base[1]:
            raise api.InvalidInput()
        base = base[: c.base[0]]
    return base


def _decode_parsed(c, base):
    """the bytes of a parsed container (base: _checked_base's): one decompress_blocks call, then every block's size against its
    raw length and, with checksums, every OK block's CRC-32 against the recorded one"""
    # A stream of s bytes can decode to far more than s bytes (64 KiB of one symbol is ~400 bytes),
    # so only the declared total bounds the capacity; but every block's stream has at least one
    # byte, so a header that declares more blocks than there are payload bytes is malformed.
    nb = len(c.offsets) - 1
    if len(c.payload) < nb - (0 if c.stored is None else int(c.stored.sum())):  # (a stored block may be empty)
        raise api.InvalidInput()
    got = None if c.crcs is None else np.zeros(nb, dtype=np.uint32)
    segment = isinstance(c.static, api.SegmentStaticModel)
    mixed = c.unit_layouts is not None
    exact = mixed or c.element_size > 1 or c.stored is not None or segment or c.filter is not None or c.base is not None \
        or c.constant is not None or c.record is not None  # (c.filter: "stride" of version 15 kind 2 included)
    cap = max(1, min(c.block_size, c.total))  # one short block never needs block_size bytes of capacity
    try:
        if mixed:
            out, sizes, status = api.decompress_blocks(c.payload, c.offsets, c.block_size, c.params, length=c.total, block_crc=got,
                                                       unit_layouts=c.unit_layouts)
        elif exact:  # (the blocks decode at their real size, into out[0 .. total))
            out, sizes, status = api.decompress_blocks(c.payload, c.offsets, c.block_size,
                                                       c.static if (c.element_size > 1 or segment) and c.static is not None else c.params,
                                                       element_size=c.element_size, length=c.total, block_crc=got,
                                                       stored=c.stored, base=base, constant=c.constant,
                                                       filter="delta" if c.record is not None and c.record[1] else c.filter,
                                                       base_op=c.base_op or "xor", lag=c.lag, order=c.order,
                                                       record_size=None if c.record is None else c.record[0], stride=c.stride)
        else:  # (straight into out[b * cap ..], no plane buffer)
            out, sizes, status = api.decompress_blocks(c.payload, c.offsets, cap, c.static or c.params, block_crc=got)
    except MemoryError:  # a header can declare far more output than this machine holds: malformed for our purposes
        raise api.InvalidInput()
    if not np.array_equal(sizes, _raw_lengths(nb, c.block_size, c.total)):
        raise api.InvalidInput()
    if c.crcs is not None and bool(((got != c.crcs) & (status == 0)).any()):  # (every OK block: its recorded CRC)
        raise api.InvalidInput()
    if exact or c.total == nb * cap:
        return out.tobytes()
    return b"".join(out[b * cap: b * cap + int(sizes[b])].tobytes() for b in range(nb))


# ---- range reads: decode only the blocks a byte range covers (include/redux_hip.h, "range reads") ----------------------------
CONTEXT_TABLES_MAX = 36 + 256 * 512  # version 7's table section at most: the total, the mask, 256 rows of 256 u16


class _Source:
    """the bytes of a container, fetched piece by piece: a bytes-like object, or a seekable binary file object.  bytes_read
    counts what was fetched."""

    def __init__(self, source):
        self.bytes_read = 0
        if hasattr(source, "read") and hasattr(source, "seek"):
            self.file, self.view = source, None
            self.size = source.seek(0, 2)
        else:
            self.file, self.view = None, memoryview(source).cast("B")
            self.size = len(self.view)

    def fetch(self, at, n):
        """the bytes [at, at + n), fewer where the source ends first"""
        n = max(0, min(n, self.size - at))
        if self.view is not None:
            got = self.view[at: at + n]
        else:
            self.file.seek(at)
            got = self.file.read(n)
        self.bytes_read += len(got)
        return got


def _index_rest_bytes(ver, nblocks):
    """the bytes of the sections between the tables and the payload: sizes, CRCs, the bitmap or the unit table"""
    n = 4 * nblocks + (4 * nblocks if ver & CRC_FLAG else 0) + ((nblocks + 7) // 8 if ver & STORED_FLAG else 0)
    if _layout(ver) == VERSION_CONST:
        n += (nblocks + 7) // 8
    if _layout(ver) == VERSION_MIXED:
        n += (nblocks + MIXED_UNIT_BLOCKS - 1) // MIXED_UNIT_BLOCKS
    return n


class Reader:
    """Random access to a container's bytes: read(start, length) decodes only the granules the range covers (a frame of E
    blocks; a unit of 8 blocks for version 10; a segment for version 5; a frame of R blocks for version 15's record layout), and read_many(ranges) does so for any number of ranges
    in ONE coder call.
    source: the container as a bytes-like object, or a seekable binary file object, from which the header and the index
    sections are read at open (every section's size follows from the header; of version 7's table section, whose size does
    not, CONTEXT_TABLES_MAX bytes are read and then parsed) and later only the streams of covered blocks: the payload of
    blocks no range covers is never read, so damage there -- a truncated file included -- does not matter to a range read.
    base: as for decompress_bytes; it is checked against the container's record here, once.
    total, block_size, nblocks, version, filter, lag, order, base_op, granule_blocks, payload_offset: the container's; bytes_read: the bytes fetched from
    the source so far."""

    def __init__(self, source, base=None):
        self._src = src = _Source(source)
        head = bytes(src.fetch(0, HEADER.size))
        ver, P, _, E, nblocks, _ = _header(head)
        res = HEADER.unpack_from(head, 0)[6]
        layout = _layout(ver)
        tables = BASE_RECORD.size if _has_base_record(ver, res) else 0
        if layout == VERSION_KINDS and _stride_word(res) is not None:
            tables += STRIDE_RECORD.size
        if layout == VERSION_STATIC:
            tables += TABLE
        elif layout == VERSION_PLANE_STATIC:
            tables += E * TABLE
        elif layout == VERSION_SEGMENT_STATIC:
            tables += max(1, -(-nblocks // (64 * E * _segment_k(head)))) * E * TABLE
        rest = _index_rest_bytes(ver, nblocks)
        if layout == VERSION_CONTEXT_STATIC:  # (the table section says how long it is)
            index = head + bytes(src.fetch(HEADER.size, CONTEXT_TABLES_MAX))
            _, at = _unpack_context_tables(memoryview(index), HEADER.size, P)
            index = index[: at + rest] + bytes(src.fetch(len(index), at + rest - len(index)))
        else:
            index = head + bytes(src.fetch(HEADER.size, tables + rest))
        self._c, self.payload_offset = _parse_index(memoryview(index))
        c = self._c
        self.version, self.total, self.block_size, self.nblocks = ver, c.total, c.block_size, nblocks
        self.filter, self.base_op, self.lag, self.order = c.filter, c.base_op, c.lag, c.order
        self.record = c.record
        self.stride = c.stride
        self.granule_blocks = MIXED_UNIT_BLOCKS if c.unit_layouts is not None \
            else c.static.segment_blocks if isinstance(c.static, api.SegmentStaticModel) \
            else c.record[0] if c.record is not None else c.element_size
        self._base = _checked_base(c, base)

    @property
    def bytes_read(self):
        return self._src.bytes_read

    def read(self, start, length):
        """the bytes [start, start + length) of the original data"""
        return self.read_many([(start, length)])[0]

    def read_many(self, ranges):
        """-> [the bytes of each (start, length) of `ranges`], which may come in any order, overlap and repeat: the granules
        they cover are decoded once, in one decompress_blocks call (none when no range has bytes), with every check
        decompress_bytes makes applied to the covered blocks.  A range that leaves [0, total] is InvalidInput; a source that
        ends inside a covered stream is Eof.  A container of the snapshot-stride filter (version 15, kind 2) raises Unsupported:
        an element there needs every snapshot before it, and the container keeps no keyframes."""
        if self.stride is not None:
            raise api.Unsupported()
        c, g, B = self._c, self.granule_blocks, self.block_size
        ranges = list(ranges)
        runs, virt_off, virt_len = api.range_plan(c.total, B, g, ranges)
        if virt_len == 0:
            return [b""] * len(ranges)
        blocks = [(f * g, min((f + n) * g, self.nblocks)) for f, n in runs]
        parts = []
        for b0, b1 in blocks:
            o0, o1 = int(c.offsets[b0]), int(c.offsets[b1])
            part = self._src.fetch(self.payload_offset + o0, o1 - o0)
            if len(part) < o1 - o0:
                raise api.Eof()
            parts.append(np.frombuffer(part, dtype=np.uint8))
        sel = np.concatenate([np.arange(b0, b1) for b0, b1 in blocks])
        offsets = np.zeros(len(sel) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(c.offsets[sel + 1] - c.offsets[sel])
        static, base = c.static, self._base
        if isinstance(static, api.SegmentStaticModel):  # (a granule is a segment: the tables of the covered ones)
            E = static.element_size
            segs = np.concatenate([np.arange(f, f + n) for f, n in runs])
            static = api.SegmentStaticModel(c.params, static.cums.reshape(-1, E, 258)[segs].reshape(-1, 258), E, g)
        if base is not None:  # (what the base holds of each run: in ascending order a prefix of the virtual input)
            base = np.concatenate([base[b0 * B: min(b1 * B, c.total)] for b0, b1 in blocks])
        pick = lambda a: None if a is None else a[sel]
        v = c._replace(total=virt_len, static=static, offsets=offsets, payload=np.concatenate(parts), crcs=pick(c.crcs),
                       stored=pick(c.stored), constant=pick(c.constant),
                       unit_layouts=None if c.unit_layouts is None else c.unit_layouts[np.unique(sel // MIXED_UNIT_BLOCKS)])
        out = _decode_parsed(v, base)
        return [out[o: o + int(n)] for o, (_, n) in zip(virt_off, ranges)]


def decompress_range(buf, start, length, base=None):
    """container bytes -> the bytes [start, start + length) of the original data, decoding only the blocks the range covers
    (Reader(buf, base).read(start, length))."""
    return Reader(buf, base).read(start, length)
