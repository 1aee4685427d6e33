// redux.hpp -- C++ host-side mirror of peterbudai/redux's public interface for the block-coding
// path, header-only, on top of the C ABI in include/redux_hip.h (link with libredux_hip.so).
//
// The reference is a Rust crate and this image has no Rust toolchain, so the host side that
// sits above the C ABI is written in C++ with the reference's names, argument meaning and
// error behaviour (file:line under the reference checkout):
//
//   redux::Error { Eof, InvalidInput, IoError }            src/lib.rs:57-64
//   redux::model::Parameters::make(symbol, freq, code)      src/model/mod.rs:63  (Parameters::new)
//   redux::model::Model / AdaptiveTreeModel::make(params)   src/model/mod.rs:17, adaptive_tree.rs:36
//   redux::compress(istream, ostream, model) -> (u64,u64)   src/lib.rs:102
//   redux::decompress(istream, ostream, model)              src/lib.rs:113
//   redux::hip::compress_blocks / decompress_blocks         the block API the GPU path adds
//   redux::hip::compress_blocks_v / decompress_blocks_v     many independent inputs in one launch (tests/corpora.rs:32-85)
//   redux::hip::compress_blocks_planes / decompress_blocks_planes   typed data in the byte-plane layout
//   redux::hip::compress_blocks_delta / decompress_blocks_delta     integer series behind the delta filter
//   redux::hip::compress_blocks_zigzag / decompress_blocks_zigzag   signed series behind the zigzag-folded delta filter
//   redux::hip::compress_blocks_lag / decompress_blocks_lag         interleaved channels behind the lagged delta filter
//   redux::hip::compress_blocks_lag_order / decompress_blocks_lag_order   sampled signals behind higher-order lagged differences
//   redux::hip::compress_blocks_record / decompress_blocks_record   tables of fixed-width structs behind the record layout
//   redux::hip::compress_blocks_base / decompress_blocks_base       a snapshot behind the XOR-against-base filter
//   redux::hip::compress_blocks_base_sub / decompress_blocks_base_sub   the same behind the folded difference against the base
//   redux::hip::compress_blocks_stored / decompress_blocks_stored   stored (raw) blocks for data that does not shrink
//   redux::hip::compress_blocks_const / decompress_blocks_const     constant blocks skipped, with or without a base
//   redux::hip::static_table / compress_blocks_static / decompress_blocks_static   semi-static coding: one table from the data
//   redux::hip::compress_blocks_segment_static / decompress_blocks_segment_static   static tables per block range
//   redux::hip::context_static_tables / compress_blocks_context_static / decompress_blocks_context_static   a table per preceding byte
//
// Every stream byte is produced by the gfx950 kernels; there is no CPU coder in this header.
#pragma once

#include <cstdint>
#include <istream>
#include <iterator>
#include <memory>
#include <ostream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/redux_hip.h"

namespace redux {

// src/lib.rs:57-96
class Error : public std::runtime_error {
public:
    enum Kind { Eof = REDUX_EOF, InvalidInput = REDUX_INVALID_INPUT, IoError = REDUX_IO_ERROR };
    Error(Kind k, int status, const std::string &what) : std::runtime_error(what), kind_(k), status_(status) {}
    Kind kind() const { return kind_; }
    int  status() const { return status_; } // the raw C-ABI status (4 OutputTooSmall, 5 Unsupported map to IoError)
    static Error from_status(int st)
    {
        switch (st) {
        case REDUX_EOF: return Error(Eof, st, "Unexpected end of file");                               // lib.rs:69
        case REDUX_INVALID_INPUT: return Error(InvalidInput, st, "Invalid data found while processing input"); // lib.rs:70
        case REDUX_OUTPUT_TOO_SMALL: return Error(IoError, st, "I/O error: output buffer too small");
        case REDUX_UNSUPPORTED: return Error(IoError, st, "I/O error: parameters not supported by the device path");
        default: return Error(IoError, st, "I/O error: HIP runtime failure");
        }
    }

private:
    Kind kind_;
    int  status_;
};

inline void check(int st)
{
    if (st != REDUX_OK)
        throw Error::from_status(st);
}

namespace model {

// src/model/mod.rs:32-81
struct Parameters {
    std::size_t   symbol_bits, symbol_eof, symbol_count, freq_bits;
    std::uint64_t freq_max;
    std::size_t   code_bits;
    std::uint64_t code_min, code_one_fourth, code_half, code_three_fourths, code_max;

    // Parameters::new: throws Error(InvalidInput) exactly where the reference returns Err (mod.rs:64)
    static Parameters make(std::size_t symbol, std::size_t frequency, std::size_t code)
    {
        check(redux_params_check((uint32_t)symbol, (uint32_t)frequency, (uint32_t)code));
        Parameters p;
        p.symbol_bits        = symbol;
        p.symbol_eof         = std::size_t(1) << symbol;
        p.symbol_count       = (std::size_t(1) << symbol) + 1;
        p.freq_bits          = frequency;
        p.freq_max           = (std::uint64_t(1) << frequency) - 1;
        p.code_bits          = code;
        p.code_min           = 0;
        p.code_one_fourth    = std::uint64_t(1) << (code - 2);
        p.code_half          = std::uint64_t(2) << (code - 2);
        p.code_three_fourths = std::uint64_t(3) << (code - 2);
        p.code_max           = (std::uint64_t(1) << code) - 1;
        return p;
    }
    redux_params c_abi() const { return redux_params{(uint32_t)symbol_bits, (uint32_t)freq_bits, (uint32_t)code_bits}; }
};

// src/model/mod.rs:17-29.  On this path a Model names WHICH model the device runs; the tree
// itself lives in LDS, one per block, so the trait's per-symbol methods have no host form.
class Model {
public:
    virtual ~Model() {}
    virtual const Parameters &parameters() const = 0;
    virtual bool              device_resident() const { return false; }
};

// src/model/adaptive_tree.rs:36
class AdaptiveTreeModel : public Model {
public:
    static std::unique_ptr<Model> make(const Parameters &p) { return std::unique_ptr<Model>(new AdaptiveTreeModel(p)); }
    const Parameters &parameters() const override { return params_; }
    bool              device_resident() const override { return true; }

private:
    explicit AdaptiveTreeModel(const Parameters &p) : params_(p) {}
    Parameters params_;
};

} // namespace model

namespace hip {

struct Blocks {
    std::vector<std::uint8_t>  data;    // dense concatenation of per-block streams (or decoded blocks)
    std::vector<std::uint64_t> offsets; // nblocks + 1
};

// one redux::compress per block_size bytes, all on the GPU
inline Blocks compress_blocks(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                              const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks(&cp, in, len, block_size, b.data.data(), b.data.size(), b.offsets.data(), nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: block b of the result is data[b*block_size .. b*block_size + sizes[b])
inline std::vector<std::uint8_t> decompress_blocks(const Blocks &streams, std::uint32_t block_size,
                                                   const model::Parameters &p, std::vector<std::uint32_t> *sizes = nullptr)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (streams.offsets.empty() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT); // (the C call reads data[offsets[b] .. offsets[b + 1]) from caller memory)
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    const std::uint64_t        nb = streams.offsets.size() - 1;
    std::vector<std::uint8_t>  out(nb * (std::uint64_t)block_size);
    std::vector<std::uint32_t> sz(nb);
    check(redux_decode_blocks(&cp, streams.data.data(), streams.offsets.data(), nb, block_size, out.data(), out.size(),
                              sz.data(), nullptr));
    if (sizes)
        *sizes = sz;
    return out;
}

// Typed data in the byte-plane layout (include/redux_hip.h): element_size 2, 4 or 8 (1 = no layout, compress_blocks'
// streams); frames of element_size * block_size bytes are transformed so that each block holds one byte plane.
inline Blocks compress_blocks_planes(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                     const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_planes(&cp, in, len, block_size, element_size, b.data.data(), b.data.size(), b.offsets.data(), nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_planes(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                          std::uint32_t element_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT); // (the C call reads data[offsets[b] .. offsets[b + 1]) from caller memory)
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_planes(&cp, streams.data.data(), streams.offsets.data(), len, block_size, element_size, out.data(),
                                     sizes.data(), nullptr));
    out.resize(len);
    return out;
}

// Integer series behind the delta filter (include/redux_hip.h, "delta filter"): element_size 1, 2, 4 or 8; the differences
// of neighbouring little-endian unsigned elements are coded, frame by frame of the byte-plane layout.  Opt-in: floating-point
// data and text get larger with it.
inline Blocks compress_blocks_delta(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                    const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_delta(&cp, in, len, block_size, element_size, b.data.data(), b.data.size(), b.offsets.data(), nullptr,
                                    nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_delta(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                         std::uint32_t element_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_delta(&cp, streams.data.data(), streams.offsets.data(), len, block_size, element_size, out.data(),
                                    sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Signed series behind the zigzag-folded delta filter (include/redux_hip.h, "zigzag-folded delta filter"): compress_blocks_delta
// with every difference folded, so that small differences of either sign leave the upper byte planes zero.
inline Blocks compress_blocks_zigzag(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                     const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_zigzag(&cp, in, len, block_size, element_size, b.data.data(), b.data.size(), b.offsets.data(), nullptr,
                                     nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_zigzag(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                          std::uint32_t element_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_zigzag(&cp, streams.data.data(), streams.offsets.data(), len, block_size, element_size, out.data(),
                                     sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Interleaved channels and fixed-width records behind the lagged delta filter (include/redux_hip.h, "lagged delta filter"):
// compress_blocks_zigzag with the predecessor `lag` elements back, 1 <= lag <= REDUX_LAG_MAX.  Opt-in: a wrong lag costs
// bytes, and the decoder needs the same one.
inline Blocks compress_blocks_lag(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                  std::uint32_t lag, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_lag_check(element_size, lag) != REDUX_OK)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_lag(&cp, in, len, block_size, element_size, lag, b.data.data(), b.data.size(), b.offsets.data(),
                                  nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_lag(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                       std::uint32_t element_size, std::uint32_t lag, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_lag_check(element_size, lag) != REDUX_OK ||
        redux_block_count(len, block_size) + 1 != streams.offsets.size() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_lag(&cp, streams.data.data(), streams.offsets.data(), len, block_size, element_size, lag, out.data(),
                                  sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Tables of fixed-width structs behind the record layout (include/redux_hip.h, "record layout"): every block holds one byte
// column of block_size records of record_size bytes, 2 <= record_size <= REDUX_RECORD_MAX; `delta`: the byte delta against the
// record before, in front of the layout.  Opt-in, and the decoder needs the same record size and flag.
inline Blocks compress_blocks_record(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t record_size,
                                     bool delta, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_record_check(record_size, delta) != REDUX_OK)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_record(&cp, in, len, block_size, record_size, delta, b.data.data(), b.data.size(), b.offsets.data(),
                                     nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_record(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                          std::uint32_t record_size, bool delta, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_record_check(record_size, delta) != REDUX_OK ||
        redux_block_count(len, block_size) + 1 != streams.offsets.size() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_record(&cp, streams.data.data(), streams.offsets.data(), len, block_size, record_size, delta, out.data(),
                                     sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Sampled signals behind higher-order lagged differences (include/redux_hip.h, "higher-order lagged differences"):
// compress_blocks_lag with the lag-S difference applied `order` times, 1 <= order <= REDUX_LAG_ORDER_MAX; order 1 gives
// compress_blocks_lag's streams.  Opt-in: on random walks a higher order costs bytes, and the decoder needs the same lag and
// order.
inline Blocks compress_blocks_lag_order(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                        std::uint32_t lag, std::uint32_t order, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_lag_order_check(element_size, lag, order) != REDUX_OK)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_lag_order(&cp, in, len, block_size, element_size, lag, order, b.data.data(), b.data.size(),
                                        b.offsets.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_lag_order(const Blocks &streams, std::uint64_t len, std::uint32_t block_size,
                                                             std::uint32_t element_size, std::uint32_t lag, std::uint32_t order,
                                                             const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_lag_order_check(element_size, lag, order) != REDUX_OK ||
        redux_block_count(len, block_size) + 1 != streams.offsets.size() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_lag_order(&cp, streams.data.data(), streams.offsets.data(), len, block_size, element_size, lag, order,
                                        out.data(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Files of several element types behind the mixed layouts (include/redux_hip.h, "mixed layouts"): every unit of 8 blocks is
// coded behind the layout -- element size 1, 2, 4 or 8, with or without the delta filter -- that costs it least, chosen on the
// device among the layouts of layouts_mask (bit k = layout 4 F + log2 E; 0xFF: all eight).  The unit table comes back next
// to the streams, and the decoder needs it.
struct MixedBlocks {
    Blocks                    blocks;
    std::vector<std::uint8_t> unit_layouts; // u8[redux_mixed_unit_count(len, block_size)], 0 .. 7
};

inline MixedBlocks compress_blocks_mixed(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                                         const model::Parameters &p, std::uint32_t layouts_mask = 0xFF)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || layouts_mask == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    MixedBlocks m;
    Blocks &b = m.blocks;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    m.unit_layouts.resize(redux_mixed_unit_count(len, block_size));
    check(redux_encode_blocks_mixed(&cp, in, len, block_size, layouts_mask, m.unit_layouts.data(), b.data.data(), b.data.size(),
                                    b.offsets.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return m;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_mixed(const MixedBlocks &m, std::uint64_t len, std::uint32_t block_size,
                                                         const model::Parameters &p)
{
    const Blocks &streams = m.blocks;
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size() || m.unit_layouts.size() != redux_mixed_unit_count(len, block_size))
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_mixed(&cp, streams.data.data(), streams.offsets.data(), m.unit_layouts.data(), len, block_size,
                                    out.data(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// A snapshot behind the XOR-against-base filter (include/redux_hip.h, "XOR-against-base filter"): base is an earlier
// snapshot of the same data, of any length; the bytewise XOR against it is coded in the byte-plane layout of element_size
// 1, 2, 4 or 8.  Opt-in, and the decoder needs the same base.
inline Blocks compress_blocks_base(const std::uint8_t *in, std::uint64_t len, const std::uint8_t *base, std::uint64_t base_len,
                                   std::uint32_t block_size, std::uint32_t element_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_base(&cp, in, len, base, base_len, block_size, element_size, b.data.data(), b.data.size(),
                                   b.offsets.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse, with the same base: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_base(const Blocks &streams, const std::uint8_t *base, std::uint64_t base_len,
                                                        std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                                        const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_base(&cp, streams.data.data(), streams.offsets.data(), base, base_len, len, block_size, element_size,
                                   out.data(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// A snapshot behind the folded difference against a base (include/redux_hip.h, "folded difference against a base"): the
// base filter's other operation, the zigzag-folded difference of the little-endian elements in place of the XOR; the
// arguments and the refusals of compress_blocks_base.  Opt-in, and the decoder needs the same base.
inline Blocks compress_blocks_base_sub(const std::uint8_t *in, std::uint64_t len, const std::uint8_t *base, std::uint64_t base_len,
                                       std::uint32_t block_size, std::uint32_t element_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_encode_blocks_base_sub(&cp, in, len, base, base_len, block_size, element_size, b.data.data(), b.data.size(),
                                       b.offsets.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse, with the same base: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_base_sub(const Blocks &streams, const std::uint8_t *base, std::uint64_t base_len,
                                                            std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                                            const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_base_sub(&cp, streams.data.data(), streams.offsets.data(), base, base_len, len, block_size,
                                       element_size, out.data(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Constant blocks skipped (include/redux_hip.h, "constant blocks"): a block of the coder's input -- the bytes, their
// byte-plane layout, or the layout of input ^ base when base_len is not 0 -- whose bytes are all equal travels as that one
// byte; `constant` receives one 0 / 1 flag per block, which the decoder needs together with the same base.  Opt-in.
inline Blocks compress_blocks_const(const std::uint8_t *in, std::uint64_t len, const std::uint8_t *base, std::uint64_t base_len,
                                    std::uint32_t block_size, std::uint32_t element_size, const model::Parameters &p,
                                    std::vector<std::uint8_t> &constant)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    constant.assign(nb, 0);
    check(redux_encode_blocks_const(&cp, in, len, base, base_len, block_size, element_size, b.data.data(), b.data.size(),
                                    b.offsets.data(), constant.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse, with the flags and the same base: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_const(const Blocks &streams, const std::vector<std::uint8_t> &constant,
                                                         const std::uint8_t *base, std::uint64_t base_len, std::uint64_t len,
                                                         std::uint32_t block_size, std::uint32_t element_size,
                                                         const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        constant.size() + 1 != streams.offsets.size() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t> out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_const(&cp, streams.data.data(), streams.offsets.data(), constant.data(), base, base_len, len, block_size,
                                    element_size, out.data(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Stored blocks (include/redux_hip.h): a block whose stream would not be smaller than store_ratio / 65536 of its bytes
// travels raw; `stored` receives one 0 / 1 flag per block, which the decoder needs.
inline Blocks compress_blocks_stored(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                     std::vector<std::uint8_t> &stored, const model::Parameters &p, std::uint32_t store_ratio = 65536)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    stored.assign(nb, 0);
    check(redux_encode_blocks_stored(&cp, in, len, block_size, element_size, store_ratio, b.data.data(), b.data.size(),
                                     b.offsets.data(), stored.data(), nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_stored(const Blocks &streams, const std::vector<std::uint8_t> &stored,
                                                          std::uint64_t len, std::uint32_t block_size, std::uint32_t element_size,
                                                          const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || redux_block_count(len, block_size) + 1 != streams.offsets.size() ||
        stored.size() + 1 != streams.offsets.size() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT); // (the C call reads data[offsets[b] .. offsets[b + 1]) from caller memory)
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t>  out(len ? len : 1);
    std::vector<std::uint32_t> sizes(streams.offsets.size() - 1);
    check(redux_decode_blocks_stored(&cp, streams.data.data(), streams.offsets.data(), stored.data(), len, block_size, element_size,
                                     out.data(), out.size(), sizes.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Semi-static coding (include/redux_hip.h): the static table of `in` by the documented rule, total 0 = the default
// min(2^16, freq_max); the table is cum[0..=257].
inline std::vector<std::uint32_t> static_table(const std::uint8_t *in, std::uint64_t len, const model::Parameters &p,
                                               std::uint32_t total = 0)
{
    const redux_params cp = p.c_abi();
    if (total == 0) {
        const std::uint64_t fmax = (1ull << p.freq_bits) - 1;
        total = (std::uint32_t)(fmax < 65536 ? fmax : 65536);
    }
    std::vector<std::uint32_t> cum(258);
    check(redux_static_table(&cp, in, len, total, cum.data()));
    return cum;
}

// every block coded under the fixed table cum
inline Blocks compress_blocks_static(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                                     const model::Parameters &p, const std::vector<std::uint32_t> &cum)
{
    const redux_params cp = p.c_abi();
    if (cum.size() != 258)
        throw Error::from_status(REDUX_INVALID_INPUT);
    check(redux_static_table_check(&cp, cum.data()));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_static_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_static_encode_blocks(&cp, cum.data(), in, len, block_size, b.data.data(), b.data.size(), b.offsets.data(), nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: block b of the result is data[b*block_size .. b*block_size + sizes[b])
inline std::vector<std::uint8_t> decompress_blocks_static(const Blocks &streams, std::uint32_t block_size, const model::Parameters &p,
                                                          const std::vector<std::uint32_t> &cum,
                                                          std::vector<std::uint32_t> *sizes = nullptr)
{
    const redux_params cp = p.c_abi();
    if (cum.size() != 258)
        throw Error::from_status(REDUX_INVALID_INPUT);
    check(redux_static_table_check(&cp, cum.data()));
    if (streams.offsets.empty() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    const std::uint64_t        nb = streams.offsets.size() - 1;
    std::vector<std::uint8_t>  out(nb * (std::uint64_t)block_size);
    std::vector<std::uint32_t> sz(nb);
    check(redux_static_decode_blocks(&cp, cum.data(), streams.data.data(), streams.offsets.data(), nb, block_size, out.data(),
                                     out.size(), sz.data(), nullptr));
    if (sizes)
        *sizes = sz;
    return out;
}

// Context-static coding (include/redux_hip.h): a static table per preceding byte.  tables: u32[256][258], all of one total
// <= 2^16 (default: min(2^16, freq_max)), built from the data by context_static_tables.
inline std::vector<std::uint32_t> context_static_tables(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                                                        const model::Parameters &p, std::uint32_t total = 0)
{
    const redux_params cp = p.c_abi();
    if (total == 0)
        total = p.freq_max < 65536 ? (std::uint32_t)p.freq_max : 65536u;
    std::vector<std::uint32_t> cum(256 * 258);
    check(redux_context_static_tables(&cp, in, len, block_size, total, cum.data()));
    return cum;
}

inline Blocks compress_blocks_context_static(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                                             const model::Parameters &p, const std::vector<std::uint32_t> &tables)
{
    const redux_params cp = p.c_abi();
    if (tables.size() != 256 * 258)
        throw Error::from_status(REDUX_INVALID_INPUT);
    check(redux_context_static_table_check(&cp, tables.data()));
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    Blocks b;
    const std::uint64_t nb = redux_block_count(len, block_size);
    b.data.resize(redux_context_static_encode_bound(&cp, len, block_size));
    b.offsets.resize(nb + 1);
    check(redux_context_static_encode_blocks_crc(&cp, tables.data(), in, len, block_size, b.data.data(), b.data.size(), b.offsets.data(),
                                                 nullptr, nullptr));
    b.data.resize(b.offsets[nb]);
    return b;
}

// inverse: block b of the result is data[b*block_size .. b*block_size + sizes[b])
inline std::vector<std::uint8_t> decompress_blocks_context_static(const Blocks &streams, std::uint32_t block_size,
                                                                  const model::Parameters &p, const std::vector<std::uint32_t> &tables,
                                                                  std::vector<std::uint32_t> *sizes = nullptr)
{
    const redux_params cp = p.c_abi();
    if (tables.size() != 256 * 258)
        throw Error::from_status(REDUX_INVALID_INPUT);
    check(redux_context_static_table_check(&cp, tables.data()));
    if (streams.offsets.empty() || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    const std::uint64_t        nb = streams.offsets.size() - 1;
    std::vector<std::uint8_t>  out(nb * (std::uint64_t)block_size);
    std::vector<std::uint32_t> sz(nb);
    check(redux_context_static_decode_blocks_crc(&cp, tables.data(), streams.data.data(), streams.offsets.data(), nb, block_size,
                                                 out.data(), out.size(), sz.data(), nullptr, nullptr));
    if (sizes)
        *sizes = sz;
    return out;
}

// Segment-static coding (include/redux_hip.h): static tables per range of segment_blocks = 64 * element_size * k blocks of
// the byte-plane layout, built from each range as it is coded (one pass).  tables: u32[nseg * element_size][258].
struct SegmentBlocks {
    Blocks                     blocks;
    std::vector<std::uint32_t> tables;
};
inline SegmentBlocks compress_blocks_segment_static(const std::uint8_t *in, std::uint64_t len, std::uint32_t block_size,
                                                    std::uint32_t element_size, std::uint32_t segment_blocks,
                                                    const model::Parameters &p, std::uint32_t total = 0)
{
    const redux_params cp = p.c_abi();
    if (total == 0) {
        const std::uint64_t fmax = (1ull << p.freq_bits) - 1;
        total = (std::uint32_t)(fmax < 65536 ? fmax : 65536);
    }
    if (block_size == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    const std::uint64_t nb = redux_block_count(len, block_size);
    const std::uint64_t nt = redux_segment_static_table_count(nb, element_size, segment_blocks);
    if (nt == 0)
        throw Error::from_status(REDUX_INVALID_INPUT);
    SegmentBlocks r;
    r.tables.resize(nt * 258);
    r.blocks.data.resize(redux_segment_static_encode_bound(&cp, len, block_size));
    r.blocks.offsets.resize(nb + 1);
    check(redux_segment_static_encode_blocks_crc(&cp, total, in, len, block_size, element_size, segment_blocks, r.tables.data(),
                                                 r.blocks.data.data(), r.blocks.data.size(), r.blocks.offsets.data(), nullptr, nullptr));
    r.blocks.data.resize(r.blocks.offsets[nb]);
    return r;
}

// inverse: the original len bytes
inline std::vector<std::uint8_t> decompress_blocks_segment_static(const SegmentBlocks &s, std::uint64_t len, std::uint32_t block_size,
                                                                  std::uint32_t element_size, std::uint32_t segment_blocks,
                                                                  const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    const Blocks      &b  = s.blocks;
    if (block_size == 0 || b.offsets.size() != redux_block_count(len, block_size) + 1 || b.offsets.back() > b.data.size() ||
        s.tables.size() % 258)
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < b.offsets.size(); i++)
        if (b.offsets[i] < b.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint8_t>  out(len ? len : 1);
    std::vector<std::uint32_t> sz(b.offsets.size() - 1);
    check(redux_segment_static_decode_blocks_crc(&cp, s.tables.data(), s.tables.size() / 258, b.data.data(), b.offsets.data(), len,
                                                 block_size, element_size, segment_blocks, out.data(), sz.data(), nullptr, nullptr));
    out.resize(len);
    return out;
}

// Many independent inputs in ONE launch (the reference's corpus harness codes file by file, tests/corpora.rs:32-85):
// every input is cut into blocks on its own; first[i] is the number of input i's first block (inputs.size() + 1 entries).
struct BlocksV {
    Blocks                     blocks;
    std::vector<std::uint64_t> first;
};
inline BlocksV compress_blocks_v(const std::vector<std::vector<std::uint8_t>> &inputs, std::uint32_t block_size,
                                 const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || inputs.empty())
        throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint64_t> off(inputs.size()), len(inputs.size());
    std::vector<std::uint8_t>  flat;
    BlocksV                    r;
    r.first.assign(inputs.size() + 1, 0);
    for (std::size_t i = 0; i < inputs.size(); i++) {
        off[i] = flat.size();
        len[i] = inputs[i].size();
        flat.insert(flat.end(), inputs[i].begin(), inputs[i].end());
        r.first[i + 1] = r.first[i] + redux_block_count(len[i], block_size);
    }
    const std::uint64_t nb = redux_block_count_v(len.data(), len.size(), block_size);
    r.blocks.data.resize(nb * redux_encode_slot_bytes(&cp, block_size));
    r.blocks.offsets.resize(nb + 1);
    check(redux_encode_blocks_v(&cp, flat.data(), off.data(), len.data(), len.size(), block_size, r.blocks.data.data(),
                                r.blocks.data.size(), r.blocks.offsets.data(), nullptr));
    r.blocks.data.resize(r.blocks.offsets[nb]);
    return r;
}
inline std::vector<std::vector<std::uint8_t>> decompress_blocks_v(const Blocks &streams, const std::vector<std::uint64_t> &lengths,
                                                                  std::uint32_t block_size, const model::Parameters &p)
{
    const redux_params cp = p.c_abi();
    check(redux_device_supports(&cp));
    if (block_size == 0 || lengths.empty() || streams.offsets.empty() ||
        redux_block_count_v(lengths.data(), lengths.size(), block_size) + 1 != streams.offsets.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    // the C call copies data[offsets.front() .. offsets.back()) from caller memory: inside `data`, in order
    if (streams.offsets.front() != 0 || streams.offsets.back() > streams.data.size())
        throw Error::from_status(REDUX_INVALID_INPUT);
    for (std::size_t i = 1; i < streams.offsets.size(); i++)
        if (streams.offsets[i] < streams.offsets[i - 1])
            throw Error::from_status(REDUX_INVALID_INPUT);
    std::vector<std::uint64_t> off(lengths.size(), 0);
    for (std::size_t i = 1; i < lengths.size(); i++)
        off[i] = off[i - 1] + lengths[i - 1];
    std::vector<std::uint8_t>  out(off.back() + lengths.back() + 1);
    std::vector<std::uint32_t> sz(streams.offsets.size() - 1);
    check(redux_decode_blocks_v(&cp, streams.data.data(), streams.offsets.data(), out.data(), off.data(), lengths.data(),
                                lengths.size(), block_size, sz.data(), nullptr));
    std::vector<std::vector<std::uint8_t>> r(lengths.size());
    for (std::size_t i = 0; i < lengths.size(); i++)
        r[i].assign(out.begin() + off[i], out.begin() + off[i] + lengths[i]);
    return r;
}

} // namespace hip

// src/lib.rs:102-109: returns (bytes in the decompressed stream, bytes in the compressed stream)
inline std::pair<std::uint64_t, std::uint64_t> compress(std::istream &istream, std::ostream &ostream,
                                                        std::unique_ptr<model::Model> model)
{
    if (!model || !model->device_resident())
        throw Error::from_status(REDUX_UNSUPPORTED);
    const redux_params        cp = model->parameters().c_abi();
    std::vector<std::uint8_t> in((std::istreambuf_iterator<char>(istream)), std::istreambuf_iterator<char>());
    std::vector<std::uint8_t> out(redux_encode_bound(&cp, in.size(), in.empty() ? 1u : (std::uint32_t)in.size()));
    std::uint64_t             bi = 0, bo = 0;
    check(redux_compress(&cp, in.data(), in.size(), out.data(), out.size(), &bi, &bo));
    ostream.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)bo);
    if (!ostream)
        throw Error(Error::IoError, REDUX_IO_ERROR, "I/O error: write failed");
    return {bi, bo};
}

// src/lib.rs:113-120
inline std::pair<std::uint64_t, std::uint64_t> decompress(std::istream &istream, std::ostream &ostream,
                                                          std::unique_ptr<model::Model> model,
                                                          std::uint64_t max_output = 0)
{
    if (!model || !model->device_resident())
        throw Error::from_status(REDUX_UNSUPPORTED);
    const redux_params        cp = model->parameters().c_abi();
    std::vector<std::uint8_t> in((std::istreambuf_iterator<char>(istream)), std::istreambuf_iterator<char>());
    if (max_output == 0)
        max_output = in.size() * 64 + (1u << 20);
    std::vector<std::uint8_t> out(max_output);
    std::uint64_t             bi = 0, bo = 0;
    check(redux_decompress(&cp, in.data(), in.size(), out.data(), out.size(), &bi, &bo));
    ostream.write(reinterpret_cast<const char *>(out.data()), (std::streamsize)bo);
    if (!ostream)
        throw Error(Error::IoError, REDUX_IO_ERROR, "I/O error: write failed");
    return {bi, bo};
}

} // namespace redux
