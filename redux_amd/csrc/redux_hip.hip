// redux_hip.hip -- the C ABI of include/redux_hip.h over the gfx950 kernels.
//
// One translation unit; the kernels (all hand-written for CDNA4, wave64) live in
//   redux_coder.hpp    device building blocks: LDS tree, interval narrowing, bit output
//   redux_encode.hpp   k_fill_rc, k_encode, k_encode_pair (default encoder)
//   redux_decode.hpp   k_decode, k_decode_lock (default decoder); redux_decode_wave.hpp: k_decode_wave (small launches, whole streams)
//   redux_pack.hpp     k_scan_sizes, k_compact: slots -> dense stream + offsets
//   redux_coop.hpp     k_coop_model, k_coop_chain: small grids, a block's model computed by 64 lanes
//   redux_any.hpp      general Parameters (symbol_bits <= 16, code_bits <= 63), one lane per block
//   redux_gen.hpp      k_encode_gen / k_encode_gen_pair: symbol widths 1 .. 12 other than 8 (code_bits <= 32) in lock-step form
//   redux_decode_cells.hpp  k_decode_cells: their decoder, the tree as cells of four levels
//   redux_synth.hpp    k_gen_iid / k_gen_zipf
//   redux_static.hpp   k_encode_static / k_decode_static: the coder core under a fixed frequency table
//   redux_planes.hpp   k_planes: the byte-plane layout of typed data, a byte transform in front of the coder
//   redux_delta.hpp    k_delta_planes / k_delta_unplanes: the delta filter for integer series, fused with the layout
//   redux_zigzag.hpp   the zigzag fold: k_delta_*<E, true> is the delta filter with folded differences, for signed series
//   redux_lag.hpp      k_lag_planes / k_lag_unplanes: the lagged delta filter for interleaved channels, the predecessor S elements back;
//                      k_lag_order_planes / k_lag_order_unplanes: its higher orders, the filter applied K times, from the same bodies
//   redux_record.hpp   k_record_planes / k_record_unplanes: the record layout for fixed-width structs, R bytes a record, with a byte delta
//   redux_base.hpp     k_base_planes / k_base_unplanes: the XOR-against-base filter for snapshot series, fused with the layout
//   redux_base_sub.hpp BaseSubFold: the base filter's folded difference, the same kernels under another operation
//   redux_stride.hpp k_stride_planes / k_stride_sum: the snapshot-stride filter, the folded difference S elements back
//   redux_hist.hpp     k_byte_hist / k_static_table: semi-static coding, the static table built from the data
//   redux_plane_static.hpp  k_plane_hist, the tables and their check: the static coder with one table per byte plane
//   redux_segment_static.hpp  k_segment_hist / k_static_tables / k_*_segment_static*: E tables per range of blocks, or for all
//   redux_context_static.hpp  k_context_hist / k_*_context_static: the static coder with a table per preceding byte
//   redux_store.hpp    k_store_select / k_store_table / k_store_unpack: stored blocks, the raw bytes of blocks that do not shrink
//   redux_const.hpp    k_const_select / k_const_table / k_const_fill: constant blocks, one byte for a block of equal bytes
//   redux_cost.hpp     k_block_cost / k_table_cost: size estimates, a block's cost under a model from its counts
//   redux_layout_cost.hpp  k_layout_cost: the adaptive cost of every block of the eight layouts, from the untransformed bytes
//   redux_lag_cost.hpp  k_lag_cost: the adaptive cost of every block behind the lagged delta filter, for a list of lags;
//                      k_lag_order_cost: the same behind its higher orders, for (lag, order) candidates, from the same bodies
//   redux_record_cost.hpp  k_record_cost: the adaptive cost of every block behind the record layout, for (record size, delta) candidates
//   redux_mixed.hpp    k_mixed_choose / k_mixed_planes: a layout per unit of 8 blocks, chosen from those costs on the device
//   redux_range.hpp    k_segment_copy: range reads, the plan of the covered granules and the segmented byte copy
// This file holds the general-parameter kernels' launch shims, the workspace geometry and the
// extern "C" entry points.
//
// Build: hipcc --offload-arch=gfx950 -O3 -shared -fPIC redux_hip.hip -o libredux_hip.so
#include "redux_coder.hpp"
#include "redux_any.hpp"
#include "redux_gen.hpp"
#include "redux_encode.hpp"
#include "redux_decode.hpp"
#include "redux_decode_adaptive.hpp"
#include "redux_decode_wave.hpp"
#include "redux_decode_cells.hpp"
#include "redux_pack.hpp"
#include "redux_table.hpp"
#include "redux_coop.hpp"
#include "redux_synth.hpp"
#include "redux_static.hpp"
#include "redux_planes.hpp"
#include "redux_delta.hpp"
#include "redux_zigzag.hpp"
#include "redux_lag.hpp"
#include "redux_record.hpp"
#include "redux_base.hpp"
#include "redux_base_sub.hpp"
#include "redux_stride.hpp"
#include "redux_hist.hpp"
#include "redux_plane_static.hpp"
#include "redux_segment_static.hpp"
#include "redux_context_static.hpp"
#include "redux_crc.hpp"
#include "redux_store.hpp"
#include "redux_const.hpp"
#include "redux_cost.hpp"
#include "redux_layout_cost.hpp"
#include "redux_lag_cost.hpp"
#include "redux_lag_order_cost_list.hpp"
#include "redux_record_cost.hpp"
#include "redux_mixed.hpp"
#include "redux_range.hpp"

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <initializer_list>
#include <memory>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>
#include <vector>

namespace redux {


// ======================================================================================
// general parameters (redux_any.hpp): one lane per block, tree in the workspace
// ======================================================================================
struct AnyEncArgs : EncCore {
    uint32_t      *trees;
    uint64_t       tree_words; // u32 entries per block
    uint32_t       block_size, slot_cap;
    uint32_t       sb, fb, cb;
};
static_assert(sizeof(AnyEncArgs) == 96, "kernarg layout");

__global__ void __launch_bounds__(64) k_encode_any(AnyEncArgs a)
{
    const uint64_t blk = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (blk >= a.nblocks)
        return;
    const uint64_t o0  = blk * a.block_size;
    const uint64_t rem = a.in_len > o0 ? a.in_len - o0 : 0;
    const uint64_t len = rem < a.block_size ? rem : a.block_size;
    const any::Params P = any::make_params(a.sb, a.fb, a.cb);
    uint64_t  bi, bo;
    const int st = any::compress_stream(P, a.trees + blk * a.tree_words, a.in + o0, len, a.slots + blk * a.slot_bytes,
                                        a.slot_cap, bi, bo);
    a.sizes[blk]  = (uint32_t)bo;
    a.status[blk] = st;
}

struct AnyDecArgs : DecCore {
    uint64_t       *in_used;
    uint32_t       *trees;
    uint64_t        tree_words;
    uint32_t        block_size;
    uint32_t        sb, fb, cb;
};
static_assert(sizeof(AnyDecArgs) == 88, "kernarg layout");

__global__ void __launch_bounds__(64) k_decode_any(AnyDecArgs a)
{
    const uint64_t blk = (uint64_t)blockIdx.x * 64 + threadIdx.x;
    if (blk >= a.nblocks)
        return;
    const uint64_t o0 = a.in_offsets[blk], o1 = a.in_offsets[blk + 1];
    const any::Params P = any::make_params(a.sb, a.fb, a.cb);
    uint64_t  bi, bo;
    const int st = any::decompress_stream(P, a.trees + blk * a.tree_words, a.in + o0, o1 - o0,
                                          a.out + blk * (uint64_t)a.block_size, a.block_size, bi, bo);
    a.out_sizes[blk] = (uint32_t)bo;
    a.status[blk]    = st;
    if (a.in_used)
        a.in_used[blk] = bi;
}

// ======================================================================================
// host side of the ABI
// ======================================================================================
static inline uint64_t align_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

struct Geometry {
    uint64_t nblocks;
    uint64_t slot_bytes; // stride between slots (16-byte multiple, >= cap + 32)
    uint32_t slot_cap;   // usable bytes
    uint32_t rc_n;       // reciprocal table entries
    uint32_t nfreeze;
    bool     u16, fixup;
    bool     any;        // general-parameter path (redux_any.hpp): symbol_bits != 8 or code_bits > 32
    bool     gen;        // ... except 4- and 12-bit symbols with code_bits <= 32: lock-step kernels of redux_gen.hpp
    uint64_t tree_bytes; // any / gen (12-bit symbols): per-block tree in the workspace
    bool     coop;       // small grid: k_coop_model + k_coop_chain (redux_coop.hpp), (low, high) pairs in the workspace
    bool     coop_linear; // ... with fewer than 64 large blocks: linear slots, nblocks + 1 of them (k_coop_chain<.., LINEAR>)
    uint32_t pair_width; // ... in rows of this many lanes
    uint32_t coop_win;   // ... one WINDOW of this many symbols of every block at a time (block_size + 1: whole blocks), coop_nwin of them
    uint32_t coop_nwin;
    // workspace layout (encode)
    uint64_t off_rc, off_sizes, off_mode, off_slots, off_trees, off_table, off_seen, off_cstate, off_pairs, total;
};

static int check_params(const redux_params *p)
{
    if (!p)
        return REDUX_INVALID_INPUT;
    const int st = redux_params_check(p->symbol_bits, p->freq_bits, p->code_bits);
    if (st != REDUX_OK)
        return st;
    if (p->symbol_bits > 16) // a tree of 2^symbol_bits + 2 entries per block
        return REDUX_UNSUPPORTED;
    return REDUX_OK;
}

static bool is_any(const redux_params *p) { return p->symbol_bits != 8 || p->code_bits > 32; }
// Symbol widths 1 .. 12 other than 8 with code_bits <= 32 -- the widths src/model/tests.rs exercises besides 8 (4 and 12)
// and everything between -- have lock-step kernels: the encoders of redux_gen.hpp, the cell decoder of
// redux_decode_cells.hpp.  Their limits, in symbols of a block (a bigger block -- whole-stream mode above all -- is one
// lane's serial chain anyway and runs on the one-lane kernels, which have none):
//   * 4 MiB: the kernels index a reciprocal table by the symbol number and address 64 slots / 64 blocks with 32-bit lane offsets;
//   * symbol_bits >= 9: u16 tree nodes holding lowbit + increments: at most 65535 - 2^(symbol_bits - 1) updates of the model
//     (symbols of a block, or fewer if the model freezes first: 12-bit symbols, 20 frequency bits: blocks of 95,230 bytes);
//   * symbol_bits <= 7: u32 nodes: any block up to the 4 MiB above; a block whose count can pass 2^17 takes the kernels'
//     fix-up instances (quotient fix-ups in scale_div, a 62-bit numerator for the decoder's code value).
static uint64_t gen_updates(const redux_params *p, uint32_t block_size) // increments a tree node of a block can receive
{
    const uint64_t nsym    = (uint64_t)block_size * 8 / p->symbol_bits;
    const uint64_t nfreeze = ((1ull << p->freq_bits) - 1) - ((1ull << p->symbol_bits) + 1);
    return nsym < nfreeze ? nsym : nfreeze;
}
// the cell decoder takes the block: see above
static bool gen_decode_cells(const redux_params *p, uint32_t block_size)
{
    if (p->symbol_bits >= 8)
        return gen_updates(p, block_size) + (1ull << (p->symbol_bits - 1)) <= 65535;
    return true;
}
// ... with the fix-up instance: the count passes 2^17 inside a block.  (By a few symbols only -- a 64 KiB block of 4-bit symbols
// ends at 2^17 + 17 -- is not worth the instance's ~10 %: the plain one stops its lock-step loop there and its per-lane loop,
// which divides exactly, codes the rest.)
static bool gen_needs_fixup(const redux_params *p, uint32_t block_size)
{
    return p->symbol_bits < 8 && (1ull << p->symbol_bits) + 1 + gen_updates(p, block_size) > (1ull << 17) + 64;
}
static bool is_gen(const redux_params *p, uint32_t block_size)
{
    if (p->code_bits > 32 || p->symbol_bits == 8 || p->symbol_bits > 12 || block_size > (1u << 22))
        return false;
    return gen_decode_cells(p, block_size);
}
// 11- and 12-bit symbols: the bottom cells (2^(symbol_bits - 4) of 32 bytes per block: 4 / 8 KiB) live in the workspace, the
// cells above them in LDS: 64 blocks per wave, four waves per CU (redux_decode_cells.hpp).  Measured against keeping everything
// in LDS (which holds 16 blocks of 12-bit symbols per CU, 32 of 11-bit): never slower from 2,048 blocks up, 2 x faster where
// the LDS form needs a second pass.  9- and 10-bit symbols fit LDS with 64 blocks per wave and are faster there
// (profiles/r04_gen_parameters.txt).
static bool gen_decode_in_workspace(const redux_params *p, uint64_t nblocks)
{
    (void)nblocks;
    return p->symbol_bits >= 11;
}
static uint64_t gen_decode_tree_bytes(const redux_params *p) { return (1ull << (p->symbol_bits - 4)) * 32; }
// 8-bit symbols in blocks above 64 KiB (which k_decode_lock's u16 nodes do not hold), in launches too big for one block per
// wave (k_decode_wave): the cell decoder with u32 nodes -- 68 KiB of cells per wave, two waves per CU -- instead of k_decode's
// per-lane control flow.  No block tables (the cell decoder takes blocks in order), blocks of at most 4 MiB (its reciprocal
// table is indexed by the symbol number).
static bool cells8_takes(const redux_params *p, uint32_t block_size, uint64_t nslots, bool table)
{
    // (nslots == 0: "a full grid", redux_decode_kernel_name)
    return p->symbol_bits == 8 && p->code_bits <= 32 && block_size > 65536 && block_size <= (1u << 22) &&
           (nslots == 0 || nslots > kWaveDecMaxBlocks || (nslots > kWaveDecManyBlocks && block_size >= kWaveDecLargeBlock)) && !table;
}
static uint32_t cells8_rc_entries(const redux_params *p, uint32_t block_size)
{
    const uint64_t nfreeze = ((1ull << p->freq_bits) - 1) - 257;
    return (uint32_t)((block_size < nfreeze ? block_size : nfreeze) + 1 + 32);
}
static bool cells8_needs_fixup(const redux_params *p, uint32_t block_size)
{
    return 257ull + cells8_rc_entries(p, block_size) - 33 > (1ull << 17) + 64;
}

static uint64_t slot_cap_for(const redux_params *p, uint32_t block_size)
{
    const uint64_t freq_max = (1ull << p->freq_bits) - 1;
    if (is_any(p)) {
        // General parameters: a symbol of frequency >= 1 out of count <= min(freq_max, K + n)
        // costs at most ceil(log2 count) bits, + 1 for the truncation of codec.rs:59-60, + 1 spare.
        const uint64_t K = (1ull << p->symbol_bits) + 1;
        const uint64_t n = (uint64_t)block_size * 8 / p->symbol_bits + 1; // symbols incl. EOF
        uint32_t       lg = 0;
        while ((1ull << lg) < K + n)
            lg++;
        const uint64_t per = (lg < p->freq_bits ? lg : p->freq_bits) + 2;
        return n * per / 8 + p->code_bits / 8 + 64;
    }
    // Worst case of one block's stream.  While the model never freezes inside a block the
    // adaptive code length is <= 8 bits/symbol + O(256 log N) and the integer truncation of
    // codec.rs:59-60 loses < 1 bit/symbol: 9 bits/symbol.  Once frozen (count == freq_max) a
    // symbol of frequency 1 costs up to freq_bits + 1 bits.
    const uint64_t n        = block_size;
    const bool     freezes  = 257ull + n > freq_max;
    const uint64_t bits     = freezes ? n * (p->freq_bits + 2) : n * 9;
    return bits / 8 + 1024;
}

// static_model: the fixed-table coder (redux_static.hpp).  A symbol of frequency >= 1 out of
// total <= freq_max costs at most freq_bits bits + 1 for the truncation of codec.rs:59-60, + 1
// spare; no reciprocal table, no tree.
static Geometry geometry(const redux_params *p, uint64_t in_len, uint32_t block_size, bool static_model = false, bool allow_coop = true)
{
    Geometry g;
    memset(&g, 0, sizeof g);
    g.nblocks = in_len == 0 ? 1 : (in_len + block_size - 1) / block_size;
    const uint64_t cap = static_model ? ((uint64_t)block_size + 1) * (p->freq_bits + 2) / 8 + 1024 : slot_cap_for(p, block_size);
    g.slot_cap   = cap > 0xFFFFFF00ull ? 0xFFFFFF00u : (uint32_t)cap;
    // Slot stride: a whole number of 128-byte lines, and an ODD one.  All lanes write their
    // slots at about the same relative offset, so a stride that is a multiple of 2^k lines
    // folds the concurrently written lines onto 1/2^k of the L2 sets and evicts them
    // half-written (measured: 2.6x the stream bytes written to HBM at a stride of 584 lines).
    g.slot_bytes = align_up((uint64_t)g.slot_cap + 32, 128);
    if (((g.slot_bytes / 128) & 1) == 0)
        g.slot_bytes += 128;
    const uint64_t freq_max = (1ull << p->freq_bits) - 1;
    g.nfreeze = (uint32_t)(freq_max - 257);
    const uint64_t maxlen = in_len < block_size ? in_len : block_size;
    g.rc_n  = (uint32_t)((maxlen < g.nfreeze ? maxlen : g.nfreeze) + 1);
    g.u16   = block_size <= 65536;
    g.fixup = (257ull + (uint64_t)(g.rc_n - 1)) >= (1ull << 17);
    g.rc_n += 32; // slack: both coders load their reciprocals a group / a chunk ahead without clamping
    g.any = !static_model && is_any(p);
    if (static_model)
        g.rc_n = 0;
    g.gen = !static_model && is_gen(p, block_size) && 64ull * g.slot_bytes < (1ull << 32); // (64 blocks: implied by is_gen)
    if (g.gen) { // reciprocal table over the symbol count (the trees are in LDS)
        const uint64_t k0      = (1ull << p->symbol_bits) + 1;
        const uint64_t nsym    = maxlen * 8 / p->symbol_bits;
        const uint64_t nfreeze = freq_max - k0;
        g.any     = false;
        g.nfreeze = (uint32_t)(nfreeze < 0xFFFFFFFFull ? nfreeze : 0xFFFFFFFFull);
        g.rc_n    = (uint32_t)((nsym < nfreeze ? nsym : nfreeze) + 1 + 32);
        g.u16     = false;
        g.fixup   = true;
        g.tree_bytes = 0;
    }
    if (g.any) { // no reciprocal table; one tree of 2^symbol_bits + 2 u32 per block
        g.rc_n       = 0;
        g.u16        = false;
        g.fixup      = true;
        g.tree_bytes = align_up(((1ull << p->symbol_bits) + 2) * 4, 256);
    }
    // a grid that leaves most SIMDs idle: the model by 64 lanes per block, the chain by one.  One block of any length --
    // redux_compress, the literal redux::compress -- is such a grid (redux_coop.hpp).
    g.pair_width = g.u16 ? 64u : 1u; // blocks of up to 64 KiB: rows of 64 lanes per symbol; larger ones: block-major (k_coop_model)
    // Blocks of up to 64 KiB: the pairs of whole blocks (8 bytes per input byte).  Larger blocks -- one stream of any length
    // above all -- are coded in windows, one (model, chain) pair of launches per window, so that the pairs area and the
    // reciprocal table hold one window whatever the block length: the largest window whose pairs fit kCoopWindowBytes, at most
    // kCoopWindowMax symbols, the windows together covering block_size + 1 symbols (the last one holds a full block's EOF).
    const uint64_t lanes_total = g.u16 ? (g.nblocks + 63) / 64 * 64 : g.nblocks;
    g.coop_win  = block_size + 1;
    g.coop_nwin = 1;
    if (!g.u16) {
        uint64_t w = kCoopWindowBytes / 2 / (8 * lanes_total); // (two buffers: the model of a window runs next to the chain of the one before)
        w = w > kCoopWindowMax ? kCoopWindowMax : w;
        w = w < 4096 ? 4096 : w;
        if (w < (uint64_t)block_size + 1) {
            g.coop_nwin = (uint32_t)(((uint64_t)block_size + 1 + w - 1) / w);
            g.coop_win  = (uint32_t)((((uint64_t)block_size + 1 + g.coop_nwin - 1) / g.coop_nwin + 31) & ~31ull);
        }
    }
    const uint64_t pair_bytes = (g.u16 ? lanes_total * ((uint64_t)g.coop_win + kCoopSlack) : 2 * lanes_total * coop_block_pitch(g.coop_win)) * 8;
    // fewer than 64 large blocks on the small-grid kernels: linear slots, one per block (a row-major group area is 64 slots
    // big whatever the number of blocks: 230 MiB to code one 3 MiB stream); a lane addresses its slot with 32-bit offsets
    const bool linear = g.nblocks < 64 && !g.u16;
    g.coop = allow_coop && !static_model && !g.any && !g.gen && g.nblocks <= (g.u16 ? kCoopMaxBlocks : kCoopMaxLargeBlocks) && block_size >= kCoopMinBlock &&
             (linear ? g.nblocks : 64ull) * g.slot_bytes < (1ull << 32) && pair_bytes <= (g.u16 ? kCoopMaxPairBytes : kCoopWindowBytes + (64ull << 20));
    if (g.coop) // the reciprocals of one window (+ what the chain wave reads ahead); blocks coded in windows: of two, alternating
        g.rc_n = g.u16 ? g.coop_win + 64 : 2 * ((g.coop_win + 64 + 31) & ~31u);
    g.coop_linear = g.coop && linear;
    g.off_rc    = 0;
    g.off_sizes = align_up(g.off_rc + (uint64_t)g.rc_n * 8, 256);
    g.off_mode  = align_up(g.off_sizes + g.nblocks * 4, 256); // one word: 0 linear slots, != 0 row-major group areas
    g.off_slots = g.off_mode + 256 + kClaimWords * 4; // mode word, then k_encode_pair's role book
    // whole groups of 64 slots (a row-major group area is 64 slots big) + 1 spare slot for the dead lanes of linear mode;
    // giant blocks (one per wave, encode_lanes()) and the small-grid kernels' linear slots: one per block
    const bool     one_each = g.coop_linear || (!g.any && !g.gen && !static_model && !g.coop && 64ull * g.slot_bytes >= (1ull << 32));
    const uint64_t nslots = one_each ? g.nblocks : (g.nblocks + 63) / 64 * 64 + 1;
    g.off_trees = align_up(g.off_slots + nslots * g.slot_bytes + (g.nblocks + 63) / 64 * 128, 256);
    // the checked copy of a `_v_dev` call's block table + the bitmap of block numbers its check uses (redux_table.hpp)
    g.off_table = align_up(g.off_trees + (g.gen ? (g.nblocks + 63) / 64 * 64 : g.nblocks) * g.tree_bytes, 256); // gen: whole waves
    g.off_seen  = g.off_table + align_up(g.nblocks * sizeof(redux_block), 256);
    // small-grid kernels, blocks coded in windows: 8 words of coder state + 256 symbol counts per block, carried between windows
    g.off_cstate = g.off_seen + align_up(table_seen_words(g.nblocks) * 4, 256);
    g.off_pairs  = g.off_cstate + ((g.coop && !g.u16) ? align_up(g.nblocks * (8 + 256) * 4, 256) : 0);
    g.total = g.off_pairs + (g.coop ? pair_bytes : 0);
    return g;
}

// The layout a launch uses in the workspace it was GIVEN.  A workspace sized for a larger input, or for a pipeline of several
// chunks, has no room for the small-grid kernels' pairs area: the launch then runs the full-grid kernels on the layout they
// need (same bytes out, the small-launch speed-up forgone).  The decision is made from (shape, workspace size) alone: once per
// call (encode_plan), and the same way by the two calls of the split pair redux_encode_slots_dev / redux_compact_slots_dev.
static Geometry geometry_ws(const redux_params *p, uint64_t in_len, uint32_t block_size, uint64_t workspace_bytes)
{
    Geometry g = geometry(p, in_len, block_size);
    if (g.coop && workspace_bytes < g.total)
        g = geometry(p, in_len, block_size, false, false);
    return g;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            fprintf(stderr, "redux_hip: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_),       \
                    __FILE__, __LINE__);                                                               \
            return REDUX_IO_ERROR;                                                                     \
        }                                                                                              \
    } while (0)

// CUs of HIP's current device (the _dev entry points launch on it and keep no other state): cached per device id
static uint32_t cu_count()
{
    static std::atomic<int> cus[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16)
        return 256;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return (uint32_t)n;
}

// ---- which kernel a call runs: ONE decision, used by the launch code and reported by
// redux_encode_kernel_name / redux_decode_kernel_name (bench.py's roofline.kernel) ------------
enum class EncKernel { PairCb32, Pair, SingleU16, SingleU32, Gen, GenPair, Any, CoopCb32, Coop };
enum class DecKernel { LockCb32, Lock, GenericU16, GenericU32, Cells, CellsFixup, CellsWorkspace, Cells8, Cells8Fixup, Any, Wave, WaveFixup };

// 64 blocks per wave while 64 slots / 64 blocks stay within a 32-bit lane offset; otherwise
// (giant blocks, whole-stream mode) one block per wave.
static uint32_t encode_lanes(const Geometry &g, uint32_t block_size)
{
    return (64ull * g.slot_bytes < (1ull << 32) && 64ull * block_size < (1ull << 32)) ? 64u : 1u;
}

static EncKernel pick_encode_kernel(const Geometry &g, const redux_params *p, bool aligned16, uint32_t block_size)
{
    if (g.gen)
        return p->symbol_bits < 8 ? EncKernel::Gen : EncKernel::GenPair;
    if (g.any)
        return EncKernel::Any;
    bool coop = g.coop;
#ifdef REDUX_AB // A/B timing builds only: REDUX_ENCODE_KERNEL=pair keeps small grids on the pair kernel
    if (getenv("REDUX_ENCODE_KERNEL"))
        coop = false;
#endif
    if (coop)
        return p->code_bits == 32 ? EncKernel::CoopCb32 : EncKernel::Coop;
    bool pair = g.u16 && aligned16 && encode_lanes(g, block_size) == 64;
#ifdef REDUX_AB // A/B timing builds only: REDUX_ENCODE_KERNEL=single pins the one-wave kernel
    const char *force = getenv("REDUX_ENCODE_KERNEL");
    if (force && !strcmp(force, "single"))
        pair = false;
#endif
    // (a u16 tree means blocks of <= 65536 symbols, so count <= 257 + 65536 < 2^17: no u16 kernel ever needs FIXUP)
    if (pair)
        return p->code_bits == 32 ? EncKernel::PairCb32 : EncKernel::Pair;
    return g.u16 ? EncKernel::SingleU16 : EncKernel::SingleU32;
}

// a decoder's geometry: no small-grid encoder, whose windows would size the reciprocal table
static Geometry decode_geometry(const redux_params *p, uint32_t block_size) { return geometry(p, block_size, block_size, false, false); }

// nslots: blocks (or table entries) of the launch; 0 = unknown (redux_decode_kernel_name: the full-grid choice).  Called by
// decode_layout alone, which decode_blocks_dev_impl, redux_decode_kernel_name_n and redux_decode_kernel_name_table read.
static DecKernel pick_decode_kernel(const Geometry &g, const redux_params *p, uint64_t nslots, uint32_t block_size, bool table)
{
    if (g.gen) {
        if (gen_needs_fixup(p, block_size))
            return DecKernel::CellsFixup;
        return gen_decode_in_workspace(p, nslots ? nslots : ~0ull) ? DecKernel::CellsWorkspace : DecKernel::Cells;
    }
    if (g.any)
        return DecKernel::Any;
    if (cells8_takes(p, block_size, nslots, table))
        return cells8_needs_fixup(p, block_size) ? DecKernel::Cells8Fixup : DecKernel::Cells8;
    // blocks the lock-step decoder does not take (u32 counts, count >= 2^17: one block of any length above all,
    // redux_decompress) in a launch that leaves SIMDs idle: one block per wave, the model across the lanes
    // (redux_decode_wave.hpp).  (For u16 blocks it measures 28.9 ms per 64 KiB block against the lock-step decoder's 24.)
    bool wave = nslots != 0 && nslots <= kWaveDecMaxBlocks && !(g.u16 && !g.fixup);
#ifdef REDUX_AB
    if (getenv("REDUX_DECODE_KERNEL"))
        wave = false;
#endif
    if (wave)
        return g.fixup ? DecKernel::WaveFixup : DecKernel::Wave;
    bool lock = g.u16 && !g.fixup;
#ifdef REDUX_AB // A/B timing builds only: REDUX_DECODE_KERNEL=generic pins k_decode
    if (getenv("REDUX_DECODE_KERNEL"))
        lock = false;
#endif
    if (lock)
        return p->code_bits == 32 ? DecKernel::LockCb32 : DecKernel::Lock;
    return g.u16 ? DecKernel::GenericU16 : DecKernel::GenericU32; // (u16: count < 2^17, as for the encoders)
}

// entries of the decoders' reciprocal table: what the block capacity (or the freeze point) asks for, but at most
// kDecRcWindow + slack -- a decoder of longer blocks computes the rest itself (rc_lookup, redux_decode.hpp)
static uint32_t dec_rc_entries(const Geometry &g)
{
    return (g.gen || g.rc_n <= kDecRcWindow + 32) ? g.rc_n : kDecRcWindow + 32;
}

// A decode launch in its workspace: the kernel, then [reciprocal table] [checked copy of a block table] [its bitmap], or
// [reciprocal table] [the cell decoder's bottom cells] (11- and 12-bit symbols: gen_decode_in_workspace), or the trees of the
// general parameters alone.  The ONE place that decides it: the size, the launch and the kernel names read these fields.
struct DecodeLayout {
    DecKernel kernel;
    uint32_t  rc_n; // reciprocal entries the launch fills
    uint64_t  off_table, off_seen, off_trees, total;
};

// nblocks: blocks (or table entries) of the launch; 0 = unknown (redux_decode_kernel_name: the full-grid choice)
static DecodeLayout decode_layout(const Geometry &g, const redux_params *p, uint64_t nblocks, uint32_t block_size, bool table)
{
    DecodeLayout L = {pick_decode_kernel(g, p, nblocks, block_size, table), 0, 0, 0, 0, 0};
    if (g.gen) {
        L.rc_n      = g.rc_n;
        L.off_trees = align_up((uint64_t)g.rc_n * 8, 256);
        L.total     = L.off_trees + (gen_decode_in_workspace(p, nblocks) ? (nblocks + 63) / 64 * 64 * gen_decode_tree_bytes(p) : 0);
    } else if (g.any) {
        L.total = (nblocks ? nblocks : 1) * g.tree_bytes;
    } else {
        // room for the table of either form of a call (the size is asked for without saying which): the cell decoder of 8-bit
        // symbols, which takes no block table, fills at least as many entries as the others (cells8_rc_entries)
        const bool     cells8 = L.kernel == DecKernel::Cells8 || L.kernel == DecKernel::Cells8Fixup;
        const uint32_t room   = cells8_takes(p, block_size, nblocks ? nblocks : 1, false) ? cells8_rc_entries(p, block_size) : dec_rc_entries(g);
        L.rc_n      = cells8 ? cells8_rc_entries(p, block_size) : dec_rc_entries(g);
        L.off_table = align_up((uint64_t)room * 8, 256);
        L.off_seen  = L.off_table + align_up(nblocks * sizeof(redux_block), 256);
        L.total     = L.off_seen + align_up(table_seen_words(nblocks) * 4, 256);
    }
    return L;
}

} // namespace redux

#include "redux_host.hpp"

using namespace redux;

// ---- the encoders of the chunked host calls (redux_host.hpp: EncodeCoder) --------------------------------------------
static host::EncodeCoder adaptive_encoder(const redux_params *p, uint32_t block_size)
{
    return {[=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
                // several chunks in flight keep the chip busy: no pairs area, so the chunks run on the pair kernel (encode_slots_impl)
                ws    = several ? geometry(p, max_in, block_size, false, false).total : redux_encode_workspace_bytes(p, max_in, block_size);
                bound = redux_encode_bound(p, max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_encode_blocks_dev(p, s.d_in.p, len, block_size, s.d_out.p, bound, s.d_off.p, s.d_st.p, s.d_sum.p, ws,
                                               ws_bytes, st);
            }};
}

// the static coder: its own workspace and bound for the largest chunk (its streams do not depend on either)
static host::EncodeCoder static_encoder(const redux_params *p, const uint32_t *cum, uint32_t block_size)
{
    return {[=](uint64_t max_in, bool, uint64_t &ws, uint64_t &bound) {
                ws    = redux_static_encode_workspace_bytes(p, max_in, block_size);
                bound = redux_static_encode_bound(p, max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_static_encode_blocks_dev(p, cum, s.d_in.p, len, block_size, s.d_out.p, bound, s.d_off.p, s.d_st.p,
                                                      s.d_sum.p, ws, ws_bytes, st);
            }};
}

// ---- the transforms in front of a coder (redux_planes.hpp, redux_delta.hpp, redux_zigzag.hpp, redux_base.hpp, redux_mixed.hpp)
// The split every transform launch makes: the fast kernel takes the `nfull` whole granules (a frame of E*B bytes, a unit of
// 8*B) of len bytes when the block size and every pointer are 16-byte multiples, and none otherwise; a byte kernel takes
// everything from byte `rest` on.
struct FastSplit {
    uint64_t nfull, rest;
};

static FastSplit fast_split(uint64_t len, uint64_t granule, uint32_t block_size, std::initializer_list<const void *> ptrs)
{
    uintptr_t bits = block_size;
    for (const void *p : ptrs)
        bits |= (uintptr_t)p;
    const uint64_t nfull = bits & 15 ? 0 : len / granule;
    return {nfull, nfull * granule};
}

// The three grid rules.  A workgroup per 256 groups, or W per unit: every workgroup has its own work, so a launch of more
// than 2^31 - 1 is refused (false).  A thread per byte and a workgroup per frame (or unit) stride over their work.
static bool grid_tiles(uint64_t wgs, uint32_t *grid)
{
    *grid = (uint32_t)wgs;
    return wgs <= 0x7FFFFFFFull;
}
static uint32_t grid_bytes(uint64_t nbytes) { return (uint32_t)std::min<uint64_t>((nbytes + 255) / 256, 8192); }
static uint32_t grid_frames(uint64_t nframes) { return (uint32_t)std::min<uint64_t>(nframes, 1u << 20); }

static PlanesArgs planes_args(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, const FastSplit &f)
{
    PlanesArgs a;
    a.src          = (const uint8_t *)d_src;
    a.dst          = (uint8_t *)d_dst;
    a.block_size   = block_size;
    a.frame_groups = block_size / 16;
    a.groups       = f.nfull * a.frame_groups;
    a.first        = f.rest;
    a.len          = len;
    return a;
}

// the byte-plane layout: one workgroup per 256 groups of the full frames, the byte kernel for the rest
template <int E>
static int launch_planes(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, bool inverse, hipStream_t s)
{
    const FastSplit  f = fast_split(len, (uint64_t)E * block_size, block_size, {d_src, d_dst});
    const PlanesArgs a = planes_args(d_src, d_dst, len, block_size, f);
    if (f.nfull) {
        uint32_t grid;
        if (!grid_tiles((a.groups + 255) / 256, &grid))
            return REDUX_UNSUPPORTED;
        if (inverse)
            k_planes<E, true><<<grid, 256, 0, s>>>(a);
        else
            k_planes<E, false><<<grid, 256, 0, s>>>(a);
    }
    if (f.rest < len) { // the short last frame, or everything the fast kernel cannot take
        if (inverse)
            k_planes_bytes<E, true><<<grid_bytes(len - f.rest), 256, 0, s>>>(a);
        else
            k_planes_bytes<E, false><<<grid_bytes(len - f.rest), 256, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// the filters with a running sum per frame -- the delta filter, its differences plain or folded (redux_delta.hpp,
// redux_zigzag.hpp), the lagged delta filter and its higher orders (redux_lag.hpp) -- through a filter's four kernels:
// forward as the layout, the inverse a workgroup per frame, the byte kernels for the rest.  extra: the kernels' arguments
// after PlanesArgs (the lag, the order)
template <int E, typename... T>
static int launch_filter(void (*planes)(PlanesArgs, T...), void (*unplanes)(PlanesArgs, T...), void (*planes_bytes)(PlanesArgs, T...),
                         void (*unplanes_bytes)(PlanesArgs, T...), const void *d_src, void *d_dst, uint64_t len, uint32_t block_size,
                         bool inverse, hipStream_t s, T... extra)
{
    const uint64_t   frame = (uint64_t)E * block_size;
    const FastSplit  f = fast_split(len, frame, block_size, {d_src, d_dst});
    const PlanesArgs a = planes_args(d_src, d_dst, len, block_size, f);
    if (f.nfull) {
        uint32_t grid;
        if (inverse)
            unplanes<<<grid_frames(f.nfull), 256, 0, s>>>(a, extra...);
        else if (!grid_tiles((a.groups + 255) / 256, &grid))
            return REDUX_UNSUPPORTED;
        else
            planes<<<grid, 256, 0, s>>>(a, extra...);
    }
    if (f.rest < len) { // the short last frame, or everything the fused kernels cannot take
        if (inverse)
            unplanes_bytes<<<grid_frames((len - f.rest + frame - 1) / frame), 256, 0, s>>>(a, extra...);
        else
            planes_bytes<<<grid_bytes(len - f.rest), 256, 0, s>>>(a, extra...);
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// the record layout (redux_record.hpp): the record size and the byte delta are kernel arguments.  Forward: tiles of T
// records, workgroups striding over them.  Inverse: a workgroup per (frame, column range); the columns are cut into ranges
// only where the frames alone would leave CUs idle.
static uint32_t record_lg_tile(uint32_t row, uint32_t items_row, uint32_t block_size)
{
    uint32_t lg = 4; // (a tile is at least the 16 records of a group)
    while (lg < 12 && (2u << lg) * (row + (row & 1 ? 0 : 1)) <= kRecordLdsBytes && (2u << lg) * items_row <= 16 * kRecordItems &&
           (1u << lg) < block_size)
        lg++;
    return lg;
}

// The shape of a record launch, decided here alone: launch_record launches what it says and redux_record_plan reports it.
// grid_fast / grid_rest are 0 where that kernel does not run.
struct RecordPlan {
    FastSplit f;
    uint32_t  lgT, PC, grid_fast, grid_rest;
};

static RecordPlan record_plan(const FastSplit &f, uint64_t len, uint32_t block_size, uint32_t R, bool delta, bool inverse, uint64_t cus)
{
    const uint64_t frame = (uint64_t)R * block_size;
    RecordPlan     p{f, 4, R, 0, 0};
    if (f.nfull) {
        if (inverse) {
            if (f.nfull < 2 * cus && R > 64) { // few frames: ranges of columns, 16-byte multiples of at least 64
                const uint64_t want = (2 * cus + f.nfull - 1) / f.nfull;
                const uint32_t pc   = (uint32_t)(((R + want - 1) / want + 15) / 16 * 16);
                p.PC = pc < 64 ? 64 : pc;
            }
            const uint32_t nr = (R + p.PC - 1) / p.PC;
            p.lgT       = record_lg_tile(nr > 1 ? p.PC : R, p.PC < R ? p.PC : R, block_size);
            p.grid_fast = (uint32_t)std::min<uint64_t>(f.nfull, 8 * cus) * nr;
        } else {
            p.lgT = record_lg_tile(R, 0, block_size);
            const uint64_t tiles = f.nfull * ((block_size + (1u << p.lgT) - 1) >> p.lgT);
            p.grid_fast = (uint32_t)std::min<uint64_t>(tiles, 8 * cus);
        }
    }
    if (f.rest < len) // the short last frame, or everything the fast kernels cannot take
        p.grid_rest = grid_bytes(inverse && delta ? (len - f.rest + frame - 1) / frame * R : len - f.rest);
    return p;
}

static int launch_record(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t R, bool delta, bool inverse,
                         hipStream_t s)
{
    const FastSplit  f = fast_split(len, (uint64_t)R * block_size, block_size, {d_src, d_dst});
    const RecordPlan p = record_plan(f, len, block_size, R, delta, inverse, f.nfull ? cu_count() : 0);
    RecordArgs a;
    a.src        = (const uint8_t *)d_src;
    a.dst        = (uint8_t *)d_dst;
    a.nfull      = f.nfull;
    a.block_size = block_size;
    a.R          = R;
    a.delta      = delta;
    a.lgT        = p.lgT;
    a.PC         = p.PC;
    a.first      = f.rest;
    a.len        = len;
    if (p.grid_fast) {
        if (inverse)
            k_record_unplanes<<<p.grid_fast, 256, 0, s>>>(a);
        else
            k_record_planes<<<p.grid_fast, 256, 0, s>>>(a);
    }
    if (p.grid_rest) {
        if (inverse)
            k_record_unplanes_bytes<<<p.grid_rest, 256, 0, s>>>(a);
        else
            k_record_planes_bytes<<<p.grid_rest, 256, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// the base filter: the fused kernels take the full frames that lie inside the base, one workgroup per 256 groups; the byte
// kernels take the rest up to the end of the frame the base ends in (or of the input); whole frames past the base have
// nothing to XOR and go to the layout alone (launch_planes).  SUB: the folded difference (redux_base_sub.hpp) in place of
// the XOR, with the same split: its fused kernels too may only take full frames that lie inside the base, where every
// element is covered
template <int E, bool SUB>
static int launch_base(const void *d_src, const void *d_base, uint64_t base_len, void *d_dst, uint64_t len, uint32_t block_size,
                       bool inverse, hipStream_t s)
{
    const uint64_t frame = (uint64_t)E * block_size;
    BaseArgs a;
    a.src          = (const uint8_t *)d_src;
    a.base         = (const uint8_t *)d_base;
    a.dst          = (uint8_t *)d_dst;
    a.block_size   = block_size;
    a.frame_groups = block_size / 16;
    a.len          = len;
    a.base_len     = base_len < len ? base_len : len;
    const FastSplit f = fast_split(a.base_len, frame, block_size, {d_src, d_base, d_dst});
    a.groups = f.nfull * a.frame_groups;
    a.first  = f.rest;
    a.end    = (a.base_len + frame - 1) / frame * frame; // the end of the frame the base ends in
    a.end    = a.end < len ? a.end : len;
    if (f.nfull) {
        uint32_t grid;
        if (!grid_tiles((a.groups + 255) / 256, &grid))
            return REDUX_UNSUPPORTED;
        typedef typename std::conditional<SUB, BaseSubFold<E>, BaseXor>::type OP;
        if (inverse)
            k_base_unplanes<E, OP><<<grid, 256, 0, s>>>(a);
        else
            k_base_planes<E, OP><<<grid, 256, 0, s>>>(a);
    }
    if (a.first < a.end) {
        const uint32_t grid = grid_bytes(a.end - a.first);
        if (SUB && inverse)
            k_base_sub_unplanes_bytes<E><<<grid, 256, 0, s>>>(a);
        else if (SUB)
            k_base_sub_planes_bytes<E><<<grid, 256, 0, s>>>(a);
        else if (inverse)
            k_base_unplanes_bytes<E><<<grid, 256, 0, s>>>(a);
        else
            k_base_planes_bytes<E><<<grid, 256, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    if (a.end < len) { // (a.end is a whole number of frames here: the layout of the rest is the rest of the layout)
        if constexpr (E == 1)
            HIP_TRY(hipMemcpyAsync(a.dst + a.end, a.src + a.end, len - a.end, hipMemcpyDeviceToDevice, s));
        else
            return launch_planes<E>(a.src + a.end, a.dst + a.end, len - a.end, block_size, inverse, s);
    }
    return REDUX_OK;
}

// f(std::integral_constant<int, E>) for a checked element size (redux_planes_check)
template <typename F>
static int for_element_size(uint32_t element_size, F &&f)
{
    switch (element_size) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// The filter in front of the byte-plane layout: none; the delta filter, its differences plain or folded (redux_delta.hpp,
// redux_zigzag.hpp); the lagged delta filter, whose lag travels next to the value, and its higher orders,
// whose order travels there too (redux_lag.hpp); the base filter, the XOR or the folded difference (redux_base.hpp,
// redux_base_sub.hpp).  The one name a filter has from the C entry points down to
// the kernel launch: a new filter is a new value here.
// RecordDelta is the byte delta of the record layout (redux_record.hpp) and goes with a record size only; the record layout
// without it is Filter::None with a record size.
// Stride is the snapshot-stride filter (redux_stride.hpp): its stride is a u64 and its inverse takes a workspace, so it has a
// transform of its own (stride_transform_dev) and never reaches transform_dev.
enum class Filter { None, Delta, Zigzag, Lag, LagOrder, BaseXor, BaseSub, RecordDelta, Stride };

static bool filter_has_base(Filter f) { return f == Filter::BaseXor || f == Filter::BaseSub; }

// the element size's check, and the lag's and the order's where the filter has them
static int filter_check(Filter f, uint32_t element_size, uint32_t lag, uint32_t order)
{
    return f == Filter::RecordDelta || f == Filter::Stride ? REDUX_INVALID_INPUT // (no element-size layout has it; its own check)
           : f == Filter::LagOrder ? redux_lag_order_check(element_size, lag, order)
           : f == Filter::Lag    ? redux_lag_check(element_size, lag)
                                 : redux_planes_check(element_size);
}

// redux_planes_dev, redux_delta_planes_dev, redux_zigzag_planes_dev, redux_lag_planes_dev, redux_lag_order_planes_dev,
// redux_base_planes_dev and redux_base_sub_planes_dev: the checks, then the transform's launch for the element size.
// d_base[0 .. base_len): the base of a base filter; lag: the lag of the lagged delta filter; order: that of its higher orders.
static int transform_dev(Filter filter, const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size,
                         int inverse, void *stream, const void *d_base = nullptr, uint64_t base_len = 0, uint32_t lag = 0,
                         uint32_t order = 0)
{
    const bool base = filter_has_base(filter);
    if (filter_check(filter, element_size, lag, order) != REDUX_OK || block_size == 0 || (len && (!d_src || !d_dst)) || (base && base_len && !d_base))
        return REDUX_INVALID_INPUT;
    if (len == 0)
        return REDUX_OK;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (s0 < d0 + len && d0 < s0 + len) // (not in place: the transform reads bytes another thread writes)
        return REDUX_INVALID_INPUT;
    const uintptr_t y0 = (uintptr_t)d_base;
    const uint64_t  used = base_len < len ? base_len : len;
    if (base && used && y0 < d0 + len && d0 < y0 + used) // (nor may the destination lie over the bytes of the base that are read)
        return REDUX_INVALID_INPUT;
    hipStream_t s = (hipStream_t)stream;
    const bool  inv = inverse != 0;
    return for_element_size(element_size, [&](auto e) -> int {
        constexpr int E = decltype(e)::value;
        switch (filter) {
        case Filter::BaseSub: return launch_base<E, true>(d_src, d_base, used, d_dst, len, block_size, inv, s);
        case Filter::BaseXor: return launch_base<E, false>(d_src, d_base, used, d_dst, len, block_size, inv, s);
        case Filter::LagOrder:
            return launch_filter<E>(k_lag_order_planes<E>, k_lag_order_unplanes<E>, k_lag_order_planes_bytes<E>,
                                    k_lag_order_unplanes_bytes<E>, d_src, d_dst, len, block_size, inv, s, lag, order);
        case Filter::Lag:
            return launch_filter<E>(k_lag_planes<E>, k_lag_unplanes<E>, k_lag_planes_bytes<E>, k_lag_unplanes_bytes<E>, d_src, d_dst,
                                    len, block_size, inv, s, lag);
        case Filter::Zigzag:
            return launch_filter<E>(k_delta_planes<E, true>, k_delta_unplanes<E, true>, k_delta_planes_bytes<E, true>,
                                    k_delta_unplanes_bytes<E, true>, d_src, d_dst, len, block_size, inv, s);
        case Filter::Delta:
            return launch_filter<E>(k_delta_planes<E, false>, k_delta_unplanes<E, false>, k_delta_planes_bytes<E, false>,
                                    k_delta_unplanes_bytes<E, false>, d_src, d_dst, len, block_size, inv, s);
        case Filter::RecordDelta: // (refused above)
        case Filter::Stride:
        case Filter::None: break;
        }
        if constexpr (E == 1) { // the layout of single bytes is the identity
            HIP_TRY(hipMemcpyAsync(d_dst, d_src, len, hipMemcpyDeviceToDevice, s));
            return REDUX_OK;
        } else {
            return launch_planes<E>(d_src, d_dst, len, block_size, inv, s);
        }
    });
}

// redux_record_planes_dev: transform_dev's checks for the record layout, then its launch
static int record_transform_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t record_size, int delta,
                                int inverse, void *stream)
{
    if (redux_record_check(record_size, delta) != REDUX_OK || block_size == 0 || (len && (!d_src || !d_dst)))
        return REDUX_INVALID_INPUT;
    if (len == 0)
        return REDUX_OK;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (s0 < d0 + len && d0 < s0 + len) // (not in place)
        return REDUX_INVALID_INPUT;
    return launch_record(d_src, d_dst, len, block_size, record_size, delta != 0, inverse != 0, (hipStream_t)stream);
}

// the snapshot-stride filter (redux_stride.hpp).  Forward: the fused kernel takes the full frames, the byte kernel the rest, as
// the layout does.  Inverse: the layout's own inverse into the destination (a copy for E = 1), then the running sums in place,
// in the shape stride_plan (redux_stride_host.hpp) gives them.  The one decision: the launches below and
// redux_stride_kernel_name both read StrideShape.
struct StrideShape {
    FastSplit  f;    // the layout's split, either direction
    StridePlan p;    // inverse: stage two
    int        form; // inverse: 0 chunks, 1 elements, 2 elements byte by byte
};

static StrideShape stride_shape(const void *d_src, const void *d_dst, uint64_t len, uint32_t block_size, uint32_t E, uint64_t S, bool inverse)
{
    StrideShape h;
    h.f    = fast_split(len, (uint64_t)E * block_size, block_size, {d_src, d_dst});
    h.p    = inverse ? stride_plan(len, E, S, ((uintptr_t)d_dst & 15) == 0) : StridePlan{};
    h.form = h.p.chunks ? 0 : (uintptr_t)d_dst % E == 0 ? 1 : 2;
    return h;
}

template <int E, int FORM>
static void launch_stride_sum(const StrideSumArgs &a, hipStream_t s)
{
    const uint32_t grid = (uint32_t)std::min<uint64_t>((a.segs * a.cols + 255) / 256, 1u << 22); // (the threads stride over the rest)
    if (a.segs > 1) {
        k_stride_totals<E, FORM><<<grid, 256, 0, s>>>(a);
        k_stride_scan<E, FORM><<<(uint32_t)std::min<uint64_t>(a.cols, 1u << 16), 256, 0, s>>>(a);
    }
    k_stride_sum<E, FORM><<<grid, 256, 0, s>>>(a);
}

template <int E>
static int launch_stride(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint64_t S, bool inverse, void *d_ws,
                         uint64_t ws_bytes, hipStream_t s)
{
    const StrideShape h = stride_shape(d_src, d_dst, len, block_size, E, S, inverse);
    if (!inverse) {
        StrideArgs a;
        a.src          = (const uint8_t *)d_src;
        a.dst          = (uint8_t *)d_dst;
        a.block_size   = block_size;
        a.frame_groups = block_size / 16;
        a.groups       = h.f.nfull * (E == 1 ? block_size / 16 : a.frame_groups);
        a.first        = h.f.rest;
        a.len          = len;
        a.S            = S;
        a.D            = S >= len / E ? ~0ull : S * E;
        if (h.f.nfull) {
            uint32_t grid;
            if (!grid_tiles((a.groups + 255) / 256, &grid))
                return REDUX_UNSUPPORTED;
            k_stride_planes<E><<<grid, 256, 0, s>>>(a);
        }
        if (h.f.rest < len)
            k_stride_planes_bytes<E><<<grid_bytes(len - h.f.rest), 256, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
        return REDUX_OK;
    }
    // (the workspace first: a call that cannot run writes nothing)
    uint8_t *ws = (uint8_t *)(((uintptr_t)d_ws + 15) & ~(uintptr_t)15);
    if (h.p.ws_bytes && (!d_ws || ws_bytes < h.p.ws_bytes + (uint64_t)(ws - (uint8_t *)d_ws)))
        return REDUX_OUTPUT_TOO_SMALL;
    if constexpr (E == 1) {
        HIP_TRY(hipMemcpyAsync(d_dst, d_src, len, hipMemcpyDeviceToDevice, s));
    } else {
        const int st = launch_planes<E>(d_src, d_dst, len, block_size, true, s);
        if (st != REDUX_OK)
            return st;
    }
    if (!h.p.run)
        return REDUX_OK;
    StrideSumArgs a;
    a.dst       = (uint8_t *)d_dst;
    a.ws        = ws;
    a.cols      = h.p.cols;
    a.rows      = h.p.rows;
    a.segs      = h.p.segs;
    a.steps     = h.p.steps;
    a.row_bytes = S * E;
    a.head      = h.p.head;
    a.S         = S;
    a.n         = h.p.n;
    if (h.p.rows >= 2) {
        if (h.form == 0)
            launch_stride_sum<E, 0>(a, s);
        else if (h.form == 1)
            launch_stride_sum<E, 1>(a, s);
        else
            launch_stride_sum<E, 2>(a, s);
    }
    if (h.p.chunks && h.p.head < h.p.n * E)
        k_stride_sum_tail<E><<<1, 64, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// redux_stride_planes_dev: transform_dev's checks for the snapshot-stride filter, then its launch
static int stride_transform_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, uint64_t stride,
                                int inverse, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    if (redux_stride_check(element_size, stride) != REDUX_OK || block_size == 0 || (len && (!d_src || !d_dst)))
        return REDUX_INVALID_INPUT;
    if (len == 0)
        return REDUX_OK;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (s0 < d0 + len && d0 < s0 + len) // (not in place: the forward reads bytes another thread would have written)
        return REDUX_INVALID_INPUT;
    return for_element_size(element_size, [&](auto e) -> int {
        return launch_stride<decltype(e)::value>(d_src, d_dst, len, block_size, stride, inverse != 0, d_workspace, workspace_bytes,
                                                 (hipStream_t)stream);
    });
}

// ---- the layout stage of the layered calls ---------------------------------------------------------------------------
// What runs between the caller's bytes and a coder: the byte-plane layout for elements of E bytes, with a filter in front
// of it or none.  The layout of single bytes is the identity; a filter over single bytes is not.
struct Layout {
    uint32_t    E;
    Filter      filter   = Filter::None;
    const void *d_base   = nullptr; // a base filter's base, d_base[0 .. base_len) on the device
    uint64_t    base_len = 0;
    uint32_t    lag      = 0;       // the lagged delta filter's lag
    uint32_t    order    = 0;       // the order of higher-order lagged differences
    uint32_t    record   = 0;       // the record layout's record size (E is 1 then, and does not say how many blocks a frame has)
    uint64_t    stride   = 0;       // the snapshot-stride filter's stride, in elements
    void       *d_ws     = nullptr; // and the workspace of its inverse's second stage, d_ws[0 .. ws_bytes)
    uint64_t    ws_bytes = 0;
    bool        record_delta() const { return filter == Filter::RecordDelta; }
    bool        is_stride() const { return filter == Filter::Stride; }
    int         check() const
    {
        if (is_stride())
            return record ? REDUX_INVALID_INPUT : redux_stride_check(E, stride);
        if (record)
            return E == 1 && (filter == Filter::None || record_delta()) ? redux_record_check(record, record_delta()) : REDUX_INVALID_INPUT;
        return filter_check(filter, E, lag, order);
    }
    bool        identity() const { return filter == Filter::None && E == 1 && !record; }
    bool        has_base() const { return filter_has_base(filter); }
    // room for the transformed copy of len bytes (none for the identity: the coder reads the caller's buffer)
    uint64_t copy_bytes(uint64_t len) const { return identity() ? 0 : planes_copy_bytes(len); }
    int transform(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, int inv, void *stream) const
    {
        if (record)
            return record_transform_dev(d_src, d_dst, len, block_size, record, record_delta(), inv, stream);
        if (is_stride())
            return stride_transform_dev(d_src, d_dst, len, block_size, E, stride, inv, d_ws, ws_bytes, stream);
        return transform_dev(filter, d_src, d_dst, len, block_size, E, inv, stream, d_base, base_len, lag, order);
    }
    int forward(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, void *stream) const
    {
        return transform(d_src, d_dst, len, block_size, 0, stream);
    }
    int inverse(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, void *stream) const
    {
        return transform(d_src, d_dst, len, block_size, 1, stream);
    }
};

static Layout record_layout(uint32_t record_size, int delta)
{
    Layout L{1, delta ? Filter::RecordDelta : Filter::None};
    L.record = record_size ? record_size : ~0u; // (0 must not mean "no record size" here: the check refuses it)
    return L;
}

// Encode side: the transformed copy x' of d_in goes to the front of the workspace (x' = d_in for the identity) and the coder
// gets x' and what is left of the workspace behind the copy.
struct Staged {
    const void *x;
    uint8_t    *ws;
    uint64_t    ws_bytes;
};

static int layout_stage(Layout L, const void *d_in, uint64_t in_len, uint32_t block_size, void *d_workspace, uint64_t workspace_bytes,
                        void *stream, Staged &o)
{
    const uint64_t copy = L.copy_bytes(in_len);
    if (workspace_bytes < copy)
        return REDUX_OUTPUT_TOO_SMALL;
    o = {L.identity() ? d_in : d_workspace, (uint8_t *)d_workspace + copy, workspace_bytes - copy};
    return L.identity() ? REDUX_OK : L.forward(d_in, d_workspace, in_len, block_size, stream);
}

// Decode side: the blocks were decoded to the plane buffer d_t at the front of the workspace, block_size bytes of room each,
// so that a damaged stream writes nothing outside it (d_t null: to d_out in place, where the layout is the identity).  Their
// sizes are checked against the layout of out_len bytes, the inverse writes d_out[0 .. out_len) and nothing else, and the
// summary is taken.  Who writes d_summary differs by caller: the adaptive decoders have begun it and k_planes_sizes adds to
// it (InSizes); the static decoders leave it to one k_summarize at the end (Summarize); the stored call zeroes it first
// (ZeroSummarize).
enum class TailSummary { InSizes, Summarize, ZeroSummarize };

static int layout_decode_tail(Layout L, const void *d_t, void *d_out, uint64_t out_len, uint32_t block_size, void *d_out_sizes,
                              void *d_block_status, void *d_summary, TailSummary how, void *stream)
{
    hipStream_t    s       = (hipStream_t)stream;
    const uint64_t nblocks = redux_block_count(out_len, block_size), wgs = (nblocks + 255) / 256;
    k_planes_sizes<<<(uint32_t)(wgs < 1024 ? wgs : 1024), 256, 0, s>>>((const uint32_t *)d_out_sizes, (int32_t *)d_block_status,
                                                                        how == TailSummary::InSizes ? (int32_t *)d_summary : nullptr,
                                                                        nblocks, out_len, block_size);
    HIP_TRY(hipGetLastError());
    if (d_t) {
        const int st = L.inverse(d_t, d_out, out_len, block_size, stream);
        if (st != REDUX_OK)
            return st;
    }
    if (d_summary && how != TailSummary::InSizes) {
        if (how == TailSummary::ZeroSummarize)
            HIP_TRY(hipMemsetAsync(d_summary, 0, 8, s));
        k_summarize<<<64, 256, 0, s>>>((const int32_t *)d_block_status, nblocks, (int32_t *)d_summary);
        HIP_TRY(hipGetLastError());
    }
    return REDUX_OK;
}

// per-block CRC-32 (redux_crc.hpp): G lanes per block, the widest power of two up to 64 that leaves every lane at least
// 16 chunks; blocks above kCrcSeg in segments (XORed into a zeroed d_crc)
static uint32_t crc_group(uint32_t block_size)
{
    uint32_t G = 1;
    while (G < 64 && 512ull * G <= block_size)
        G *= 2;
    return G;
}

static int launch_crc32(const void *d_in, uint64_t in_len, const void *d_sizes, uint64_t nblocks, uint32_t block_size, void *d_crc,
                        hipStream_t s)
{
    if (nblocks == 0)
        return REDUX_OK;
    CrcArgs a;
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.sizes      = (const uint32_t *)d_sizes;
    a.nblocks    = nblocks;
    a.block_size = block_size;
    a.nseg       = block_size > kCrcSeg ? (uint32_t)((block_size + kCrcSeg - 1) / kCrcSeg) : 1;
    a.nitems     = nblocks * a.nseg;
    a.crc        = (uint32_t *)d_crc;
    const uint32_t G    = crc_group(block_size);
    const uint64_t per  = kCrcThreads / G, wgs = (a.nitems + per - 1) / per, cap = 4ull * cu_count(); // (32 KiB of LDS each)
    const uint32_t grid = (uint32_t)(wgs < cap ? wgs : cap);
    if (a.nseg > 1)
        HIP_TRY(hipMemsetAsync(d_crc, 0, nblocks * 4, s));
    switch (G) {
    case 1: k_crc32<1><<<grid, kCrcThreads, 0, s>>>(a); break;
    case 2: k_crc32<2><<<grid, kCrcThreads, 0, s>>>(a); break;
    case 4: k_crc32<4><<<grid, kCrcThreads, 0, s>>>(a); break;
    case 8: k_crc32<8><<<grid, kCrcThreads, 0, s>>>(a); break;
    case 16: k_crc32<16><<<grid, kCrcThreads, 0, s>>>(a); break;
    case 32: k_crc32<32><<<grid, kCrcThreads, 0, s>>>(a); break;
    default: k_crc32<64><<<grid, kCrcThreads, 0, s>>>(a); break;
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// ---- layout estimates (redux_layout_cost.hpp) ------------------------------------------------------------------------
// frames the fast kernel takes: all full ones when block size and buffer are 16-byte multiples, none otherwise
static uint64_t layout_cost_full_frames(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t E)
{
    return block_size % 16 == 0 && ((uintptr_t)d_in & 15) == 0 ? in_len / ((uint64_t)E * block_size) : 0;
}

template <int E>
static int launch_layout_cost(const void *d_in, uint64_t in_len, uint32_t block_size, bool plain, bool delta, double *bits,
                              hipStream_t s)
{
    LayoutCostArgs a;
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.nblocks    = redux_block_count(in_len, block_size);
    a.nfull      = layout_cost_full_frames(d_in, in_len, block_size, E);
    a.block_size = block_size;
    a.nfilt      = 0;
    constexpr uint32_t log2E = E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : 3;
    a.filt[1] = 0;
    a.bits[1] = nullptr;
    if (plain) {
        a.filt[a.nfilt]   = 0;
        a.bits[a.nfilt++] = bits + (uint64_t)log2E * a.nblocks;
    }
    if (delta) {
        a.filt[a.nfilt]   = 1;
        a.bits[a.nfilt++] = bits + (uint64_t)(4 + log2E) * a.nblocks;
    }
    if (a.nfull) { // four waves per CU: 160 KiB of LDS
        const uint64_t cap  = (a.nfilt == 2 ? 2ull : 4ull) * cu_count();
        const uint32_t grid = (uint32_t)(a.nfull < cap ? a.nfull : cap);
        if (a.nfilt == 2)
            k_layout_cost<E, 2><<<grid, 128, 0, s>>>(a);
        else
            k_layout_cost<E, 1><<<grid, 64, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t nrest = a.nblocks - a.nfull * E;
    if (nrest) { // the short last frame, or everything the fast kernel cannot take
        const uint64_t work = nrest * a.nfilt, cap = (uint64_t)kHistWgsPerCu * cu_count();
        k_layout_cost_bytes<E><<<(uint32_t)(work < cap ? work : cap), 64, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
    }
    return REDUX_OK;
}

// ---- lag and order estimates (redux_lag_cost.hpp) ---------------------------------------------------------------------
// the selected frames (0, T, 2T, ...) of an input of nblocks blocks, and the blocks they have: all but the last E each
static uint64_t lag_cost_selected(uint64_t nblocks, uint32_t E, uint32_t frame_step, uint64_t *row_blocks)
{
    const uint64_t frames = (nblocks + E - 1) / E, nsel = (frames + frame_step - 1) / frame_step;
    const uint64_t left = nblocks - (nsel - 1) * frame_step * E; // blocks from the last selected frame on
    *row_blocks = (nsel - 1) * E + (left < E ? left : E);
    return nsel;
}

// the lag and the order estimates: the fast kernel for the selected full frames, the byte kernel for the rest of a row.
// a.lags and a.orders (and a.ncand) are filled by the caller: redux_lag_cost_dev, redux_lag_order_cost_dev
template <int E>
static int launch_lag_cost(void (*fast)(LagCostArgs), void (*bytes)(LagCostArgs), LagCostArgs &a, const void *d_in, uint64_t in_len,
                           uint32_t block_size, uint32_t frame_step, double *bits, hipStream_t s)
{
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.nblocks    = redux_block_count(in_len, block_size);
    a.bits       = bits;
    a.block_size = block_size;
    a.frame_step = frame_step;
    lag_cost_selected(a.nblocks, E, frame_step, &a.row_blocks);
    const uint64_t nfull = layout_cost_full_frames(d_in, in_len, block_size, E);
    a.nsel_fast  = (nfull + frame_step - 1) / frame_step;
    if (a.nsel_fast) { // one workgroup of four waves per CU: 160 KiB of LDS
        const uint64_t jobs = a.nsel_fast * ((a.ncand + kLagCostWaves - 1) / kLagCostWaves), cap = cu_count();
        fast<<<(uint32_t)(jobs < cap ? jobs : cap), 64 * kLagCostWaves, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
    }
    const uint64_t nrest = a.row_blocks - a.nsel_fast * E;
    if (nrest) { // a selected short last frame, or everything the fast kernel cannot take
        const uint64_t work = nrest * a.ncand, cap = (uint64_t)kHistWgsPerCu * cu_count();
        bytes<<<(uint32_t)(work < cap ? work : cap), 64, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
    }
    return REDUX_OK;
}

// ---- record estimates (redux_record_cost.hpp) --------------------------------------------------------------------------
// a.records, a.deltas and a.ncand are filled by the caller.  k_record_cost takes the selected full frames of every candidate,
// k_record_cost_bytes the rest of every row; each gets the running count of its own jobs.
static int launch_record_cost(RecordCostArgs &a, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t sample_blocks,
                              double *bits, hipStream_t s)
{
    a.in            = (const uint8_t *)d_in;
    a.in_len        = in_len;
    a.stride        = redux_block_count(in_len, block_size);
    a.bits          = bits;
    a.block_size    = block_size;
    a.sample_blocks = sample_blocks;
    a.fast          = block_size % 16 == 0 && ((uintptr_t)d_in & 15) == 0;
    for (int pass = 0; pass < 2; pass++) { // 0: the fast kernel, 1: the byte kernel
        uint64_t jobs = 0;
        for (uint32_t c = 0; c <= REDUX_RECORD_COST_MAX; c++) {
            a.jobs[c] = jobs;
            if (c >= a.ncand)
                continue;
            const uint32_t         R  = a.records[c];
            const RecordCostSample sm = record_cost_sample(in_len, block_size, R, sample_blocks);
            const uint64_t         nf = record_cost_fast_frames(in_len, block_size, R, a.fast, sm);
            jobs += pass ? sm.row_blocks - nf * R : nf * (R > kRecordCostPC ? (R + kRecordCostPC - 1) / kRecordCostPC : 1);
        }
        if (!jobs)
            continue;
        if (pass == 0) {
            const uint64_t cap = (uint64_t)kRecordCostWgsPerCu * cu_count();
            k_record_cost<<<(uint32_t)(jobs < cap ? jobs : cap), 256, 0, s>>>(a);
        } else {
            const uint64_t cap = (uint64_t)kHistWgsPerCu * cu_count();
            k_record_cost_bytes<<<(uint32_t)(jobs < cap ? jobs : cap), 64, 0, s>>>(a);
        }
        HIP_TRY(hipGetLastError());
    }
    return REDUX_OK;
}

// ---- mixed layouts (redux_mixed.hpp) ----------------------------------------------------------------------------------
// the transform of d_src[0 .. len) under the device table: W workgroups per full unit (what E = 8 needs: the others loop),
// the byte kernel for the rest -- forward a thread per byte, inverse a workgroup per unit
static int launch_mixed(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, const void *d_table, bool inverse,
                        hipStream_t s)
{
    const uint64_t  unit = (uint64_t)kMixedUnit * block_size;
    const FastSplit f = fast_split(len, unit, block_size, {d_src, d_dst});
    MixedArgs a;
    a.src          = (const uint8_t *)d_src;
    a.dst          = (uint8_t *)d_dst;
    a.table        = (const uint8_t *)d_table;
    a.block_size   = block_size;
    a.frame_groups = block_size / 16;
    a.nfull        = f.nfull;
    a.wgs          = (a.frame_groups + 255) / 256;
    a.len          = len;
    a.first        = f.rest;
    if (f.nfull) {
        uint32_t grid;
        if (!grid_tiles(a.nfull * a.wgs, &grid))
            return REDUX_UNSUPPORTED;
        if (inverse)
            k_mixed_planes<true><<<grid, 256, 0, s>>>(a);
        else
            k_mixed_planes<false><<<grid, 256, 0, s>>>(a);
    }
    if (f.rest < len) { // the short last unit, or everything the fast kernel cannot take
        if (inverse)
            k_mixed_bytes<true><<<grid_frames((len - f.rest + unit - 1) / unit), 256, 0, s>>>(a);
        else
            k_mixed_bytes<false><<<grid_bytes(len - f.rest), 256, 0, s>>>(a);
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

static int mixed_layout_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, const void *d_table, int inverse,
                            void *stream)
{
    if (block_size == 0 || block_size > (1u << 30) || !d_table || (len && (!d_src || !d_dst)))
        return REDUX_INVALID_INPUT;
    if (len == 0)
        return REDUX_OK;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (s0 < d0 + len && d0 < s0 + len) // (not in place: the transform reads bytes another thread writes)
        return REDUX_INVALID_INPUT;
    return launch_mixed(d_src, d_dst, len, block_size, d_table, inverse != 0, (hipStream_t)stream);
}

static int mixed_choose_dev(const void *d_bits, uint64_t nblocks, uint32_t layouts_mask, void *d_table, void *d_sum_bits, void *stream)
{
    if (!d_bits || !d_table || nblocks == 0 || layouts_mask == 0 || layouts_mask > 0xFF)
        return REDUX_INVALID_INPUT;
    hipStream_t s = (hipStream_t)stream;
    MixedChooseArgs a;
    a.bits    = (const double *)d_bits;
    a.nblocks = nblocks;
    a.nunits  = (nblocks + kMixedUnit - 1) / kMixedUnit;
    a.mask    = layouts_mask;
    a.table   = (uint8_t *)d_table;
    a.sum     = (unsigned long long *)d_sum_bits;
    if (d_sum_bits)
        HIP_TRY(hipMemsetAsync(d_sum_bits, 0, 8, s));
    const uint64_t wgs = (a.nunits + 255) / 256;
    k_mixed_choose<<<(uint32_t)(wgs < 4096 ? wgs : 4096), 256, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// bytes of the cost rows in the workspace of redux_encode_mixed_dev: f64[8][nblocks], a 256-byte multiple
static uint64_t mixed_cost_bytes(uint64_t nblocks) { return (nblocks * 64 + 255) / 256 * 256; }


extern "C" {

const char *redux_version(void) { return "redux_hip 0.3.0 gfx950"; }

#ifndef REDUX_SOURCE_HASH
#define REDUX_SOURCE_HASH "unknown"
#endif
const char *redux_source_hash(void) { return REDUX_SOURCE_HASH; }

static const char *encode_kernel_name_of(const Geometry &g, const redux_params *p, const void *d_in, uint32_t block_size)
{
    const bool aligned16 = (((uintptr_t)d_in) & 15) == 0 && (block_size & 15) == 0;
    switch (pick_encode_kernel(g, p, aligned16, block_size)) {
    case EncKernel::CoopCb32: return "k_coop_model + k_coop_chain<true> (small grid: model by 64 lanes per block, chain wave + bit-writer wave, code_bits 32)";
    case EncKernel::Coop: return "k_coop_model + k_coop_chain<false> (small grid: model by 64 lanes per block, chain wave + bit-writer wave)";
    case EncKernel::PairCb32: return "k_encode_pair<false, true> (u16 tree, model wave + coder wave, code_bits 32)";
    case EncKernel::Pair: return "k_encode_pair<false, false> (u16 tree, model wave + coder wave)";
    case EncKernel::SingleU16: return "k_encode<true, false> (u16 tree, one wave per 64 blocks)";
    case EncKernel::SingleU32: return "k_encode<false, true> (u32 tree)";
    case EncKernel::Gen: {
        static const char *const names[8] = {"", "k_encode_gen<1>", "k_encode_gen<2>", "k_encode_gen<3>", "k_encode_gen<4>", "k_encode_gen<5>",
                                              "k_encode_gen<6>", "k_encode_gen<7>"};
        return names[p->symbol_bits]; // (lock-step, u32 tree in LDS, one wave per 64 blocks)
    }
    case EncKernel::GenPair: {
        // lock-step, u16 tree in LDS, one workgroup per 64 / 64 / 32 / 16 blocks: three model waves + a coder wave
        static const char *const names[4] = {"k_encode_gen_pair<9>", "k_encode_gen_pair<10>", "k_encode_gen_pair<11>", "k_encode_gen_pair<12>"};
        return names[p->symbol_bits - 9];
    }
    case EncKernel::Any: return "k_encode_any (general parameters, one lane per block)";
    }
    return "";
}

const char *redux_encode_kernel_name(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return "";
    return encode_kernel_name_of(geometry(p, in_len, block_size), p, d_in, block_size);
}

const char *redux_encode_kernel_name_ws(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint64_t workspace_bytes)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return "";
    return encode_kernel_name_of(geometry_ws(p, in_len, block_size, workspace_bytes), p, d_in, block_size);
}

const char *redux_decode_kernel_name(const redux_params *p, const void *d_out, uint32_t block_size)
{
    return redux_decode_kernel_name_n(p, d_out, block_size, 0);
}

static const char *decode_kernel_name_of(DecKernel k, const redux_params *p)
{
    switch (k) {
    case DecKernel::LockCb32: return "k_decode_lock<true> (u16 tree, one wave per 64 blocks, code_bits 32)";
    case DecKernel::Lock: return "k_decode_lock<false> (u16 tree, one wave per 64 blocks)";
    case DecKernel::GenericU16: return "k_decode<true, false> (u16 tree, per-lane control flow)";
    case DecKernel::GenericU32: return "k_decode<false, true> (u32 tree)";
    case DecKernel::CellsFixup: {
        // lock-step, the tree as cells of four levels in LDS; the instance for counts of 2^17 and more (widths 1 ... 7)
        static const char *const names[8] = {"", "k_decode_cells<1> (fix-up: count past 2^17)", "k_decode_cells<2> (fix-up: count past 2^17)",
                                             "k_decode_cells<3> (fix-up: count past 2^17)", "k_decode_cells<4> (fix-up: count past 2^17)",
                                             "k_decode_cells<5> (fix-up: count past 2^17)", "k_decode_cells<6> (fix-up: count past 2^17)",
                                             "k_decode_cells<7> (fix-up: count past 2^17)"};
        return p->symbol_bits < 8 ? names[p->symbol_bits] : "";
    }
    case DecKernel::Cells:
    case DecKernel::CellsWorkspace: {
        // lock-step, the tree as cells of four levels: all of them in LDS (symbol_bits <= 10), or the bottom ones in the workspace
        static const char *const names[13] = {"", "k_decode_cells<1> (cells in LDS)", "k_decode_cells<2> (cells in LDS)",
                                               "k_decode_cells<3> (cells in LDS)", "k_decode_cells<4> (cells in LDS)",
                                               "k_decode_cells<5> (cells in LDS)", "k_decode_cells<6> (cells in LDS)",
                                               "k_decode_cells<7> (cells in LDS)", "", "k_decode_cells<9> (cells in LDS)",
                                               "k_decode_cells<10> (cells in LDS)", "k_decode_cells<11> (bottom cells in the workspace)",
                                               "k_decode_cells<12> (bottom cells in the workspace)"};
        return names[p->symbol_bits];
    }
    case DecKernel::Cells8: return "k_decode_cells<8> (u32 cells, blocks above 64 KiB, one wave per 64 blocks)";
    case DecKernel::Cells8Fixup: return "k_decode_cells<8> (u32 cells, blocks above 64 KiB, one wave per 64 blocks; fix-up: count past 2^17)";
    case DecKernel::Any: return "k_decode_any (general parameters, one lane per block)";
    case DecKernel::Wave: return "k_decode_wave (one block per wave, cumulative table across the lanes)";
    case DecKernel::WaveFixup: return "k_decode_wave (one block per wave, cumulative table across the lanes; fix-up: count past 2^17)";
    }
    return "";
}

const char *redux_decode_kernel_name_n(const redux_params *p, const void *d_out, uint32_t block_size, uint64_t nblocks)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return "";
    (void)d_out; // every decoder takes any alignment (it only picks the store width inside the kernel)
    return decode_kernel_name_of(decode_layout(decode_geometry(p, block_size), p, nblocks, block_size, false).kernel, p);
}

// the launch given a block table (decode_blocks_dev_impl with d_table: the `_v` calls, redux_decode_stored_dev)
const char *redux_decode_kernel_name_table(const redux_params *p, uint32_t block_size, uint64_t nentries)
{
    if (check_params(p) != REDUX_OK || block_size == 0 || nentries == 0)
        return "";
    const Geometry g = decode_geometry(p, block_size);
    if (g.gen || g.any) // (decode_blocks_dev_impl: UNSUPPORTED with a table)
        return "";
    return decode_kernel_name_of(decode_layout(g, p, nentries, block_size, true).kernel, p);
}

int redux_params_check(uint32_t symbol, uint32_t frequency, uint32_t code) /* model/mod.rs:64 */
{
    if (symbol < 1 || frequency < symbol + 2 || code < frequency + 2 || 64 < code + frequency)
        return REDUX_INVALID_INPUT;
    return REDUX_OK;
}

int redux_device_supports(const redux_params *p) { return check_params(p); }

uint64_t redux_block_count(uint64_t in_len, uint32_t block_size)
{
    if (block_size == 0)
        return 0;
    return in_len == 0 ? 1 : (in_len + block_size - 1) / block_size;
}

uint64_t redux_encode_slot_bytes(const redux_params *p, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return 0;
    return geometry(p, block_size, block_size).slot_cap;
}

uint64_t redux_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return 0;
    const Geometry g = geometry(p, in_len, block_size);
    return g.nblocks * (uint64_t)g.slot_cap;
}

uint64_t redux_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return 0;
    return geometry(p, in_len, block_size).total;
}

// ---- the adaptive coder's launch layer ----------------------------------------------------------------------------------
// The plan of an encode call: its Geometry, decided ONCE from (shape, workspace size) and handed to every stage of the
// call -- the coder, the compaction and whatever the caller runs between them.  in_len is what sizes the launch: the input
// bytes, or entries * block_size for the table form of a call.  Refuses what geometry() cannot take.
static int encode_plan(const redux_params *p, uint64_t in_len, uint32_t block_size, uint64_t workspace_bytes, Geometry &g)
{
    const int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0)
        return REDUX_INVALID_INPUT;
    g = geometry_ws(p, in_len, block_size, workspace_bytes);
    return REDUX_OK;
}

// The table form of a call (the `_v` calls, stored and constant blocks), in both directions: slot j of the launch takes the
// block entries[j] names.  The launch counts entries; sizes, statuses and the summary are per block.  No entries: the plain
// form, block b at b * block_size.
struct BlockTable {
    const redux_block *entries   = nullptr;
    bool               aligned16 = false; // every entry's offset is a 16-byte multiple
    uint64_t           nblocks   = 0;     // the blocks the entries name
    bool               trusted   = false; // the library's own, or the checked copy of a caller's: the kernels may read it
};

// the raw bytes the compaction copies for the blocks flagged in `stored` (redux_store.hpp); none: every block is its stream
struct RawCopy {
    const uint8_t *stored     = nullptr;
    const void    *raw        = nullptr;
    uint32_t       block_size = 0;
};

// what the one filler of each argument core writes
static EncCore enc_core(const Geometry &g, const void *d_in, uint64_t in_len, uint8_t *ws, void *d_block_status)
{
    EncCore c;
    c.in         = (const uint8_t *)d_in;
    c.in_len     = in_len;
    c.nblocks    = g.nblocks;
    c.slots      = ws + g.off_slots;
    c.slot_bytes = g.slot_bytes;
    c.sizes      = (uint32_t *)(ws + g.off_sizes);
    c.status     = (int32_t *)d_block_status;
    return c;
}

static DecCore dec_core(const void *d_in, const void *d_in_offsets, uint64_t nblocks, void *d_out, void *d_out_sizes, void *d_block_status)
{
    DecCore c;
    c.in         = (const uint8_t *)d_in;
    c.in_offsets = (const uint64_t *)d_in_offsets;
    c.nblocks    = nblocks;
    c.out        = (uint8_t *)d_out;
    c.out_sizes  = (uint32_t *)d_out_sizes;
    c.status     = (int32_t *)d_block_status;
    return c;
}

// A caller's block table is caller data: the kernels read a checked copy (redux_table.hpp).  t: the table as given, nentries
// of them over `bytes` bytes of blocks; the copy goes to `copy`, the bitmap of block numbers to `seen`, and what the check
// finds to the per-block sizes and statuses.  Returns the copy and the word k_table_verdict reads after the call's summary.
struct CheckedTable {
    const redux_block *entries;
    const uint32_t    *failed;
};

static CheckedTable table_check_stage(const BlockTable &t, uint64_t nentries, uint64_t bytes, uint32_t block_size, redux_block *copy,
                                      uint32_t *seen, uint32_t *sizes, int32_t *status, hipStream_t s)
{
    TableCheckArgs ta;
    ta.in         = t.entries;
    ta.out        = copy;
    ta.nentries   = nentries;
    ta.nblocks    = t.nblocks;
    ta.bytes      = bytes;
    ta.block_size = block_size;
    ta.aligned16  = t.aligned16 ? 1u : 0u;
    ta.seen       = seen;
    ta.sizes      = sizes;
    ta.status     = status;
    const uint64_t n0 = std::max(t.nblocks, table_seen_words(t.nblocks));
    k_table_prepare<<<(uint32_t)((n0 + 255) / 256), 256, 0, s>>>(ta);
    k_table_check<<<(uint32_t)((nentries + 255) / 256), 256, 0, s>>>(ta);
    return {copy, seen + table_seen_words(t.nblocks) - 1};
}

// The small-grid encoder (redux_coop.hpp): a block's model by 64 lanes, its chain by one.  a: the launch's arguments as for
// the full-grid kernels; longest: the longest block of the launch.  The instances, by [code_bits 32][fix-up]([linear slots]):
typedef void (*CoopChainFn)(EncArgs, const uint2 *);
typedef void (*CoopStepFn)(EncArgs, EncArgs, const uint2 *, uint2 *, uint32_t);
static constexpr CoopChainFn kCoopChain[2][2] = {{k_coop_chain<false, false>, k_coop_chain<false, true>},
                                                 {k_coop_chain<true, false>, k_coop_chain<true, true>}};
static constexpr CoopChainFn kCoopLastChain[2][2][2] = {
    {{k_coop_chain<false, false, false, true>, k_coop_chain<false, false, true, true>},
     {k_coop_chain<false, true, false, true>, k_coop_chain<false, true, true, true>}},
    {{k_coop_chain<true, false, false, true>, k_coop_chain<true, false, true, true>},
     {k_coop_chain<true, true, false, true>, k_coop_chain<true, true, true, true>}}};
static constexpr CoopStepFn kCoopStep[2][2][2] = {
    {{k_coop_step<false, false, false>, k_coop_step<false, false, true>}, {k_coop_step<false, true, false>, k_coop_step<false, true, true>}},
    {{k_coop_step<true, false, false>, k_coop_step<true, false, true>}, {k_coop_step<true, true, false>, k_coop_step<true, true, true>}}};

static void launch_coop(const Geometry &g, EncArgs a, bool cb32, uint64_t longest, uint8_t *ws, hipStream_t s)
{
    uint2         *pairs = (uint2 *)(ws + g.off_pairs);
    const uint32_t cgrid = (uint32_t)((g.nblocks + 63) / 64);
    {
        const double r = 1.0 / (double)(257ull + g.nfreeze); // the frozen model's reciprocal, biased as k_fill_rc's
        uint64_t     u;
        memcpy(&u, &r, 8);
        u += 4;
        memcpy(&a.rc_frozen, &u, 8);
    }
    a.winlen = g.coop_win;
    a.cstate = !g.u16 ? (uint32_t *)(ws + g.off_cstate) : nullptr;
    a.cbase  = a.cstate ? a.cstate + g.nblocks * 8 : nullptr;
    if (g.u16) { // whole blocks
        k_coop_model<false><<<(uint32_t)g.nblocks, 64, 0, s>>>(a, pairs);
        const CoopChainFn chain = kCoopChain[cb32][g.fixup];
        chain<<<cgrid, 128, 0, s>>>(a, pairs);
        return;
    }
    // Blocks above 64 KiB, window by window.  Window w's chain runs in ONE launch with window w + 1's model (k_coop_step):
    // two pairs buffers and two reciprocal tables, alternating.  The longest block of the launch decides the number of
    // windows: its EOF symbol (symbol number `length`) is the last one coded.
    const uint32_t rc_half   = g.rc_n / 2;
    const uint64_t pair_half = g.nblocks * coop_block_pitch(g.coop_win);
    double        *rcs[2]    = {(double *)(ws + g.off_rc), (double *)(ws + g.off_rc) + rc_half};
    uint2         *prs[2]    = {pairs, pairs + pair_half};
    const CoopStepFn  step = kCoopStep[cb32][g.fixup][g.coop_linear];
    const CoopChainFn last = kCoopLastChain[cb32][g.fixup][g.coop_linear];
    k_coop_model<true><<<(uint32_t)g.nblocks, 64, 0, s>>>(a, prs[0]); // (win0 = 0)
    for (uint32_t w = 0; w < g.coop_nwin && (uint64_t)w * g.coop_win <= longest; w++) {
        EncArgs ac = a, am = a;
        ac.win0 = w * g.coop_win;
        ac.rc   = rcs[w & 1];
        am.win0 = (w + 1) * g.coop_win;
        // (the table of the first window was filled by the caller, as k_fill_rc fills it, in the first half)
        if (w)
            k_fill_rc_from<<<(rc_half + 255) / 256, 256, 0, s>>>(rcs[w & 1], rc_half, 257u + ac.win0);
        const bool more = w + 1 < g.coop_nwin && (uint64_t)am.win0 <= longest; // (a window that only holds EOF symbols has no model)
        if (more)
            step<<<cgrid + (uint32_t)g.nblocks, 128, 0, s>>>(ac, am, prs[w & 1], prs[(w + 1) & 1], cgrid);
        else
            last<<<cgrid, 128, 0, s>>>(ac, prs[w & 1]);
    }
}

// The coder stage of a call planned as g: the blocks' streams into the slots of the workspace.  t: the table form (in_len is
// then the bytes of d_in); a caller's table is checked here, and *checked says where its copy and the check's verdict are.
static int encode_slots_impl(const Geometry &g, const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                             const BlockTable &t, void *d_block_status, void *d_workspace, uint64_t workspace_bytes, void *stream,
                             CheckedTable *checked)
{
    if (!d_workspace || !d_block_status || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    if (t.entries && (g.gen || g.any || in_len > 0xFFFFFFFFull)) // lane offsets into d_in are 32-bit
        return REDUX_UNSUPPORTED;
    if (workspace_bytes < g.total)
        return REDUX_OUTPUT_TOO_SMALL;
    if (((uintptr_t)d_workspace) & 255)
        return REDUX_INVALID_INPUT;
    hipStream_t s  = (hipStream_t)stream;
    uint8_t    *ws = (uint8_t *)d_workspace;

    const redux_block *table = t.entries;
    if (table && !t.trusted) {
        *checked = table_check_stage(t, g.nblocks, in_len, block_size, (redux_block *)(ws + g.off_table), (uint32_t *)(ws + g.off_seen),
                                     (uint32_t *)(ws + g.off_sizes), (int32_t *)d_block_status, s);
        table    = checked->entries;
    }
    HIP_TRY(hipMemsetAsync(ws + g.off_mode, 0, 256 + kClaimWords * 4, s)); // linear slots unless the pair kernel runs (below); empty role book
    const EncCore core = enc_core(g, d_in, in_len, ws, d_block_status);
    if (g.gen) {
        GenEncArgs ga;
        static_cast<EncCore &>(ga) = core;
        ga.rc         = (const double *)(ws + g.off_rc);
        ga.block_size = block_size;
        ga.slot_cap   = g.slot_cap;
        ga.nfreeze    = g.nfreeze;
        ga.code_bits  = p->code_bits;
        // (64 slots / blocks within a 32-bit lane offset: geometry())
        k_fill_rc_from<<<(g.rc_n + 255) / 256, 256, 0, s>>>((double *)(ws + g.off_rc), g.rc_n, (1u << p->symbol_bits) + 1u);
        const uint32_t grid64 = (uint32_t)((g.nblocks + 63) / 64);
        switch (p->symbol_bits) {
#define REDUX_GEN_ENC(SB) case SB: k_encode_gen<SB><<<grid64, 64, 0, s>>>(ga); break;
#define REDUX_GEN_ENC_PAIR(SB)                                                                                         \
    case SB: k_encode_gen_pair<SB><<<(uint32_t)((g.nblocks + GenTree<SB>::kBlocks - 1) / GenTree<SB>::kBlocks), 256, 0, s>>>(ga); break;
            REDUX_GEN_ENC(1) REDUX_GEN_ENC(2) REDUX_GEN_ENC(3) REDUX_GEN_ENC(4) REDUX_GEN_ENC(5) REDUX_GEN_ENC(6) REDUX_GEN_ENC(7)
            REDUX_GEN_ENC_PAIR(9) REDUX_GEN_ENC_PAIR(10) REDUX_GEN_ENC_PAIR(11) REDUX_GEN_ENC_PAIR(12)
#undef REDUX_GEN_ENC
#undef REDUX_GEN_ENC_PAIR
        default: return REDUX_UNSUPPORTED;
        }
        HIP_TRY(hipGetLastError());
        return REDUX_OK;
    }
    if (g.any) {
        AnyEncArgs aa;
        static_cast<EncCore &>(aa) = core;
        aa.trees      = (uint32_t *)(ws + g.off_trees);
        aa.tree_words = g.tree_bytes / 4;
        aa.block_size = block_size;
        aa.slot_cap   = g.slot_cap;
        aa.sb = p->symbol_bits; aa.fb = p->freq_bits; aa.cb = p->code_bits;
        k_encode_any<<<(uint32_t)((g.nblocks + 63) / 64), 64, 0, s>>>(aa);
        HIP_TRY(hipGetLastError());
        return REDUX_OK;
    }

    k_fill_rc<<<(g.rc_n + 255) / 256, 256, 0, s>>>((double *)(ws + g.off_rc), g.rc_n);

    EncArgs a;
    static_cast<EncCore &>(a) = core;
    a.rc         = (const double *)(ws + g.off_rc);
    a.block_size = block_size;
    a.slot_cap   = g.slot_cap;
    a.nfreeze    = g.nfreeze;
    a.code_bits  = p->code_bits;
    a.aligned16  = ((((uintptr_t)d_in) & 15) == 0 && (table ? t.aligned16 : (block_size & 15) == 0)) ? 1 : 0;
    a.claims     = (uint32_t *)(ws + g.off_mode + 256);
    a.table      = table;
    a.pair_width = g.pair_width;
    a.win0 = 0; a.winlen = block_size + 1; a.rc_frozen = 0.0; a.cstate = nullptr; a.cbase = nullptr;
    // 64 blocks per wave while 64 slots / 64 blocks stay within a 32-bit lane offset;
    // otherwise (giant blocks, whole-stream mode) one block per wave.
    a.lanes = encode_lanes(g, block_size);
    const uint32_t grid = (uint32_t)((g.nblocks + a.lanes - 1) / a.lanes);
    const EncKernel which = pick_encode_kernel(g, p, a.aligned16 != 0, block_size);
    const bool      coop  = which == EncKernel::CoopCb32 || which == EncKernel::Coop;
    // what the pair kernel leaves in the slots (CompactArgs::mode): byte 0x01 -> row-major group
    // areas, 0x02 -> linear slots whose dwords are byte-reversed
    if (which == EncKernel::PairCb32 || which == EncKernel::Pair || coop)
        HIP_TRY(hipMemsetAsync(ws + g.off_mode, g.coop_linear ? 2 : (1 | 2), 4, s));
    switch (which) {
    case EncKernel::CoopCb32:
    case EncKernel::Coop:
        launch_coop(g, a, which == EncKernel::CoopCb32, table ? block_size : (in_len < block_size ? in_len : block_size), ws, s);
        break;
    case EncKernel::PairCb32: k_encode_pair<false, true><<<grid, 128, 0, s>>>(a); break;
    case EncKernel::Pair: k_encode_pair<false, false><<<grid, 128, 0, s>>>(a); break;
    case EncKernel::SingleU16: k_encode<true, false><<<grid, 64, 0, s>>>(a); break;
    case EncKernel::SingleU32: k_encode<false, true><<<grid, 64, 0, s>>>(a); break;
    case EncKernel::Gen:
    case EncKernel::GenPair:
    case EncKernel::Any: break; // handled above
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_encode_slots_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                           void *d_block_status, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    Geometry  g;
    const int st = encode_plan(p, in_len, block_size, workspace_bytes, g);
    if (st != REDUX_OK)
        return st;
    return encode_slots_impl(g, p, d_in, in_len, block_size, BlockTable{}, d_block_status, d_workspace, workspace_bytes, stream, nullptr);
}

// The tile height k_compact_rows runs at (redux_pack.hpp): the tall tile where a group area is at least four of them tall,
// the 64-row tile below that, so that small launches keep their workgroups.  redux_debug_compact_tile_rows dictates it.
static std::atomic<uint32_t> g_compact_tile_rows{0};
static uint32_t compact_tile_rows(uint32_t cap_rows)
{
    const uint32_t forced = g_compact_tile_rows.load(std::memory_order_relaxed);
    if (forced)
        return forced;
    return cap_rows >= 4 * kTallTileRows ? kTallTileRows : kTileRows;
}

// Diagnostic (tests only): every later row gather of this process runs k_compact_rows at this tile height (64 or 256);
// 0 gives the choice back to the launch code.
int redux_debug_compact_tile_rows(uint32_t rows)
{
    if (rows != 0 && rows != kTileRows && rows != kTallTileRows)
        return REDUX_INVALID_INPUT;
    g_compact_tile_rows.store(rows, std::memory_order_relaxed);
    return REDUX_OK;
}

// The compaction stage: scan + gather of the slots a coder kernel left in the workspace laid out by g.  t: the (checked) table
// the coder ran on; raw: the stored blocks' bytes.
static int compact_with(const Geometry &g, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status,
                        void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream, const BlockTable &t,
                        const RawCopy &raw)
{
    if (!d_workspace || !d_block_status || !d_out_offsets || !d_out)
        return REDUX_INVALID_INPUT;
    if (workspace_bytes < g.off_pairs) // (the compaction reads nothing behind the slots and trees: a workspace without the pairs area will do)
        return REDUX_OUTPUT_TOO_SMALL;
    hipStream_t s  = (hipStream_t)stream;
    uint8_t    *ws = (uint8_t *)d_workspace;

    ScanArgs sa;
    sa.sizes   = (const uint32_t *)(ws + g.off_sizes);
    sa.status  = (const int32_t *)d_block_status;
    sa.offsets = (uint64_t *)d_out_offsets;
    sa.summary = (int32_t *)d_summary;
    sa.nblocks = t.entries ? t.nblocks : g.nblocks; // (g counts slots = table entries; sizes and status are per block)
    if (scan_is_coalesced(sa))
        k_scan_sizes_coalesced<<<1, 1024, 0, s>>>(sa);
    else
        k_scan_sizes<<<1, 1024, 0, s>>>(sa);

    CompactArgs ca;
    ca.slots      = ws + g.off_slots;
    ca.slot_bytes = g.slot_bytes;
    ca.offsets    = (const uint64_t *)d_out_offsets;
    ca.out        = (uint8_t *)d_out;
    ca.out_cap    = out_cap;
    ca.status     = (int32_t *)d_block_status;
    ca.summary    = (int32_t *)d_summary;
    ca.nblocks    = g.nblocks;
    ca.mode       = (const uint32_t *)(ws + g.off_mode);
    ca.cap_rows   = (uint32_t)(g.slot_bytes / 4);
    ca.table      = t.entries;
    ca.stored     = raw.stored;
    ca.raw        = (const uint8_t *)raw.raw;
    ca.block_size = raw.block_size;
    k_compact<<<(uint32_t)g.nblocks, 256, 0, s>>>(ca);
    if (!g.any && !g.gen && (g.u16 || g.coop)) { // (every launch that may have left row-major group areas: the kernel reads the mode word)
        const uint32_t rows   = compact_tile_rows(ca.cap_rows);
        const uint32_t sets   = (uint32_t)((g.nblocks + 63) / 64 + 7) / 8 * 8; // (whole sets of 8 groups: k_compact_rows' XCD-aware mapping)
        if (rows == kTallTileRows)
            k_compact_rows<kTallTileRows><<<sets * compact_tiles(ca.cap_rows, kTallTileRows), 256, 0, s>>>(ca);
        else
            k_compact_rows<kTileRows><<<sets * compact_tiles(ca.cap_rows, kTileRows), 256, 0, s>>>(ca);
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_compact_slots_dev(const redux_params *p, uint64_t in_len, uint32_t block_size, void *d_out,
                            uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    Geometry  g;
    const int st = encode_plan(p, in_len, block_size, workspace_bytes, g);
    if (st != REDUX_OK)
        return st;
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream, BlockTable{},
                        RawCopy{});
}

int redux_encode_blocks_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size,
                            void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status,
                            void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    Geometry g;
    int      st = encode_plan(p, in_len, block_size, workspace_bytes, g);
    if (st != REDUX_OK)
        return st;
    st = encode_slots_impl(g, p, d_in, in_len, block_size, BlockTable{}, d_block_status, d_workspace, workspace_bytes, stream, nullptr);
    if (st != REDUX_OK)
        return st;
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream, BlockTable{},
                        RawCopy{});
}

int redux_encode_blocks_v_dev(const redux_params *p, const void *d_in, uint64_t in_bytes, const void *d_table,
                              uint64_t nentries, uint64_t nblocks, uint32_t block_size, uint32_t flags, void *d_out,
                              uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                              uint64_t workspace_bytes, void *stream)
{
    if (!d_table || nblocks == 0 || nentries < nblocks)
        return REDUX_INVALID_INPUT;
    if (nentries > 0xFFFFFFF0ull || nblocks > 0xFFFFFFF0ull || !d_block_status || !d_workspace)
        return REDUX_INVALID_INPUT;
    Geometry g;
    int      st = encode_plan(p, nentries * (uint64_t)block_size, block_size, workspace_bytes, g);
    if (st != REDUX_OK)
        return st;
    const BlockTable given = {(const redux_block *)d_table, (flags & REDUX_V_ALIGNED16) != 0, nblocks, false};
    CheckedTable     checked;
    st = encode_slots_impl(g, p, d_in, in_bytes, block_size, given, d_block_status, d_workspace, workspace_bytes, stream, &checked);
    if (st != REDUX_OK)
        return st;
    st = compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream,
                      BlockTable{checked.entries, given.aligned16, nblocks, true}, RawCopy{});
    if (st != REDUX_OK)
        return st;
    k_table_verdict<<<1, 1, 0, (hipStream_t)stream>>>(checked.failed, (int32_t *)d_summary);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

uint64_t redux_block_count_v(const uint64_t *in_len, uint64_t ninputs, uint32_t block_size)
{
    if (block_size == 0 || (ninputs && !in_len))
        return 0;
    uint64_t n = 0;
    for (uint64_t i = 0; i < ninputs; i++)
        n += redux_block_count(in_len[i], block_size);
    return n;
}

uint64_t redux_block_table_v(const uint64_t *in_off, const uint64_t *in_len, uint64_t ninputs, uint32_t block_size,
                             redux_block *table)
{
    const uint64_t nb = redux_block_count_v(in_len, ninputs, block_size);
    if (nb == 0 || nb > 0xFFFFFFF0ull || !in_off)
        return 0;
    // whole blocks first, in block order; then the short ones (at most one per input), longest first
    std::vector<redux_block> whole, tails;
    uint64_t b = 0;
    for (uint64_t i = 0; i < ninputs; i++) {
        const uint64_t cnt = redux_block_count(in_len[i], block_size);
        for (uint64_t j = 0; j < cnt; j++, b++) {
            const uint64_t o   = j * (uint64_t)block_size;
            const uint64_t rem = in_len[i] - o;
            redux_block    e;
            e.offset = in_off[i] + o;
            e.length = rem < block_size ? (uint32_t)rem : block_size;
            e.index  = (uint32_t)b;
            (e.length == block_size ? whole : tails).push_back(e);
        }
    }
    std::stable_sort(tails.begin(), tails.end(), [](const redux_block &x, const redux_block &y) { return x.length > y.length; });
    // a new wave wherever the length has dropped by an eighth (small blocks: by 512 bytes) since the wave's first entry
    std::vector<redux_block> t(whole);
    const redux_block idle = {0, 0, REDUX_BLOCK_IDLE};
    uint32_t first_len = block_size;
    for (const redux_block &e : tails) {
        const uint32_t slack = first_len / 8 > 512 ? first_len / 8 : 512;
        if (t.size() % 64 == 0)
            first_len = e.length;
        else if (e.length + slack < first_len) {
            while (t.size() % 64)
                t.push_back(idle);
            first_len = e.length;
        }
        t.push_back(e);
    }
    if (table)
        memcpy(table, t.data(), t.size() * sizeof(redux_block));
    return t.size();
}

int redux_encode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_off, const uint64_t *in_len,
                          uint64_t ninputs, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                          int32_t *block_status)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || ninputs == 0 || !in_off || !in_len || !out || !out_offsets)
        return REDUX_INVALID_INPUT;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    return host::encode_blocks_v(p, in, in_off, in_len, ninputs, block_size, out, out_cap, out_offsets, block_status);
}

int redux_encode_blocks_crc(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status, adaptive_encoder(p, block_size),
                               block_crc); // redux_host.hpp
}

int redux_encode_blocks(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                        uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status)
{
    return redux_encode_blocks_crc(p, in, in_len, block_size, out, out_cap, out_offsets, block_status, nullptr);
}

int redux_compress(const redux_params *p, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                   uint64_t *bytes_in, uint64_t *bytes_out) /* src/lib.rs:102-109 */
{
    if (in_len > 0xFFFFFF00ull)
        return REDUX_UNSUPPORTED;
    uint64_t  offs[2] = {0, 0};
    int32_t   st      = 0;
    const int rc = redux_encode_blocks(p, in, in_len, in_len ? (uint32_t)in_len : 1u, out, out_cap, offs, &st);
    if (rc == REDUX_OK) {
        if (bytes_in)
            *bytes_in = in_len;
        if (bytes_out)
            *bytes_out = offs[1];
    }
    return rc;
}

uint64_t redux_decode_workspace_bytes(const redux_params *p, uint64_t nblocks, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || block_size == 0)
        return 0;
    return decode_layout(decode_geometry(p, block_size), p, nblocks, block_size, false).total;
}

// The decoders.  t: the table form (nblocks counts its entries, out_cap the bytes of d_out they may name); d_in_used (optional,
// u64[nblocks]): bytes of each stream the reader fetched; only redux_decompress asks for it (the (u64, u64) of src/lib.rs:119)
static int decode_blocks_dev_impl(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t nblocks,
                                  uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_sizes,
                                  void *d_block_status, void *d_summary, void *d_workspace,
                                  uint64_t workspace_bytes, void *stream, void *d_in_used, const BlockTable &t)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_in_offsets || !d_out_sizes || !d_block_status || !d_workspace)
        return REDUX_INVALID_INPUT;
    if (nblocks == 0)
        return REDUX_OK;
    if (!t.entries && out_cap < nblocks * (uint64_t)block_size)
        return REDUX_OUTPUT_TOO_SMALL;
    const Geometry     g = decode_geometry(p, block_size);
    const DecodeLayout L = decode_layout(g, p, nblocks, block_size, t.entries != nullptr);
    if (workspace_bytes < L.total)
        return REDUX_OUTPUT_TOO_SMALL;
    if (t.entries && (g.gen || g.any))
        return REDUX_UNSUPPORTED;
    hipStream_t    s      = (hipStream_t)stream;
    uint8_t       *ws     = (uint8_t *)d_workspace;
    const DecCore  core   = dec_core(d_in, d_in_offsets, nblocks, d_out, d_out_sizes, d_block_status);
    const uint32_t grid64 = (uint32_t)((nblocks + 63) / 64);
    CheckedTable   table  = {t.entries, nullptr};

    GenDecArgs ga; // the cell decoders, of every width
    static_cast<DecCore &>(ga) = core;
    ga.rc         = (const double *)ws;
    ga.trees      = g.gen ? (uint32_t *)(ws + L.off_trees) : nullptr;
    ga.in_used    = (uint64_t *)d_in_used;
    ga.block_size = block_size;
    ga.nfreeze    = g.nfreeze;
    ga.code_bits  = p->code_bits;
    if (g.gen)
        k_fill_rc_from<<<(L.rc_n + 255) / 256, 256, 0, s>>>((double *)ws, L.rc_n, (1u << p->symbol_bits) + 1u);
    else if (!g.any)
        k_fill_rc<<<(L.rc_n + 255) / 256, 256, 0, s>>>((double *)ws, L.rc_n);

    switch (L.kernel) {
    case DecKernel::CellsFixup:
        switch (p->symbol_bits) {
#define REDUX_GEN_DEC(SB) case SB: k_decode_cells<SB, 64, false, true><<<grid64, 64, 0, s>>>(ga); break;
            REDUX_GEN_DEC(1) REDUX_GEN_DEC(2) REDUX_GEN_DEC(3) REDUX_GEN_DEC(4) REDUX_GEN_DEC(5) REDUX_GEN_DEC(6) REDUX_GEN_DEC(7)
#undef REDUX_GEN_DEC
        default: return REDUX_UNSUPPORTED;
        }
        break;
    case DecKernel::CellsWorkspace: {
        // every tree starts at all-ones frequencies: a node = its lowbit
        const uint64_t npieces = (uint64_t)grid64 * 64 * gen_decode_tree_bytes(p) / 16;
        k_fill_cells16<<<(uint32_t)((npieces + 255) / 256), 256, 0, s>>>((cl_u32x4 *)ga.trees, npieces);
        if (p->symbol_bits == 11)
            k_decode_cells<11, 64, true><<<grid64, 64, 0, s>>>(ga);
        else
            k_decode_cells<12, 64, true><<<grid64, 64, 0, s>>>(ga);
        break;
    }
    case DecKernel::Cells:
        switch (p->symbol_bits) {
#define REDUX_GEN_DEC(SB) case SB: k_decode_cells<SB, 64, false><<<grid64, 64, 0, s>>>(ga); break;
            REDUX_GEN_DEC(1) REDUX_GEN_DEC(2) REDUX_GEN_DEC(3) REDUX_GEN_DEC(4) REDUX_GEN_DEC(5) REDUX_GEN_DEC(6) REDUX_GEN_DEC(7)
            REDUX_GEN_DEC(9) REDUX_GEN_DEC(10)
#undef REDUX_GEN_DEC
        default: return REDUX_UNSUPPORTED;
        }
        break;
    case DecKernel::Cells8: k_decode_cells<8, 64, false, false><<<grid64, 64, 0, s>>>(ga); break;
    case DecKernel::Cells8Fixup: k_decode_cells<8, 64, false, true><<<grid64, 64, 0, s>>>(ga); break;
    case DecKernel::Any: {
        AnyDecArgs aa;
        static_cast<DecCore &>(aa) = core;
        aa.in_used    = (uint64_t *)d_in_used;
        aa.trees      = (uint32_t *)ws;
        aa.tree_words = g.tree_bytes / 4;
        aa.block_size = block_size;
        aa.sb = p->symbol_bits; aa.fb = p->freq_bits; aa.cb = p->code_bits;
        k_decode_any<<<grid64, 64, 0, s>>>(aa);
        break;
    }
    default: { // the decoders of 8-bit symbols that take a block table
        if (table.entries && !t.trusted)
            table = table_check_stage(t, nblocks, out_cap, block_size, (redux_block *)(ws + L.off_table), (uint32_t *)(ws + L.off_seen),
                                      (uint32_t *)d_out_sizes, (int32_t *)d_block_status, s);
        DecArgs a;
        static_cast<DecCore &>(a) = core;
        a.rc         = (const double *)ws;
        a.block_size = block_size;
        a.nfreeze    = g.nfreeze;
        a.code_bits  = p->code_bits;
        a.aligned4   = ((((uintptr_t)d_out) & 3) == 0 && (block_size & 3) == 0) ? 1 : 0;
        if (a.aligned4 && (((uintptr_t)d_out) & 15) == 0 && (block_size & 15) == 0)
            a.aligned4 = 2; // 16-byte aligned blocks: the lock-step decoder stages four dwords per store
        if (table.entries) // where a block starts is the table's business: all of them 16-byte aligned, or nothing is assumed
            a.aligned4 = (t.aligned16 && (((uintptr_t)d_out) & 15) == 0) ? 2 : 0;
        a.in_used    = (uint64_t *)d_in_used;
        a.table      = table.entries;
        a.rc_n       = L.rc_n - 32; // (the last 32 entries are slack for the lock-step decoder's look-ahead)
        switch (L.kernel) {
        case DecKernel::Wave: k_decode_wave<false><<<(uint32_t)nblocks, 64, 0, s>>>(a); break;
        case DecKernel::WaveFixup: k_decode_wave<true><<<(uint32_t)nblocks, 64, 0, s>>>(a); break;
        case DecKernel::LockCb32: k_decode_lock<true><<<grid64, 64, 0, s>>>(a); break;
        case DecKernel::Lock: k_decode_lock<false><<<grid64, 64, 0, s>>>(a); break;
        case DecKernel::GenericU16: k_decode<true, false><<<grid64, 64, 0, s>>>(a); break;
        default: k_decode<false, true><<<grid64, 64, 0, s>>>(a); break; // (GenericU32)
        }
    }
    }
    if (d_summary) // (with a block table nblocks counts its entries: statuses are per block)
        k_summarize<<<64, 256, 0, s>>>((const int32_t *)d_block_status, table.entries ? t.nblocks : nblocks, (int32_t *)d_summary);
    if (table.failed)
        k_table_verdict<<<1, 1, 0, s>>>(table.failed, (int32_t *)d_summary);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// Diagnostic (tests only): where the encoder's per-CU role book sits in the workspace.
int redux_debug_role_book(const redux_params *p, uint64_t in_len, uint32_t block_size, uint64_t *offset, uint64_t *bytes)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !offset || !bytes)
        return REDUX_INVALID_INPUT;
    const Geometry g = geometry(p, in_len, block_size);
    *offset          = g.off_mode + 256;
    *bytes           = kClaimWords * 4;
    return REDUX_OK;
}

// Diagnostic (tests only): max |v_rcp_f64(x) * x - 1| over the integers lo..hi, on the device.
int redux_debug_rcp_check(uint64_t lo, uint64_t hi, double *max_err)
{
    unsigned long long *d = nullptr, h = 0;
    HIP_TRY(hipMalloc(&d, 8));
    HIP_TRY(hipMemset(d, 0, 8));
    k_rcp_check<<<4096, 256>>>(lo, hi, d);
    HIP_TRY(hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipFree(d));
    memcpy(max_err, &h, 8);
    return REDUX_OK;
}

int redux_decode_blocks_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t nblocks,
                            uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_sizes,
                            void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes,
                            void *stream)
{
    return decode_blocks_dev_impl(p, d_in, d_in_offsets, nblocks, block_size, d_out, out_cap, d_out_sizes,
                                  d_block_status, d_summary, d_workspace, workspace_bytes, stream, nullptr, BlockTable{});
}

int redux_decode_blocks_v_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_table,
                              uint64_t nentries, uint64_t nblocks, uint32_t block_size, uint32_t flags, void *d_out,
                              uint64_t out_bytes, void *d_out_sizes, void *d_block_status, void *d_summary, void *d_workspace,
                              uint64_t workspace_bytes, void *stream)
{
    if (!d_table || nblocks == 0 || nentries < nblocks || !d_out || nentries > 0xFFFFFFF0ull)
        return REDUX_INVALID_INPUT;
    return decode_blocks_dev_impl(p, d_in, d_in_offsets, nentries, block_size, d_out, out_bytes, d_out_sizes, d_block_status,
                                  d_summary, d_workspace, workspace_bytes, stream, nullptr,
                                  BlockTable{(const redux_block *)d_table, (flags & REDUX_V_ALIGNED16) != 0, nblocks, false});
}

int redux_decode_blocks_v(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint8_t *out,
                          const uint64_t *out_off, const uint64_t *out_len, uint64_t ninputs, uint32_t block_size,
                          uint32_t *out_sizes, int32_t *block_status)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || ninputs == 0 || !in_offsets || !out_off || !out_len || !out_sizes)
        return REDUX_INVALID_INPUT;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    return host::decode_blocks_v(p, in, in_offsets, out, out_off, out_len, ninputs, block_size, out_sizes, block_status);
}

// the decoders of the chunked host calls (redux_host.hpp: DecodeCoder)
static host::DecodeCoder adaptive_decoder(const redux_params *p, uint32_t block_size)
{
    return {[=](uint64_t cb) { return redux_decode_workspace_bytes(p, cb, block_size); },
            [=](host::Slot &s, uint64_t nb, uint64_t out_bytes, void *d_in_used, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return decode_blocks_dev_impl(p, s.d_in.p, s.d_off.p, nb, block_size, s.d_out.p, out_bytes, s.d_sz.p, s.d_st.p,
                                              s.d_sum.p, ws, ws_bytes, st, d_in_used, BlockTable{});
            }};
}

// the static decoder takes no workspace
static host::DecodeCoder static_decoder(const redux_params *p, const uint32_t *cum, uint32_t block_size)
{
    return {[](uint64_t) { return (uint64_t)0; },
            [=](host::Slot &s, uint64_t nb, uint64_t out_bytes, void *, void *, uint64_t, hipStream_t st) {
                return redux_static_decode_blocks_dev(p, cum, s.d_in.p, s.d_off.p, nb, block_size, s.d_out.p, out_bytes, s.d_sz.p,
                                                      s.d_st.p, s.d_sum.p, st);
            }};
}

// The host-pointer decoders: `params` is the status of the entry's own parameter checks, then the checks they share.  The
// blocks decode to out_len bytes (nblocks * block_size, or exactly out_len in the planes layout) in out[0 .. out_cap).
static int decode_blocks_host(int params, const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks, uint32_t block_size,
                              uint8_t *out, uint64_t out_len, uint64_t out_cap, uint32_t *out_sizes, int32_t *block_status,
                              uint64_t *in_used, const host::DecodeCoder &coder, uint32_t *block_crc = nullptr,
                              const uint8_t *stored = nullptr, host::SegmentTablesIo tables = {}, host::BaseIo base = {},
                              host::UnitTableIo units = {}, uint32_t frame_blocks = 1)
{
    if (params != REDUX_OK)
        return params;
    if (block_size == 0 || !in_offsets || !out_sizes || (out_len && !out))
        return REDUX_INVALID_INPUT;
    if (nblocks == 0)
        return REDUX_OK;
    if (out_cap < out_len)
        return REDUX_OUTPUT_TOO_SMALL;
    if (in_offsets[nblocks] && !in)
        return REDUX_INVALID_INPUT;
    return host::decode_blocks(in, in_offsets, nblocks, block_size, out, out_len, out_sizes, block_status, in_used, coder,
                               block_crc, stored, tables, base, units, frame_blocks); // redux_host.hpp
}

int redux_decode_blocks_crc(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks,
                            uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                            int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_host(check_params(p), in, in_offsets, nblocks, block_size, out, nblocks * (uint64_t)block_size, out_cap,
                              out_sizes, block_status, nullptr, adaptive_decoder(p, block_size), block_crc);
}

int redux_decode_blocks(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t nblocks,
                        uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                        int32_t *block_status)
{
    return redux_decode_blocks_crc(p, in, in_offsets, nblocks, block_size, out, out_cap, out_sizes, block_status, nullptr);
}

int redux_decompress(const redux_params *p, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap,
                     uint64_t *bytes_in, uint64_t *bytes_out) /* src/lib.rs:113-120 */
{
    if (out_cap == 0 || out_cap > 0xFFFFFF00ull)
        out_cap = out_cap ? 0xFFFFFF00ull : 1;
    uint64_t  offs[2] = {0, in_len};
    uint32_t  sz      = 0;
    int32_t   st      = 0;
    uint64_t  used    = 0;
    const int rc = decode_blocks_host(check_params(p), in, offs, 1, (uint32_t)out_cap, out, out_cap, out_cap, &sz, &st, &used,
                                      adaptive_decoder(p, (uint32_t)out_cap));
    if (rc == REDUX_OK) {
        if (bytes_out)
            *bytes_out = sz;
        // input.get_count() (lib.rs:119): the bytes the BitReader fetched -- the decoder reads
        // exactly the bits the encoder wrote, so trailing bytes after the stream are not counted
        if (bytes_in)
            *bytes_in = used;
    }
    return rc;
}

// ---- static-table model (redux_static.hpp) ----------------------------
static int static_check(const redux_params *p, const uint32_t *cum)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p)) // 8-bit symbols, code_bits <= 32: the widths the fast coder core covers
        return REDUX_UNSUPPORTED;
    if (!cum || cum[0] != 0)
        return REDUX_INVALID_INPUT;
    for (uint32_t i = 0; i + 1 < kStaticEntries; i++)
        if (cum[i + 1] <= cum[i]) // every symbol, EOF included, must be codable
            return REDUX_INVALID_INPUT;
    if ((uint64_t)cum[kStaticEntries - 1] > (1ull << p->freq_bits) - 1) // total <= freq_max (model/mod.rs)
        return REDUX_INVALID_INPUT;
    return REDUX_OK;
}

// which static kernel a call runs: ONE decision, used by the launch code and reported by
// redux_static_encode_kernel_name / redux_static_decode_kernel_name.  "solo": at most one wave per SIMD
enum class StaticEncKernel { Fixup, Cb32Solo, Cb32, Narrow };
enum class StaticDecKernel { Fixup, LutCb32Solo, LutSolo, LutCb32, Lut, LockCb32Solo, LockCb32, LockSolo, Lock };

static bool static_solo(uint64_t nblocks) { return (nblocks + 63) / 64 <= 4ull * cu_count(); }

static StaticEncKernel pick_static_encode_kernel(const redux_params *p, uint32_t total, uint64_t nblocks)
{
    if (total >= (1u << 17))
        return StaticEncKernel::Fixup;
    if (p->code_bits == 32)
        return static_solo(nblocks) ? StaticEncKernel::Cb32Solo : StaticEncKernel::Cb32;
    return StaticEncKernel::Narrow;
}

static StaticDecKernel pick_static_decode_kernel(const redux_params *p, uint32_t total, uint64_t nblocks)
{
    if (total >= (1u << 17))
        return StaticDecKernel::Fixup;
    const bool solo = static_solo(nblocks), cb32 = p->code_bits == 32;
    if (total <= 65536u) // get_symbol by direct lookup
        return solo ? (cb32 ? StaticDecKernel::LutCb32Solo : StaticDecKernel::LutSolo) : (cb32 ? StaticDecKernel::LutCb32 : StaticDecKernel::Lut);
    return solo ? (cb32 ? StaticDecKernel::LockCb32Solo : StaticDecKernel::LockSolo) : (cb32 ? StaticDecKernel::LockCb32 : StaticDecKernel::Lock);
}

// 64 slots / blocks of one wave, E apart (E = 1: the one-table and context-static coders), within a 32-bit lane offset
static bool static_lanes_fit(const Geometry &g, uint32_t block_size, uint32_t E)
{
    return 64ull * E * g.slot_bytes < (1ull << 32) && 64ull * E * block_size < (1ull << 32);
}

const char *redux_static_encode_kernel_name(const redux_params *p, const uint32_t *cum, uint64_t in_len, uint32_t block_size)
{
    if (static_check(p, cum) != REDUX_OK || block_size == 0)
        return "";
    const Geometry g = geometry(p, in_len, block_size, true);
    if (!static_lanes_fit(g, block_size, 1)) // as redux_static_encode_blocks_dev
        return "";
    switch (pick_static_encode_kernel(p, cum[kStaticEntries - 1], g.nblocks)) {
    case StaticEncKernel::Fixup: return "k_encode_static<true, false> (total >= 2^17: quotient fix-up)";
    case StaticEncKernel::Cb32Solo: return "k_encode_static<false, true, true> (code_bits 32, one wave per SIMD)";
    case StaticEncKernel::Cb32: return "k_encode_static<false, true> (code_bits 32)";
    case StaticEncKernel::Narrow: return "k_encode_static<false, false> (code_bits < 32)";
    }
    return "";
}

const char *redux_static_decode_kernel_name(const redux_params *p, const uint32_t *cum, uint64_t nblocks)
{
    if (static_check(p, cum) != REDUX_OK || nblocks == 0) // (no blocks: the call launches nothing)
        return "";
    switch (pick_static_decode_kernel(p, cum[kStaticEntries - 1], nblocks)) {
    case StaticDecKernel::Fixup: return "k_decode_static<true> (total >= 2^17: quotient fix-up, per-lane control flow)";
    case StaticDecKernel::LutCb32Solo: return "k_decode_static_lut<true, 4> (total <= 2^16: lookup table, 4 waves per group, code_bits 32)";
    case StaticDecKernel::LutSolo: return "k_decode_static_lut<false, 4> (total <= 2^16: lookup table, 4 waves per group)";
    case StaticDecKernel::LutCb32: return "k_decode_static_lut<true, 8> (total <= 2^16: lookup table, 8 waves per group, code_bits 32)";
    case StaticDecKernel::Lut: return "k_decode_static_lut<false, 8> (total <= 2^16: lookup table, 8 waves per group)";
    case StaticDecKernel::LockCb32Solo: return "k_decode_static_lock<true, true> (lock-step, code_bits 32, one wave per SIMD)";
    case StaticDecKernel::LockCb32: return "k_decode_static_lock<true, false> (lock-step, code_bits 32)";
    case StaticDecKernel::LockSolo: return "k_decode_static_lock<false, true> (lock-step, one wave per SIMD)";
    case StaticDecKernel::Lock: return "k_decode_static_lock<false, false> (lock-step)";
    }
    return "";
}

static double static_rc(uint32_t total)
{
    double  r = 1.0 / (double)total;
    int64_t b;
    memcpy(&b, &r, 8);
    b += 4; // as k_fill_rc: never below the true quotient (scale_div)
    memcpy(&r, &b, 8);
    return r;
}

// what every static encoder kernel takes: x' in blocks -> linear slots and sizes in the workspace at ws
static StaticEncCore static_enc_args(const Geometry &g, const redux_params *p, const void *d_x, uint64_t in_len, uint32_t block_size,
                                     uint8_t *ws, void *d_block_status, uint32_t total)
{
    StaticEncCore c;
    static_cast<EncCore &>(c) = enc_core(g, d_x, in_len, ws, d_block_status);
    c.rc         = static_rc(total);
    c.block_size = block_size;
    c.slot_cap   = g.slot_cap;
    c.code_bits  = p->code_bits;
    c.aligned16  = ((((uintptr_t)d_x) & 15) == 0 && (block_size & 15) == 0) ? 1 : 0;
    return c;
}

// what every per-lane static decoder kernel takes: nblocks streams -> block b at d_out + b * block_size
static StaticDecCore static_dec_args(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t nblocks,
                                     uint32_t block_size, void *d_out, void *d_out_sizes, void *d_block_status, uint32_t total)
{
    StaticDecCore c;
    static_cast<DecCore &>(c) = dec_core(d_in, d_in_offsets, nblocks, d_out, d_out_sizes, d_block_status);
    c.rc         = static_rc(total);
    c.block_size = block_size;
    c.code_bits  = p->code_bits;
    c.aligned4   = ((((uintptr_t)d_out) & 3) == 0 && (block_size & 3) == 0) ? 1 : 0;
    return c;
}

// the same for the lock-step and lookup decoders, which take the adaptive decoders' DecArgs (no reciprocal table, no freeze,
// no block table; aligned4 = 2 where output and block size are 16-byte multiples) and c.rc next to them
static DecArgs lock_args_from(const StaticDecCore &c)
{
    DecArgs d;
    memset(&d, 0, sizeof d);
    static_cast<DecCore &>(d) = c;
    d.block_size = c.block_size;
    d.nfreeze    = 0xFFFFFFFFu;
    d.code_bits  = c.code_bits;
    d.aligned4   = c.aligned4 && (((uintptr_t)c.out) & 15) == 0 && (c.block_size & 15) == 0 ? 2 : c.aligned4;
    return d;
}

int redux_static_table_check(const redux_params *p, const uint32_t *cum) { return static_check(p, cum); }

uint64_t redux_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || is_any(p) || block_size == 0)
        return 0;
    const Geometry g = geometry(p, in_len, block_size, true);
    return g.nblocks * (uint64_t)g.slot_cap;
}

uint64_t redux_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    if (check_params(p) != REDUX_OK || is_any(p) || block_size == 0)
        return 0;
    return geometry(p, in_len, block_size, true).total;
}

int redux_static_encode_blocks_dev(const redux_params *p, const uint32_t *cum, const void *d_in, uint64_t in_len,
                                   uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                                   void *d_block_status, void *d_summary, void *d_workspace,
                                   uint64_t workspace_bytes, void *stream)
{
    int st = static_check(p, cum);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || (!d_in && in_len) || !d_block_status || !d_workspace)
        return REDUX_INVALID_INPUT;
    if (((uintptr_t)d_workspace) & 255)
        return REDUX_INVALID_INPUT;
    const Geometry g = geometry(p, in_len, block_size, true);
    if (workspace_bytes < g.total)
        return REDUX_OUTPUT_TOO_SMALL;
    if (!static_lanes_fit(g, block_size, 1))
        return REDUX_UNSUPPORTED;
    hipStream_t s  = (hipStream_t)stream;
    uint8_t    *ws = (uint8_t *)d_workspace;
    HIP_TRY(hipMemsetAsync(ws + g.off_mode, 0, 256, s)); // linear slots, stream byte order
    StaticEncArgs a;
    static_cast<StaticEncCore &>(a) = static_enc_args(g, p, d_in, in_len, block_size, ws, d_block_status, cum[kStaticEntries - 1]);
    memcpy(a.tab.cum, cum, sizeof a.tab.cum);
    const uint32_t grid = (uint32_t)((g.nblocks + 63) / 64);
    switch (pick_static_encode_kernel(p, cum[kStaticEntries - 1], g.nblocks)) { // solo as k_decode_static_lock: one wave per SIMD, not two on some
    case StaticEncKernel::Fixup: k_encode_static<true, false><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Cb32Solo: k_encode_static<false, true, true><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Cb32: k_encode_static<false, true><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Narrow: k_encode_static<false, false><<<grid, 64, 0, s>>>(a); break;
    }
    HIP_TRY(hipGetLastError());
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream, BlockTable{}, RawCopy{});
}

int redux_static_decode_blocks_dev(const redux_params *p, const uint32_t *cum, const void *d_in,
                                   const void *d_in_offsets, uint64_t nblocks, uint32_t block_size, void *d_out,
                                   uint64_t out_cap, void *d_out_sizes, void *d_block_status, void *d_summary,
                                   void *stream)
{
    int st = static_check(p, cum);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_in_offsets || !d_out_sizes || !d_block_status)
        return REDUX_INVALID_INPUT;
    if (nblocks == 0)
        return REDUX_OK;
    if (out_cap < nblocks * (uint64_t)block_size)
        return REDUX_OUTPUT_TOO_SMALL;
    hipStream_t   s = (hipStream_t)stream;
    StaticDecArgs a;
    static_cast<StaticDecCore &>(a) = static_dec_args(p, d_in, d_in_offsets, nblocks, block_size, d_out, d_out_sizes, d_block_status,
                                                      cum[kStaticEntries - 1]);
    memcpy(a.tab.cum, cum, sizeof a.tab.cum);
    const uint32_t        grid = (uint32_t)((nblocks + 63) / 64);
    const StaticDecKernel k    = pick_static_decode_kernel(p, cum[kStaticEntries - 1], nblocks);
    if (k == StaticDecKernel::Fixup)
        k_decode_static<true><<<grid, 64, 0, s>>>(a);
    else {
        StaticLockArgs la;
        memset(&la, 0, sizeof la);
        la.d   = lock_args_from(a);
        la.rc  = a.rc;
        la.tab = a.tab;
        switch (k) { // solo: at most one wave per SIMD, to keep the dispatcher from doubling them up
        case StaticDecKernel::LutCb32Solo: k_decode_static_lut<true, 4><<<(grid + 3) / 4, 256, 0, s>>>(la); break;
        case StaticDecKernel::LutSolo: k_decode_static_lut<false, 4><<<(grid + 3) / 4, 256, 0, s>>>(la); break;
        case StaticDecKernel::LutCb32: k_decode_static_lut<true, 8><<<(grid + 7) / 8, 512, 0, s>>>(la); break;
        case StaticDecKernel::Lut: k_decode_static_lut<false, 8><<<(grid + 7) / 8, 512, 0, s>>>(la); break;
        case StaticDecKernel::LockCb32Solo: k_decode_static_lock<true, true><<<grid, 64, 0, s>>>(la); break;
        case StaticDecKernel::LockCb32: k_decode_static_lock<true, false><<<grid, 64, 0, s>>>(la); break;
        case StaticDecKernel::LockSolo: k_decode_static_lock<false, true><<<grid, 64, 0, s>>>(la); break;
        case StaticDecKernel::Lock: k_decode_static_lock<false, false><<<grid, 64, 0, s>>>(la); break;
        case StaticDecKernel::Fixup: break;
        }
    }
    if (d_summary)
        k_summarize<<<64, 256, 0, s>>>((const int32_t *)d_block_status, nblocks, (int32_t *)d_summary);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// ---- semi-static coding (redux_hist.hpp) ------------------------------------------------------------
// the parameter and total checks of the rule: what static_check says about the parameters, then 257 <= total <= freq_max
static int static_total_check(const redux_params *p, uint32_t total)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    if (total < kStaticEntries - 1 || (uint64_t)total > (1ull << p->freq_bits) - 1)
        return REDUX_INVALID_INPUT;
    return REDUX_OK;
}

int redux_static_table_from_counts(const redux_params *p, const uint64_t *counts, uint32_t total, uint32_t *cum)
{
    int st = static_total_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (!counts || !cum)
        return REDUX_INVALID_INPUT;
    unsigned __int128 n128 = 0;
    for (int s = 0; s < 256; s++)
        n128 += counts[s];
    const uint64_t N = (uint64_t)n128, R = total - 257ull;
    if ((n128 >> 64) || (unsigned __int128)N * R >> 64)
        return REDUX_UNSUPPORTED;
    uint32_t f[257];
    uint64_t r[256];
    uint64_t sum = 1; // EOF
    for (int s = 0; s < 256; s++) {
        f[s] = 1;
        r[s] = 0;
        if (N) {
            const uint64_t cr = counts[s] * R;
            f[s] += (uint32_t)(cr / N);
            r[s] = cr % N;
        }
        sum += f[s];
    }
    f[256] = 1;
    if (N) {
        const uint64_t D = total - sum; // in [0, 255]
        for (int s = 0; s < 256; s++) {
            uint64_t rank = 0;
            for (int j = 0; j < 256; j++)
                rank += (r[j] > r[s] || (r[j] == r[s] && j < s)) ? 1 : 0;
            if (rank < D)
                f[s]++;
        }
    }
    cum[0] = 0;
    for (int s = 0; s < 257; s++)
        cum[s + 1] = cum[s] + f[s];
    return REDUX_OK;
}

uint64_t redux_histogram_workspace_bytes(uint64_t in_len)
{
    (void)in_len; // (k_byte_hist keeps everything in LDS and registers)
    return 0;
}

int redux_histogram_dev(const void *d_in, uint64_t in_len, void *d_counts, void *d_workspace, uint64_t workspace_bytes,
                        void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    if (!d_counts || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    if (in_len == 0)
        return REDUX_OK;
    HistArgs a;
    a.in     = (const uint8_t *)d_in;
    a.counts = (unsigned long long *)d_counts;
    const uint64_t lead = (16 - ((uintptr_t)d_in & 15)) & 15;
    if (lead >= in_len) {
        a.head = in_len;
        a.nvec = 0;
        a.tail = 0;
    } else {
        a.head = lead;
        a.nvec = (in_len - lead) / 16;
        a.tail = in_len - lead - a.nvec * 16;
    }
    const uint64_t rows = (a.nvec + 63) / 64, per = rows / kHistUnroll; // (rows per workgroup-step)
    const uint64_t cap  = (uint64_t)kHistWgsPerCu * cu_count();
    const uint32_t grid = (uint32_t)(per < 1 ? 1 : per < cap ? per : cap);
    k_byte_hist<<<grid, 64, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_static_table_dev(const redux_params *p, const void *d_counts, uint32_t total, void *d_cum, void *stream)
{
    int st = static_total_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (!d_counts || !d_cum)
        return REDUX_INVALID_INPUT;
    k_static_table<<<1, 256, 0, (hipStream_t)stream>>>((const unsigned long long *)d_counts, total, (uint32_t *)d_cum);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_static_table(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t total, uint32_t *cum)
{
    int st = static_total_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (!cum || (in_len && !in))
        return REDUX_INVALID_INPUT;
    uint64_t counts[256];
    if ((st = host::byte_histogram(in, in_len, counts)) != REDUX_OK) // redux_host.hpp
        return st;
    return redux_static_table_from_counts(p, counts, total, cum);
}

int redux_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                   uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                                   uint32_t *block_crc)
{
    int st = static_check(p, cum);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status, static_encoder(p, cum, block_size),
                               block_crc); // redux_host.hpp
}

int redux_static_encode_blocks(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                               uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status)
{
    return redux_static_encode_blocks_crc(p, cum, in, in_len, block_size, out, out_cap, out_offsets, block_status, nullptr);
}

int redux_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, const uint64_t *in_offsets,
                                   uint64_t nblocks, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                                   int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_host(static_check(p, cum), in, in_offsets, nblocks, block_size, out, nblocks * (uint64_t)block_size, out_cap,
                              out_sizes, block_status, nullptr, static_decoder(p, cum, block_size), block_crc);
}

int redux_static_decode_blocks(const redux_params *p, const uint32_t *cum, const uint8_t *in, const uint64_t *in_offsets,
                               uint64_t nblocks, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                               int32_t *block_status)
{
    return redux_static_decode_blocks_crc(p, cum, in, in_offsets, nblocks, block_size, out, out_cap, out_sizes, block_status, nullptr);
}

// ---- the layered adaptive calls: byte-plane layout, delta, zigzag, lag, lag_order, base and base_sub ------------------
// Seven families of eight entry points (redux_planes.hpp, redux_delta.hpp, redux_zigzag.hpp, redux_lag.hpp twice,
// redux_base.hpp, redux_base_sub.hpp), one Filter each: every body below the shared functions is one call into them.
int redux_planes_check(uint32_t element_size)
{
    return (element_size == 1 || element_size == 2 || element_size == 4 || element_size == 8) ? REDUX_OK : REDUX_INVALID_INPUT;
}
int redux_delta_check(uint32_t element_size) { return redux_planes_check(element_size); }
int redux_zigzag_check(uint32_t element_size) { return redux_planes_check(element_size); }
int redux_lag_check(uint32_t element_size, uint32_t lag)
{
    return redux_planes_check(element_size) == REDUX_OK && lag >= 1 && lag <= REDUX_LAG_MAX ? REDUX_OK : REDUX_INVALID_INPUT;
}
int redux_lag_order_check(uint32_t element_size, uint32_t lag, uint32_t order)
{
    return redux_lag_check(element_size, lag) == REDUX_OK && order >= 1 && order <= REDUX_LAG_ORDER_MAX ? REDUX_OK : REDUX_INVALID_INPUT;
}
int redux_base_check(uint32_t element_size) { return redux_planes_check(element_size); }
int redux_base_sub_check(uint32_t element_size) { return redux_planes_check(element_size); }

// (the copy for a filter at E = 1 too: it changes the bytes, so the coder needs the transformed copy; without one, E = 1 is
// the plain call on the caller's buffer)
static uint64_t encode_layout_workspace_bytes(Filter f, const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    if (redux_planes_check(element_size) != REDUX_OK)
        return 0;
    const uint64_t ws = redux_encode_workspace_bytes(p, in_len, block_size);
    return ws ? Layout{element_size, f}.copy_bytes(in_len) + ws : 0;
}

// (the same for every filter: the plane buffer for every element size, 1 included)
uint64_t redux_decode_planes_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    if (redux_planes_check(element_size) != REDUX_OK || block_size == 0)
        return 0;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const uint64_t ws      = redux_decode_workspace_bytes(p, nblocks, block_size);
    return ws ? planes_copy_bytes(nblocks * (uint64_t)block_size) + ws : 0;
}

// the layout stage (layout_stage, layout_decode_tail), the plain coder behind it
static int encode_layout_dev(Layout L, const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, void *d_out,
                             uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                             uint64_t workspace_bytes, void *stream)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (L.check() != REDUX_OK || block_size == 0 || !d_workspace || (in_len && !d_in) ||
        (L.has_base() && L.base_len && !L.d_base))
        return REDUX_INVALID_INPUT;
    Staged x;
    if ((st = layout_stage(L, d_in, in_len, block_size, d_workspace, workspace_bytes, stream, x)) != REDUX_OK)
        return st;
    return redux_encode_blocks_dev(p, x.x, in_len, block_size, d_out, out_cap, d_out_offsets, d_block_status, d_summary, x.ws,
                                   x.ws_bytes, stream);
}

// (the plane buffer for every element size, 1 included: the decoders never write a damaged stream's bytes to d_out.  The
// inverse writes d_out[0 .. out_len) and nothing else: a frame's running sum never leaves the frame, and a base filter writes
// a byte for every byte of the plane buffer it reads)
static int decode_layout_dev(Layout L, const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len,
                             uint32_t block_size, void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary,
                             void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (L.check() != REDUX_OK || block_size == 0 || !d_workspace || !d_in_offsets || !d_out_sizes || !d_block_status ||
        (out_len && !d_out) || (L.has_base() && L.base_len && !L.d_base))
        return REDUX_INVALID_INPUT;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const uint64_t copy    = planes_copy_bytes(nblocks * (uint64_t)block_size);
    // (the snapshot-stride filter's inverse has a workspace of its own, behind the decoder's)
    const uint64_t coder_ws = redux_decode_planes_workspace_bytes(p, out_len, block_size, L.E);
    const uint64_t sum_ws   = L.is_stride() ? stride_workspace_bytes(out_len, L.E, L.stride) : 0;
    if (workspace_bytes < (sum_ws ? align_up(coder_ws, 256) + sum_ws : coder_ws))
        return REDUX_OUTPUT_TOO_SMALL;
    uint8_t *t = (uint8_t *)d_workspace;
    if (sum_ws) {
        L.d_ws     = t + align_up(coder_ws, 256);
        L.ws_bytes = sum_ws;
    }
    st = decode_blocks_dev_impl(p, d_in, d_in_offsets, nblocks, block_size, t, nblocks * (uint64_t)block_size, d_out_sizes,
                                d_block_status, d_summary, t + copy, (sum_ws ? coder_ws : workspace_bytes) - copy, stream, nullptr,
                                BlockTable{});
    if (st != REDUX_OK)
        return st;
    return layout_decode_tail(L, t, d_out, out_len, block_size, d_out_sizes, d_block_status, d_summary, TailSummary::InSizes, stream);
}

// The coders of the chunked host calls (redux_host.hpp).  The transformed copy of a chunk goes in front of the adaptive
// coder's workspace; a chunk is whole 64-block waves, so whole frames of the layout for every element size that divides 64,
// and the record layout's chunks are rounded up to whole frames of its record size (host::chunk_blocks_framed).
// The base filter's layout takes the chunk's share of the base from the slot (host::BaseIo).
static Layout layout_of_slot(Layout L, const host::Slot &s)
{
    if (L.has_base()) {
        L.d_base   = s.d_base.p;
        L.base_len = s.base_len;
    }
    return L;
}

static host::EncodeCoder layout_encoder(const redux_params *p, uint32_t block_size, Layout L)
{
    const host::EncodeCoder plain = adaptive_encoder(p, block_size);
    return {[=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
                plain.size(max_in, several, ws, bound);
                ws += L.copy_bytes(max_in);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return encode_layout_dev(layout_of_slot(L, s), p, s.d_in.p, len, block_size, s.d_out.p, bound, s.d_off.p, s.d_st.p,
                                         s.d_sum.p, ws, ws_bytes, st);
            }};
}

// decodes exactly the chunk's share of out_len
static host::DecodeCoder layout_decoder(const redux_params *p, uint32_t block_size, Layout L)
{
    return {[=](uint64_t cb) {
                const uint64_t ws = redux_decode_planes_workspace_bytes(p, cb * (uint64_t)block_size, block_size, L.E);
                return L.is_stride() ? align_up(ws, 256) + stride_workspace_bytes(cb * (uint64_t)block_size, L.E, L.stride) : ws;
            },
            [=](host::Slot &s, uint64_t, uint64_t out_bytes, void *, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return decode_layout_dev(layout_of_slot(L, s), p, s.d_in.p, s.d_off.p, out_bytes, block_size, s.d_out.p, s.d_sz.p, s.d_st.p,
                                         s.d_sum.p, ws, ws_bytes, st);
            },
            true};
}

// The snapshot-stride filter's predecessor lies S elements back, wherever that is: a chunk cut would put the inverse's
// predecessors in another chunk.  Its host pair therefore runs as ONE chunk, which the chunk loop hands to the call's first
// context: frames of as many blocks as the call has make it so (host::chunk_blocks_framed).
static bool stride_one_chunk(uint64_t nblocks, uint32_t *frame_blocks)
{
    if (nblocks > 0xFFFFFFFFull)
        return false;
    *frame_blocks = nblocks > 1 ? (uint32_t)nblocks : 1;
    return true;
}

// the host-pointer calls (redux_host.hpp); base[0 .. base_len): a base filter's base, the chunks take their shares of it
static int encode_blocks_layout(Layout L, const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base,
                                uint64_t base_len, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                int32_t *block_status, uint32_t *block_crc)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (L.check() != REDUX_OK || block_size == 0 || !out || !out_offsets || (in_len && !in) ||
        (L.has_base() && base_len && !base))
        return REDUX_INVALID_INPUT;
    const host::EncodeCoder coder = L.identity() ? adaptive_encoder(p, block_size) : layout_encoder(p, block_size, L);
    uint32_t frame_blocks = L.record;
    if (L.is_stride() && !stride_one_chunk(redux_block_count(in_len, block_size), &frame_blocks))
        return REDUX_UNSUPPORTED;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status, coder, block_crc, nullptr, {},
                               host::BaseIo{base, base_len, L.has_base()}, {}, frame_blocks);
}

static int encode_blocks_layout(Filter f, const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base,
                                uint64_t base_len, uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc, uint32_t lag = 0,
                                uint32_t order = 0)
{
    return encode_blocks_layout(Layout{element_size, f, nullptr, 0, lag, order}, p, in, in_len, base, base_len, block_size, out,
                                out_cap, out_offsets, block_status, block_crc);
}

static int decode_blocks_layout(Layout L, const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                                uint64_t base_len, uint64_t out_len, uint32_t block_size, uint8_t *out, uint32_t *out_sizes,
                                int32_t *block_status, uint32_t *block_crc)
{
    int st = check_params(p);
    if (st == REDUX_OK && (L.check() != REDUX_OK || (L.has_base() && base_len && !base)))
        st = REDUX_INVALID_INPUT;
    uint32_t frame_blocks = L.record;
    if (st == REDUX_OK && block_size && L.is_stride() && !stride_one_chunk(redux_block_count(out_len, block_size), &frame_blocks))
        st = REDUX_UNSUPPORTED;
    return decode_blocks_host(st, in, in_offsets, redux_block_count(out_len, block_size), block_size, out, out_len, out_len, out_sizes,
                              block_status, nullptr, layout_decoder(p, block_size, L), block_crc, nullptr, {},
                              host::BaseIo{base, base_len, L.has_base()}, {}, frame_blocks);
}

static int decode_blocks_layout(Filter f, const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                                uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                                uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc, uint32_t lag = 0,
                                uint32_t order = 0)
{
    return decode_blocks_layout(Layout{element_size, f, nullptr, 0, lag, order}, p, in, in_offsets, base, base_len, out_len, block_size,
                                out, out_sizes, block_status, block_crc);
}

// -- byte-plane layout
int redux_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                     void *stream)
{
    return transform_dev(Filter::None, d_src, d_dst, len, block_size, element_size, inverse, stream);
}

uint64_t redux_encode_planes_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::None, p, in_len, block_size, element_size);
}

int redux_encode_planes_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size}, p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets, d_block_status,
                             d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_planes_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes, void *d_block_status,
                            void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size}, p, d_in, d_in_offsets, out_len, block_size, d_out, d_out_sizes, d_block_status,
                             d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_planes_crc(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                   uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                                   uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::None, p, in, in_len, nullptr, 0, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_encode_blocks_planes(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                               uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status)
{
    return redux_encode_blocks_planes_crc(p, in, in_len, block_size, element_size, out, out_cap, out_offsets, block_status, nullptr);
}

int redux_decode_blocks_planes_crc(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                                   uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                                   uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::None, p, in, in_offsets, nullptr, 0, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc);
}

int redux_decode_blocks_planes(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status)
{
    return redux_decode_blocks_planes_crc(p, in, in_offsets, out_len, block_size, element_size, out, out_sizes, block_status, nullptr);
}

// -- delta filter
int redux_delta_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                        void *stream)
{
    return transform_dev(Filter::Delta, d_src, d_dst, len, block_size, element_size, inverse, stream);
}

uint64_t redux_encode_delta_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::Delta, p, in_len, block_size, element_size);
}

uint64_t redux_decode_delta_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_planes_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_delta_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                        void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                        void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::Delta}, p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_delta_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len,
                        uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes, void *d_block_status,
                        void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::Delta}, p, d_in, d_in_offsets, out_len, block_size, d_out, d_out_sizes,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_delta(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::Delta, p, in, in_len, nullptr, 0, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_delta(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                           uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                           uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::Delta, p, in, in_offsets, nullptr, 0, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc);
}

// -- zigzag-folded delta filter
int redux_zigzag_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, int inverse,
                         void *stream)
{
    return transform_dev(Filter::Zigzag, d_src, d_dst, len, block_size, element_size, inverse, stream);
}

uint64_t redux_encode_zigzag_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::Zigzag, p, in_len, block_size, element_size);
}

uint64_t redux_decode_zigzag_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_planes_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_zigzag_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                         void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                         void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::Zigzag}, p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_zigzag_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len,
                         uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes, void *d_block_status,
                         void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::Zigzag}, p, d_in, d_in_offsets, out_len, block_size, d_out, d_out_sizes,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_zigzag(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::Zigzag, p, in, in_len, nullptr, 0, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_zigzag(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                            uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::Zigzag, p, in, in_offsets, nullptr, 0, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc);
}

// -- lagged delta filter
int redux_lag_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, uint32_t lag,
                         int inverse, void *stream)
{
    return transform_dev(Filter::Lag, d_src, d_dst, len, block_size, element_size, inverse, stream, nullptr, 0, lag);
}

uint64_t redux_encode_lag_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return redux_encode_zigzag_workspace_bytes(p, in_len, block_size, element_size);
}

uint64_t redux_decode_lag_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_zigzag_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_lag_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                         uint32_t lag, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                         void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::Lag, nullptr, 0, lag}, p, d_in, in_len, block_size, d_out, out_cap,
                             d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_lag_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len, uint32_t block_size,
                         uint32_t element_size, uint32_t lag, void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary,
                         void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::Lag, nullptr, 0, lag}, p, d_in, d_in_offsets, out_len, block_size, d_out,
                             d_out_sizes, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_lag(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint32_t lag, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                            uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::Lag, p, in, in_len, nullptr, 0, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc, lag);
}

int redux_decode_blocks_lag(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                            uint32_t block_size, uint32_t element_size, uint32_t lag, uint8_t *out, uint32_t *out_sizes,
                            int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::Lag, p, in, in_offsets, nullptr, 0, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc, lag);
}

// -- higher-order lagged differences
int redux_lag_order_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, uint32_t lag,
                               uint32_t order, int inverse, void *stream)
{
    return transform_dev(Filter::LagOrder, d_src, d_dst, len, block_size, element_size, inverse, stream, nullptr, 0, lag, order);
}

uint64_t redux_encode_lag_order_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return redux_encode_zigzag_workspace_bytes(p, in_len, block_size, element_size);
}

uint64_t redux_decode_lag_order_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_zigzag_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_lag_order_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                               uint32_t lag, uint32_t order, void *d_out, uint64_t out_cap, void *d_out_offsets,
                               void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::LagOrder, nullptr, 0, lag, order}, p, d_in, in_len, block_size, d_out,
                             out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_lag_order_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len, uint32_t block_size,
                               uint32_t element_size, uint32_t lag, uint32_t order, void *d_out, void *d_out_sizes,
                               void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::LagOrder, nullptr, 0, lag, order}, p, d_in, d_in_offsets, out_len, block_size,
                             d_out, d_out_sizes, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_lag_order(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                  uint32_t element_size, uint32_t lag, uint32_t order, uint8_t *out, uint64_t out_cap,
                                  uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::LagOrder, p, in, in_len, nullptr, 0, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc, lag, order);
}

int redux_decode_blocks_lag_order(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                                  uint32_t block_size, uint32_t element_size, uint32_t lag, uint32_t order, uint8_t *out,
                                  uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::LagOrder, p, in, in_offsets, nullptr, 0, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc, lag, order);
}

// -- record layout (redux_record.hpp): a record size in place of an element size, the byte delta a flag
int redux_record_check(uint32_t record_size, int delta)
{
    return record_size >= 2 && record_size <= REDUX_RECORD_MAX && (delta == 0 || delta == 1) ? REDUX_OK : REDUX_INVALID_INPUT;
}

int redux_record_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t record_size, int delta,
                            int inverse, void *stream)
{
    return record_transform_dev(d_src, d_dst, len, block_size, record_size, delta, inverse, stream);
}

uint64_t redux_encode_record_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t record_size)
{
    if (redux_record_check(record_size, 0) != REDUX_OK)
        return 0;
    const uint64_t ws = redux_encode_workspace_bytes(p, in_len, block_size);
    return ws ? planes_copy_bytes(in_len) + ws : 0;
}

uint64_t redux_decode_record_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t record_size)
{
    return redux_record_check(record_size, 0) == REDUX_OK ? redux_decode_planes_workspace_bytes(p, out_len, block_size, 1) : 0;
}

int redux_encode_record_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t record_size,
                            int delta, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(record_layout(record_size, delta), p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_record_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len, uint32_t block_size,
                            uint32_t record_size, int delta, void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(record_layout(record_size, delta), p, d_in, d_in_offsets, out_len, block_size, d_out, d_out_sizes,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_record(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t record_size,
                               int delta, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                               uint32_t *block_crc)
{
    return encode_blocks_layout(record_layout(record_size, delta), p, in, in_len, nullptr, 0, block_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_record(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t record_size, int delta, uint8_t *out, uint32_t *out_sizes,
                               int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(record_layout(record_size, delta), p, in, in_offsets, nullptr, 0, out_len, block_size, out, out_sizes,
                                block_status, block_crc);
}

const char *redux_record_kernel_name_at(const void *d_src, const void *d_dst, uint64_t len, uint32_t block_size, uint32_t record_size,
                                        int inverse)
{
    static const char *const names[2][3] = {
        {"k_record_planes", "k_record_planes + k_record_planes_bytes", "k_record_planes_bytes"},
        {"k_record_unplanes", "k_record_unplanes + k_record_unplanes_bytes", "k_record_unplanes_bytes"},
    };
    if (block_size == 0 || redux_record_check(record_size, 0) != REDUX_OK)
        return "";
    const FastSplit f = fast_split(len, (uint64_t)record_size * block_size, block_size, {d_src, d_dst});
    return names[inverse != 0][f.nfull == 0 ? 2 : f.rest < len ? 1 : 0];
}

const char *redux_record_kernel_name(uint64_t len, uint32_t block_size, uint32_t record_size, int inverse)
{
    return redux_record_kernel_name_at(nullptr, nullptr, len, block_size, record_size, inverse);
}

int redux_record_plan(uint64_t len, uint32_t block_size, uint32_t record_size, int delta, int inverse, uint32_t cus, uint32_t *plan)
{
    if (block_size == 0 || redux_record_check(record_size, delta) != REDUX_OK || !plan)
        return REDUX_INVALID_INPUT;
    const FastSplit  f = fast_split(len, (uint64_t)record_size * block_size, block_size, {});
    const RecordPlan p = record_plan(f, len, block_size, record_size, delta != 0, inverse != 0, cus ? cus : cu_count());
    plan[0] = p.lgT;
    plan[1] = p.PC;
    plan[2] = p.grid_fast;
    plan[3] = p.grid_rest;
    return REDUX_OK;
}

// -- XOR-against-base filter
int redux_base_planes_dev(const void *d_src, const void *d_base, uint64_t base_len, void *d_dst, uint64_t len, uint32_t block_size,
                       uint32_t element_size, int inverse, void *stream)
{
    return transform_dev(Filter::BaseXor, d_src, d_dst, len, block_size, element_size, inverse, stream, d_base, base_len);
}

uint64_t redux_encode_base_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::BaseXor, p, in_len, block_size, element_size);
}

uint64_t redux_decode_base_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_planes_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_base_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                       uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                       void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::BaseXor, d_base, base_len}, p, d_in, in_len, block_size, d_out, out_cap,
                             d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_base_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_base, uint64_t base_len,
                       uint64_t out_len, uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes,
                       void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::BaseXor, d_base, base_len}, p, d_in, d_in_offsets, out_len, block_size, d_out,
                             d_out_sizes, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_base(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                          uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                          int32_t *block_status, uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::BaseXor, p, in, in_len, base, base_len, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_base(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                          uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                          uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::BaseXor, p, in, in_offsets, base, base_len, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc);
}

// -- folded difference against a base
int redux_base_sub_planes_dev(const void *d_src, const void *d_base, uint64_t base_len, void *d_dst, uint64_t len, uint32_t block_size,
                           uint32_t element_size, int inverse, void *stream)
{
    return transform_dev(Filter::BaseSub, d_src, d_dst, len, block_size, element_size, inverse, stream, d_base, base_len);
}

uint64_t redux_encode_base_sub_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::BaseSub, p, in_len, block_size, element_size);
}

uint64_t redux_decode_base_sub_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_decode_planes_workspace_bytes(p, out_len, block_size, element_size);
}

int redux_encode_base_sub_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                           uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                           void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(Layout{element_size, Filter::BaseSub, d_base, base_len}, p, d_in, in_len, block_size, d_out, out_cap,
                             d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_base_sub_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_base, uint64_t base_len,
                           uint64_t out_len, uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes,
                           void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(Layout{element_size, Filter::BaseSub, d_base, base_len}, p, d_in, d_in_offsets, out_len, block_size, d_out,
                             d_out_sizes, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_base_sub(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                              uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                              int32_t *block_status, uint32_t *block_crc)
{
    return encode_blocks_layout(Filter::BaseSub, p, in, in_len, base, base_len, block_size, element_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_base_sub(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *base,
                              uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                              uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(Filter::BaseSub, p, in, in_offsets, base, base_len, out_len, block_size, element_size, out, out_sizes,
                                block_status, block_crc);
}

// -- snapshot-stride filter (redux_stride.hpp): the stride, a u64, behind the element size; the inverse takes a workspace
int redux_stride_check(uint32_t element_size, uint64_t stride) { return stride_args_ok(element_size, stride) ? REDUX_OK : REDUX_INVALID_INPUT; }

uint64_t redux_stride_workspace_bytes(uint64_t len, uint32_t element_size, uint64_t stride)
{
    return stride_workspace_bytes(len, element_size, stride); // (0 for bad arguments too)
}

int redux_stride_planes_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, uint32_t element_size, uint64_t stride,
                            int inverse, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return stride_transform_dev(d_src, d_dst, len, block_size, element_size, stride, inverse, d_workspace, workspace_bytes, stream);
}

uint64_t redux_encode_stride_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return encode_layout_workspace_bytes(Filter::Stride, p, in_len, block_size, element_size);
}

uint64_t redux_decode_stride_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                                             uint64_t stride)
{
    if (redux_stride_check(element_size, stride) != REDUX_OK)
        return 0;
    const uint64_t ws = redux_decode_planes_workspace_bytes(p, out_len, block_size, element_size);
    return ws ? align_up(ws, 256) + stride_workspace_bytes(out_len, element_size, stride) : 0;
}

static Layout stride_layout(uint32_t element_size, uint64_t stride)
{
    Layout L{element_size, Filter::Stride};
    L.stride = stride;
    return L;
}

int redux_encode_stride_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint64_t stride, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_layout_dev(stride_layout(element_size, stride), p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_decode_stride_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, uint64_t out_len, uint32_t block_size,
                            uint32_t element_size, uint64_t stride, void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return decode_layout_dev(stride_layout(element_size, stride), p, d_in, d_in_offsets, out_len, block_size, d_out, d_out_sizes,
                             d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

int redux_encode_blocks_stride(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                               uint64_t stride, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                               uint32_t *block_crc)
{
    return encode_blocks_layout(stride_layout(element_size, stride), p, in, in_len, nullptr, 0, block_size, out, out_cap, out_offsets,
                                block_status, block_crc);
}

int redux_decode_blocks_stride(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, uint64_t out_len,
                               uint32_t block_size, uint32_t element_size, uint64_t stride, uint8_t *out, uint32_t *out_sizes,
                               int32_t *block_status, uint32_t *block_crc)
{
    return decode_blocks_layout(stride_layout(element_size, stride), p, in, in_offsets, nullptr, 0, out_len, block_size, out, out_sizes,
                                block_status, block_crc);
}

const char *redux_stride_kernel_name(uint64_t len, uint32_t block_size, uint32_t element_size, uint64_t stride, int inverse,
                                     const void *d_src, const void *d_dst)
{
    static thread_local std::string name;
    name.clear();
    if (block_size == 0 || redux_stride_check(element_size, stride) != REDUX_OK || len == 0)
        return "";
    const StrideShape h = stride_shape(d_src, d_dst, len, block_size, element_size, stride, inverse != 0);
    auto add = [&](const char *s) {
        if (!name.empty())
            name += " + ";
        name += s;
    };
    if (!inverse) {
        if (h.f.nfull)
            add("k_stride_planes");
        if (h.f.rest < len)
            add("k_stride_planes_bytes");
        return name.c_str();
    }
    if (element_size == 1)
        add("copy");
    else {
        if (h.f.nfull)
            add("k_planes");
        if (h.f.rest < len)
            add("k_planes_bytes");
    }
    if (h.p.run && h.p.rows >= 2) {
        const bool bytes = h.form != 0;
        if (h.p.segs > 1) {
            add(bytes ? "k_stride_totals_bytes" : "k_stride_totals");
            add(bytes ? "k_stride_scan_bytes" : "k_stride_scan");
        }
        add(bytes ? "k_stride_sum_bytes" : "k_stride_sum");
    }
    if (h.p.run && h.p.chunks && h.p.head < h.p.n * element_size)
        add("k_stride_sum_tail");
    return name.c_str();
}

// ---- plane-static coding (redux_plane_static.hpp) ------------------------------------------------
// E tables, table b mod E for block b of the byte-plane layout.  The launch shape: table t's blocks are cut into wave slots
// of 64, every table gets as many slots as table 0 (which owns the most blocks), and workgroup g serves t = g mod E.  The
// coders are segment-static's with a single segment (the tables_static_* functions below, k = 0).
static uint64_t plane_slots(uint64_t nblocks, uint32_t E) { return ((nblocks + E - 1) / E + 63) / 64; } // wave slots per table

static int plane_static_check(const redux_params *p, uint32_t element_size, uint32_t total)
{
    int st = static_total_check(p, total);
    if (st != REDUX_OK)
        return st;
    return redux_planes_check(element_size);
}

// what the host-side check asks of a batch of tables: each one a static table, and one common total among those that own
// bytes (a table that owns none is all ones: total 257)
static int tables_check(const redux_params *p, const uint32_t *cum, uint64_t ntables)
{
    uint32_t total = 0;
    for (uint64_t i = 0; i < ntables; i++) {
        const uint32_t *c  = cum + kStaticEntries * i;
        const int       st = static_check(p, c);
        if (st != REDUX_OK)
            return st;
        if (c[kStaticEntries - 1] == kStaticEntries - 1)
            continue;
        if (total && c[kStaticEntries - 1] != total)
            return REDUX_INVALID_INPUT;
        total = c[kStaticEntries - 1];
    }
    return REDUX_OK;
}

// the largest last entry of a batch of tables
static uint32_t tables_total(const uint32_t *cum, uint64_t ntables)
{
    uint32_t total = kStaticEntries - 1;
    for (uint64_t i = 0; cum && i < ntables; i++)
        if (cum[kStaticEntries * i + kStaticEntries - 1] > total)
            total = cum[kStaticEntries * i + kStaticEntries - 1];
    return total;
}

int redux_plane_static_table_check(const redux_params *p, const uint32_t *cum, uint32_t element_size)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    if (redux_planes_check(element_size) != REDUX_OK || !cum)
        return REDUX_INVALID_INPUT;
    return tables_check(p, cum, element_size);
}

uint32_t redux_plane_static_total(const uint32_t *cum, uint32_t element_size) { return tables_total(cum, element_size); }

int redux_plane_static_tables_from_counts(const redux_params *p, const uint64_t *counts, uint32_t element_size, uint32_t total,
                                          uint32_t *cum)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    if (!counts || !cum)
        return REDUX_INVALID_INPUT;
    for (uint32_t t = 0; t < element_size; t++)
        if ((st = redux_static_table_from_counts(p, counts + 256 * t, total, cum + kStaticEntries * t)) != REDUX_OK)
            return st;
    return REDUX_OK;
}

uint64_t redux_plane_histogram_workspace_bytes(uint64_t in_len)
{
    (void)in_len; // (k_plane_hist keeps everything in LDS and registers)
    return 0;
}

int redux_plane_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size, void *d_counts,
                              void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    (void)d_workspace;
    (void)workspace_bytes;
    if (redux_planes_check(element_size) != REDUX_OK || block_size == 0 || !d_counts || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    if (in_len == 0)
        return REDUX_OK;
    PlaneHistArgs a;
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.nfull      = in_len / block_size;
    a.block_size = block_size;
    a.E          = element_size;
    a.vec        = ((((uintptr_t)d_in) & 15) == 0 && (block_size & 15) == 0) ? 1 : 0;
    const uint32_t V = block_size / 16;
    a.vshift     = a.vec && (V & (V - 1)) == 0 ? (uint32_t)__builtin_ctz(V) : 0xFFFFFFFFu;
    a.counts     = (unsigned long long *)d_counts;
    // workgroups per table: as redux_histogram_dev over a table's share of the bytes
    const uint64_t share = in_len / element_size, per = a.vec ? share / (16ull * 64 * kHistUnroll) : (share + block_size - 1) / block_size;
    const uint64_t cap   = (uint64_t)kHistWgsPerCu * cu_count() / element_size;
    a.wgs                = (uint32_t)(per < 1 ? 1 : per < cap ? per : cap < 1 ? 1 : cap);
    k_plane_hist<<<a.wgs * element_size, 64, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_plane_static_tables_dev(const redux_params *p, const void *d_counts, uint32_t element_size, uint32_t total, void *d_cum,
                                  void *stream)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    if (!d_counts || !d_cum)
        return REDUX_INVALID_INPUT;
    for (uint32_t t = 0; t < element_size; t++)
        k_static_table<<<1, 256, 0, (hipStream_t)stream>>>((const unsigned long long *)d_counts + 256 * t, total,
                                                           (uint32_t *)d_cum + kStaticEntries * t);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_plane_static_tables(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                              uint32_t total, uint32_t *cum)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !cum || (in_len && !in))
        return REDUX_INVALID_INPUT;
    uint64_t counts[8 * 256];
    if ((st = host::byte_histogram(in, in_len, counts, block_size, element_size)) != REDUX_OK) // redux_host.hpp
        return st;
    return redux_plane_static_tables_from_counts(p, counts, element_size, total, cum);
}

// The lookup decoder's WAVES wave slots share a table, so they must share a segment: k a multiple of WAVES (k = 0, a single
// segment, is one).  Where the 8-wave instance does not suit, the 4-wave one is tried; where neither does (k = 1, 2, 3, 5,
// ...), the lock-step decoder.
static StaticDecKernel pick_segment_decode_kernel(const redux_params *p, uint32_t total, uint64_t launch_blocks, uint32_t k)
{
    const StaticDecKernel d    = pick_static_decode_kernel(p, total, launch_blocks);
    const bool            cb32 = p->code_bits == 32;
    switch (d) {
    case StaticDecKernel::LutCb32:
    case StaticDecKernel::Lut:
        if (k % 8 == 0)
            return d;
        if (k % 4 == 0)
            return cb32 ? StaticDecKernel::LutCb32Solo : StaticDecKernel::LutSolo;
        return cb32 ? StaticDecKernel::LockCb32 : StaticDecKernel::Lock;
    case StaticDecKernel::LutCb32Solo:
    case StaticDecKernel::LutSolo:
        if (k % 4 == 0)
            return d;
        return cb32 ? StaticDecKernel::LockCb32Solo : StaticDecKernel::LockSolo;
    default: return d;
    }
}

// the coders of redux_segment_static.hpp, which plane-static (k = 0) and segment-static (k = G / (64 E)) share
static const char *tables_static_encode_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size, uint32_t E)
{
    static const char *const enc[4] = {"k_encode_segment_static<true, false> (total >= 2^17: quotient fix-up)",
                                       "k_encode_segment_static<false, true, true> (code_bits 32, one wave per SIMD)",
                                       "k_encode_segment_static<false, true> (code_bits 32)",
                                       "k_encode_segment_static<false, false> (code_bits < 32)"};
    const Geometry g = geometry(p, in_len, block_size, true);
    if (!static_lanes_fit(g, block_size, E))
        return "";
    return enc[(int)pick_static_encode_kernel(p, total, 64 * E * plane_slots(g.nblocks, E))];
}

static const char *tables_static_decode_name(const redux_params *p, uint32_t total, uint64_t nblocks, uint32_t E, uint32_t k)
{
    static const char *const dec[9] = {
        "k_decode_segment_static<true> (total >= 2^17: quotient fix-up, per-lane control flow)",
        "k_decode_segment_static_lut<true, 4> (total <= 2^16: lookup table, 4 waves per group, code_bits 32)",
        "k_decode_segment_static_lut<false, 4> (total <= 2^16: lookup table, 4 waves per group)",
        "k_decode_segment_static_lut<true, 8> (total <= 2^16: lookup table, 8 waves per group, code_bits 32)",
        "k_decode_segment_static_lut<false, 8> (total <= 2^16: lookup table, 8 waves per group)",
        "k_decode_segment_static_lock<true, true> (lock-step, code_bits 32, one wave per SIMD)",
        "k_decode_segment_static_lock<true, false> (lock-step, code_bits 32)",
        "k_decode_segment_static_lock<false, true> (lock-step, one wave per SIMD)",
        "k_decode_segment_static_lock<false, false> (lock-step)"};
    return dec[(int)pick_segment_decode_kernel(p, total, 64 * E * plane_slots(nblocks, E), k)];
}

const char *redux_plane_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size,
                                                  uint32_t element_size)
{
    if (plane_static_check(p, element_size, total) != REDUX_OK || block_size == 0)
        return "";
    return tables_static_encode_name(p, total, in_len, block_size, element_size);
}

const char *redux_plane_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks, uint32_t element_size)
{
    if (plane_static_check(p, element_size, total) != REDUX_OK || nblocks == 0)
        return "";
    return tables_static_decode_name(p, total, nblocks, element_size, 0);
}

uint64_t redux_plane_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    return redux_static_encode_bound(p, in_len, block_size);
}

uint64_t redux_plane_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    if (redux_planes_check(element_size) != REDUX_OK)
        return 0;
    const uint64_t ws = redux_static_encode_workspace_bytes(p, in_len, block_size);
    return ws ? Layout{element_size}.copy_bytes(in_len) + ws : 0;
}

uint64_t redux_plane_static_decode_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    if (check_params(p) != REDUX_OK || is_any(p) || redux_planes_check(element_size) != REDUX_OK || block_size == 0)
        return 0;
    return planes_copy_bytes(redux_block_count(out_len, block_size) * (uint64_t)block_size);
}

static SegmentTables segment_tables(const void *d_cum, uint32_t E, uint32_t k, uint32_t total)
{
    SegmentTables t;
    t.p.cum   = (const uint32_t *)d_cum;
    t.p.E     = E;
    t.p.total = total;
    t.p.rc257 = static_rc(kStaticEntries - 1);
    t.k       = k;
    return t;
}

// the static coder over x' (d_x: the layout of the input, or the input itself for E = 1) under the tables at d_cum; k wave
// slots of a plane per segment, 0 for a single segment (SegmentTables)
static int tables_static_encode_x(const redux_params *p, const void *d_cum, uint32_t total, const void *d_x, uint64_t in_len,
                                  uint32_t block_size, uint32_t E, uint32_t k, void *d_out, uint64_t out_cap, void *d_out_offsets,
                                  void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    const Geometry g = geometry(p, in_len, block_size, true);
    if (workspace_bytes < g.total)
        return REDUX_OUTPUT_TOO_SMALL;
    if (!static_lanes_fit(g, block_size, E))
        return REDUX_UNSUPPORTED;
    hipStream_t s  = (hipStream_t)stream;
    uint8_t    *ws = (uint8_t *)d_workspace;
    HIP_TRY(hipMemsetAsync(ws + g.off_mode, 0, 256, s)); // linear slots, stream byte order
    SegmentStaticEncArgs a;
    a.c = static_enc_args(g, p, d_x, in_len, block_size, ws, d_block_status, total);
    a.t = segment_tables(d_cum, E, k, total);
    const uint64_t slots = plane_slots(g.nblocks, E);
    const uint32_t grid  = (uint32_t)(slots * E);
    switch (pick_static_encode_kernel(p, total, 64 * E * slots)) {
    case StaticEncKernel::Fixup: k_encode_segment_static<true, false><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Cb32Solo: k_encode_segment_static<false, true, true><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Cb32: k_encode_segment_static<false, true><<<grid, 64, 0, s>>>(a); break;
    case StaticEncKernel::Narrow: k_encode_segment_static<false, false><<<grid, 64, 0, s>>>(a); break;
    }
    HIP_TRY(hipGetLastError());
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream, BlockTable{}, RawCopy{});
}

// the layout stage (layout_stage), then the coder over x'
static int tables_static_encode(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                uint32_t block_size, uint32_t E, uint32_t k, void *d_out, uint64_t out_cap, void *d_out_offsets,
                                void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    Staged    x;
    const int st = layout_stage(Layout{E}, d_in, in_len, block_size, d_workspace, workspace_bytes, stream, x);
    if (st != REDUX_OK)
        return st;
    return tables_static_encode_x(p, d_cum, total, x.x, in_len, block_size, E, k, d_out, out_cap, d_out_offsets, d_block_status,
                                  d_summary, x.ws, x.ws_bytes, stream);
}

int redux_plane_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                  uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                                  void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || (!d_in && in_len) || !d_block_status || !d_workspace || (((uintptr_t)d_workspace) & 255))
        return REDUX_INVALID_INPUT;
    return tables_static_encode(p, d_cum, total, d_in, in_len, block_size, element_size, 0, d_out, out_cap, d_out_offsets,
                                d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

// the static decoders under the tables at d_cum (k as above): nblocks streams -> block b at d_planes + b * block_size
static int tables_static_decode_x(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, const void *d_in_offsets,
                                  uint64_t nblocks, uint32_t block_size, uint32_t E, uint32_t k, void *d_planes, void *d_out_sizes,
                                  void *d_block_status, hipStream_t s)
{
    const StaticDecCore   c = static_dec_args(p, d_in, d_in_offsets, nblocks, block_size, d_planes, d_out_sizes, d_block_status, total);
    SegmentStaticLockArgs la;
    memset(&la, 0, sizeof la);
    la.d  = lock_args_from(c);
    la.rc = c.rc;
    la.t  = segment_tables(d_cum, E, k, total);
    const uint64_t slots = plane_slots(nblocks, E);
    const uint32_t grid  = (uint32_t)(slots * E), grid4 = (uint32_t)((slots + 3) / 4 * E), grid8 = (uint32_t)((slots + 7) / 8 * E);
    switch (pick_segment_decode_kernel(p, total, 64 * E * slots, k)) {
    case StaticDecKernel::Fixup: {
        SegmentStaticDecArgs a;
        a.c = c;
        a.t = la.t;
        k_decode_segment_static<true><<<grid, 64, 0, s>>>(a);
        break;
    }
    case StaticDecKernel::LutCb32Solo: k_decode_segment_static_lut<true, 4><<<grid4, 256, 0, s>>>(la); break;
    case StaticDecKernel::LutSolo: k_decode_segment_static_lut<false, 4><<<grid4, 256, 0, s>>>(la); break;
    case StaticDecKernel::LutCb32: k_decode_segment_static_lut<true, 8><<<grid8, 512, 0, s>>>(la); break;
    case StaticDecKernel::Lut: k_decode_segment_static_lut<false, 8><<<grid8, 512, 0, s>>>(la); break;
    case StaticDecKernel::LockCb32Solo: k_decode_segment_static_lock<true, true><<<grid, 64, 0, s>>>(la); break;
    case StaticDecKernel::LockCb32: k_decode_segment_static_lock<true, false><<<grid, 64, 0, s>>>(la); break;
    case StaticDecKernel::LockSolo: k_decode_segment_static_lock<false, true><<<grid, 64, 0, s>>>(la); break;
    case StaticDecKernel::Lock: k_decode_segment_static_lock<false, false><<<grid, 64, 0, s>>>(la); break;
    }
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// the blocks decode into the plane buffer at the front of the workspace (for every E, 1 included), then the layout's decode
// tail (layout_decode_tail); the summary comes last
static int tables_static_decode(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, const void *d_in_offsets,
                                uint64_t out_len, uint32_t block_size, uint32_t E, uint32_t k, void *d_out, void *d_out_sizes,
                                void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    if (workspace_bytes < redux_plane_static_decode_workspace_bytes(p, out_len, block_size, E))
        return REDUX_OUTPUT_TOO_SMALL;
    const int st = tables_static_decode_x(p, d_cum, total, d_in, d_in_offsets, nblocks, block_size, E, k, d_workspace, d_out_sizes,
                                          d_block_status, (hipStream_t)stream);
    if (st != REDUX_OK)
        return st;
    return layout_decode_tail(Layout{E}, d_workspace, d_out, out_len, block_size, d_out_sizes, d_block_status, d_summary,
                              TailSummary::Summarize, stream);
}

int redux_plane_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, const void *d_in_offsets,
                                  uint64_t out_len, uint32_t block_size, uint32_t element_size, void *d_out, void *d_out_sizes,
                                  void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || !d_workspace || !d_in_offsets || !d_out_sizes || !d_block_status || (out_len && !d_out))
        return REDUX_INVALID_INPUT;
    return tables_static_decode(p, d_cum, total, d_in, d_in_offsets, out_len, block_size, element_size, 0, d_out, d_out_sizes,
                                d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

// The tables of a chunked static call travel to each chunk's device at the front of the chunk's workspace, stream-ordered:
// `bytes` of them from the host at `cum`, in tables_bytes(bytes) of room.  The coder gets them at the workspace's old start
// and its own workspace (ws, ws_bytes, moved on here) behind them.
static uint64_t tables_bytes(uint64_t bytes) { return align_up(bytes, 256); }

static int stage_tables(const uint32_t *cum, uint64_t bytes, uint8_t *&ws, uint64_t &ws_bytes, hipStream_t st)
{
    const uint64_t tb = tables_bytes(bytes);
    if (ws_bytes < tb)
        return REDUX_OUTPUT_TOO_SMALL;
    HIP_TRY(hipMemcpyAsync(ws, cum, bytes, hipMemcpyHostToDevice, st));
    ws += tb;
    ws_bytes -= tb;
    return REDUX_OK;
}

// The coders of the chunked host calls (8 KiB of tables at most).  A chunk is whole 64-block waves, so its first block is a
// multiple of every E and b mod E inside the chunk is the global one: checked (a call of one chunk starts at block 0
// whatever its size).
static host::EncodeCoder plane_static_encoder(const redux_params *p, const uint32_t *cum, uint32_t block_size, uint32_t E)
{
    const uint32_t total = redux_plane_static_total(cum, E);
    const uint64_t bytes = (uint64_t)E * kStaticEntries * 4;
    auto           chunk = std::make_shared<uint64_t>(0); // bytes of a full chunk when the call has several
    return {[=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
                *chunk = several ? max_in : 0;
                ws     = tables_bytes(bytes) + redux_plane_static_encode_workspace_bytes(p, max_in, block_size, E);
                bound  = redux_plane_static_encode_bound(p, max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *d_cum, uint64_t ws_bytes, hipStream_t st) -> int {
                if (*chunk % ((uint64_t)E * block_size) != 0)
                    return REDUX_UNSUPPORTED;
                uint8_t  *ws = (uint8_t *)d_cum;
                const int rc = stage_tables(cum, bytes, ws, ws_bytes, st);
                if (rc != REDUX_OK)
                    return rc;
                return redux_plane_static_encode_dev(p, d_cum, total, s.d_in.p, len, block_size, E, s.d_out.p, bound, s.d_off.p,
                                                     s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            }};
}

static host::DecodeCoder plane_static_decoder(const redux_params *p, const uint32_t *cum, uint32_t block_size, uint32_t E)
{
    const uint32_t total = redux_plane_static_total(cum, E);
    const uint64_t bytes = (uint64_t)E * kStaticEntries * 4;
    auto           cbs   = std::make_shared<uint64_t>(0); // blocks of a full chunk
    return {[=](uint64_t cb) {
                *cbs = cb;
                return tables_bytes(bytes) + redux_plane_static_decode_workspace_bytes(p, cb * (uint64_t)block_size, block_size, E);
            },
            [=](host::Slot &s, uint64_t nb, uint64_t out_bytes, void *, void *d_cum, uint64_t ws_bytes, hipStream_t st) -> int {
                if (*cbs % E != 0 && nb != *cbs) // (a chunk size that is no multiple of E: the call's only chunk)
                    return REDUX_UNSUPPORTED;
                uint8_t  *ws = (uint8_t *)d_cum;
                const int rc = stage_tables(cum, bytes, ws, ws_bytes, st);
                if (rc != REDUX_OK)
                    return rc;
                return redux_plane_static_decode_dev(p, d_cum, total, s.d_in.p, s.d_off.p, out_bytes, block_size, E, s.d_out.p,
                                                     s.d_sz.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            },
            true};
}

int redux_plane_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                         uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap,
                                         uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    int st = redux_plane_static_table_check(p, cum, element_size);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status,
                               plane_static_encoder(p, cum, block_size, element_size), block_crc); // redux_host.hpp
}

int redux_plane_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, const uint64_t *in_offsets,
                                         uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out,
                                         uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    const int st = redux_plane_static_table_check(p, cum, element_size);
    return decode_blocks_host(st, in, in_offsets, redux_block_count(out_len, block_size), block_size, out, out_len, out_len, out_sizes,
                              block_status, nullptr, plane_static_decoder(p, cum, block_size, st == REDUX_OK ? element_size : 1),
                              block_crc);
}

// ---- segment-static coding (redux_segment_static.hpp) ----------------------------------------------
// nseg * E tables, table (b / G) E + b mod E for block b of the byte-plane layout; G = 64 E k.  The launch shape is
// plane-static's (plane_slots wave slots per plane, workgroup g serves t = g mod E); slot w lies in segment w / k.
static int segment_static_check(const redux_params *p, uint32_t element_size, uint32_t segment_blocks, uint32_t total)
{
    int st = plane_static_check(p, element_size, total);
    if (st != REDUX_OK)
        return st;
    return segment_blocks != 0 && segment_blocks % (64 * element_size) == 0 ? REDUX_OK : REDUX_INVALID_INPUT;
}

uint64_t redux_segment_static_table_count(uint64_t nblocks, uint32_t element_size, uint32_t segment_blocks)
{
    if (redux_planes_check(element_size) != REDUX_OK || segment_blocks == 0 || segment_blocks % (64 * element_size) != 0)
        return 0;
    const uint64_t nseg = nblocks / segment_blocks + (nblocks % segment_blocks ? 1 : 0);
    return (nseg ? nseg : 1) * element_size;
}

int redux_segment_static_table_check(const redux_params *p, const uint32_t *cum, uint64_t ntables, uint64_t nblocks,
                                     uint32_t element_size, uint32_t segment_blocks)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    const uint64_t want = redux_segment_static_table_count(nblocks, element_size, segment_blocks);
    if (want == 0 || ntables != want || !cum)
        return REDUX_INVALID_INPUT;
    return tables_check(p, cum, ntables);
}

uint32_t redux_segment_static_total(const uint32_t *cum, uint64_t ntables) { return tables_total(cum, ntables); }

int redux_segment_static_tables_from_counts(const redux_params *p, const uint64_t *counts, uint64_t nblocks, uint32_t element_size,
                                            uint32_t segment_blocks, uint32_t total, uint32_t *cum)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (!counts || !cum)
        return REDUX_INVALID_INPUT;
    const uint64_t n = redux_segment_static_table_count(nblocks, element_size, segment_blocks);
    for (uint64_t i = 0; i < n; i++)
        if ((st = redux_static_table_from_counts(p, counts + 256 * i, total, cum + kStaticEntries * i)) != REDUX_OK)
            return st;
    return REDUX_OK;
}

int redux_segment_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size, uint32_t segment_blocks,
                                void *d_counts, void *stream)
{
    if (block_size == 0 || !d_counts || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    const uint64_t npairs = redux_segment_static_table_count(redux_block_count(in_len, block_size), element_size, segment_blocks);
    if (npairs == 0)
        return REDUX_INVALID_INPUT;
    if (in_len == 0)
        return REDUX_OK;
    SegmentHistArgs a;
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.nfull      = in_len / block_size;
    a.npairs     = npairs;
    a.block_size = block_size;
    a.E          = element_size;
    a.G          = segment_blocks;
    a.vec        = ((((uintptr_t)d_in) & 15) == 0 && (block_size & 15) == 0) ? 1 : 0;
    const uint32_t V = block_size / 16;
    a.vshift     = a.vec && (V & (V - 1)) == 0 ? (uint32_t)__builtin_ctz(V) : 0xFFFFFFFFu;
    a.counts     = (unsigned long long *)d_counts;
    // The grid: what the device holds (kHistWgsPerCu one-wave workgroups per CU), dealt over the pairs.  Few pairs: several
    // workgroups walk one pair, as many as its bytes give a step's work to.  More pairs than that: one workgroup per pair, a
    // pair after the other.
    const uint64_t cap   = (uint64_t)kHistWgsPerCu * cu_count();
    const uint64_t share = (uint64_t)(segment_blocks / element_size) * block_size; // bytes of a full pair
    const uint64_t per   = a.vec ? share / (16ull * 64 * kHistUnroll) : segment_blocks / element_size;
    uint64_t       wgs   = npairs >= cap ? 1 : cap / npairs;
    wgs                  = wgs > per ? per : wgs;
    a.wgs                = (uint32_t)(wgs < 1 ? 1 : wgs);
    a.pstep              = npairs < cap ? npairs : cap;
    k_segment_hist<<<(uint32_t)(a.pstep * a.wgs), 64, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_segment_static_tables_dev(const redux_params *p, const void *d_counts, uint64_t nblocks, uint32_t element_size,
                                    uint32_t segment_blocks, uint32_t total, void *d_cum, void *stream)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (!d_counts || !d_cum)
        return REDUX_INVALID_INPUT;
    const uint64_t n = redux_segment_static_table_count(nblocks, element_size, segment_blocks);
    if (n > 0x7FFFFFFFull)
        return REDUX_UNSUPPORTED;
    k_static_tables<<<(uint32_t)n, 256, 0, (hipStream_t)stream>>>((const unsigned long long *)d_counts, total, (uint32_t *)d_cum);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

const char *redux_segment_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size,
                                                    uint32_t element_size, uint32_t segment_blocks)
{
    if (segment_static_check(p, element_size, segment_blocks, total) != REDUX_OK || block_size == 0)
        return "";
    return tables_static_encode_name(p, total, in_len, block_size, element_size);
}

const char *redux_segment_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks, uint32_t element_size,
                                                    uint32_t segment_blocks)
{
    if (segment_static_check(p, element_size, segment_blocks, total) != REDUX_OK || nblocks == 0)
        return "";
    return tables_static_decode_name(p, total, nblocks, element_size, segment_blocks / (64 * element_size));
}

uint64_t redux_segment_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    return redux_static_encode_bound(p, in_len, block_size);
}

uint64_t redux_segment_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return redux_plane_static_encode_workspace_bytes(p, in_len, block_size, element_size);
}

uint64_t redux_segment_static_decode_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    return redux_plane_static_decode_workspace_bytes(p, out_len, block_size, element_size);
}

static uint64_t segment_counts_bytes(uint64_t ntables) { return align_up(ntables * 256 * 8, 256); }

uint64_t redux_segment_static_build_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size,
                                                           uint32_t element_size, uint32_t segment_blocks)
{
    if (block_size == 0)
        return 0;
    const uint64_t n  = redux_segment_static_table_count(redux_block_count(in_len, block_size), element_size, segment_blocks);
    const uint64_t ws = redux_segment_static_encode_workspace_bytes(p, in_len, block_size, element_size);
    return n && ws ? segment_counts_bytes(n) + ws : 0;
}

int redux_segment_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                    uint32_t block_size, uint32_t element_size, uint32_t segment_blocks, void *d_out, uint64_t out_cap,
                                    void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                                    uint64_t workspace_bytes, void *stream)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || (!d_in && in_len) || !d_block_status || !d_workspace || (((uintptr_t)d_workspace) & 255))
        return REDUX_INVALID_INPUT;
    return tables_static_encode(p, d_cum, total, d_in, in_len, block_size, element_size, segment_blocks / (64 * element_size), d_out,
                                out_cap, d_out_offsets, d_block_status, d_summary, d_workspace, workspace_bytes, stream);
}

// Layout once, the histogram of that copy, the tables, the coder over the same copy.  The workspace: the counts, then what
// redux_segment_static_encode_dev takes.
int redux_segment_static_build_encode_dev(const redux_params *p, uint32_t total, const void *d_in, uint64_t in_len, uint32_t block_size,
                                          uint32_t element_size, uint32_t segment_blocks, void *d_cum, void *d_out, uint64_t out_cap,
                                          void *d_out_offsets, void *d_block_status, void *d_summary, void *d_workspace,
                                          uint64_t workspace_bytes, void *stream)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || (!d_in && in_len) || !d_block_status || !d_workspace || (((uintptr_t)d_workspace) & 255))
        return REDUX_INVALID_INPUT;
    const uint64_t nblocks = redux_block_count(in_len, block_size);
    const uint64_t cb      = segment_counts_bytes(redux_segment_static_table_count(nblocks, element_size, segment_blocks));
    const Layout   L{element_size};
    if (workspace_bytes < cb + L.copy_bytes(in_len)) // (before the counts are cleared: layout_stage checks its share again)
        return REDUX_OUTPUT_TOO_SMALL;
    uint8_t *counts = (uint8_t *)d_workspace;
    HIP_TRY(hipMemsetAsync(counts, 0, cb, (hipStream_t)stream));
    Staged x;
    if ((st = layout_stage(L, d_in, in_len, block_size, counts + cb, workspace_bytes - cb, stream, x)) != REDUX_OK)
        return st;
    if ((st = redux_segment_histogram_dev(x.x, in_len, block_size, element_size, segment_blocks, counts, stream)) != REDUX_OK)
        return st;
    if ((st = redux_segment_static_tables_dev(p, counts, nblocks, element_size, segment_blocks, total, d_cum, stream)) != REDUX_OK)
        return st;
    return tables_static_encode_x(p, d_cum, total, x.x, in_len, block_size, element_size, segment_blocks / (64 * element_size), d_out,
                                  out_cap, d_out_offsets, d_block_status, d_summary, x.ws, x.ws_bytes, stream);
}

int redux_segment_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, const void *d_in_offsets,
                                    uint64_t out_len, uint32_t block_size, uint32_t element_size, uint32_t segment_blocks, void *d_out,
                                    void *d_out_sizes, void *d_block_status, void *d_summary, void *d_workspace,
                                    uint64_t workspace_bytes, void *stream)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || !d_workspace || !d_in_offsets || !d_out_sizes || !d_block_status || (out_len && !d_out))
        return REDUX_INVALID_INPUT;
    return tables_static_decode(p, d_cum, total, d_in, d_in_offsets, out_len, block_size, element_size,
                                segment_blocks / (64 * element_size), d_out, d_out_sizes, d_block_status, d_summary, d_workspace,
                                workspace_bytes, stream);
}

// The coders of the chunked host calls.  Chunks are whole segments (host::SegmentTablesIo), so a chunk's segment numbers are
// the call's minus a constant and its tables are a contiguous run of the call's: encode builds them from the chunk into the
// slot's d_tab, decode finds them staged there.
static host::EncodeCoder segment_static_encoder(const redux_params *p, uint32_t total, uint32_t block_size, uint32_t E, uint32_t G)
{
    return {[=](uint64_t max_in, bool, uint64_t &ws, uint64_t &bound) {
                ws    = redux_segment_static_build_encode_workspace_bytes(p, max_in, block_size, E, G);
                bound = redux_segment_static_encode_bound(p, max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) -> int {
                return redux_segment_static_build_encode_dev(p, total, s.d_in.p, len, block_size, E, G, s.d_tab.p, s.d_out.p, bound,
                                                             s.d_off.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            }};
}

static host::DecodeCoder segment_static_decoder(const redux_params *p, uint32_t total, uint32_t block_size, uint32_t E, uint32_t G)
{
    return {[=](uint64_t cb) { return redux_segment_static_decode_workspace_bytes(p, cb * (uint64_t)block_size, block_size, E); },
            [=](host::Slot &s, uint64_t, uint64_t out_bytes, void *, void *ws, uint64_t ws_bytes, hipStream_t st) -> int {
                return redux_segment_static_decode_dev(p, s.d_tab.p, total, s.d_in.p, s.d_off.p, out_bytes, block_size, E, G, s.d_out.p,
                                                       s.d_sz.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            },
            true};
}

int redux_segment_static_encode_blocks_crc(const redux_params *p, uint32_t total, const uint8_t *in, uint64_t in_len, uint32_t block_size,
                                           uint32_t element_size, uint32_t segment_blocks, uint32_t *cum, uint8_t *out, uint64_t out_cap,
                                           uint64_t *out_offsets, int32_t *block_status, uint32_t *block_crc)
{
    int st = segment_static_check(p, element_size, segment_blocks, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !cum || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status,
                               segment_static_encoder(p, total, block_size, element_size, segment_blocks), block_crc, nullptr,
                               host::SegmentTablesIo{cum, element_size, segment_blocks}); // redux_host.hpp
}

int redux_segment_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, uint64_t ntables, const uint8_t *in,
                                           const uint64_t *in_offsets, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                                           uint32_t segment_blocks, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                                           uint32_t *block_crc)
{
    if (block_size == 0)
        return REDUX_INVALID_INPUT;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const int      st      = redux_segment_static_table_check(p, cum, ntables, nblocks, element_size, segment_blocks);
    if (st != REDUX_OK)
        return st;
    return decode_blocks_host(st, in, in_offsets, nblocks, block_size, out, out_len, out_len, out_sizes, block_status, nullptr,
                              segment_static_decoder(p, redux_segment_static_total(cum, ntables), block_size, element_size, segment_blocks),
                              block_crc, nullptr, host::SegmentTablesIo{const_cast<uint32_t *>(cum), element_size, segment_blocks});
}

// ---- context-static coding (redux_context_static.hpp) ----------------------------------------------
// 256 tables, table c for the bytes that follow a byte c.  Every coder launch is k_context_image (the tables checked and
// packed into the 128 KiB image at the front of the workspace) and then one persistent workgroup per CU.
// Waves per workgroup.  The 128 KiB image allows one workgroup per CU, so the grid is first spread over the CUs and only then
// deepened: W = the smallest built instance that holds ceil(wave slots / CUs), up to the largest (encode 8: sixteen waves
// would be four per SIMD at 128 registers each, and the coder wave needs 132; decode 16).  65,536 blocks on 256 CUs are 1024
// wave slots: 256 workgroups of 4 waves.  (REDUX_CTX_WAVES, variant builds only: one value for every launch, to measure the
// values the rule does not choose.)
constexpr uint64_t kCtxHead = kCtxImageBytes + 256; // the image and its flag, in front of a coder's own workspace

static uint32_t context_waves(uint64_t nblocks, uint32_t max_waves)
{
#ifdef REDUX_CTX_WAVES
    (void)nblocks;
    return REDUX_CTX_WAVES < max_waves ? REDUX_CTX_WAVES : max_waves;
#else
    const uint64_t per_cu = ((nblocks + 63) / 64 + cu_count() - 1) / cu_count();
    uint32_t       w      = 4;
    while (w < max_waves && w < per_cu)
        w *= 2;
    return w;
#endif
}

static int context_static_check(const redux_params *p, uint32_t total)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p) || total > kCtxTotalMax)
        return REDUX_UNSUPPORTED;
    return static_total_check(p, total);
}

int redux_context_static_table_check(const redux_params *p, const uint32_t *cum)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p))
        return REDUX_UNSUPPORTED;
    if (!cum)
        return REDUX_INVALID_INPUT;
    for (uint32_t c = 0; c < kCtxTables; c++) {
        const uint32_t *t = cum + kStaticEntries * c;
        if ((st = static_check(p, t)) != REDUX_OK)
            return st;
        if (t[kStaticEntries - 1] != cum[kStaticEntries - 1])
            return REDUX_INVALID_INPUT;
    }
    return cum[kStaticEntries - 1] > kCtxTotalMax ? REDUX_UNSUPPORTED : REDUX_OK;
}

uint32_t redux_context_static_total(const uint32_t *cum) { return cum ? cum[kStaticEntries - 1] : 0; }

int redux_context_static_tables_from_counts(const redux_params *p, const uint64_t *counts, uint32_t total, uint32_t *cum)
{
    int st = context_static_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (!counts || !cum)
        return REDUX_INVALID_INPUT;
    uint64_t ones[256];
    for (int s = 0; s < 256; s++)
        ones[s] = 1;
    for (uint32_t c = 0; c < kCtxTables; c++) {
        const uint64_t *row = counts + 256 * c;
        bool            any = false;
        for (int s = 0; s < 256; s++)
            any |= row[s] != 0;
        if ((st = redux_static_table_from_counts(p, any ? row : ones, total, cum + kStaticEntries * c)) != REDUX_OK)
            return st;
    }
    return REDUX_OK;
}

int redux_context_histogram_dev(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_counts, void *stream)
{
    if (block_size == 0 || !d_counts || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    if (in_len == 0)
        return REDUX_OK;
    ContextHistArgs a;
    a.in         = (const uint8_t *)d_in;
    a.block_size = block_size;
    a.counts     = (unsigned long long *)d_counts;
    const uint64_t lead = (16 - ((uintptr_t)d_in & 15)) & 15;
    if (lead >= in_len) {
        a.head = in_len;
        a.nvec = 0;
        a.tail = 0;
    } else {
        a.head = lead;
        a.nvec = (in_len - lead) / 16;
        a.tail = in_len - lead - a.nvec * 16;
    }
    const uint64_t rows = (a.nvec + kCtxHistThreads - 1) / kCtxHistThreads, cap = cu_count();
    const uint32_t grid = (uint32_t)(rows < 1 ? 1 : rows < cap ? rows : cap);
    k_context_hist<<<grid, kCtxHistThreads, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_context_static_tables_dev(const redux_params *p, const void *d_counts, uint32_t total, void *d_cum, void *stream)
{
    int st = context_static_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (!d_counts || !d_cum)
        return REDUX_INVALID_INPUT;
    k_context_static_tables<<<kCtxTables, 256, 0, (hipStream_t)stream>>>((const unsigned long long *)d_counts, total, (uint32_t *)d_cum);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_context_static_tables(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t total,
                                uint32_t *cum)
{
    int st = context_static_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !cum || (in_len && !in))
        return REDUX_INVALID_INPUT;
    std::vector<uint64_t> counts((size_t)kCtxTables * 256);
    if ((st = host::byte_histogram(in, in_len, counts.data(), block_size, 1, true)) != REDUX_OK) // redux_host.hpp
        return st;
    return redux_context_static_tables_from_counts(p, counts.data(), total, cum);
}

uint64_t redux_context_static_encode_bound(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    return redux_static_encode_bound(p, in_len, block_size);
}

uint64_t redux_context_static_encode_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    const uint64_t ws = redux_static_encode_workspace_bytes(p, in_len, block_size);
    return ws == 0 ? 0 : kCtxHead + ws;
}

uint64_t redux_context_static_decode_workspace_bytes(const redux_params *p, uint64_t nblocks, uint32_t block_size)
{
    (void)nblocks;
    if (check_params(p) != REDUX_OK || is_any(p) || block_size == 0)
        return 0;
    return kCtxHead;
}

// the tables at d_cum -> the checked image and its flag at the front of the workspace
static int context_image(const void *d_cum, uint32_t total, uint8_t *ws, hipStream_t s)
{
    HIP_TRY(hipMemsetAsync(ws + kCtxImageBytes, 0, 256, s));
    k_context_image<<<kCtxTables, 256, 0, s>>>((const uint32_t *)d_cum, total, (uint16_t *)ws, (uint32_t *)(ws + kCtxImageBytes));
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// which context-static kernel a call runs: ONE decision, used by the launch code and reported by
// redux_context_static_encode_kernel_name / redux_context_static_decode_kernel_name
struct ContextEncKernel {
    uint32_t waves; // 4 or 8
    bool     cb32;
};

static ContextEncKernel pick_context_encode_kernel(const redux_params *p, uint64_t nblocks)
{
    return {context_waves(nblocks, 8), p->code_bits == 32};
}

static uint32_t pick_context_decode_kernel(uint64_t nblocks) { return context_waves(nblocks, 16); } // 4, 8 or 16 waves

const char *redux_context_static_encode_kernel_name(const redux_params *p, uint32_t total, uint64_t in_len, uint32_t block_size)
{
    if (context_static_check(p, total) != REDUX_OK || block_size == 0)
        return "";
    const Geometry g = geometry(p, in_len, block_size, true);
    if (!static_lanes_fit(g, block_size, 1)) // as redux_context_static_encode_dev
        return "";
    const ContextEncKernel k = pick_context_encode_kernel(p, g.nblocks);
    if (k.waves == 4)
        return k.cb32 ? "k_encode_context_static<true, 4> (code_bits 32, 4 waves per group)"
                      : "k_encode_context_static<false, 4> (code_bits < 32, 4 waves per group)";
    return k.cb32 ? "k_encode_context_static<true, 8> (code_bits 32, 8 waves per group)"
                  : "k_encode_context_static<false, 8> (code_bits < 32, 8 waves per group)";
}

const char *redux_context_static_decode_kernel_name(const redux_params *p, uint32_t total, uint64_t nblocks)
{
    if (context_static_check(p, total) != REDUX_OK || nblocks == 0) // (no blocks: the call launches nothing)
        return "";
    switch (pick_context_decode_kernel(nblocks)) {
    case 4: return "k_decode_context_static<4> (4 waves per group)";
    case 8: return "k_decode_context_static<8> (8 waves per group)";
    default: return "k_decode_context_static<16> (16 waves per group)";
    }
}

static void launch_context_encode(const ContextEncKernel &k, uint32_t grid, const ContextEncArgs &a, hipStream_t s)
{
    switch (k.waves * 2 + (k.cb32 ? 1 : 0)) {
    case 8: k_encode_context_static<false, 4><<<grid, 256, 0, s>>>(a); break;
    case 9: k_encode_context_static<true, 4><<<grid, 256, 0, s>>>(a); break;
    case 17: k_encode_context_static<true, 8><<<grid, 512, 0, s>>>(a); break;
    default: k_encode_context_static<false, 8><<<grid, 512, 0, s>>>(a); break;
    }
}

int redux_context_static_encode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, uint64_t in_len,
                                    uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status,
                                    void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = context_static_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || (!d_in && in_len) || !d_block_status || !d_workspace || (((uintptr_t)d_workspace) & 255))
        return REDUX_INVALID_INPUT;
    const Geometry g = geometry(p, in_len, block_size, true);
    if (workspace_bytes < kCtxHead + g.total)
        return REDUX_OUTPUT_TOO_SMALL;
    if (!static_lanes_fit(g, block_size, 1))
        return REDUX_UNSUPPORTED;
    hipStream_t s    = (hipStream_t)stream;
    uint8_t    *head = (uint8_t *)d_workspace, *ws = head + kCtxHead;
    if ((st = context_image(d_cum, total, head, s)) != REDUX_OK)
        return st;
    HIP_TRY(hipMemsetAsync(ws + g.off_mode, 0, 256, s)); // linear slots, stream byte order
    ContextEncArgs a;
    a.c            = static_enc_args(g, p, d_in, in_len, block_size, ws, d_block_status, total);
    a.image        = (const uint16_t *)head;
    a.bad          = (const uint32_t *)(head + kCtxImageBytes);
    a.total        = total;
    const ContextEncKernel k = pick_context_encode_kernel(p, g.nblocks);
    const uint64_t groups = ((g.nblocks + 63) / 64 + k.waves - 1) / k.waves, cus = cu_count();
    const uint32_t grid   = (uint32_t)(groups < cus ? groups : cus);
    launch_context_encode(k, grid, a, s);
    HIP_TRY(hipGetLastError());
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, ws, workspace_bytes - kCtxHead, stream, BlockTable{}, RawCopy{});
}

int redux_context_static_decode_dev(const redux_params *p, const void *d_cum, uint32_t total, const void *d_in, const void *d_in_offsets,
                                    uint64_t nblocks, uint32_t block_size, void *d_out, uint64_t out_cap, void *d_out_sizes,
                                    void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = context_static_check(p, total);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !d_cum || !d_in_offsets || !d_out_sizes || !d_block_status || !d_workspace || (((uintptr_t)d_workspace) & 255))
        return REDUX_INVALID_INPUT;
    if (nblocks == 0)
        return REDUX_OK;
    if (out_cap < nblocks * (uint64_t)block_size || workspace_bytes < kCtxHead)
        return REDUX_OUTPUT_TOO_SMALL;
    hipStream_t s    = (hipStream_t)stream;
    uint8_t    *head = (uint8_t *)d_workspace;
    if ((st = context_image(d_cum, total, head, s)) != REDUX_OK)
        return st;
    ContextDecArgs a;
    a.c            = static_dec_args(p, d_in, d_in_offsets, nblocks, block_size, d_out, d_out_sizes, d_block_status, total);
    a.image        = (const uint16_t *)head;
    a.bad          = (const uint32_t *)(head + kCtxImageBytes);
    a.total        = total;
    const uint32_t W      = pick_context_decode_kernel(nblocks);
    const uint64_t groups = ((nblocks + 63) / 64 + W - 1) / W, cus = cu_count();
    const uint32_t grid   = (uint32_t)(groups < cus ? groups : cus);
    switch (W) {
    case 4: k_decode_context_static<4><<<grid, 256, 0, s>>>(a); break;
    case 8: k_decode_context_static<8><<<grid, 512, 0, s>>>(a); break;
    default: k_decode_context_static<16><<<grid, 1024, 0, s>>>(a); break;
    }
    if (d_summary)
        k_summarize<<<64, 256, 0, s>>>((const int32_t *)d_block_status, nblocks, (int32_t *)d_summary);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// The coders of the chunked host calls: 258 KiB of tables in front of each chunk's workspace (stage_tables).  Chunks are whole
// blocks and blocks are independent, so a chunk needs nothing from its neighbours.
constexpr uint64_t kCtxTablesBytes = (uint64_t)kCtxTables * kStaticEntries * 4;

static host::EncodeCoder context_static_encoder(const redux_params *p, const uint32_t *cum, uint32_t block_size)
{
    const uint32_t total = redux_context_static_total(cum);
    return {[=](uint64_t max_in, bool, uint64_t &ws, uint64_t &bound) {
                ws    = tables_bytes(kCtxTablesBytes) + redux_context_static_encode_workspace_bytes(p, max_in, block_size);
                bound = redux_context_static_encode_bound(p, max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *d_cum, uint64_t ws_bytes, hipStream_t st) -> int {
                uint8_t  *ws = (uint8_t *)d_cum;
                const int rc = stage_tables(cum, kCtxTablesBytes, ws, ws_bytes, st);
                if (rc != REDUX_OK)
                    return rc;
                return redux_context_static_encode_dev(p, d_cum, total, s.d_in.p, len, block_size, s.d_out.p, bound, s.d_off.p,
                                                       s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            }};
}

static host::DecodeCoder context_static_decoder(const redux_params *p, const uint32_t *cum, uint32_t block_size)
{
    const uint32_t total = redux_context_static_total(cum);
    return {[=](uint64_t cb) { return tables_bytes(kCtxTablesBytes) + redux_context_static_decode_workspace_bytes(p, cb, block_size); },
            [=](host::Slot &s, uint64_t nb, uint64_t out_bytes, void *, void *d_cum, uint64_t ws_bytes, hipStream_t st) -> int {
                uint8_t  *ws = (uint8_t *)d_cum;
                const int rc = stage_tables(cum, kCtxTablesBytes, ws, ws_bytes, st);
                if (rc != REDUX_OK)
                    return rc;
                return redux_context_static_decode_dev(p, d_cum, total, s.d_in.p, s.d_off.p, nb, block_size, s.d_out.p, out_bytes,
                                                       s.d_sz.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            }};
}

int redux_context_static_encode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, uint64_t in_len,
                                           uint32_t block_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                                           int32_t *block_status, uint32_t *block_crc)
{
    int st = redux_context_static_table_check(p, cum);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status, context_static_encoder(p, cum, block_size),
                               block_crc); // redux_host.hpp
}

int redux_context_static_decode_blocks_crc(const redux_params *p, const uint32_t *cum, const uint8_t *in, const uint64_t *in_offsets,
                                           uint64_t nblocks, uint32_t block_size, uint8_t *out, uint64_t out_cap, uint32_t *out_sizes,
                                           int32_t *block_status, uint32_t *block_crc)
{
    const int st = redux_context_static_table_check(p, cum);
    if (st != REDUX_OK)
        return st;
    return decode_blocks_host(st, in, in_offsets, nblocks, block_size, out, nblocks * (uint64_t)block_size, out_cap, out_sizes,
                              block_status, nullptr, context_static_decoder(p, cum, block_size), block_crc);
}

// ---- stored blocks (redux_store.hpp) --------------------------------------------------------------
// the adaptive model with 8-bit symbols and code_bits <= 32: the coders whose decoders have the table form
static int stored_check(const redux_params *p, uint32_t block_size, uint32_t element_size)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (redux_planes_check(element_size) != REDUX_OK || block_size == 0)
        return REDUX_INVALID_INPUT;
    return is_any(p) ? REDUX_UNSUPPORTED : REDUX_OK;
}

uint64_t redux_encode_stored_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    if (stored_check(p, block_size, element_size) != REDUX_OK)
        return 0;
    return redux_encode_planes_workspace_bytes(p, in_len, block_size, element_size);
}

// [plane buffer (E > 1)] [the coded blocks' table] [the adaptive decoder's workspace]
static uint64_t store_table_bytes(uint64_t nblocks) { return align_up(nblocks * sizeof(redux_block), 256); }

uint64_t redux_decode_stored_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    if (stored_check(p, block_size, element_size) != REDUX_OK)
        return 0;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    return Layout{element_size}.copy_bytes(nblocks * (uint64_t)block_size) + store_table_bytes(nblocks) +
           redux_decode_workspace_bytes(p, nblocks, block_size);
}

// the plain coder over x' (the input, or its layout at the front of the workspace), then the rule, then the scan and the
// compaction, which copies x' for the stored blocks
int redux_encode_stored_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                            uint32_t store_ratio, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_stored,
                            void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = stored_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (store_ratio > kStoreRatioOne || !d_workspace || !d_stored || !d_block_status || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    hipStream_t s = (hipStream_t)stream;
    Staged      staged; // (the coder checks the rest: a workspace without the small-grid pairs area will do, geometry_ws)
    if ((st = layout_stage(Layout{element_size}, d_in, in_len, block_size, d_workspace, workspace_bytes, stream, staged)) != REDUX_OK)
        return st;
    const void    *x   = staged.x;
    uint8_t       *ws  = staged.ws;
    const uint64_t wsb = staged.ws_bytes;
    Geometry       g;
    if ((st = encode_plan(p, in_len, block_size, wsb, g)) != REDUX_OK)
        return st;
    if ((st = encode_slots_impl(g, p, x, in_len, block_size, BlockTable{}, d_block_status, ws, wsb, stream, nullptr)) != REDUX_OK)
        return st;
    StoreSelectArgs sa;
    sa.status     = (const int32_t *)d_block_status;
    sa.sizes      = (uint32_t *)(ws + g.off_sizes);
    sa.stored     = (uint8_t *)d_stored;
    sa.nblocks    = g.nblocks;
    sa.in_len     = in_len;
    sa.block_size = block_size;
    sa.ratio      = store_ratio;
    const uint64_t wgs = (g.nblocks + 255) / 256;
    k_store_select<<<(uint32_t)(wgs < 1024 ? wgs : 1024), 256, 0, s>>>(sa);
    HIP_TRY(hipGetLastError());
    return compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, ws, wsb, stream, BlockTable{},
                        RawCopy{(const uint8_t *)d_stored, x, block_size});
}

// coded blocks through the table form of the adaptive decoders, stored ones copied, into T (d_out, or the plane buffer);
// then the length rule, the inverse layout and the summary
int redux_decode_stored_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_stored,
                            uint64_t out_len, uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap,
                            void *d_out_sizes, void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes,
                            void *stream)
{
    int st = stored_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (!d_workspace || !d_in_offsets || !d_stored || !d_out_sizes || !d_block_status || (out_len && !d_out))
        return REDUX_INVALID_INPUT;
    if (out_cap < out_len || workspace_bytes < redux_decode_stored_workspace_bytes(p, out_len, block_size, element_size))
        return REDUX_OUTPUT_TOO_SMALL;
    if (((uintptr_t)d_workspace) & 255)
        return REDUX_INVALID_INPUT;
    hipStream_t    s       = (hipStream_t)stream;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const Layout   L{element_size};
    const uint64_t copy    = L.copy_bytes(nblocks * (uint64_t)block_size);
    uint8_t       *t       = L.identity() ? (uint8_t *)d_out : (uint8_t *)d_workspace;
    redux_block   *table   = (redux_block *)((uint8_t *)d_workspace + copy);
    uint8_t       *dws     = (uint8_t *)table + store_table_bytes(nblocks);

    StoreTableArgs ta;
    ta.stored     = (const uint8_t *)d_stored;
    ta.table      = table;
    ta.nblocks    = nblocks;
    ta.out_len    = out_len;
    ta.block_size = block_size;
    k_store_table<<<1, 1024, 0, s>>>(ta);
    HIP_TRY(hipGetLastError());
    // (the library's own table, coded blocks first: no k_table_check, whose "a block no entry codes" rule is wrong here)
    st = decode_blocks_dev_impl(p, d_in, d_in_offsets, nblocks, block_size, t, out_len, d_out_sizes, d_block_status, nullptr, dws,
                                workspace_bytes - (uint64_t)(dws - (uint8_t *)d_workspace), stream, nullptr,
                                BlockTable{table, (block_size & 15) == 0, nblocks, true});
    if (st != REDUX_OK)
        return st;
    StoreUnpackArgs ua;
    ua.in         = (const uint8_t *)d_in;
    ua.in_offsets = (const uint64_t *)d_in_offsets;
    ua.stored     = (const uint8_t *)d_stored;
    ua.out        = t;
    ua.out_sizes  = (uint32_t *)d_out_sizes;
    ua.status     = (int32_t *)d_block_status;
    ua.nblocks    = nblocks;
    ua.out_len    = out_len;
    ua.block_size = block_size;
    k_store_unpack<<<(uint32_t)nblocks, 256, 0, s>>>(ua);
    return layout_decode_tail(L, L.identity() ? nullptr : t, d_out, out_len, block_size, d_out_sizes, d_block_status, d_summary,
                              TailSummary::ZeroSummarize, stream);
}

// the chunked host calls: flags travel in the slot's d_stf (redux_host.hpp)
static host::EncodeCoder stored_encoder(const redux_params *p, uint32_t block_size, uint32_t element_size, uint32_t store_ratio)
{
    const host::EncodeCoder plain = adaptive_encoder(p, block_size);
    return {[=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
                plain.size(max_in, several, ws, bound);
                ws += Layout{element_size}.copy_bytes(max_in);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_encode_stored_dev(p, s.d_in.p, len, block_size, element_size, store_ratio, s.d_out.p, bound, s.d_off.p,
                                               s.d_stf.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            }};
}

static host::DecodeCoder stored_decoder(const redux_params *p, uint32_t block_size, uint32_t element_size)
{
    return {[=](uint64_t cb) { return redux_decode_stored_workspace_bytes(p, cb * (uint64_t)block_size, block_size, element_size); },
            [=](host::Slot &s, uint64_t, uint64_t out_bytes, void *, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_decode_stored_dev(p, s.d_in.p, s.d_off.p, s.d_stf.p, out_bytes, block_size, element_size, s.d_out.p,
                                               out_bytes, s.d_sz.p, s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            },
            true};
}

int redux_encode_blocks_stored(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                               uint32_t store_ratio, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, uint8_t *stored,
                               int32_t *block_status, uint32_t *block_crc)
{
    int st = stored_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (store_ratio > kStoreRatioOne || !out || !out_offsets || !stored || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status,
                               stored_encoder(p, block_size, element_size, store_ratio), block_crc, stored); // redux_host.hpp
}

int redux_decode_blocks_stored(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *stored,
                               uint64_t out_len, uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap,
                               uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    int st = stored_check(p, block_size, element_size);
    if (st == REDUX_OK && !stored)
        st = REDUX_INVALID_INPUT;
    return decode_blocks_host(st, in, in_offsets, redux_block_count(out_len, block_size), block_size, out, out_len, out_cap, out_sizes,
                              block_status, nullptr, stored_decoder(p, block_size, element_size), block_crc, stored);
}

// ---- constant blocks (redux_const.hpp) ------------------------------------------------------------
// the coders of stored blocks: the ones whose kernels have the table form in both directions
static int const_check(const redux_params *p, uint32_t block_size, uint32_t element_size) { return stored_check(p, block_size, element_size); }

// x' of a call: the byte-plane layout, behind the XOR against the base when there is one (base_len 0: no base)
static Layout const_layout(uint32_t element_size, const void *d_base, uint64_t base_len)
{
    return base_len ? Layout{element_size, Filter::BaseXor, d_base, base_len} : Layout{element_size};
}

static int launch_const_select(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_flags, hipStream_t s)
{
    ConstSelectArgs a;
    a.in         = (const uint8_t *)d_in;
    a.flags      = (uint8_t *)d_flags;
    a.nblocks    = redux_block_count(in_len, block_size);
    a.in_len     = in_len;
    a.block_size = block_size;
    const uint64_t wgs = (a.nblocks + kConstWaves - 1) / kConstWaves;
    k_const_select<<<(uint32_t)(wgs < (1u << 20) ? wgs : (1u << 20)), 64 * kConstWaves, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_const_blocks_dev(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_flags, void *stream)
{
    if (block_size == 0 || !d_flags || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    return launch_const_select(d_in, in_len, block_size, d_flags, (hipStream_t)stream);
}

static uint64_t const_front_bytes(uint64_t in_len, uint32_t block_size)
{
    return planes_copy_bytes(in_len) + store_table_bytes(redux_block_count(in_len, block_size));
}

// [x' (always: the size does not depend on whether a base is given)] [the coder blocks' table] [the adaptive encoder's
// workspace for whole blocks: the table form sizes its launch by entries, redux_encode_blocks_v_dev]
uint64_t redux_encode_const_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    if (const_check(p, block_size, element_size) != REDUX_OK)
        return 0;
    return const_front_bytes(in_len, block_size) +
           redux_encode_workspace_bytes(p, redux_block_count(in_len, block_size) * (uint64_t)block_size, block_size);
}

// [plane buffer (always)] [the coder blocks' table] [the adaptive decoder's workspace]
uint64_t redux_decode_const_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size, uint32_t element_size)
{
    if (const_check(p, block_size, element_size) != REDUX_OK)
        return 0;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    return planes_copy_bytes(nblocks * (uint64_t)block_size) + store_table_bytes(nblocks) + redux_decode_workspace_bytes(p, nblocks, block_size);
}

// the layout, the detection, the table of the blocks that are left, the table form of the coder over it, then size 1 for
// the constant blocks, the scan, the compaction of the coded streams and the constant blocks' bytes
int redux_encode_const_dev(const redux_params *p, const void *d_in, uint64_t in_len, const void *d_base, uint64_t base_len,
                           uint32_t block_size, uint32_t element_size, void *d_out, uint64_t out_cap, void *d_out_offsets,
                           void *d_const, void *d_block_status, void *d_summary, void *d_workspace, uint64_t workspace_bytes,
                           void *stream)
{
    int st = const_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (!d_workspace || !d_const || !d_block_status || !d_out || !d_out_offsets || (in_len && !d_in) || (base_len && !d_base))
        return REDUX_INVALID_INPUT;
    if (in_len > 0xFFFFFFFFull) // the table encoder's lane offsets into x' are 32-bit
        return REDUX_UNSUPPORTED;
    if (workspace_bytes < const_front_bytes(in_len, block_size)) // (the coder checks its own part: geometry_ws)
        return REDUX_OUTPUT_TOO_SMALL;
    if (((uintptr_t)d_workspace) & 255)
        return REDUX_INVALID_INPUT;
    hipStream_t  s = (hipStream_t)stream;
    const Layout L = const_layout(element_size, d_base, base_len);
    if (in_len == 0) { // one empty block, never constant: the call without the option
        HIP_TRY(hipMemsetAsync(d_const, 0, 1, s));
        return encode_layout_dev(L, p, d_in, in_len, block_size, d_out, out_cap, d_out_offsets, d_block_status, d_summary,
                                 d_workspace, workspace_bytes, stream);
    }
    const uint64_t nblocks = redux_block_count(in_len, block_size);
    const uint64_t copy    = planes_copy_bytes(in_len);
    const void    *x       = d_in;
    if (!L.identity()) {
        if ((st = L.forward(d_in, d_workspace, in_len, block_size, stream)) != REDUX_OK)
            return st;
        x = d_workspace;
    }
    redux_block   *table = (redux_block *)((uint8_t *)d_workspace + copy);
    uint8_t       *ws    = (uint8_t *)table + store_table_bytes(nblocks);
    const uint64_t wsb   = workspace_bytes - (uint64_t)(ws - (uint8_t *)d_workspace);
    if ((st = launch_const_select(x, in_len, block_size, d_const, s)) != REDUX_OK)
        return st;
    StoreTableArgs ta;
    ta.stored     = (const uint8_t *)d_const;
    ta.table      = table;
    ta.nblocks    = nblocks;
    ta.out_len    = in_len;
    ta.block_size = block_size;
    k_const_table<<<1, 1024, 0, s>>>(ta);
    HIP_TRY(hipGetLastError());
    Geometry g; // (the table form sizes its launch by entries: here one per block)
    if ((st = encode_plan(p, nblocks * (uint64_t)block_size, block_size, wsb, g)) != REDUX_OK)
        return st;
    const BlockTable left = {table, (block_size & 15) == 0, nblocks, false};
    CheckedTable     checked;
    if ((st = encode_slots_impl(g, p, x, in_len, block_size, left, d_block_status, ws, wsb, stream, &checked)) != REDUX_OK)
        return st;
    ConstPlaceArgs pa;
    pa.flags      = (const uint8_t *)d_const;
    pa.raw        = (const uint8_t *)x;
    pa.sizes      = (uint32_t *)(ws + g.off_sizes);
    pa.status     = (int32_t *)d_block_status;
    pa.offsets    = (const uint64_t *)d_out_offsets;
    pa.out        = (uint8_t *)d_out;
    pa.out_cap    = out_cap;
    pa.summary    = (int32_t *)d_summary;
    pa.nblocks    = nblocks;
    pa.block_size = block_size;
    const uint64_t wgs  = (nblocks + 255) / 256;
    const uint32_t grid = (uint32_t)(wgs < 1024 ? wgs : 1024);
    k_const_sizes<<<grid, 256, 0, s>>>(pa);
    HIP_TRY(hipGetLastError());
    // (from here on the table is its checked copy in the coder's workspace)
    if ((st = compact_with(g, d_out, out_cap, d_out_offsets, d_block_status, d_summary, ws, wsb, stream,
                           BlockTable{checked.entries, left.aligned16, nblocks, true}, RawCopy{})) != REDUX_OK)
        return st;
    k_const_place<<<grid, 256, 0, s>>>(pa);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// coded blocks through the table form of the adaptive decoders, constant ones filled, into the plane buffer (d_out where
// the layout is the identity); then the length rule, the inverse layout and filter, and the summary
int redux_decode_const_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_const,
                           const void *d_base, uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                           void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary, void *d_workspace,
                           uint64_t workspace_bytes, void *stream)
{
    int st = const_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (!d_workspace || !d_in_offsets || !d_const || !d_out_sizes || !d_block_status || (out_len && !d_out) || (base_len && !d_base))
        return REDUX_INVALID_INPUT;
    if (workspace_bytes < redux_decode_const_workspace_bytes(p, out_len, block_size, element_size))
        return REDUX_OUTPUT_TOO_SMALL;
    if (((uintptr_t)d_workspace) & 255)
        return REDUX_INVALID_INPUT;
    hipStream_t    s       = (hipStream_t)stream;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const Layout   L       = const_layout(element_size, d_base, base_len);
    const uint64_t copy    = planes_copy_bytes(nblocks * (uint64_t)block_size);
    uint8_t       *t       = L.identity() ? (uint8_t *)d_out : (uint8_t *)d_workspace;
    redux_block   *table   = (redux_block *)((uint8_t *)d_workspace + copy);
    uint8_t       *dws     = (uint8_t *)table + store_table_bytes(nblocks);

    StoreTableArgs ta;
    ta.stored     = (const uint8_t *)d_const;
    ta.table      = table;
    ta.nblocks    = nblocks;
    ta.out_len    = out_len;
    ta.block_size = block_size;
    k_const_table<<<1, 1024, 0, s>>>(ta);
    HIP_TRY(hipGetLastError());
    // (the library's own table, as in redux_decode_stored_dev: no k_table_check)
    st = decode_blocks_dev_impl(p, d_in, d_in_offsets, nblocks, block_size, t, out_len, d_out_sizes, d_block_status, nullptr, dws,
                                workspace_bytes - (uint64_t)(dws - (uint8_t *)d_workspace), stream, nullptr,
                                BlockTable{table, (block_size & 15) == 0, nblocks, true});
    if (st != REDUX_OK)
        return st;
    ConstFillArgs fa;
    fa.in         = (const uint8_t *)d_in;
    fa.in_offsets = (const uint64_t *)d_in_offsets;
    fa.flags      = (const uint8_t *)d_const;
    fa.out        = t;
    fa.out_sizes  = (uint32_t *)d_out_sizes;
    fa.status     = (int32_t *)d_block_status;
    fa.nblocks    = nblocks;
    fa.out_len    = out_len;
    fa.block_size = block_size;
    k_const_fill<<<(uint32_t)nblocks, 256, 0, s>>>(fa);
    HIP_TRY(hipGetLastError());
    return layout_decode_tail(L, L.identity() ? nullptr : t, d_out, out_len, block_size, d_out_sizes, d_block_status, d_summary,
                              TailSummary::ZeroSummarize, stream);
}

// the chunked host calls: flags travel in the slot's d_stf as the stored flags do, a chunk's share of the base in its d_base
static host::EncodeCoder const_encoder(const redux_params *p, uint32_t block_size, uint32_t element_size, bool with_base)
{
    const host::EncodeCoder plain = adaptive_encoder(p, block_size);
    return {[=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
                plain.size(redux_block_count(max_in, block_size) * (uint64_t)block_size, several, ws, bound);
                ws += const_front_bytes(max_in, block_size);
            },
            [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_encode_const_dev(p, s.d_in.p, len, with_base ? s.d_base.p : nullptr, with_base ? s.base_len : 0,
                                              block_size, element_size, s.d_out.p, bound, s.d_off.p, s.d_stf.p, s.d_st.p, s.d_sum.p,
                                              ws, ws_bytes, st);
            }};
}

static host::DecodeCoder const_decoder(const redux_params *p, uint32_t block_size, uint32_t element_size, bool with_base)
{
    return {[=](uint64_t cb) { return redux_decode_const_workspace_bytes(p, cb * (uint64_t)block_size, block_size, element_size); },
            [=](host::Slot &s, uint64_t, uint64_t out_bytes, void *, void *ws, uint64_t ws_bytes, hipStream_t st) {
                return redux_decode_const_dev(p, s.d_in.p, s.d_off.p, s.d_stf.p, with_base ? s.d_base.p : nullptr,
                                              with_base ? s.base_len : 0, out_bytes, block_size, element_size, s.d_out.p, s.d_sz.p,
                                              s.d_st.p, s.d_sum.p, ws, ws_bytes, st);
            },
            true};
}

int redux_encode_blocks_const(const redux_params *p, const uint8_t *in, uint64_t in_len, const uint8_t *base, uint64_t base_len,
                              uint32_t block_size, uint32_t element_size, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets,
                              uint8_t *const_flags, int32_t *block_status, uint32_t *block_crc)
{
    int st = const_check(p, block_size, element_size);
    if (st != REDUX_OK)
        return st;
    if (!out || !out_offsets || !const_flags || (in_len && !in) || (base_len && !base))
        return REDUX_INVALID_INPUT;
    const bool with_base = base_len != 0;
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status,
                               const_encoder(p, block_size, element_size, with_base), block_crc, const_flags, {},
                               host::BaseIo{base, base_len, with_base}); // redux_host.hpp
}

int redux_decode_blocks_const(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *const_flags,
                              const uint8_t *base, uint64_t base_len, uint64_t out_len, uint32_t block_size, uint32_t element_size,
                              uint8_t *out, uint32_t *out_sizes, int32_t *block_status, uint32_t *block_crc)
{
    int st = const_check(p, block_size, element_size);
    if (st == REDUX_OK && (!const_flags || (base_len && !base)))
        st = REDUX_INVALID_INPUT;
    const bool with_base = base_len != 0;
    return decode_blocks_host(st, in, in_offsets, redux_block_count(out_len, block_size), block_size, out, out_len, out_len, out_sizes,
                              block_status, nullptr, const_decoder(p, block_size, element_size, with_base), block_crc, const_flags, {},
                              host::BaseIo{base, base_len, with_base});
}

// ---- per-block CRC-32 (redux_crc.hpp) -------------------------------------------------------------
int redux_crc32_blocks_dev(const void *d_in, uint64_t in_len, uint32_t block_size, void *d_crc, void *stream)
{
    if (block_size == 0 || !d_crc || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    return launch_crc32(d_in, in_len, nullptr, redux_block_count(in_len, block_size), block_size, d_crc, (hipStream_t)stream);
}

int redux_crc32_sizes_dev(const void *d_in, uint64_t nblocks, uint32_t block_size, const void *d_sizes, void *d_crc, void *stream)
{
    if (block_size == 0 || (nblocks && (!d_in || !d_sizes || !d_crc)))
        return REDUX_INVALID_INPUT;
    return launch_crc32(d_in, 0, d_sizes, nblocks, block_size, d_crc, (hipStream_t)stream);
}

uint32_t redux_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2)
{
    uint32_t p = 0x80000000u, sq = 0x80000000u; // x^0; then sq = x^(8 * 2^k)
    for (int i = 0; i < 8; i++)
        sq = crc_mulx(sq);
    for (; len2; len2 >>= 1) {
        if (len2 & 1)
            p = crc_mulmod(sq, p);
        sq = crc_mulmod(sq, sq);
    }
    return crc_mulmod(p, crc1) ^ crc2;
}

int redux_crc32_blocks(const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t *crc)
{
    if (block_size == 0 || !crc || (in_len && !in))
        return REDUX_INVALID_INPUT;
    return host::crc32_blocks(in, in_len, block_size, crc); // redux_host.hpp
}

int redux_host_release(void) { return host::ctx_release_all(); }

int redux_host_set_devices(const int32_t *device_ids, uint32_t n) { return host::set_devices(device_ids, n); }

int redux_host_set_chunk_bytes(uint64_t min_bytes, uint64_t max_bytes)
{
    if (max_bytes && max_bytes < min_bytes)
        return REDUX_INVALID_INPUT;
    host::g_chunk_min.store(min_bytes);
    host::g_chunk_max.store(max_bytes);
    return REDUX_OK;
}

int redux_host_chunk_plan(uint64_t nblocks, uint32_t block_size, uint32_t ncontexts, int decode, uint64_t *chunk_blocks,
                          uint64_t *nchunks)
{
    if (nblocks == 0 || block_size == 0 || ncontexts == 0 || ncontexts > 16 || !chunk_blocks || !nchunks)
        return REDUX_INVALID_INPUT;
    *chunk_blocks = host::chunk_blocks_for(nblocks, block_size, decode ? host::kDecChunkMax : host::kEncChunkMax, ncontexts);
    *nchunks      = (nblocks + *chunk_blocks - 1) / *chunk_blocks;
    return REDUX_OK;
}

int redux_host_chunk_plan_record(uint64_t nblocks, uint32_t block_size, uint32_t record_size, uint32_t ncontexts, int decode,
                                 uint64_t *chunk_blocks, uint64_t *nchunks)
{
    if (redux_record_check(record_size, 0) != REDUX_OK)
        return REDUX_INVALID_INPUT;
    const int st = redux_host_chunk_plan(nblocks, block_size, ncontexts, decode, chunk_blocks, nchunks);
    if (st != REDUX_OK)
        return st;
    *chunk_blocks = host::chunk_blocks_framed(*chunk_blocks, nblocks, record_size);
    *nchunks      = (nblocks + *chunk_blocks - 1) / *chunk_blocks;
    return REDUX_OK;
}

uint64_t redux_host_allocations(void)
{
    uint64_t n = 0;
    for (host::Ctx &c : host::g_ctx) {
        std::lock_guard<std::mutex> l(c.mu);
        n += c.allocs;
    }
    return n;
}

uint64_t redux_host_resident_bytes(void)
{
    uint64_t n = 0;
    for (host::Ctx &c : host::g_ctx) {
        std::lock_guard<std::mutex> l(c.mu);
        if (!c.ready)
            continue;
        for (host::Slot &s : c.slot)
            for (const host::Buf *b : s.bufs())
                n += b->pinned ? 0 : b->cap;
    }
    return n;
}

/* Diagnostic: timeline of the last host-pointer call on the current device (redux_host.hpp, Ctx::trace). */
uint64_t redux_host_trace(double *out, uint64_t cap)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16)
        return 0;
    host::Ctx &c = host::g_ctx[dev];
    std::lock_guard<std::mutex> l(c.mu);
    const uint64_t n = c.trace.size() < cap ? c.trace.size() : cap;
    for (uint64_t i = 0; i < n; i++)
        out[i] = c.trace[i];
    return c.trace.size();
}

int redux_gen_iid_dev(void *d_out, uint64_t len, uint64_t first_byte, uint64_t seed, void *stream)
{
    if (len == 0)
        return REDUX_OK;
    k_gen_iid<<<2048, 256, 0, (hipStream_t)stream>>>((uint8_t *)d_out, len, first_byte, seed);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_gen_zipf_dev(void *d_out, uint64_t len, uint64_t first_byte, uint64_t seed, void *stream)
{
    if (len == 0)
        return REDUX_OK;
    k_gen_zipf<<<2048, 256, 0, (hipStream_t)stream>>>((uint8_t *)d_out, len, first_byte, seed);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

const uint32_t *redux_zipf_thresholds(void) { return h_zipf; }

// ---- size estimates (redux_cost.hpp) ---------------------------------------------------------------------------------
// what the adaptive estimate needs of the parameters: the fast kernels' model (8-bit symbols, code_bits <= 32), and a block
// of `longest` bytes that cannot freeze it: the total starts at 257 and grows by one per symbol, and a frozen model's cost
// depends on the order of the bytes
static int adaptive_cost_check(const redux_params *p, uint64_t longest)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (is_any(p) || 256 + longest >= (1ull << p->freq_bits) - 1)
        return REDUX_UNSUPPORTED;
    return REDUX_OK;
}

int redux_adaptive_cost_from_counts(const redux_params *p, const uint64_t *counts, uint64_t n, double *bits)
{
    if (!p || (n && (!counts || !bits)))
        return REDUX_INVALID_INPUT;
    uint64_t longest = 0;
    for (uint64_t r = 0; r < n; r++) {
        unsigned __int128 sum = 0;
        for (int s = 0; s < 256; s++)
            sum += counts[256 * r + s];
        const uint64_t len = sum >> 62 ? 1ull << 62 : (uint64_t)sum; // (saturated: any such row freezes the model)
        longest = len > longest ? len : longest;
    }
    int st = adaptive_cost_check(p, longest);
    if (st != REDUX_OK)
        return st;
    int          sign;
    const double lg257 = lgamma_r(257.0, &sign);
    for (uint64_t r = 0; r < n; r++) {
        uint64_t len = 0;
        double   sum = 0;
        for (int s = 0; s < 256; s++) {
            const uint64_t c = counts[256 * r + s];
            len += c;
            if (c > 1)
                sum += lgamma_r((double)c + 1.0, &sign);
        }
        bits[r] = (lgamma_r((double)len + 258.0, &sign) - lg257 - sum) * kInvLn2;
    }
    return REDUX_OK;
}

int redux_table_cost_from_counts(const uint64_t *counts, const uint32_t *cum, uint64_t n, double *bits)
{
    if (n && (!counts || !cum || !bits))
        return REDUX_INVALID_INPUT;
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t *c = counts + 256 * r;
        const uint32_t *t = cum + 258 * r;
        const uint32_t  T = t[257];
        const double    log2T = T ? log2((double)T) : 0.0;
        double          sum = 0;
        for (int s = 0; s < 256; s++)
            sum += table_cost_term(c[s], t[s], t[s + 1], log2T);
        bits[r] = T ? sum : INFINITY;
    }
    return REDUX_OK;
}

int redux_block_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, void *d_bits, void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || !d_bits || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    BlockCostArgs a;
    a.in         = (const uint8_t *)d_in;
    a.in_len     = in_len;
    a.nblocks    = redux_block_count(in_len, block_size);
    a.block_size = block_size;
    a.bits       = (double *)d_bits;
    const uint64_t cap  = (uint64_t)kHistWgsPerCu * cu_count();
    const uint32_t grid = (uint32_t)(a.nblocks < cap ? a.nblocks : cap);
    k_block_cost<<<grid, 64, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

int redux_layout_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t layouts,
                          void *d_bits, void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || layouts == 0 || layouts > 0xFF || !d_bits || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    hipStream_t s = (hipStream_t)stream;
    for (uint32_t e = 0; e < 4 && st == REDUX_OK; e++) {
        const bool plain = layouts >> e & 1, delta = layouts >> (4 + e) & 1;
        if (!plain && !delta)
            continue;
        switch (e) {
        case 0: st = launch_layout_cost<1>(d_in, in_len, block_size, plain, delta, (double *)d_bits, s); break;
        case 1: st = launch_layout_cost<2>(d_in, in_len, block_size, plain, delta, (double *)d_bits, s); break;
        case 2: st = launch_layout_cost<4>(d_in, in_len, block_size, plain, delta, (double *)d_bits, s); break;
        default: st = launch_layout_cost<8>(d_in, in_len, block_size, plain, delta, (double *)d_bits, s); break;
        }
    }
    return st;
}

const char *redux_layout_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t layout)
{
    static const char *const names[4][3] = {
        {"k_layout_cost<1>", "k_layout_cost<1> + k_layout_cost_bytes<1>", "k_layout_cost_bytes<1>"},
        {"k_layout_cost<2>", "k_layout_cost<2> + k_layout_cost_bytes<2>", "k_layout_cost_bytes<2>"},
        {"k_layout_cost<4>", "k_layout_cost<4> + k_layout_cost_bytes<4>", "k_layout_cost_bytes<4>"},
        {"k_layout_cost<8>", "k_layout_cost<8> + k_layout_cost_bytes<8>", "k_layout_cost_bytes<8>"},
    };
    if (block_size == 0 || block_size > (1u << 30) || layout > 7)
        return "";
    const uint32_t e = layout & 3, E = 1u << e;
    const uint64_t nfull = layout_cost_full_frames(d_in, in_len, block_size, E);
    return names[e][nfull == 0 ? 2 : nfull * E < redux_block_count(in_len, block_size) ? 1 : 0];
}

const char *redux_layout_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t layout)
{
    return redux_layout_cost_kernel_name_at(nullptr, in_len, block_size, layout);
}

uint64_t redux_lag_cost_block_count(uint64_t in_len, uint32_t block_size, uint32_t element_size, uint32_t frame_step)
{
    if (block_size == 0 || frame_step == 0 || redux_planes_check(element_size) != REDUX_OK)
        return 0;
    uint64_t row_blocks;
    lag_cost_selected(redux_block_count(in_len, block_size), element_size, frame_step, &row_blocks);
    return row_blocks;
}

int redux_lag_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                       const uint32_t *lags, uint32_t nlags, uint32_t frame_step, void *d_bits, void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || redux_planes_check(element_size) != REDUX_OK || !lags || nlags == 0 ||
        nlags > REDUX_LAG_MAX || frame_step == 0 || !d_bits || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    for (uint32_t j = 0; j < nlags; j++)
        if (redux_lag_check(element_size, lags[j]) != REDUX_OK)
            return REDUX_INVALID_INPUT;
    const int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    LagCostArgs a = {}; // (the list travels in the kernels' arguments: consumed before the call returns)
    a.ncand = nlags;
    for (uint32_t j = 0; j < nlags; j++)
        a.lags[j] = (uint16_t)lags[j];
    return for_element_size(element_size, [&](auto e) -> int {
        constexpr int E = decltype(e)::value;
        return launch_lag_cost<E>(k_lag_cost<E>, k_lag_cost_bytes<E>, a, d_in, in_len, block_size, frame_step, (double *)d_bits,
                                  (hipStream_t)stream);
    });
}

// what launch_lag_cost launches, from a family's names for E = 1, 2, 4, 8: {fast, both, bytes}
static const char *lag_cost_kernel_name(const char *const (&names)[4][3], const void *d_in, uint64_t in_len, uint32_t block_size,
                                        uint32_t element_size)
{
    if (block_size == 0 || block_size > (1u << 30) || redux_planes_check(element_size) != REDUX_OK)
        return "";
    const uint32_t E = element_size, e = E == 1 ? 0 : E == 2 ? 1 : E == 4 ? 2 : 3;
    const uint64_t nfull = layout_cost_full_frames(d_in, in_len, block_size, E);
    return names[e][nfull == 0 ? 2 : nfull * E < redux_block_count(in_len, block_size) ? 1 : 0];
}

const char *redux_lag_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    static const char *const names[4][3] = {
        {"k_lag_cost<1>", "k_lag_cost<1> + k_lag_cost_bytes<1>", "k_lag_cost_bytes<1>"},
        {"k_lag_cost<2>", "k_lag_cost<2> + k_lag_cost_bytes<2>", "k_lag_cost_bytes<2>"},
        {"k_lag_cost<4>", "k_lag_cost<4> + k_lag_cost_bytes<4>", "k_lag_cost_bytes<4>"},
        {"k_lag_cost<8>", "k_lag_cost<8> + k_lag_cost_bytes<8>", "k_lag_cost_bytes<8>"},
    };
    return lag_cost_kernel_name(names, d_in, in_len, block_size, element_size);
}

const char *redux_lag_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return redux_lag_cost_kernel_name_at(nullptr, in_len, block_size, element_size);
}

int redux_lag_order_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size,
                             const uint32_t *lags, const uint32_t *orders, uint32_t ncand, uint32_t frame_step, void *d_bits,
                             void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || redux_planes_check(element_size) != REDUX_OK || frame_step == 0 ||
        !d_bits || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    LagCostArgs a; // (the lists travel in the kernels' arguments: consumed before the call returns)
    if (!lag_order_cost_list(element_size, lags, orders, ncand, REDUX_LAG_ORDER_COST_MAX, a.lags, a.orders, redux_lag_order_check))
        return REDUX_INVALID_INPUT;
    a.ncand = ncand;
    const int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    return for_element_size(element_size, [&](auto e) -> int {
        constexpr int E = decltype(e)::value;
        return launch_lag_cost<E>(k_lag_order_cost<E>, k_lag_order_cost_bytes<E>, a, d_in, in_len, block_size, frame_step,
                                  (double *)d_bits, (hipStream_t)stream);
    });
}

const char *redux_lag_order_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    static const char *const names[4][3] = {
        {"k_lag_order_cost<1>", "k_lag_order_cost<1> + k_lag_order_cost_bytes<1>", "k_lag_order_cost_bytes<1>"},
        {"k_lag_order_cost<2>", "k_lag_order_cost<2> + k_lag_order_cost_bytes<2>", "k_lag_order_cost_bytes<2>"},
        {"k_lag_order_cost<4>", "k_lag_order_cost<4> + k_lag_order_cost_bytes<4>", "k_lag_order_cost_bytes<4>"},
        {"k_lag_order_cost<8>", "k_lag_order_cost<8> + k_lag_order_cost_bytes<8>", "k_lag_order_cost_bytes<8>"},
    };
    return lag_cost_kernel_name(names, d_in, in_len, block_size, element_size);
}

const char *redux_lag_order_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t element_size)
{
    return redux_lag_order_cost_kernel_name_at(nullptr, in_len, block_size, element_size);
}

uint32_t redux_record_cost_frame_step(uint64_t in_len, uint32_t block_size, uint32_t record_size, uint32_t sample_blocks)
{
    if (block_size == 0 || block_size > (1u << 30) || redux_record_check(record_size, 0) != REDUX_OK)
        return 0;
    const uint64_t step = record_cost_sample(in_len, block_size, record_size, sample_blocks).step;
    return step > 0xFFFFFFFFull ? 0 : (uint32_t)step;
}

uint64_t redux_record_cost_block_count(uint64_t in_len, uint32_t block_size, uint32_t record_size, uint32_t sample_blocks)
{
    if (block_size == 0 || block_size > (1u << 30) || redux_record_check(record_size, 0) != REDUX_OK)
        return 0;
    return record_cost_sample(in_len, block_size, record_size, sample_blocks).row_blocks;
}

int redux_record_cost_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, const uint32_t *records,
                          const uint8_t *deltas, uint32_t ncand, uint32_t sample_blocks, void *d_bits, void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || !d_bits || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    RecordCostArgs a; // (the lists travel in the kernels' arguments: consumed before the call returns)
    if (!record_cost_list(records, deltas, ncand, REDUX_RECORD_COST_MAX, a.records, a.deltas, redux_record_check))
        return REDUX_INVALID_INPUT;
    a.ncand = ncand;
    const int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    return launch_record_cost(a, d_in, in_len, block_size, sample_blocks, (double *)d_bits, (hipStream_t)stream);
}

const char *redux_record_cost_kernel_name_at(const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t record_size)
{
    static const char *const names[3] = {"k_record_cost", "k_record_cost + k_record_cost_bytes", "k_record_cost_bytes"};
    if (block_size == 0 || block_size > (1u << 30) || redux_record_check(record_size, 0) != REDUX_OK)
        return "";
    const uint64_t nfull = layout_cost_full_frames(d_in, in_len, block_size, record_size);
    return names[nfull == 0 ? 2 : nfull * record_size < redux_block_count(in_len, block_size) ? 1 : 0];
}

const char *redux_record_cost_kernel_name(uint64_t in_len, uint32_t block_size, uint32_t record_size)
{
    return redux_record_cost_kernel_name_at(nullptr, in_len, block_size, record_size);
}

int redux_table_cost_dev(const void *d_counts, const void *d_cum, uint64_t n, void *d_bits, void *stream)
{
    if (n && (!d_counts || !d_cum || !d_bits))
        return REDUX_INVALID_INPUT;
    if (n == 0)
        return REDUX_OK;
    k_table_cost<<<(uint32_t)(n < 65536 ? n : 65536), 64, 0, (hipStream_t)stream>>>((const unsigned long long *)d_counts,
                                                                                   (const uint32_t *)d_cum, n, (double *)d_bits);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

// ---- mixed layouts (redux_mixed.hpp) ----------------------------------------------------------------
uint64_t redux_mixed_unit_count(uint64_t in_len, uint32_t block_size)
{
    return (redux_block_count(in_len, block_size) + kMixedUnit - 1) / kMixedUnit;
}

int redux_mixed_choose_dev(const void *d_bits, uint64_t nblocks, uint32_t layouts_mask, void *d_table, void *d_sum_bits, void *stream)
{
    return mixed_choose_dev(d_bits, nblocks, layouts_mask, d_table, d_sum_bits, stream);
}

int redux_mixed_layout_dev(const void *d_src, void *d_dst, uint64_t len, uint32_t block_size, const void *d_table, int inverse,
                           void *stream)
{
    return mixed_layout_dev(d_src, d_dst, len, block_size, d_table, inverse, stream);
}

// the transformed copy, the cost rows, the coder's workspace
uint64_t redux_encode_mixed_workspace_bytes(const redux_params *p, uint64_t in_len, uint32_t block_size)
{
    const uint64_t ws = redux_encode_workspace_bytes(p, in_len, block_size);
    return ws ? planes_copy_bytes(in_len) + mixed_cost_bytes(redux_block_count(in_len, block_size)) + ws : 0;
}

uint64_t redux_decode_mixed_workspace_bytes(const redux_params *p, uint64_t out_len, uint32_t block_size)
{
    return redux_decode_planes_workspace_bytes(p, out_len, block_size, 1);
}

// ws_cost: the chunks of a multi-chunk host call run the coder on a workspace without the pairs area (adaptive_encoder)
static int encode_mixed_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t layouts_mask,
                            void *d_table, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                            void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || layouts_mask > 0xFF || !d_table || !d_workspace || (in_len && !d_in))
        return REDUX_INVALID_INPUT;
    int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    const uint64_t nblocks = redux_block_count(in_len, block_size);
    const uint64_t copy = planes_copy_bytes(in_len), cost = mixed_cost_bytes(nblocks);
    if (workspace_bytes < copy + cost)
        return REDUX_OUTPUT_TOO_SMALL;
    uint8_t *x = (uint8_t *)d_workspace, *bits = x + copy;
    if (layouts_mask) {
        if ((st = redux_layout_cost_dev(p, d_in, in_len, block_size, layouts_mask, bits, stream)) != REDUX_OK)
            return st;
        if ((st = mixed_choose_dev(bits, nblocks, layouts_mask, d_table, nullptr, stream)) != REDUX_OK)
            return st;
    }
    if ((st = mixed_layout_dev(d_in, x, in_len, block_size, d_table, 0, stream)) != REDUX_OK)
        return st;
    return redux_encode_blocks_dev(p, x, in_len, block_size, d_out, out_cap, d_out_offsets, d_block_status, d_summary, bits + cost,
                                   workspace_bytes - copy - cost, stream);
}

int redux_encode_mixed_dev(const redux_params *p, const void *d_in, uint64_t in_len, uint32_t block_size, uint32_t layouts_mask,
                           void *d_table, void *d_out, uint64_t out_cap, void *d_out_offsets, void *d_block_status, void *d_summary,
                           void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    return encode_mixed_dev(p, d_in, in_len, block_size, layouts_mask, d_table, d_out, out_cap, d_out_offsets, d_block_status,
                            d_summary, d_workspace, workspace_bytes, stream);
}

// the blocks decode into the plane buffer at the front of the workspace, then layout_decode_tail's sizes check and summary with
// the mixed inverse in place of a single layout's (d_t null: the tail runs no inverse of its own)
int redux_decode_mixed_dev(const redux_params *p, const void *d_in, const void *d_in_offsets, const void *d_table, uint64_t out_len,
                           uint32_t block_size, void *d_out, void *d_out_sizes, void *d_block_status, void *d_summary,
                           void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    int st = check_params(p);
    if (st != REDUX_OK)
        return st;
    if (block_size == 0 || block_size > (1u << 30) || !d_table || !d_workspace || !d_in_offsets || !d_out_sizes || !d_block_status ||
        (out_len && !d_out))
        return REDUX_INVALID_INPUT;
    const uint64_t nblocks = redux_block_count(out_len, block_size);
    const uint64_t copy    = planes_copy_bytes(nblocks * (uint64_t)block_size);
    if (workspace_bytes < redux_decode_mixed_workspace_bytes(p, out_len, block_size))
        return REDUX_OUTPUT_TOO_SMALL;
    uint8_t *t = (uint8_t *)d_workspace;
    st = decode_blocks_dev_impl(p, d_in, d_in_offsets, nblocks, block_size, t, nblocks * (uint64_t)block_size, d_out_sizes,
                                d_block_status, d_summary, t + copy, workspace_bytes - copy, stream, nullptr, BlockTable{});
    if (st != REDUX_OK)
        return st;
    st = layout_decode_tail(Layout{1}, nullptr, d_out, out_len, block_size, d_out_sizes, d_block_status, d_summary,
                            TailSummary::InSizes, stream);
    if (st != REDUX_OK)
        return st;
    return mixed_layout_dev(t, d_out, out_len, block_size, d_table, 1, stream);
}

// The host-pointer pair: a chunk is whole 64-block waves, hence whole units, so chunk [b0, b0 + nb) owns table bytes b0 / 8 ..;
// they travel through the slot's d_stf / h_stf (host::UnitTableIo).
static int mixed_table_check(const uint8_t *table, uint64_t nunits)
{
    for (uint64_t u = 0; u < nunits; u++)
        if (table[u] > 7)
            return REDUX_INVALID_INPUT;
    return REDUX_OK;
}

int redux_encode_blocks_mixed(const redux_params *p, const uint8_t *in, uint64_t in_len, uint32_t block_size, uint32_t layouts_mask,
                              uint8_t *table, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, int32_t *block_status,
                              uint32_t *block_crc)
{
    if (!p || block_size == 0 || block_size > (1u << 30) || layouts_mask > 0xFF || !table || !out || !out_offsets || (in_len && !in))
        return REDUX_INVALID_INPUT;
    int st = adaptive_cost_check(p, block_size);
    if (st != REDUX_OK)
        return st;
    if (!layouts_mask && (st = mixed_table_check(table, redux_mixed_unit_count(in_len, block_size))) != REDUX_OK)
        return st;
    const host::EncodeCoder plain = adaptive_encoder(p, block_size);
    const host::EncodeCoder coder = {
        [=](uint64_t max_in, bool several, uint64_t &ws, uint64_t &bound) {
            plain.size(max_in, several, ws, bound);
            ws += planes_copy_bytes(max_in) + mixed_cost_bytes(redux_block_count(max_in, block_size));
        },
        [=](host::Slot &s, uint64_t len, uint64_t bound, void *ws, uint64_t ws_bytes, hipStream_t stream) {
            return encode_mixed_dev(p, s.d_in.p, len, block_size, layouts_mask, s.d_stf.p, s.d_out.p, bound, s.d_off.p, s.d_st.p,
                                    s.d_sum.p, ws, ws_bytes, stream);
        }};
    return host::encode_blocks(in, in_len, block_size, out, out_cap, out_offsets, block_status, coder, block_crc, nullptr, {}, {},
                               host::UnitTableIo{table, layouts_mask == 0});
}

int redux_decode_blocks_mixed(const redux_params *p, const uint8_t *in, const uint64_t *in_offsets, const uint8_t *table,
                              uint64_t out_len, uint32_t block_size, uint8_t *out, uint32_t *out_sizes, int32_t *block_status,
                              uint32_t *block_crc)
{
    int st = check_params(p);
    if (st == REDUX_OK && (block_size == 0 || block_size > (1u << 30) || !table))
        st = REDUX_INVALID_INPUT;
    if (st == REDUX_OK)
        st = mixed_table_check(table, redux_mixed_unit_count(out_len, block_size));
    const host::DecodeCoder coder = {
        [=](uint64_t cb) { return redux_decode_mixed_workspace_bytes(p, cb * (uint64_t)block_size, block_size); },
        [=](host::Slot &s, uint64_t, uint64_t out_bytes, void *, void *ws, uint64_t ws_bytes, hipStream_t stream) {
            return redux_decode_mixed_dev(p, s.d_in.p, s.d_off.p, s.d_stf.p, out_bytes, block_size, s.d_out.p, s.d_sz.p, s.d_st.p,
                                          s.d_sum.p, ws, ws_bytes, stream);
        },
        true};
    return decode_blocks_host(st, in, in_offsets, redux_block_count(out_len, block_size), block_size, out, out_len, out_len, out_sizes,
                              block_status, nullptr, coder, block_crc, nullptr, {}, {}, host::UnitTableIo{(uint8_t *)table, true});
}

const char *redux_mixed_kernel_name_at(const void *d_src, const void *d_dst, uint64_t in_len, uint32_t block_size, int inverse)
{
    static const char *const names[2][3] = {
        {"k_mixed_planes<0>", "k_mixed_planes<0> + k_mixed_bytes<0>", "k_mixed_bytes<0>"},
        {"k_mixed_planes<1>", "k_mixed_planes<1> + k_mixed_bytes<1>", "k_mixed_bytes<1>"},
    };
    if (block_size == 0 || block_size > (1u << 30) || in_len == 0)
        return "";
    const FastSplit f = fast_split(in_len, (uint64_t)kMixedUnit * block_size, block_size, {d_src, d_dst});
    return names[inverse != 0][f.nfull == 0 ? 2 : f.rest < in_len ? 1 : 0];
}

const char *redux_mixed_kernel_name(uint64_t in_len, uint32_t block_size, int inverse)
{
    return redux_mixed_kernel_name_at(nullptr, nullptr, in_len, block_size, inverse);
}

// ---- range reads (redux_range.hpp) ----------------------------------------------------------------------------------------
int redux_range_plan(uint64_t total_len, uint32_t block_size, uint64_t granule_blocks, const uint64_t *starts, const uint64_t *lens,
                     uint64_t nranges, uint64_t *run_first, uint64_t *run_count, uint64_t *nruns, uint64_t *virt_off,
                     uint64_t *virt_len)
{
    return range_plan(total_len, block_size, granule_blocks, starts, lens, nranges, run_first, run_count, nruns, virt_off, virt_len);
}

uint64_t redux_segment_tiles(const redux_segment *segs, uint64_t nsegs, redux_segment *tiles)
{
    return segs ? segment_tiles(segs, nsegs, tiles) : 0;
}

uint64_t redux_segment_copy_workspace_bytes(const redux_segment *segs, uint64_t nsegs)
{
    return align_up(redux_segment_tiles(segs, nsegs, nullptr) * sizeof(redux_segment), 256);
}

int redux_segment_copy_dev(const void *d_src, uint64_t src_bytes, void *d_dst, uint64_t dst_bytes, const redux_segment *segs,
                           uint64_t nsegs, void *d_workspace, uint64_t workspace_bytes, void *stream)
{
    const int st = segment_table_check(d_src, src_bytes, d_dst, dst_bytes, segs, nsegs);
    if (st != REDUX_OK)
        return st;
    const uint64_t ntiles = segment_tiles(segs, nsegs, nullptr);
    if (ntiles == 0)
        return REDUX_OK;
    if (!d_workspace || ((uintptr_t)d_workspace & 7))
        return REDUX_INVALID_INPUT;
    if (workspace_bytes < ntiles * sizeof(redux_segment))
        return REDUX_OUTPUT_TOO_SMALL;
    std::vector<redux_segment> tiles(ntiles);
    segment_tiles(segs, nsegs, tiles.data());
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d_workspace, tiles.data(), ntiles * sizeof(redux_segment), hipMemcpyHostToDevice, s));
    SegmentCopyArgs a;
    a.src    = (const uint8_t *)d_src;
    a.dst    = (uint8_t *)d_dst;
    a.tiles  = (const redux_segment *)d_workspace;
    a.ntiles = ntiles;
    const uint64_t cap = (uint64_t)cu_count() * 8; // eight workgroups of 256 per CU keep every wave slot busy; the rest is the stride
    k_segment_copy<<<(uint32_t)(ntiles < cap ? ntiles : cap), kSegmentThreads, 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    return REDUX_OK;
}

const char *redux_segment_copy_kernel_name(void) { return "k_segment_copy"; }

} // extern "C"
