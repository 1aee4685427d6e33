// redux_context_static.hpp -- context-static coding: the static coder with one table per preceding byte (gfx950 only).
//
// The rule (include/redux_hip.h, "context-static coding"): the context of byte i of a block is byte i - 1 of the same block
// (0 for the first byte), table c is the semi-static table of the bytes whose context is c, and a block's stream is what the
// static coder writes when every symbol is coded under the table of its context.  Totals are at most 2^16, every table has
// the same total, and cum[1..256] of all 256 tables fits a u16[256][256] image of exactly 128 KiB.
//
//   k_context_hist            counts (context, byte) pairs into u64[256][256] (added to).  65,536 bins do not fit k_byte_hist's
//                             per-lane counters; one workgroup of 1024 threads per CU shares packed u16 counters in LDS
//                             (128 KiB, ds_add_u32 on the bin's half of a dword) and folds them into the global u64 counts
//                             before any of them can reach 65,536: at most 3 * 16,384 + 30 bytes between two folds, whatever
//                             the data.  Global atomics per byte were the alternative: text sends most of its pairs to a few
//                             hundred bins, which a single L2 channel would then serialise; in LDS the same collisions cost a
//                             few cycles, and a fold reads 8 x 16 bytes per thread and touches memory for nonzero bins only.
//   k_context_static_tables   static_table_build (redux_hist.hpp) for all 256 contexts in one launch; a context that owns no
//                             bytes is given a count of one for every byte value first, so every table has the same total
//   k_context_image           d_cum (u32[256][258]) -> the checked image: u16[256][256] of cum[1..256] and a flag that goes up
//                             when any table is not strictly increasing from 0 to the launch's total.  Runs in front of every
//                             coder launch on whatever d_cum the caller passed; with the flag up the coders write
//                             INVALID_INPUT for every block and nothing else.
//   k_encode_context_static   W waves per workgroup, one workgroup per CU, the image loaded into LDS once; every wave then
//                             walks wave slots of 64 blocks, one lane per block: static_encode_body (redux_static.hpp) under
//                             a ContextModel, which is the image and a ctx register per lane
//   k_decode_context_static   the inverse: static_decode_body under the same model; get_symbol tests EOF against the row's
//                             last entry and then searches the lane's own row in 8 steps
//
// The lock-step and lookup-table decoder forms of redux_static.hpp are not built here: both share ONE table among the lanes of
// a wave (a Fenwick tree, a 64 KiB lookup), and here every lane is in a row of its own.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_hist.hpp"
#include "redux_static.hpp"

namespace redux {

constexpr uint32_t kCtxTables      = 256;
constexpr uint32_t kCtxImageBytes  = kCtxTables * 256 * 2; // u16[256][256]
constexpr uint32_t kCtxImagePad    = 8;                    // u16 entries in front of the image in LDS: row[-1] of context 0 is readable
constexpr uint32_t kCtxTotalMax    = 65536;
constexpr uint32_t kCtxHistThreads = 1024;
constexpr uint32_t kCtxHistSteps   = 3; // 16-byte vectors a thread counts between two folds: 3 * 1024 * 16 + 30 < 65,536

// ---- pair histogram -----------------------------------------------------------------------------------------------------
struct ContextHistArgs {
    const uint8_t      *in;
    uint64_t            head;       // bytes before the first 16-byte boundary (< 16, or all of a short buffer)
    uint64_t            nvec;       // 16-byte vectors of the aligned body, which starts at in + head
    uint64_t            tail;       // bytes after it (< 16)
    uint32_t            block_size;
    unsigned long long *counts;     // u64[256][256]
};

__device__ __forceinline__ void ctx_hist_pair(uint32_t *lds, uint32_t c, uint32_t s)
{
    const uint32_t bin = c * 256 + s;
    atomicAdd(lds + (bin >> 1), 1u << ((bin & 1) << 4)); // ds_add_u32, no return
}

// byte i of the buffer (i % block_size == r): its context is the byte before it, or 0 at a block's start
__device__ __forceinline__ void ctx_hist_one(uint32_t *lds, const uint8_t *in, uint64_t i, uint32_t r)
{
    ctx_hist_pair(lds, r ? in[i - 1] : 0u, in[i]);
}

// the workgroup's counters -> counts, the counters back to zero (every thread calls this: barriers)
__device__ __forceinline__ void ctx_hist_fold(uint32_t *lds, unsigned long long *counts)
{
    __syncthreads();
    uint4 *v = reinterpret_cast<uint4 *>(lds);
    for (uint32_t i = threadIdx.x; i < kCtxImageBytes / 16; i += kCtxHistThreads) {
        const uint4 x = v[i];
        if ((x.x | x.y | x.z | x.w) == 0)
            continue;
        v[i] = make_uint4(0, 0, 0, 0);
        const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            if (w[k] & 0xFFFFu)
                atomicAdd(counts + 8 * i + 2 * k, (unsigned long long)(w[k] & 0xFFFFu));
            if (w[k] >> 16)
                atomicAdd(counts + 8 * i + 2 * k + 1, (unsigned long long)(w[k] >> 16));
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kCtxHistThreads) k_context_hist(ContextHistArgs a)
{
    __shared__ __align__(16) uint32_t lds[kCtxImageBytes / 4];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < kCtxImageBytes / 16; i += kCtxHistThreads)
        reinterpret_cast<uint4 *>(lds)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const uint32_t B = a.block_size;
    if (blockIdx.x == 0) { // the unaligned head and tail, a byte per thread
        if (t < a.head)
            ctx_hist_one(lds, a.in, t, t % B);
        if (t < a.tail) {
            const uint64_t i = a.head + a.nvec * 16 + t;
            ctx_hist_one(lds, a.in, i, (uint32_t)(i % B));
        }
    }
    // rows of 1024 vectors: workgroup g takes rows g, g + G, ...; the loop is uniform over the workgroup (the fold has
    // barriers), a thread past the end loads nothing
    const uint64_t rows  = (a.nvec + kCtxHistThreads - 1) / kCtxHistThreads;
    uint32_t       since = 0;
    for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint64_t i = row * kCtxHistThreads + t;
        if (i < a.nvec) {
            const uint64_t g   = a.head + i * 16; // the vector's first byte
            const uint4    x   = *reinterpret_cast<const uint4 *>(a.in + g);
            uint32_t       r   = (uint32_t)(g % B);
            uint32_t       ctx = r ? a.in[g - 1] : 0u;
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (uint32_t k = 0; k < 16; k++) {
                const uint32_t s = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                ctx_hist_pair(lds, r ? ctx : 0u, s);
                ctx = s;
                r   = r + 1 == B ? 0 : r + 1;
            }
        }
        if (++since == kCtxHistSteps) {
            ctx_hist_fold(lds, a.counts);
            since = 0;
        }
    }
    ctx_hist_fold(lds, a.counts);
}

// ---- the 256 tables ----------------------------------------------------------------------------------------------------
// workgroup c: the table of context c.  A context without bytes is counted as one of every byte value (rule 3).
__global__ void __launch_bounds__(256) k_context_static_tables(const unsigned long long *counts, uint32_t total, uint32_t *cum)
{
    __shared__ unsigned long long row[256];
    const unsigned long long c = counts[256ull * blockIdx.x + threadIdx.x];
    const bool any = __syncthreads_or(c != 0) != 0;
    row[threadIdx.x] = any ? c : 1ull;
    __syncthreads();
    static_table_build(row, total, cum + (uint64_t)kStaticEntries * blockIdx.x);
}

// workgroup c, thread s: image[c][s] = cum_c[s + 1]; *bad |= 1 unless 0 = cum_c[0] < cum_c[1] < ... < cum_c[257] = total
__global__ void __launch_bounds__(256) k_context_image(const uint32_t *cum, uint32_t total, uint16_t *image, uint32_t *bad)
{
    const uint32_t *c = cum + (uint64_t)kStaticEntries * blockIdx.x;
    const uint32_t  s = threadIdx.x;
    const uint32_t  v = c[s + 1], prev = c[s];
    bool            b = v <= prev;
    if (s == 0)
        b |= prev != 0;
    if (s == 255) {
        const uint32_t last = c[kStaticEntries - 1];
        b |= last <= v || last != total;
    }
    image[256 * blockIdx.x + s] = (uint16_t)v;
    if (b)
        atomicOr(bad, 1u);
}

// the image into LDS behind its pad (every thread of the workgroup calls this: a barrier)
__device__ __forceinline__ const uint16_t *ctx_image_load(uint32_t *lds, const uint16_t *image)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(image);
    uint4       *dst = reinterpret_cast<uint4 *>(lds) + kCtxImagePad * 2 / 16;
    if (threadIdx.x == 0)
        reinterpret_cast<uint4 *>(lds)[0] = make_uint4(0, 0, 0, 0);
    for (uint32_t i = threadIdx.x; i < kCtxImageBytes / 16; i += blockDim.x)
        dst[i] = src[i];
    __syncthreads();
    return reinterpret_cast<const uint16_t *>(lds) + kCtxImagePad;
}

struct ContextEncArgs {
    StaticEncCore   c;     // c.rc: the reciprocal of `total`
    const uint16_t *image; // u16[256][256], device memory (k_context_image)
    const uint32_t *bad;   // nonzero: refuse
    uint32_t        total;
};

// The model of a lane (redux_static.hpp): the table of the byte before, 0 at a block's start, in the image in LDS.  Row c of
// the image is cum_c[1..256], so row[s - 1] = cum[s] with row[-1] = 0 (the pad in front of row 0 makes it readable).
struct ContextModel {
    const uint16_t *img;
    uint32_t        tot; // every table's total
    uint32_t        ctx;
    __device__ __forceinline__ uint32_t total() const { return tot; }
    // [row[s - 1], row[s]): two ds_read_u16
    __device__ __forceinline__ uint2 range(uint32_t s) const
    {
        const uint16_t *e = img + ctx * 256u + s;
        return make_uint2(s ? (uint32_t)e[-1] : 0u, (uint32_t)e[0]);
    }
    __device__ __forceinline__ uint32_t eof_lo() const { return img[ctx * 256u + 255u]; }
    // EOF owns [cum[256], total); else the s in 0..255 with cum[s] <= v < cum[s + 1], in 8 steps over the lane's own row
    __device__ __forceinline__ bool find(uint32_t v, uint32_t &s) const
    {
        const uint16_t *row = img + ctx * 256u;
        if (v >= (uint32_t)row[255])
            return true;
        s = 0;
#pragma unroll
        for (int b = 7; b >= 0; b--) {
            const uint32_t t = s | (1u << b);
            if ((uint32_t)row[t - 1] <= v)
                s = t;
        }
        return false;
    }
    __device__ __forceinline__ void advance(uint32_t s) { ctx = s; }
};

template <bool CB32, int W>
__global__ void __launch_bounds__(64 * W) k_encode_context_static(ContextEncArgs a)
{
    __shared__ __align__(16) uint32_t lds[(kCtxImageBytes + kCtxImagePad * 2) / 4];
    const uint64_t nwaves = (a.c.nblocks + 63) / 64;
    const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (*a.bad) { // a table failed the check: every block is refused, nothing else is written
        for (uint64_t blk = (uint64_t)blockIdx.x * (64 * W) + threadIdx.x; blk < a.c.nblocks; blk += (uint64_t)gridDim.x * (64 * W)) {
            a.c.sizes[blk]  = 0;
            a.c.status[blk] = REDUX_INVALID_INPUT;
        }
        return;
    }
    const uint16_t *img = ctx_image_load(lds, a.image);
    for (uint64_t slot = (uint64_t)blockIdx.x * W + wave; slot < nwaves; slot += (uint64_t)gridDim.x * W) {
        ContextModel m{img, a.total, 0};
        static_encode_body<false, CB32>(a.c, m, slot * 64, threadIdx.x & 63u, 1);
    }
}

// ---- decoder -----------------------------------------------------------------------------------------------------------
struct ContextDecArgs {
    StaticDecCore   c;
    const uint16_t *image;
    const uint32_t *bad;
    uint32_t        total;
};

template <int W>
__global__ void __launch_bounds__(64 * W) k_decode_context_static(ContextDecArgs a)
{
    __shared__ __align__(16) uint32_t lds[(kCtxImageBytes + kCtxImagePad * 2) / 4];
    const uint64_t nwaves = (a.c.nblocks + 63) / 64;
    const uint32_t wave   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (*a.bad) {
        for (uint64_t blk = (uint64_t)blockIdx.x * (64 * W) + threadIdx.x; blk < a.c.nblocks; blk += (uint64_t)gridDim.x * (64 * W)) {
            a.c.out_sizes[blk] = 0;
            a.c.status[blk]    = REDUX_INVALID_INPUT;
        }
        return;
    }
    const uint16_t *img = ctx_image_load(lds, a.image);
    for (uint64_t slot = (uint64_t)blockIdx.x * W + wave; slot < nwaves; slot += (uint64_t)gridDim.x * W) {
        ContextModel m{img, a.total, 0};
        static_decode_body<false>(a.c, m, slot * 64 + (threadIdx.x & 63u));
    }
}

} // namespace redux
