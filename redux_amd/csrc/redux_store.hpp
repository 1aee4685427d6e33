// redux_store.hpp -- stored blocks: a block whose stream does not shrink it travels as its raw coder input (gfx950 only).
//
// The rule (include/redux_hip.h, "stored blocks"): block b, L_b bytes of coder input x' (the input, or its byte-plane
// layout), stream of s_b bytes, threshold t in [0, 65536]:  stored_b <=> status_b == OK && s_b * 65536 >= t * L_b.
//
//   k_store_select   encode: after the coder, before k_scan_sizes: the flag, and a stored block's size becomes L_b (so the
//                    scan yields the final offsets); k_compact then copies x' for stored blocks (CompactArgs::raw)
//   k_store_table    decode: the coded blocks as a redux_block table in block order, packed from entry 0, IDLE entries after
//                    them, for the table form of the adaptive decoders (one workgroup, a scan like k_scan_sizes)
//   k_store_unpack   decode: each stored payload -> its block's place (16-byte stores, byte realignment)
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace redux {

constexpr uint32_t kStoreRatioOne = 65536; // t = 65536: store exactly the blocks that do not shrink

// bytes of block b of a len-byte input cut into blocks of block_size (0 past the end: the empty input's one block)
__device__ __forceinline__ uint64_t store_block_len(uint64_t b, uint64_t len, uint32_t block_size)
{
    const uint64_t o = b * block_size;
    return len > o ? (len - o < block_size ? len - o : block_size) : 0;
}

// n bytes src -> dst by nth threads: bytes up to dst's first 16-byte boundary, then 16-byte stores, each assembled from
// the one or two ALIGNED 16-byte source chunks that hold its bytes (so no load touches a chunk without a wanted byte:
// the source may end anywhere), then the tail bytes.
__device__ __forceinline__ void store_copy(const uint8_t *src, uint8_t *dst, uint32_t n, uint32_t tid, uint32_t nth)
{
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > n)
        head = n;
    if (tid < head)
        dst[tid] = src[tid];
    const uint32_t  nchunks = (n - head) >> 4;
    const uint8_t  *s0      = src + head;
    const uint32_t  sh      = (uint32_t)((uintptr_t)s0 & 15);
    const uint32_t  dq = sh >> 2, r = sh & 3;
    const uint4    *s16 = reinterpret_cast<const uint4 *>(s0 - sh);
    uint4          *d16 = reinterpret_cast<uint4 *>(dst + head);
    auto shift = [&](const uint4 &A, const uint4 &B) {
        const uint32_t d[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
        uint32_t       v[5];
#pragma unroll
        for (int k = 0; k < 5; k++)
            v[k] = dq == 0 ? d[k] : dq == 1 ? d[k + 1] : dq == 2 ? d[k + 2] : d[k + 3];
        uint4 o;
        o.x = __builtin_amdgcn_alignbyte(v[1], v[0], r);
        o.y = __builtin_amdgcn_alignbyte(v[2], v[1], r);
        o.z = __builtin_amdgcn_alignbyte(v[3], v[2], r);
        o.w = __builtin_amdgcn_alignbyte(v[4], v[3], r);
        return o;
    };
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint32_t    i    = tid;
    // four chunks per thread in flight: all loads first
    for (; i + 3 * nth < nchunks; i += 4 * nth) {
        uint4 A[4], B[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            A[k] = s16[i + k * nth];
            B[k] = sh ? s16[i + k * nth + 1] : zero;
        }
#pragma unroll
        for (int k = 0; k < 4; k++)
            d16[i + k * nth] = shift(A[k], B[k]);
    }
    for (; i < nchunks; i += nth)
        d16[i] = shift(s16[i], sh ? s16[i + 1] : zero);
    const uint32_t done = head + (nchunks << 4);
    if (tid < n - done)
        dst[done + tid] = src[done + tid];
}

// ======================================================================================
// encode
// ======================================================================================
struct StoreSelectArgs {
    const int32_t *status;
    uint32_t      *sizes;  // the coder's stream sizes (workspace); a stored block's becomes L_b
    uint8_t       *stored; // u8[nblocks]: 0 coded, 1 stored
    uint64_t       nblocks, in_len;
    uint32_t       block_size, ratio;
};

__global__ void __launch_bounds__(256) k_store_select(StoreSelectArgs a)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.nblocks; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t L = store_block_len(b, a.in_len, a.block_size);
        const uint32_t s = a.sizes[b];
        const bool     st = a.status[b] == REDUX_OK && (uint64_t)s * kStoreRatioOne >= (uint64_t)a.ratio * L;
        a.stored[b] = st ? 1 : 0;
        if (st)
            a.sizes[b] = (uint32_t)L;
    }
}

// ======================================================================================
// decode
// ======================================================================================
struct StoreTableArgs {
    const uint8_t *stored;
    redux_block   *table; // nblocks entries
    uint64_t       nblocks, out_len;
    uint32_t       block_size;
};

// Entry j < C (C = blocks flagged 0): the j-th coded block in block order, at b * block_size with room L_b; entries C ..
// nblocks - 1 are IDLE, so every wave that holds one holds only IDLE entries after its coded ones.  A flag other than 0 / 1
// is no coded block (k_store_unpack reports it).
// (the body, shared with k_const_table of redux_const.hpp: the flag array is either feature's, the predicate -- flag 0 is a
// block the coder owns -- the same)
__device__ __forceinline__ void flags_to_table(const StoreTableArgs &a, uint64_t *part)
{
    const uint32_t tid = threadIdx.x;
    const uint64_t per = (a.nblocks + 1023) / 1024;
    const uint64_t b0  = per * tid < a.nblocks ? per * tid : a.nblocks;
    const uint64_t b1  = b0 + per < a.nblocks ? b0 + per : a.nblocks;
    uint64_t       cnt = 0;
    for (uint64_t b = b0; b < b1; b++)
        cnt += a.stored[b] == 0 ? 1 : 0;
    part[tid] = cnt;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) { // Hillis-Steele inclusive scan over the 1024 partials
        const uint64_t v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    uint64_t j = tid ? part[tid - 1] : 0;
    for (uint64_t b = b0; b < b1; b++)
        if (a.stored[b] == 0) {
            redux_block e;
            e.offset   = b * a.block_size;
            e.length   = (uint32_t)store_block_len(b, a.out_len, a.block_size);
            e.index    = (uint32_t)b;
            a.table[j++] = e;
        }
    const redux_block idle = {0, 0, REDUX_BLOCK_IDLE};
    for (uint64_t k = part[1023] + tid; k < a.nblocks; k += 1024)
        a.table[k] = idle;
}

__global__ void __launch_bounds__(1024) k_store_table(StoreTableArgs a)
{
    __shared__ uint64_t part[1024];
    flags_to_table(a, part);
}

struct StoreUnpackArgs {
    const uint8_t  *in;
    const uint64_t *in_offsets; // nblocks + 1
    const uint8_t  *stored;
    uint8_t        *out;        // block b at out + b * block_size, room L_b
    uint32_t       *out_sizes;
    int32_t        *status;
    uint64_t        nblocks, out_len;
    uint32_t        block_size;
};

// one workgroup per block; coded blocks are the decoder's
__global__ void __launch_bounds__(256) k_store_unpack(StoreUnpackArgs a)
{
    const uint64_t b = blockIdx.x;
    if (b >= a.nblocks)
        return;
    const uint8_t f = a.stored[b];
    if (f == 0)
        return;
    const uint32_t tid = threadIdx.x;
    const uint64_t o0 = a.in_offsets[b], s = a.in_offsets[b + 1] - o0;
    const uint64_t room = store_block_len(b, a.out_len, a.block_size);
    if (f != 1 || s > room) { // not a flag / a payload longer than its block: report, never write
        if (tid == 0) {
            a.out_sizes[b] = 0;
            a.status[b]    = f != 1 ? REDUX_INVALID_INPUT : REDUX_OUTPUT_TOO_SMALL;
        }
        return;
    }
    store_copy(a.in + o0, a.out + b * a.block_size, (uint32_t)s, tid, 256);
    if (tid == 0) {
        a.out_sizes[b] = (uint32_t)s;
        a.status[b]    = REDUX_OK;
    }
}

} // namespace redux
