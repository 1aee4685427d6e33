// redux_const.hpp -- constant blocks: a block whose bytes are all equal travels as that one byte and never meets the coder
// (gfx950 only).
//
// The rule (include/redux_hip.h, "constant blocks"): block b, L_b bytes of coder input x' (the input, its byte-plane layout,
// or the layout of input ^ base):  const_b <=> L_b >= 1 && x'[b * B + i] == x'[b * B] for every i < L_b.
//
//   k_const_select   encode: x' -> flags, one wave per block, 16-byte loads against the first byte broadcast, the wave leaves
//                    the block at the first difference it sees (so a block that is not constant costs its first 4 KiB)
//   k_const_table    both directions: the blocks flagged 0 as a redux_block table in block order, packed from entry 0, IDLE
//                    entries after them (k_store_table's body: redux_store.hpp), for the table forms of the coder kernels
//   k_const_sizes    encode: after the coder, before the size scan: a constant block's size is 1, its status OK
//   k_const_place    encode: after the scan: a constant block's byte -> out + offsets[b]
//   k_const_fill     decode: a constant block's byte -> its L_b bytes of the plane buffer (16-byte stores, byte head and tail)
//
// Included by redux_hip.hip (one translation unit), after redux_store.hpp.
#pragma once

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace redux {

// ======================================================================================
// detection
// ======================================================================================
struct ConstSelectArgs {
    const uint8_t *in;    // x'
    uint8_t       *flags; // u8[nblocks]: 0 coded, 1 constant
    uint64_t       nblocks, in_len;
    uint32_t       block_size;
};

constexpr uint32_t kConstWaves = 4; // waves (= blocks in flight) per workgroup

// One wave per block.  Bytes up to the block's first 16-byte boundary and behind its last one go bytewise, a lane each (at
// most 15 of either); between them every load is an aligned 16-byte chunk that lies wholly inside the block, four per lane
// in flight, so nothing is read that holds no byte of the block.  The differences are ORed per lane; the ballot after each
// round of 256 chunks is the wave-level OR, and the wave stops reading at the first round that saw one.
__global__ void __launch_bounds__(64 * kConstWaves) k_const_select(ConstSelectArgs a)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t w0   = (uint64_t)blockIdx.x * kConstWaves + (threadIdx.x >> 6);
    for (uint64_t b = w0; b < a.nblocks; b += (uint64_t)gridDim.x * kConstWaves) {
        const uint32_t L = (uint32_t)store_block_len(b, a.in_len, a.block_size);
        if (L == 0) { // (the empty input's one block)
            if (lane == 0)
                a.flags[b] = 0;
            continue;
        }
        const uint8_t *p  = a.in + b * a.block_size;
        const uint32_t v  = p[0];
        const uint32_t v4 = v * 0x01010101u;
        uint32_t       diff = 0;
        uint32_t       head = (uint32_t)((16 - ((uintptr_t)p & 15)) & 15);
        if (head > L)
            head = L;
        if (lane < head)
            diff |= p[lane] ^ v;
        const uint32_t nchunks = (L - head) >> 4;
        const uint4   *c16     = reinterpret_cast<const uint4 *>(p + head);
        for (uint32_t base = 0; base < nchunks; base += 256) {
            uint4 q[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t i = base + 64 * k + lane;
                q[k] = i < nchunks ? c16[i] : make_uint4(v4, v4, v4, v4);
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                diff |= (q[k].x ^ v4) | (q[k].y ^ v4) | (q[k].z ^ v4) | (q[k].w ^ v4);
            if (__builtin_amdgcn_ballot_w64(diff != 0)) // (wave-uniform)
                break;
        }
        const uint32_t done = head + (nchunks << 4);
        if (lane < L - done)
            diff |= p[done + lane] ^ v;
        const bool any = __builtin_amdgcn_ballot_w64(diff != 0) != 0;
        if (lane == 0)
            a.flags[b] = any ? 0 : 1;
    }
}

// the table: k_store_table's scan over another flag array (a flag other than 0 is no coder block in either)
__global__ void __launch_bounds__(1024) k_const_table(StoreTableArgs a)
{
    __shared__ uint64_t part[1024];
    flags_to_table(a, part);
}

// ======================================================================================
// encode
// ======================================================================================
struct ConstPlaceArgs {
    const uint8_t  *flags;
    const uint8_t  *raw;     // x'
    uint32_t       *sizes;   // the coder's stream sizes (workspace)
    int32_t        *status;
    const uint64_t *offsets; // nblocks + 1, after the scan
    uint8_t        *out;
    uint64_t        out_cap;
    int32_t        *summary; // may be null
    uint64_t        nblocks;
    uint32_t        block_size;
};

// (the table check has left size 0 / INVALID_INPUT for every block no entry codes: redux_table.hpp)
__global__ void __launch_bounds__(256) k_const_sizes(ConstPlaceArgs a)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.nblocks; b += (uint64_t)gridDim.x * blockDim.x)
        if (a.flags[b] == 1) {
            a.sizes[b]  = 1;
            a.status[b] = REDUX_OK;
        }
}

__global__ void __launch_bounds__(256) k_const_place(ConstPlaceArgs a)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.nblocks; b += (uint64_t)gridDim.x * blockDim.x) {
        if (a.flags[b] != 1)
            continue;
        if (a.offsets[b + 1] > a.out_cap) { // the dense buffer is too small for this block: report, never write (k_compact)
            a.status[b] = REDUX_OUTPUT_TOO_SMALL;
            if (a.summary) {
                atomicCAS(&a.summary[0], REDUX_OK, REDUX_OUTPUT_TOO_SMALL);
                atomicAdd(&a.summary[1], 1);
            }
            continue;
        }
        a.out[a.offsets[b]] = a.raw[b * a.block_size];
    }
}

// ======================================================================================
// decode
// ======================================================================================
struct ConstFillArgs {
    const uint8_t  *in;
    const uint64_t *in_offsets; // nblocks + 1
    const uint8_t  *flags;
    uint8_t        *out;        // block b at out + b * block_size, room L_b
    uint32_t       *out_sizes;
    int32_t        *status;
    uint64_t        nblocks, out_len;
    uint32_t        block_size;
};

// one workgroup per block; coded blocks (flag 0) are the decoder's.  A flag other than 0 / 1, a payload of another size
// than 1 and a constant block without bytes: size 0, INVALID_INPUT, nothing written.
__global__ void __launch_bounds__(256) k_const_fill(ConstFillArgs a)
{
    const uint64_t b = blockIdx.x;
    if (b >= a.nblocks)
        return;
    const uint8_t f = a.flags[b];
    if (f == 0)
        return;
    const uint32_t tid  = threadIdx.x;
    const uint64_t o0   = a.in_offsets[b], s = a.in_offsets[b + 1] - o0;
    const uint32_t room = (uint32_t)store_block_len(b, a.out_len, a.block_size);
    if (f != 1 || s != 1 || room == 0) {
        if (tid == 0) {
            a.out_sizes[b] = 0;
            a.status[b]    = REDUX_INVALID_INPUT;
        }
        return;
    }
    const uint8_t  v   = a.in[o0];
    const uint32_t v4  = v * 0x01010101u;
    uint8_t       *dst = a.out + b * a.block_size;
    uint32_t       head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > room)
        head = room;
    if (tid < head)
        dst[tid] = v;
    const uint32_t nchunks = (room - head) >> 4;
    uint4         *d16     = reinterpret_cast<uint4 *>(dst + head);
    for (uint32_t i = tid; i < nchunks; i += 256)
        d16[i] = make_uint4(v4, v4, v4, v4);
    const uint32_t done = head + (nchunks << 4);
    if (tid < room - done)
        dst[done + tid] = v;
    if (tid == 0) {
        a.out_sizes[b] = room;
        a.status[b]    = REDUX_OK;
    }
}

} // namespace redux
