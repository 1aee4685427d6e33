// redux_base.hpp -- the XOR-against-base filter for series of snapshots (checkpoint N against checkpoint N - 1, a
// fine-tuned model against its base), fused with the byte-plane layout (redux_planes.hpp): a byte transform in front of
// the coder, next to k_planes and k_delta_planes, with a second input.
//
//   k_base_planes<E, OP>      forward, full frames inside the base: the forward tile (redux_planes.hpp) with a second
//                             coalesced 16-byte load, from the base, XORed in by the stage-in hook on the way into LDS;
//                             E = 1: a plain 16-byte XOR stream, no LDS
//   k_base_unplanes<E, OP>    inverse, full frames inside the base: the plain inverse tile, the base's chunks loaded ahead of
//                             it and XORed in by the stage-out hook; no scan and no carry along the frame
//                             (OP = BaseXor: this filter; the folded difference of redux_base_sub.hpp is the other)
//   k_base_planes_bytes<E>    one destination byte per thread under the frame index rule, any alignment and block size: the
//   k_base_unplanes_bytes<E>  short last frame, the frame the end of the base falls into, and everything when a pointer or
//                             the block size is no 16-byte multiple
//
// Rule (E = element size, B = block size, x = the input of len bytes, y = the base of base_len bytes): y'[i] = y[i] for
// i < min(len, base_len) and 0 beyond; d[i] = x[i] ^ y'[i] for every byte; the byte-plane layout of E is applied to d (none
// for E = 1).  The inverse undoes the layout and XORs with y' again.  The filter is bytewise: no elements, no frames, no
// arithmetic, so blocks and frames stay as independent as the layout leaves them.
//
// Traffic: two reads and one write per byte (the fused form), against the five of an XOR pass followed by k_planes.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_planes.hpp"

namespace redux {

struct BaseArgs {
    const uint8_t *src;
    const uint8_t *base;
    uint8_t       *dst;
    uint64_t       groups;       // fused kernels: full frames inside the base * frame_groups, 16-element groups
    uint32_t       frame_groups; // block_size / 16
    uint32_t       block_size;
    uint64_t       first, end;   // byte kernels: destination bytes [first, end) of the whole buffer
    uint64_t       len;          // of the whole buffer: where the short last frame ends
    uint64_t       base_len;     // bytes of the base that are used: min(len, the caller's base_len)
};

__device__ __forceinline__ uint4 base_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }

// What the fused kernels do where a 16-byte chunk of the source meets the base's: OP::forward(x, y) on the way into LDS,
// OP::inverse(z, y) where the wave writes its contiguous bytes.  BaseXor is this filter; BaseSubFold<E> (redux_base_sub.hpp)
// is the folded difference.
struct BaseXor {
    __device__ __forceinline__ static uint4 forward(uint4 x, uint4 y) { return base_xor(x, y); }
    __device__ __forceinline__ static uint4 inverse(uint4 z, uint4 y) { return base_xor(z, y); }
};

// Forward, full frames inside the base.  The wave's 1024*E contiguous bytes of the source and of the base are loaded with
// the same coalesced 16-byte accesses and meet on the way into LDS.
template <int E, typename OP>
__global__ void __launch_bounds__(256) k_base_planes(BaseArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (E == 1) { // no layout: group g is 16 bytes of the stream
        if (g < a.groups)
            ((uint4 *)a.dst)[g] = OP::forward(((const uint4 *)a.src)[g], ((const uint4 *)a.base)[g]);
    } else {
        __shared__ uint4 lds[4 * 64 * E];
        const uint4 *y = (const uint4 *)(a.base + (g - (threadIdx.x & 63)) * 16 * E); // the wave's chunks of the base
        tile_forward<E, PlainForward<E>, 1>(a.src, a.dst, a.groups, (uint64_t)blockIdx.x * blockDim.x, a.frame_groups, a.block_size, lds,
                                            [y](uint4 v, int, uint32_t c) { return OP::forward(v, y[c]); });
    }
}

// Inverse, full frames inside the base: the base combined in where the wave writes its contiguous bytes.
template <int E, typename OP>
__global__ void __launch_bounds__(256) k_base_unplanes(BaseArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (E == 1) {
        if (g < a.groups)
            ((uint4 *)a.dst)[g] = OP::inverse(((const uint4 *)a.src)[g], ((const uint4 *)a.base)[g]);
    } else {
        __shared__ uint4 lds[4 * 64 * E];
        // the base's chunks first: they depend on nothing, and are in flight while the planes are permuted
        const uint32_t lane = threadIdx.x & 63, wave_chunks = tile_wave_chunks<E, uint64_t>(a.groups, g - lane);
        const uint4   *y    = (const uint4 *)(a.base + (g - lane) * 16 * E);
        uint4 yb[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint32_t c = k * 64 + lane;
            yb[k] = c < wave_chunks ? y[c] : make_uint4(0, 0, 0, 0);
        }
        tile_inverse<E>(a.src, a.dst, a.groups, (uint64_t)blockIdx.x * blockDim.x, a.frame_groups, a.block_size, lds,
                        [&yb](uint4 v, int k, uint32_t) { return OP::inverse(v, yb[k]); });
    }
}

// Destination bytes [first, end) of the whole buffer, one per thread; the base byte is the one at the INTERLEAVED position
// (the source's forward, the destination's inverse), zero from base_len on.
template <int E, bool INVERSE>
__device__ __forceinline__ void base_bytes(const BaseArgs &a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.end; o += (uint64_t)gridDim.x * blockDim.x) {
        const FramePos f  = frame_pos(o, a.len, E, a.block_size);
        const uint64_t s  = f.base + frame_src<INVERSE>(f, E);
        const uint64_t yi = INVERSE ? o : s;
        const uint8_t  y  = yi < a.base_len ? a.base[yi] : (uint8_t)0;
        a.dst[o] = a.src[s] ^ y;
    }
}

template <int E>
__global__ void __launch_bounds__(256) k_base_planes_bytes(BaseArgs a)
{
    base_bytes<E, false>(a);
}

template <int E>
__global__ void __launch_bounds__(256) k_base_unplanes_bytes(BaseArgs a)
{
    base_bytes<E, true>(a);
}

} // namespace redux
