// redux_base_sub.hpp -- the folded difference against a base: the base filter's second operation (redux_base.hpp is the
// first, XOR), fused with the byte-plane layout.  The fused kernels are redux_base.hpp's with another operation.
//
//   k_base_planes<E, BaseSubFold<E>>    forward, full frames inside the base: the stage-in hook subtracts the base's chunk
//                                       from the source's and folds the 16 / E differences in registers; E = 1: a 16-byte
//                                       stream kernel, no LDS
//   k_base_unplanes<E, BaseSubFold<E>>  inverse, full frames inside the base: the base's chunks loaded ahead, the
//                                       stage-out hook unfolding and adding them
//   k_base_sub_planes_bytes<E>    one element per thread under the frame index rule, any alignment and block size: the
//   k_base_sub_unplanes_bytes<E>  short last frame, the frame the end of the base falls into, and everything when a pointer
//                                 or the block size is no 16-byte multiple
//
// Rule (E, B, x, y, y' as in redux_base.hpp; U = min(len, base_len)): an element of a frame -- one of the N = L / E
// little-endian words of its L bytes -- is COVERED when all E of its bytes lie below U.  A covered element becomes
// z = fold(x - y mod 2^(8E)), the fold of redux_zigzag.hpp: z = (d << 1) ^ (0 - (d >> (8E-1))).  Every other byte (an
// element the base ends inside, a frame's L - N*E trailing bytes, everything past the base) is x ^ y', as in redux_base.hpp.
// The byte-plane layout of E is applied behind it (none for E = 1).  The inverse undoes the layout, unfolds and adds y.
// x == y gives all zeros; the rule is local to a frame and to a prefix of the base.
//
// A 16-byte chunk of a full frame inside the base holds 16 / E whole covered elements, the source's and the base's at the
// same offsets, so the hooks need nothing but the two chunks.  Arithmetic is per element: delta_sub / delta_add
// (redux_delta.hpp) and zigzag_fold_dword / zigzag_unfold_dword (redux_zigzag.hpp) for E <= 4, 64-bit values for E = 8.
//
// Traffic: two reads and one write per byte, as k_base_planes.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_base.hpp"
#include "redux_delta.hpp"

namespace redux {

// fold(x - y) / unfold(z) + y on the two elements of a chunk's half (E = 8)
__device__ __forceinline__ void base_sub_fold64(uint32_t &lo, uint32_t &hi, uint32_t ylo, uint32_t yhi)
{
    const uint64_t d = ((uint64_t)hi << 32 | lo) - ((uint64_t)yhi << 32 | ylo);
    const uint64_t z = d << 1 ^ (uint64_t)((int64_t)d >> 63);
    lo = (uint32_t)z; hi = (uint32_t)(z >> 32);
}

__device__ __forceinline__ void base_sub_unfold64(uint32_t &lo, uint32_t &hi, uint32_t ylo, uint32_t yhi)
{
    const uint64_t z = (uint64_t)hi << 32 | lo;
    const uint64_t x = (z >> 1 ^ (0ull - (z & 1))) + ((uint64_t)yhi << 32 | ylo);
    lo = (uint32_t)x; hi = (uint32_t)(x >> 32);
}

// the 16 / E elements of a chunk: z = fold(x - y), and x = unfold(z) + y
template <int E>
__device__ __forceinline__ uint4 base_sub_fold(uint4 x, uint4 y)
{
    if constexpr (E == 8) {
        base_sub_fold64(x.x, x.y, y.x, y.y);
        base_sub_fold64(x.z, x.w, y.z, y.w);
        return x;
    } else {
        return make_uint4(zigzag_fold_dword<E>(delta_sub<E>(x.x, y.x)), zigzag_fold_dword<E>(delta_sub<E>(x.y, y.y)),
                          zigzag_fold_dword<E>(delta_sub<E>(x.z, y.z)), zigzag_fold_dword<E>(delta_sub<E>(x.w, y.w)));
    }
}

template <int E>
__device__ __forceinline__ uint4 base_sub_unfold(uint4 z, uint4 y)
{
    if constexpr (E == 8) {
        base_sub_unfold64(z.x, z.y, y.x, y.y);
        base_sub_unfold64(z.z, z.w, y.z, y.w);
        return z;
    } else {
        return make_uint4(delta_add<E>(zigzag_unfold_dword<E>(z.x), y.x), delta_add<E>(zigzag_unfold_dword<E>(z.y), y.y),
                          delta_add<E>(zigzag_unfold_dword<E>(z.z), y.z), delta_add<E>(zigzag_unfold_dword<E>(z.w), y.w));
    }
}

// the operation of k_base_planes / k_base_unplanes (redux_base.hpp)
template <int E>
struct BaseSubFold {
    __device__ __forceinline__ static uint4 forward(uint4 x, uint4 y) { return base_sub_fold<E>(x, y); }
    __device__ __forceinline__ static uint4 inverse(uint4 z, uint4 y) { return base_sub_unfold<E>(z, y); }
};

// Bytes [first, end) of the whole buffer by their INTERLEAVED position o (the source's forward, the destination's inverse),
// one per thread: the thread of an element's first byte does the element, the threads of a frame's trailing bytes XOR them.
// An element the base does not cover is XORed with y', byte by byte, which is what the 64-bit XOR below does.
template <int E, bool INVERSE>
__device__ __forceinline__ void base_sub_bytes(const BaseArgs &a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.end; o += (uint64_t)gridDim.x * blockDim.x) {
        const FramePos f = frame_pos(o, a.len, E, a.block_size);
        if (f.r >= f.n * E) { // trailing bytes: in place
            a.dst[o] = a.src[o] ^ (o < a.base_len ? a.base[o] : (uint8_t)0);
            continue;
        }
        if (f.r % E)
            continue;
        const uint64_t i = f.r / E, p0 = f.base + i; // the element, and its byte of plane 0
        uint64_t v = 0, y = 0;
#pragma unroll
        for (uint32_t q = 0; q < E; q++) {
            v |= (uint64_t)a.src[INVERSE ? p0 + q * f.n : o + q] << (8 * q);
            y |= (uint64_t)(o + q < a.base_len ? a.base[o + q] : (uint8_t)0) << (8 * q);
        }
        if (o + E > a.base_len) {
            v ^= y;
        } else if (INVERSE) {
            v = (v >> 1 ^ (0 - (v & 1))) + y;
        } else { // (the bits above the element's 8*E are dropped below)
            v -= y;
            v = v << 1 ^ (0 - (v >> (8 * E - 1) & 1));
        }
#pragma unroll
        for (uint32_t q = 0; q < E; q++)
            a.dst[INVERSE ? o + q : p0 + q * f.n] = (uint8_t)(v >> (8 * q));
    }
}

template <int E>
__global__ void __launch_bounds__(256) k_base_sub_planes_bytes(BaseArgs a)
{
    base_sub_bytes<E, false>(a);
}

template <int E>
__global__ void __launch_bounds__(256) k_base_sub_unplanes_bytes(BaseArgs a)
{
    base_sub_bytes<E, true>(a);
}

} // namespace redux
