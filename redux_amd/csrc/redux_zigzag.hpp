// redux_zigzag.hpp -- the zigzag fold: every difference folded so that small magnitudes of either sign become small unsigned
// numbers.  The arithmetic alone: the delta kernels (redux_delta.hpp) take it as their compile-time FOLD, which makes them
// the zigzag-folded delta filter for signed series, and the folded difference against a base (redux_base_sub.hpp) folds
// with it too.
//
// Rule (E, B and the frames as for the delta filter): d[0] = x[0], d[i] = x[i] - x[i-1] mod 2^(8E);
// z[i] = (d[i] << 1) ^ (0 - (d[i] >> (8E-1))) mod 2^(8E) for every i, 0 included: read as signed, d >= 0 maps to 2d and
// d < 0 to -2d - 1.  The L - N*E trailing bytes of a frame stay as they are; the layout is applied to the z's (none for
// E = 1).  The inverse undoes the layout, unfolds with d = (z >> 1) ^ (0 - (z & 1)) and takes the running sum mod 2^(8E)
// inside each frame.  The fold is a bijection on E-byte words, so any input round-trips.
//
// Why: a small negative difference puts 0xFF into every upper byte and a small positive one 0x00, so a series that moves
// both ways leaves each of the E - 1 upper planes an even mix of the two, about one bit per element per plane to a coder
// that sees one plane per block.  Folded, the upper bytes of both are 0x00.
//
// Arithmetic is per element: for E = 1 and 2 the 4 / E elements of a dword are folded together, the top bit masked off
// before the shift and the sign bit (fold) or low bit (unfold) spread into a whole-element mask, so nothing crosses an
// element boundary; E = 8 is the same on 64-bit values.
//
// Included by redux_delta.hpp.
#pragma once

#include "redux_planes.hpp"

namespace redux {

// the fold / unfold of the 4 / E elements packed in a dword
template <int E>
__device__ __forceinline__ uint32_t zigzag_fold_dword(uint32_t d)
{
    if constexpr (E >= 4) {
        return d << 1 ^ (uint32_t)((int32_t)d >> 31);
    } else {
        constexpr uint32_t H = E == 2 ? 0x80008000u : 0x80808080u; // the elements' top bits
        constexpr uint32_t L = E == 2 ? 0x00010001u : 0x01010101u; // and their low bits
        const uint32_t s = d >> (8 * E - 1) & L;                   // every element's sign bit, in its low bit
        // (s << 8E) - s: 2^(8E) - 1 times each sign bit, an all-ones element per negative one (the top element's 2^32
        // drops out of the dword)
        return (d & ~H) << 1 ^ ((s << 8 * E) - s);
    }
}

template <int E>
__device__ __forceinline__ uint32_t zigzag_unfold_dword(uint32_t z)
{
    if constexpr (E >= 4) {
        return z >> 1 ^ (0u - (z & 1));
    } else {
        constexpr uint32_t H = E == 2 ? 0x80008000u : 0x80808080u;
        constexpr uint32_t L = E == 2 ? 0x00010001u : 0x01010101u;
        const uint32_t s = z & L; // every element's low bit
        return (z >> 1 & ~H) ^ ((s << 8 * E) - s);
    }
}

// v's 16 elements folded / unfolded in place.  The unfold of 0 is 0: a lane of zeros stays a lane of zeros.
template <int E>
__device__ __forceinline__ void zigzag_fold(uint32_t (&v)[4 * E])
{
    if constexpr (E == 8) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t d = (uint64_t)v[2 * j + 1] << 32 | v[2 * j];
            const uint64_t z = d << 1 ^ (uint64_t)((int64_t)d >> 63);
            v[2 * j] = (uint32_t)z; v[2 * j + 1] = (uint32_t)(z >> 32);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * E; j++)
            v[j] = zigzag_fold_dword<E>(v[j]);
    }
}

template <int E>
__device__ __forceinline__ void zigzag_unfold(uint32_t (&v)[4 * E])
{
    if constexpr (E == 8) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t z = (uint64_t)v[2 * j + 1] << 32 | v[2 * j];
            const uint64_t d = z >> 1 ^ (0ull - (z & 1));
            v[2 * j] = (uint32_t)d; v[2 * j + 1] = (uint32_t)(d >> 32);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * E; j++)
            v[j] = zigzag_unfold_dword<E>(v[j]);
    }
}

} // namespace redux
