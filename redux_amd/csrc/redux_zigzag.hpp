// redux_zigzag.hpp -- the zigzag-folded delta filter for signed series, fused with the byte-plane layout: the delta filter
// (redux_delta.hpp) with every difference folded so that small magnitudes of either sign become small unsigned numbers.
//
//   k_zigzag_planes<E>          forward, full frames: the forward tile (redux_planes.hpp) with ZigzagForward in front of the
//                               permutation: DeltaForward's predecessor rule and subtraction, then the fold of the lane's 16
//                               elements in registers; one read and one write
//   k_zigzag_unplanes<E>        inverse, full frames: the frame walk of k_delta_unplanes with the unfold between the
//                               permutation and the serial prefix
//   k_zigzag_planes_bytes<E>    the byte path, one element per thread: bytes_forward (redux_planes.hpp) and
//   k_zigzag_unplanes_bytes<E>  bytes_inverse_frame (redux_delta.hpp) with the fold on
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
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_delta.hpp"

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

// The forward tile's filter: DeltaForward's predecessor rule and differences, then the fold.
template <int E>
struct ZigzagForward {
    typedef typename DeltaForward<E>::Pred Pred;
    __device__ __forceinline__ static Pred before(const uint8_t *src, uint64_t g, bool inside, uint32_t lane)
    {
        return DeltaForward<E>::before(src, g, inside, lane);
    }
    __device__ __forceinline__ static void apply(const uint4 *row, uint32_t lane, bool inside, Pred prev, uint32_t (&v)[4 * E])
    {
        DeltaForward<E>::apply(row, lane, inside, prev, v);
        zigzag_fold<E>(v);
    }
};

// Forward, full frames: the forward tile with the subtraction and the fold in front of the permutation.
template <int E>
__global__ void __launch_bounds__(256) k_zigzag_planes(PlanesArgs a)
{
    __shared__ uint4 lds[4 * 64 * E];
    tile_forward<E, ZigzagForward<E>, 1>(a.src, a.dst, a.groups, (uint64_t)blockIdx.x * blockDim.x, a.frame_groups, a.block_size, lds,
                                         TileNoHook());
}

// Inverse, full frames: k_delta_unplanes' frame walk (one workgroup per frame, one row of 256 groups per iteration, the
// next row's plane loads in flight across the scan) with the unfold between the permutation and the prefix.  A lane past
// the frame's end holds zeros, their unfold is zeros, so its total is still 0, which the scan relies on.
template <int E>
__global__ void __launch_bounds__(256) k_zigzag_unplanes(PlanesArgs a)
{
    typedef typename DeltaSum<E>::T T;
    __shared__ uint4 lds[4 * 64 * E];
    __shared__ T     wtot[2][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 *wl = lds + wave * 64 * E;
    const uint64_t nframes = a.groups / a.frame_groups;
    uint32_t row = 0;
    for (uint64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        const uint64_t fbase = f * (uint64_t)E * a.block_size;
        T        carry = 0; // the sum of the frame's elements before this iteration
        uint32_t nxt[4 * E];
#pragma unroll
        for (int q = 0; q < 4 * E; q++)
            nxt[q] = 0;
        if (threadIdx.x < a.frame_groups)
            plane_load<E>(a.src + fbase, a.block_size, threadIdx.x, nxt);
        for (uint32_t i0 = 0; i0 < a.frame_groups; i0 += 256, row ^= 1) {
            const uint32_t i    = i0 + threadIdx.x;
            const bool     live = i < a.frame_groups;
            uint32_t in[4 * E], v[4 * E];
#pragma unroll
            for (int q = 0; q < 4 * E; q++)
                in[q] = nxt[q];
            if ((uint64_t)i + 256 < a.frame_groups) {
                plane_load<E>(a.src + fbase, a.block_size, (uint64_t)i + 256, nxt);
            } else {
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    nxt[q] = 0;
            }
            planes_permute<E, true>(in, v); // (lanes past the frame: zeros, unfolded to zeros, a total of 0)
            zigzag_unfold<E>(v);
            const T total = delta_prefix<E>(v);
            const T incl  = delta_wave_scan<T>(total, lane);
            if (lane == 63)
                wtot[row][wave] = incl;
            __syncthreads();
            T before = carry + incl - total;
#pragma unroll
            for (uint32_t w = 0; w < 4; w++) {
                const T t = wtot[row][w];
                before += w < wave ? t : 0;
                carry += t;
            }
            delta_offset<E>(v, before);
            if (live)
                tile_put<E>(wl, lane, v);
            __syncthreads();
            const uint32_t w0 = i0 + wave * 64; // the wave's first group of the frame
            if (w0 < a.frame_groups) {
                const uint32_t left = a.frame_groups - w0;
                tile_stage_out<E>(wl, (uint4 *)(a.dst + fbase + (uint64_t)w0 * 16 * E), (left < 64 ? left : 64) * E, lane, TileNoHook());
            }
        }
    }
}

// Forward, any alignment and block size: source bytes [first, len) of the whole buffer, one per thread.
template <int E>
__global__ void __launch_bounds__(256) k_zigzag_planes_bytes(PlanesArgs a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x)
        bytes_forward(a.src, a.dst, o, a.len, E, a.block_size, true, true);
}

// Inverse, any alignment and block size: workgroup w takes frames w, w + gridDim.x, ... of [first, len).
template <int E>
__global__ void __launch_bounds__(256) k_zigzag_unplanes_bytes(PlanesArgs a)
{
    __shared__ uint64_t wtot[2][4];
    const uint64_t frame = (uint64_t)E * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    uint32_t row = 0;
    for (uint64_t fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
        const uint64_t base = a.first + fi * frame;
        bytes_inverse_frame(a.src, a.dst, base, a.len - base < frame ? a.len - base : frame, E, true, wtot, row, true);
    }
}

} // namespace redux
