// redux_mixed.hpp -- per-unit layouts for inputs of mixed element types: the layout in front of the adaptive coder chosen
// for every unit of 8 blocks on its own, from the costs k_layout_cost leaves (redux_layout_cost.hpp), gfx950 only.
//
//   k_mixed_choose             bits f64[8][nblocks] and a mask of layouts -> table u8[nunits]: the lowest selected layout with
//                              the smallest sum of the unit's bits (f64, ascending block order from 0.0); the chosen sums are
//                              added to one u64 in 2^-16 bit with a vector atomic.  One thread per unit.
//   k_mixed_planes<INVERSE>    full units, block size and buffers 16-byte multiples: W workgroups per unit read the unit's
//                              layout k = table[u] & 7 once and branch on it, workgroup-uniformly, into the frame-tile pieces
//                              (redux_planes.hpp, redux_delta.hpp) with the unit in place of the buffer.  A unit holds 8 / E
//                              frames of B / 16 groups each; W = ceil(B / 16 / 256) workgroups are what E = 8 needs at one
//                              group per lane, and the smaller element sizes take 8 / E rows of 256 groups per round (forward,
//                              delta inverse: 128 bytes per lane and barrier pair whatever E) or 8 / E rounds (plain inverse),
//                              so no workgroup of a plain or forward unit is idle whatever the table holds.  The delta inverse
//                              has 8 / E frames per unit: workgroups past them leave before the first barrier.
//   k_mixed_bytes<INVERSE>     everything else -- the short last unit, unaligned buffers, blocks not a multiple of 16 -- the
//                              byte path with the element size and the filter read from the table; the inverse one workgroup
//                              per unit, frame by frame.  Right, not fast.
//
// Rule: unit u is blocks 8u .. 8u + 7 (the last may have fewer), 8 B bytes.  8 is a multiple of every element size, so a
// unit boundary is a frame boundary of every layout, and frames start afresh: the bytes of unit u of the result are the bytes
// of unit u of what redux_planes_dev / redux_delta_planes_dev write for the whole buffer under layout table[u].  A table byte
// is taken & 7, and every offset is formed from the unit's own range, so no table content reads or writes outside [0, len).
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_delta.hpp"

namespace redux {

constexpr uint32_t kMixedUnit = REDUX_MIXED_UNIT_BLOCKS;

struct MixedChooseArgs {
    const double       *bits;    // f64[8][nblocks]
    uint64_t            nblocks, nunits;
    uint32_t            mask;    // bit k = layout k may be chosen (not 0)
    uint8_t            *table;   // u8[nunits]
    unsigned long long *sum;     // may be null: += the chosen sums in 2^-16 bit
};

__global__ void __launch_bounds__(256) k_mixed_choose(MixedChooseArgs a)
{
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < a.nunits; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b0 = u * kMixedUnit, b1 = b0 + kMixedUnit < a.nblocks ? b0 + kMixedUnit : a.nblocks;
        double   best = 0;
        uint32_t pick = 8;
        for (uint32_t k = 0; k < 8; k++) {
            if (!(a.mask >> k & 1))
                continue;
            double s = 0.0;
            for (uint64_t b = b0; b < b1; b++)
                s += a.bits[(uint64_t)k * a.nblocks + b];
            if (pick == 8 || s < best) {
                best = s;
                pick = k;
            }
        }
        a.table[u] = (uint8_t)pick;
        if (a.sum)
            atomicAdd(a.sum, (unsigned long long)(best * 65536.0 + 0.5));
    }
}

struct MixedArgs {
    const uint8_t *src;
    uint8_t       *dst;
    const uint8_t *table;        // u8[ceil(len / (8 * block_size))]
    uint64_t       nfull;        // k_mixed_planes: the full units it takes
    uint32_t       wgs;          // k_mixed_planes: workgroups per unit
    uint32_t       frame_groups; // block_size / 16
    uint32_t       block_size;
    uint64_t       first, len;   // k_mixed_bytes: bytes [first, len), first a unit boundary
};

// ---- the fast path: one unit (src, dst: its first byte), workgroup wg of nwg ------------------------------------------
// plain copy (layout 0, either direction)
__device__ __forceinline__ void mixed_copy(const uint8_t *src, uint8_t *dst, uint32_t groups, uint32_t wg, uint32_t nwg)
{
    for (uint32_t g = wg * 256 + threadIdx.x; g < groups; g += nwg * 256)
        ((uint4 *)dst)[g] = ((const uint4 *)src)[g];
}

// forward, E > 1 or DELTA: 8 / E rows of 256 groups per round and barrier pair -- 128 bytes per lane whatever the element
// size, so that a unit is one round of each of its workgroups (with one row per round, E = 1 behind the filter ran 8 rounds
// and measured 25 % behind k_delta_planes<1>)
template <int E, typename F>
__device__ __forceinline__ void mixed_forward(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                              uint32_t wg, uint32_t nwg, uint4 *lds)
{
    constexpr int  R      = 8 / E;
    const uint32_t groups = frame_groups * R; // of the unit: 8 / E frames
    for (uint32_t t0 = wg * 256 * R; t0 < groups; t0 += nwg * 256 * R) { // (uniform over the workgroup)
        tile_forward<E, F, R>(src, dst, groups, t0, frame_groups, block_size, lds, TileNoHook());
        __syncthreads(); // (the next round stages into the same rows)
    }
}

// inverse of the plain layouts, E > 1: a row of 256 groups per round
template <int E>
__device__ __forceinline__ void mixed_unplanes(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                               uint32_t wg, uint32_t nwg, uint4 *lds)
{
    const uint32_t groups = frame_groups * (8 / E);
    for (uint32_t t0 = wg * 256; t0 < groups; t0 += nwg * 256) {
        tile_inverse<E>(src, dst, groups, t0, frame_groups, block_size, lds, TileNoHook());
        __syncthreads();
    }
}

// inverse of the delta layouts: workgroup wg walks frames wg, wg + nwg, ... of the unit's 8 / E.  An iteration takes 8 / E
// rows of 256 groups under one pair of barriers -- 128 bytes per lane whatever the element size: the walk along a frame is a
// chain of barriers, and with one row per iteration the small element sizes moved too few bytes per link (E = 1: 4.0 ms for
// 4 GiB against k_delta_unplanes<1>'s 1.6, which has 8 workgroups on a CU where this kernel has 3).
template <int E>
__device__ __forceinline__ void mixed_delta_unplanes(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                                     uint32_t wg, uint32_t nwg, uint4 *lds, uint64_t (*wtot)[8][4])
{
    delta_inverse_walk<E, 8 / E, uint32_t>(src, dst, frame_groups, block_size, wg, nwg, 8 / E, lds,
                                           (typename DeltaSum<E>::T (*)[8 / E][4])wtot);
}

// (three waves per SIMD, k_delta_unplanes<8>'s occupancy: the hint keeps the inverse inside the 168 VGPRs that fit; it is at 163)
template <bool INVERSE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 8))) k_mixed_planes(MixedArgs a)
{
    __shared__ uint4    lds[4 * 64 * 8];
    __shared__ uint64_t wtot[2][8][4];
    const uint64_t u  = blockIdx.x / a.wgs; // (the launch has nfull * wgs workgroups)
    // the unit's workgroups are rotated from unit to unit: the few that walk the frames of a delta inverse (8 / E of the W) would
    // otherwise be the same residues of blockIdx.x in every unit, and workgroups go to the chip's eight dies by blockIdx.x mod 8
    // -- with W = 16 and E = 8 all of the work landed on one die (measured: 9.2 ms for 4 GiB against k_delta_unplanes<8>'s 1.7).
    // The rotation is not u alone, so that a table of period 8 does not meet the dies' period either.
    const uint32_t wg = (uint32_t)((blockIdx.x - u * a.wgs + u + (u >> 3) + (u >> 6)) % a.wgs);
    const uint32_t k  = a.table[u] & 7;     // one address for the workgroup: a scalar load, the branches below are uniform
    const uint64_t ub = u * (uint64_t)kMixedUnit * a.block_size;
    const uint8_t *src = a.src + ub;
    uint8_t       *dst = a.dst + ub;
    const uint32_t fg = a.frame_groups, B = a.block_size, W = a.wgs;
    if (!INVERSE) {
        switch (k) {
        case 0: mixed_copy(src, dst, fg * 8, wg, W); break;
        case 1: mixed_forward<2, PlainForward<2>>(src, dst, fg, B, wg, W, lds); break;
        case 2: mixed_forward<4, PlainForward<4>>(src, dst, fg, B, wg, W, lds); break;
        case 3: mixed_forward<8, PlainForward<8>>(src, dst, fg, B, wg, W, lds); break;
        case 4: mixed_forward<1, DeltaForward<1, false>>(src, dst, fg, B, wg, W, lds); break;
        case 5: mixed_forward<2, DeltaForward<2, false>>(src, dst, fg, B, wg, W, lds); break;
        case 6: mixed_forward<4, DeltaForward<4, false>>(src, dst, fg, B, wg, W, lds); break;
        default: mixed_forward<8, DeltaForward<8, false>>(src, dst, fg, B, wg, W, lds); break;
        }
    } else {
        switch (k) {
        case 0: mixed_copy(src, dst, fg * 8, wg, W); break;
        case 1: mixed_unplanes<2>(src, dst, fg, B, wg, W, lds); break;
        case 2: mixed_unplanes<4>(src, dst, fg, B, wg, W, lds); break;
        case 3: mixed_unplanes<8>(src, dst, fg, B, wg, W, lds); break;
        case 4: mixed_delta_unplanes<1>(src, dst, fg, B, wg, W, lds, wtot); break;
        case 5: mixed_delta_unplanes<2>(src, dst, fg, B, wg, W, lds, wtot); break;
        case 6: mixed_delta_unplanes<4>(src, dst, fg, B, wg, W, lds, wtot); break;
        default: mixed_delta_unplanes<8>(src, dst, fg, B, wg, W, lds, wtot); break;
        }
    }
}

// ---- the general path -------------------------------------------------------------------------------------------------
// Forward: source bytes [first, len) of the whole buffer, bytes_forward with the element size and the filter read from the
// table.  Inverse: workgroup w takes units w, w + gridDim.x, ... from `first` on, frame by frame with bytes_inverse_frame.
template <bool INVERSE>
__global__ void __launch_bounds__(256) k_mixed_bytes(MixedArgs a)
{
    const uint64_t unit = (uint64_t)kMixedUnit * a.block_size;
    if (!INVERSE) {
        for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
            const uint32_t k = a.table[o / unit] & 7;
            bytes_forward(a.src, a.dst, o, a.len, 1u << (k & 3), a.block_size, k >= 4);
        }
    } else {
        __shared__ uint64_t wtot[2][4];
        const uint64_t nunits = (a.len - a.first + unit - 1) / unit;
        uint32_t row = 0;
        for (uint64_t ui = blockIdx.x; ui < nunits; ui += gridDim.x) { // (every loop below is uniform over the workgroup)
            const uint64_t ubase = a.first + ui * unit;
            const uint32_t k = a.table[ubase / unit] & 7, E = 1u << (k & 3);
            const uint64_t frame = (uint64_t)E * a.block_size;
            const uint64_t uend = a.len - ubase < unit ? a.len : ubase + unit;
            for (uint64_t base = ubase; base < uend; base += frame)
                bytes_inverse_frame(a.src, a.dst, base, uend - base < frame ? uend - base : frame, E, k >= 4, wtot, row);
        }
    }
}

} // namespace redux
