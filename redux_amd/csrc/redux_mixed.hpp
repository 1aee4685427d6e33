// redux_mixed.hpp -- per-unit layouts for inputs of mixed element types: the layout in front of the adaptive coder chosen
// for every unit of 8 blocks on its own, from the costs k_layout_cost leaves (redux_layout_cost.hpp), gfx950 only.
//
//   k_mixed_choose             bits f64[8][nblocks] and a mask of layouts -> table u8[nunits]: the lowest selected layout with
//                              the smallest sum of the unit's bits (f64, ascending block order from 0.0); the chosen sums are
//                              added to one u64 in 2^-16 bit with a vector atomic.  One thread per unit.
//   k_mixed_planes<INVERSE>    full units, block size and buffers 16-byte multiples: W workgroups per unit read the unit's
//                              layout k = table[u] & 7 once and branch on it, workgroup-uniformly, into k_planes' /
//                              k_delta_planes' / k_delta_unplanes' bodies with the unit in place of the buffer: 16 elements
//                              per lane, 16-byte accesses, the interleaved side through LDS, planes_permute, delta_diff, the
//                              delta inverse one workgroup per frame with one running carry.  A unit holds 8 / E frames of
//                              B / 16 groups each; W = ceil(B / 16 / 256) workgroups are what E = 8 needs at one group per
//                              lane, and the smaller element sizes take 8 / E rows of 256 groups per round (forward, delta
//                              inverse: 128 bytes per lane and barrier pair whatever E) or 8 / E rounds (plain inverse), so
//                              no workgroup of a plain or forward unit is idle whatever the table holds.  The delta inverse
//                              has 8 / E frames per unit: workgroups past them leave before the first barrier.
//   k_mixed_bytes<INVERSE>     everything else -- the short last unit, unaligned buffers, blocks not a multiple of 16 -- one
//                              element per thread; the inverse one workgroup per unit, frame by frame, with the scan of
//                              k_delta_unplanes_bytes (the plain layouts skip the sum).  Right, not fast.
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

// forward, E > 1 or DELTA: k_delta_planes' body (k_planes' staged forward body without the subtraction), 8 / E rows of 256
// groups per round and barrier pair -- 128 bytes per lane whatever the element size, so that a unit is one round of each
// of its workgroups (with one row per round, E = 1 behind the filter ran 8 rounds and measured 25 % behind k_delta_planes<1>)
template <int E, bool DELTA>
__device__ __forceinline__ void mixed_forward(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                              uint32_t wg, uint32_t nwg, uint4 *lds)
{
    typedef typename DeltaSum<E>::T T;
    constexpr int      R      = 8 / E;
    const uint32_t     groups = frame_groups * R; // of the unit: 8 / E frames
    const uint32_t     lane   = threadIdx.x & 63;
    uint4             *wl     = lds + (threadIdx.x >> 6) * 64 * 8; // R rows of 64 * E chunks
    for (uint32_t t0 = wg * 256 * R; t0 < groups; t0 += nwg * 256 * R) { // (uniform over the workgroup)
        T prev[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t g = t0 + r * 256 + threadIdx.x, g0 = g - lane;
            const uint32_t left = g0 < groups ? groups - g0 : 0;
            const uint32_t wave_chunks = (left < 64 ? left : 64) * E;
            prev[r] = 0;
            if (DELTA && g < groups && g % frame_groups != 0 && lane == 0) // (the bytes before belong to the same frame)
                prev[r] = *(const T *)(src + (uint64_t)g * 16 * E - sizeof(T));
            const uint4 *s = (const uint4 *)(src + (uint64_t)g0 * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint32_t c = k * 64 + lane;
                if (c < wave_chunks)
                    wl[r * 64 * E + planes_lds_slot<E>(c)] = s[c];
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const uint32_t g = t0 + r * 256 + threadIdx.x;
            if (g < groups) {
                const uint32_t f     = g / frame_groups, i = g - f * frame_groups;
                const uint64_t fbase = (uint64_t)f * E * block_size;
                const uint4   *row   = wl + r * 64 * E;
                uint32_t in[4 * E], out[4 * E];
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const uint4 v = row[planes_lds_slot<E>(lane * E + k)];
                    in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
                }
                if constexpr (DELTA) {
                    T p = prev[r];
                    if (i != 0 && lane != 0) {
                        const uint4 *c = &row[planes_lds_slot<E>(lane * E - 1)];
                        if constexpr (E == 8)
                            p = ((const uint64_t *)c)[1];
                        else
                            p = ((const uint32_t *)c)[3];
                    }
                    uint32_t d[4 * E];
                    delta_diff<E>(in, p, d);
                    planes_permute<E, false>(d, out);
                } else {
                    planes_permute<E, false>(in, out);
                }
#pragma unroll
                for (int p = 0; p < E; p++)
                    *(uint4 *)(dst + fbase + (uint64_t)p * block_size + (uint64_t)i * 16) = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
            }
        }
        __syncthreads(); // (the next round stages into the same rows)
    }
}

// inverse of the plain layouts, E > 1: k_planes' staged inverse body
template <int E>
__device__ __forceinline__ void mixed_unplanes(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                               uint32_t wg, uint32_t nwg, uint4 *lds)
{
    const uint32_t groups = frame_groups * (8 / E);
    const uint32_t lane   = threadIdx.x & 63;
    uint4         *wl     = lds + (threadIdx.x >> 6) * 64 * E;
    for (uint32_t t0 = wg * 256; t0 < groups; t0 += nwg * 256) {
        const uint32_t g = t0 + threadIdx.x, g0 = g - lane;
        if (g < groups) {
            const uint32_t f     = g / frame_groups, i = g - f * frame_groups;
            const uint64_t fbase = (uint64_t)f * E * block_size;
            uint32_t in[4 * E], out[4 * E];
#pragma unroll
            for (int p = 0; p < E; p++) {
                const uint4 v = *(const uint4 *)(src + fbase + (uint64_t)p * block_size + (uint64_t)i * 16);
                in[4 * p] = v.x; in[4 * p + 1] = v.y; in[4 * p + 2] = v.z; in[4 * p + 3] = v.w;
            }
            planes_permute<E, true>(in, out);
#pragma unroll
            for (int k = 0; k < E; k++)
                wl[planes_lds_slot<E>(lane * E + k)] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
        }
        __syncthreads();
        if (g0 < groups) {
            const uint32_t left = groups - g0, wave_chunks = (left < 64 ? left : 64) * E;
            uint4 *d = (uint4 *)(dst + (uint64_t)g0 * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint32_t c = k * 64 + lane;
                if (c < wave_chunks)
                    d[c] = wl[planes_lds_slot<E>(c)];
            }
        }
        __syncthreads();
    }
}

// inverse of the delta layouts: k_delta_unplanes' body, workgroup wg walks frames wg, wg + nwg, ... of the unit's 8 / E.  An
// iteration takes 8 / E rows of 256 groups under one pair of barriers -- 128 bytes per lane whatever the element size: the
// walk along a frame is a chain of barriers, and with one row per iteration the small element sizes moved too few bytes per
// link (E = 1: 4.0 ms for 4 GiB against k_delta_unplanes<1>'s 1.6, which has 8 workgroups on a CU where this kernel has 3).
// Row r's running sum starts from the carry behind rows 0 .. r - 1: the totals of every row's waves are in LDS after the
// first barrier.
template <int E>
__device__ __forceinline__ void mixed_delta_unplanes(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size,
                                                     uint32_t wg, uint32_t nwg, uint4 *lds, uint64_t (*wtot64)[8][4])
{
    typedef typename DeltaSum<E>::T T;
    constexpr int R = 8 / E;
    T (*wtot)[8][4] = (T (*)[8][4])wtot64;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 *wl = lds + wave * 64 * 8; // R rows of 64 * E chunks
    uint32_t row = 0;
    for (uint32_t f = wg; f < 8 / E; f += nwg) {
        const uint64_t fbase = (uint64_t)f * E * block_size;
        T        carry = 0; // the sum of the frame's elements before this iteration
        uint32_t nxt[R][4 * E];
        auto load = [&](uint32_t i0) { // rows i0 / 256 .. of the frame; a lane past the frame's end gets zeros (a total of 0)
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t i = i0 + r * 256 + threadIdx.x;
#pragma unroll
                for (int p = 0; p < E; p++) {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (i < frame_groups)
                        v = *(const uint4 *)(src + fbase + (uint64_t)p * block_size + (uint64_t)i * 16);
                    nxt[r][4 * p] = v.x; nxt[r][4 * p + 1] = v.y; nxt[r][4 * p + 2] = v.z; nxt[r][4 * p + 3] = v.w;
                }
            }
        };
        load(0);
        for (uint32_t i0 = 0; i0 < frame_groups; i0 += 256 * R, row ^= 1) {
            uint32_t v[R][4 * E];
            T        total[R], incl[R];
#pragma unroll
            for (int r = 0; r < R; r++)
                planes_permute<E, true>(nxt[r], v[r]);
            if (i0 + 256 * R < frame_groups) // the next iteration's loads are in flight while this one scans
                load(i0 + 256 * R);
#pragma unroll
            for (int r = 0; r < R; r++) {
                total[r] = delta_prefix<E>(v[r]);
                incl[r]  = delta_wave_scan<T>(total[r], lane);
                if (lane == 63)
                    wtot[row][r][wave] = incl[r];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; r++) {
                T before = carry + incl[r] - total[r];
#pragma unroll
                for (uint32_t w = 0; w < 4; w++) {
                    const T t = wtot[row][r][w];
                    before += w < wave ? t : 0;
                    carry += t;
                }
                delta_offset<E>(v[r], before);
                if (i0 + r * 256 + threadIdx.x < frame_groups)
#pragma unroll
                    for (int k = 0; k < E; k++)
                        wl[r * 64 * E + planes_lds_slot<E>(lane * E + k)] = make_uint4(v[r][4 * k], v[r][4 * k + 1], v[r][4 * k + 2], v[r][4 * k + 3]);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t w0 = i0 + r * 256 + wave * 64; // the wave's first group of the row
                if (w0 < frame_groups) {
                    const uint32_t left = frame_groups - w0, wave_chunks = (left < 64 ? left : 64) * E;
                    uint4 *d = (uint4 *)(dst + fbase + (uint64_t)w0 * 16 * E);
#pragma unroll
                    for (int k = 0; k < E; k++) {
                        const uint32_t c = k * 64 + lane;
                        if (c < wave_chunks)
                            d[c] = wl[r * 64 * E + planes_lds_slot<E>(c)];
                    }
                }
            }
        }
    }
}

// (three waves per SIMD, k_delta_unplanes<8>'s occupancy: without the hint the inverse takes 170 VGPRs, two over the 168 that fit)
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
        case 1: mixed_forward<2, false>(src, dst, fg, B, wg, W, lds); break;
        case 2: mixed_forward<4, false>(src, dst, fg, B, wg, W, lds); break;
        case 3: mixed_forward<8, false>(src, dst, fg, B, wg, W, lds); break;
        case 4: mixed_forward<1, true>(src, dst, fg, B, wg, W, lds); break;
        case 5: mixed_forward<2, true>(src, dst, fg, B, wg, W, lds); break;
        case 6: mixed_forward<4, true>(src, dst, fg, B, wg, W, lds); break;
        default: mixed_forward<8, true>(src, dst, fg, B, wg, W, lds); break;
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
// Forward: source bytes [first, len) of the whole buffer; the thread of an element's first byte does the element, the threads
// of a frame's trailing bytes copy them (k_delta_planes_bytes with the element size and the filter read from the table).
// Inverse: workgroup w takes units w, w + gridDim.x, ... from `first` on, frame by frame, 256 elements per iteration, one per
// lane, summed in 64 bits (congruent mod 2^(8E)) by a wave scan and the wave totals in LDS; a plain layout skips the sum.
template <bool INVERSE>
__global__ void __launch_bounds__(256) k_mixed_bytes(MixedArgs a)
{
    const uint64_t unit = (uint64_t)kMixedUnit * a.block_size;
    if (!INVERSE) {
        for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
            const uint32_t k = a.table[o / unit] & 7, E = 1u << (k & 3);
            const bool     delta = k >= 4;
            const uint64_t frame = (uint64_t)E * a.block_size;
            const uint64_t f = o / frame, base = f * frame, r = o - base;
            const uint64_t L = a.len - base < frame ? a.len - base : frame;
            const uint64_t n = L / E;
            if (r >= n * E) {
                a.dst[o] = a.src[o];
                continue;
            }
            if (r % E)
                continue;
            const uint64_t i = r / E;
            uint64_t x = 0, p = 0;
            for (uint32_t q = 0; q < E; q++) {
                x |= (uint64_t)a.src[o + q] << (8 * q);
                if (delta && i)
                    p |= (uint64_t)a.src[o - E + q] << (8 * q);
            }
            const uint64_t d = x - p;
            for (uint32_t q = 0; q < E; q++)
                a.dst[base + (uint64_t)q * n + i] = (uint8_t)(d >> (8 * q));
        }
    } else {
        __shared__ uint64_t wtot[2][4];
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint64_t nunits = (a.len - a.first + unit - 1) / unit;
        uint32_t row = 0;
        for (uint64_t ui = blockIdx.x; ui < nunits; ui += gridDim.x) { // (every loop below is uniform over the workgroup)
            const uint64_t ubase = a.first + ui * unit;
            const uint32_t k = a.table[ubase / unit] & 7, E = 1u << (k & 3);
            const bool     delta = k >= 4;
            const uint64_t frame = (uint64_t)E * a.block_size;
            const uint64_t uend = a.len - ubase < unit ? a.len : ubase + unit;
            for (uint64_t base = ubase; base < uend; base += frame) {
                const uint64_t L = uend - base < frame ? uend - base : frame;
                const uint64_t n = L / E;
                if (n * E + threadIdx.x < L) // (at most E - 1 trailing bytes)
                    a.dst[base + n * E + threadIdx.x] = a.src[base + n * E + threadIdx.x];
                uint64_t carry = 0;
                for (uint64_t i0 = 0; i0 < n; i0 += 256) {
                    const uint64_t i = i0 + threadIdx.x;
                    uint64_t d = 0;
                    if (i < n)
                        for (uint32_t q = 0; q < E; q++)
                            d |= (uint64_t)a.src[base + (uint64_t)q * n + i] << (8 * q);
                    uint64_t x = d;
                    if (delta) { // (the rows alternate from one barrier to the next: only these iterations have one)
                        row ^= 1;
                        const uint64_t incl = delta_wave_scan<uint64_t>(d, lane);
                        if (lane == 63)
                            wtot[row][wave] = incl;
                        __syncthreads();
                        x = carry + incl;
#pragma unroll
                        for (uint32_t w = 0; w < 4; w++) {
                            const uint64_t t = wtot[row][w];
                            x += w < wave ? t : 0;
                            carry += t;
                        }
                    }
                    if (i < n)
                        for (uint32_t q = 0; q < E; q++)
                            a.dst[base + i * E + q] = (uint8_t)(x >> (8 * q));
                }
            }
        }
    }
}

} // namespace redux
