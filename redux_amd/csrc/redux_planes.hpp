// redux_planes.hpp -- the byte-plane layout of typed data ("shuffle" filter), a byte transform in front of the coder.
//
//   k_planes<E, INVERSE>        full frames: 16 elements per lane, E 16-byte loads, v_perm_b32, E 16-byte stores; the
//                               interleaved side moved by the wave with coalesced 16-byte accesses through LDS
//   k_planes_bytes<E, INVERSE>  one byte per thread: the short last frame, unaligned buffers, blocks not a multiple of 16
//
// Layout (E = element size, B = block size): the input is cut into frames of E*B bytes (only the last may be shorter); a
// frame of L bytes holds N = L / E elements, byte p of element i moves to frame offset p*N + i, and the L - N*E trailing
// bytes stay where they are.  A full frame thus becomes E blocks, block j of the frame being plane j of B elements.  The
// adaptive model's cost of a block does not depend on the order of its bytes, so the layout only pays because each BLOCK
// holds one plane ("Byte planes").
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace redux {

struct PlanesArgs {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       groups;       // full frames * frame_groups: 16-element groups of the fast path
    uint32_t       frame_groups; // block_size / 16
    uint32_t       block_size;
    uint64_t       first, len;   // k_planes_bytes: destination bytes [first, len)
};

// Lane-local permutation of 16 elements (16*E bytes, 4*E dwords).  Forward: byte q = 16*p + i of the result (plane p,
// element i) is byte i*E + p of the elements; inverse the other way round.
template <int E, bool INVERSE>
__device__ __forceinline__ constexpr int planes_src_byte(int q)
{
    return INVERSE ? (q % E) * 16 + q / E : (q % 16) * E + q / 16;
}

template <int E, bool INVERSE>
__device__ __forceinline__ void planes_permute(const uint32_t (&in)[4 * E], uint32_t (&out)[4 * E])
{
#pragma unroll
    for (int d = 0; d < 4 * E; d++) {
        const int s0 = planes_src_byte<E, INVERSE>(4 * d), s1 = planes_src_byte<E, INVERSE>(4 * d + 1);
        const int s2 = planes_src_byte<E, INVERSE>(4 * d + 2), s3 = planes_src_byte<E, INVERSE>(4 * d + 3);
        // v_perm_b32(hi, lo, sel): selector 0-3 = a byte of lo, 4-7 = a byte of hi, 0x0c = zero.  All selectors are
        // constants after unrolling; two source bytes in one dword fold into one perm.
        const uint32_t lo = __builtin_amdgcn_perm(in[s1 >> 2], in[s0 >> 2], (uint32_t)(s0 & 3) | (uint32_t)(4 + (s1 & 3)) << 8 | 0x0c0c0000u);
        const uint32_t hi = __builtin_amdgcn_perm(in[s3 >> 2], in[s2 >> 2], (uint32_t)(s2 & 3) | (uint32_t)(4 + (s3 & 3)) << 8 | 0x0c0c0000u);
        out[d]            = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
    }
}

// Where chunk c (16 bytes) of a wave's interleaved region sits in LDS: chunk k of lane l's 16*E bytes is rotated by l
// inside the lane's own E chunks, so that 16 lanes reading (or writing) their k-th chunk hit 16 different bank groups.
template <int E>
__device__ __forceinline__ uint32_t planes_lds_slot(uint32_t c)
{
    const uint32_t l = c / E;
    return l * E + ((c + l) & (E - 1));
}

// One group of 16 elements per lane.  The planes side is always read / written straight from / to memory: a wave's 64
// lanes cover 1 KiB of each plane.  The interleaved side (16*E bytes per lane) is either accessed lane-strided
// (STAGED = false: E 16-byte accesses per lane at a stride of 16*E bytes) or staged through LDS (STAGED = true: the wave
// moves its 1024*E contiguous bytes with fully coalesced 16-byte accesses and the lanes exchange them in LDS).
// Every thread of the workgroup must call this (the staged form has barriers).
template <int E, bool INVERSE, bool STAGED>
__device__ __forceinline__ void planes_group(const PlanesArgs &a, uint4 *lds)
{
    const uint64_t g     = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane  = threadIdx.x & 63;
    const uint64_t g0    = g - lane;                                      // the wave's first group
    const bool     live  = g < a.groups;
    const uint64_t f     = live ? g / a.frame_groups : 0;
    const uint64_t i     = live ? g - f * a.frame_groups : 0;
    const uint64_t fbase = f * (uint64_t)E * a.block_size;
    const uint64_t left  = g0 < a.groups ? a.groups - g0 : 0;
    const uint32_t wave_chunks = (uint32_t)((left < 64 ? left : 64) * E); // 16-byte chunks the wave owns
    uint4 *wl = lds + (threadIdx.x >> 6) * 64 * E;

    uint32_t in[4 * E], out[4 * E];
    if (!INVERSE) {
        if (STAGED) {
            const uint4 *s = (const uint4 *)(a.src + g0 * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint32_t c = k * 64 + lane;
                if (c < wave_chunks)
                    wl[planes_lds_slot<E>(c)] = s[c];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint4 v = wl[planes_lds_slot<E>(lane * E + k)];
                in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
            }
        } else if (live) {
            const uint4 *s = (const uint4 *)(a.src + g * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint4 v = s[k];
                in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
            }
        }
        if (!live)
            return;
        planes_permute<E, false>(in, out);
#pragma unroll
        for (int p = 0; p < E; p++)
            *(uint4 *)(a.dst + fbase + (uint64_t)p * a.block_size + i * 16) = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
    } else {
        if (live) {
#pragma unroll
            for (int p = 0; p < E; p++) {
                const uint4 v = *(const uint4 *)(a.src + fbase + (uint64_t)p * a.block_size + i * 16);
                in[4 * p] = v.x; in[4 * p + 1] = v.y; in[4 * p + 2] = v.z; in[4 * p + 3] = v.w;
            }
            planes_permute<E, true>(in, out);
        }
        if (STAGED) {
            if (live)
#pragma unroll
                for (int k = 0; k < E; k++)
                    wl[planes_lds_slot<E>(lane * E + k)] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
            __syncthreads();
            uint4 *d = (uint4 *)(a.dst + g0 * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++) {
                const uint32_t c = k * 64 + lane;
                if (c < wave_chunks)
                    d[c] = wl[planes_lds_slot<E>(c)];
            }
        } else if (live) {
            uint4 *d = (uint4 *)(a.dst + g * 16 * E);
#pragma unroll
            for (int k = 0; k < E; k++)
                d[k] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
        }
    }
}

// LDS staging measured faster than lane-strided direct access, by up to 14 % at E = 8 and never slower beyond noise
// (4 GiB, B = 64 KiB: DESIGN.md, "Byte planes"; tools/ab/planes_ab.hip).
constexpr bool kPlanesStaged = true;

template <int E, bool INVERSE>
__global__ void __launch_bounds__(256) k_planes(PlanesArgs a)
{
    __shared__ uint4 lds[kPlanesStaged ? 4 * 64 * E : 1];
    planes_group<E, INVERSE, kPlanesStaged>(a, lds);
}

// Destination bytes [first, len) of the whole buffer, one per thread: any alignment, any block size.
template <int E, bool INVERSE>
__global__ void __launch_bounds__(256) k_planes_bytes(PlanesArgs a)
{
    const uint64_t frame = (uint64_t)E * a.block_size;
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f = o / frame, base = f * frame, r = o - base;
        const uint64_t L = a.len - base < frame ? a.len - base : frame;
        const uint64_t n = L / E; // elements of this frame
        uint64_t s = r;           // trailing bytes: in place
        if (r < n * E)
            s = INVERSE ? (r % E) * n + r / E  // interleaved byte r = byte r%E of element r/E <- plane r%E
                        : (r % n) * E + r / n; // plane r/n, element r%n <- byte r/n of element r%n
        a.dst[o] = a.src[base + s];
    }
}

// A decoded plane block must have exactly the size its place in the frame gives it: min(B, out_len - b*B) bytes.  A block
// that decoded OK to another size becomes INVALID_INPUT and is counted in the summary (the decoder has summarised already).
__global__ void __launch_bounds__(256) k_planes_sizes(const uint32_t *sizes, int32_t *status, int32_t *summary, uint64_t nblocks,
                                                      uint64_t out_len, uint32_t block_size)
{
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < nblocks; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t o    = b * block_size;
        const uint64_t want = out_len > o ? (out_len - o < block_size ? out_len - o : block_size) : 0;
        if (status[b] == REDUX_OK && sizes[b] != want) {
            status[b] = REDUX_INVALID_INPUT;
            if (summary) {
                atomicAdd(&summary[1], 1);
                atomicCAS(&summary[0], REDUX_OK, REDUX_INVALID_INPUT);
            }
        }
    }
}

// Bytes the layout calls carve from the FRONT of a workspace for the transformed copy of len bytes (16 bytes of slack for
// the coder's last 16-byte load, a 256-byte multiple so that what follows stays aligned).
static inline uint64_t planes_copy_bytes(uint64_t len) { return (len + 16 + 255) / 256 * 256; }

} // namespace redux
