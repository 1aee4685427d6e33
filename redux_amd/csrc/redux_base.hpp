// redux_base.hpp -- the XOR-against-base filter for series of snapshots (checkpoint N against checkpoint N - 1, a
// fine-tuned model against its base), fused with the byte-plane layout (redux_planes.hpp): a byte transform in front of
// the coder, next to k_planes and k_delta_planes, with a second input.
//
//   k_base_planes<E>          forward, full frames inside the base: k_planes's shape (16 elements per lane, the interleaved
//                             side staged through LDS) with a second coalesced 16-byte load, from the base, XORed in on the
//                             way into LDS, in front of planes_permute; E = 1: a plain 16-byte XOR stream, no LDS
//   k_base_unplanes<E>        inverse, full frames inside the base: the plane loads, planes_permute inverse, the interleaved
//                             side through LDS and XORed with the base's 16-byte chunk on the way out; no scan and no carry
//                             along the frame, so k_planes's inverse shape
//   k_base_planes_bytes<E>    one destination byte per thread, any alignment and block size: the short last frame, the frame
//   k_base_unplanes_bytes<E>  the end of the base falls into, and everything when a pointer or the block size is no 16-byte
//                             multiple
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

// Forward, full frames inside the base.  The wave's 1024*E contiguous bytes of the source and of the base are loaded with
// the same coalesced 16-byte accesses and meet on the way into LDS; from there on it is planes_group's forward form.
template <int E>
__global__ void __launch_bounds__(256) k_base_planes(BaseArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (E == 1) { // no layout: group g is 16 bytes of the stream
        if (g < a.groups)
            ((uint4 *)a.dst)[g] = base_xor(((const uint4 *)a.src)[g], ((const uint4 *)a.base)[g]);
    } else {
        __shared__ uint4 lds[4 * 64 * E];
        const uint32_t lane  = threadIdx.x & 63;
        const uint64_t g0    = g - lane;
        const bool     live  = g < a.groups;
        const uint64_t f     = live ? g / a.frame_groups : 0;
        const uint64_t i     = live ? g - f * a.frame_groups : 0;
        const uint64_t fbase = f * (uint64_t)E * a.block_size;
        const uint64_t left  = g0 < a.groups ? a.groups - g0 : 0;
        const uint32_t wave_chunks = (uint32_t)((left < 64 ? left : 64) * E);
        uint4 *wl = lds + (threadIdx.x >> 6) * 64 * E;

        const uint4 *s = (const uint4 *)(a.src + g0 * 16 * E);
        const uint4 *y = (const uint4 *)(a.base + g0 * 16 * E);
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint32_t c = k * 64 + lane;
            if (c < wave_chunks)
                wl[planes_lds_slot<E>(c)] = base_xor(s[c], y[c]);
        }
        __syncthreads();
        if (!live)
            return;
        uint32_t in[4 * E], out[4 * E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint4 v = wl[planes_lds_slot<E>(lane * E + k)];
            in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
        }
        planes_permute<E, false>(in, out);
#pragma unroll
        for (int p = 0; p < E; p++)
            *(uint4 *)(a.dst + fbase + (uint64_t)p * a.block_size + i * 16) = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
    }
}

// Inverse, full frames inside the base: planes_group's inverse staged form, the base XORed in where the wave writes its
// contiguous bytes.
template <int E>
__global__ void __launch_bounds__(256) k_base_unplanes(BaseArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (E == 1) {
        if (g < a.groups)
            ((uint4 *)a.dst)[g] = base_xor(((const uint4 *)a.src)[g], ((const uint4 *)a.base)[g]);
    } else {
        __shared__ uint4 lds[4 * 64 * E];
        const uint32_t lane  = threadIdx.x & 63;
        const uint64_t g0    = g - lane;
        const bool     live  = g < a.groups;
        const uint64_t f     = live ? g / a.frame_groups : 0;
        const uint64_t i     = live ? g - f * a.frame_groups : 0;
        const uint64_t fbase = f * (uint64_t)E * a.block_size;
        const uint64_t left  = g0 < a.groups ? a.groups - g0 : 0;
        const uint32_t wave_chunks = (uint32_t)((left < 64 ? left : 64) * E);
        uint4 *wl = lds + (threadIdx.x >> 6) * 64 * E;

        // the base's chunks first: they depend on nothing, and are in flight while the planes are permuted
        const uint4 *y = (const uint4 *)(a.base + g0 * 16 * E);
        uint4 yb[E];
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint32_t c = k * 64 + lane;
            yb[k] = c < wave_chunks ? y[c] : make_uint4(0, 0, 0, 0);
        }
        if (live) {
            uint32_t in[4 * E], out[4 * E];
#pragma unroll
            for (int p = 0; p < E; p++) {
                const uint4 v = *(const uint4 *)(a.src + fbase + (uint64_t)p * a.block_size + i * 16);
                in[4 * p] = v.x; in[4 * p + 1] = v.y; in[4 * p + 2] = v.z; in[4 * p + 3] = v.w;
            }
            planes_permute<E, true>(in, out);
#pragma unroll
            for (int k = 0; k < E; k++)
                wl[planes_lds_slot<E>(lane * E + k)] = make_uint4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
        }
        __syncthreads();
        uint4 *d = (uint4 *)(a.dst + g0 * 16 * E);
#pragma unroll
        for (int k = 0; k < E; k++) {
            const uint32_t c = k * 64 + lane;
            if (c < wave_chunks)
                d[c] = base_xor(wl[planes_lds_slot<E>(c)], yb[k]);
        }
    }
}

// Destination bytes [first, end) of the whole buffer, one per thread: k_planes_bytes's index rule; the base byte is the one
// at the INTERLEAVED position (the source's forward, the destination's inverse), zero from base_len on.
template <int E, bool INVERSE>
__device__ __forceinline__ void base_bytes(const BaseArgs &a)
{
    const uint64_t frame = (uint64_t)E * a.block_size;
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.end; o += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t f = o / frame, fb = f * frame, r = o - fb;
        const uint64_t L = a.len - fb < frame ? a.len - fb : frame;
        const uint64_t n = L / E; // elements of this frame
        uint64_t s = r;           // trailing bytes: in place
        if (r < n * E)
            s = INVERSE ? (r % E) * n + r / E : (r % n) * E + r / n;
        const uint64_t yi = INVERSE ? o : fb + s;
        const uint8_t  y  = yi < a.base_len ? a.base[yi] : (uint8_t)0;
        a.dst[o] = a.src[fb + s] ^ y;
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
