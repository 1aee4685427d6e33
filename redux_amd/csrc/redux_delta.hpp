// redux_delta.hpp -- the delta filter for integer series, fused with the byte-plane layout (redux_planes.hpp): a byte
// transform in front of the coder, next to k_planes.
//
//   k_delta_planes<E>          forward, full frames: k_planes's shape (16 elements per lane, the interleaved side staged
//                              through LDS) with one subtraction in front of planes_permute; one read and one write
//   k_delta_unplanes<E>        inverse, full frames: one workgroup walks one frame, 256 lanes x 16 elements per iteration:
//                              E plane loads, planes_permute inverse, a serial prefix over the lane's 16 elements in
//                              registers, the lane totals scanned across the wave with __shfl_up, the wave totals carried
//                              through LDS, a running carry along the frame, the interleaved side written through LDS
//   k_delta_planes_bytes<E>    forward, one element per thread: the short last frame, unaligned buffers, blocks not a
//   k_delta_unplanes_bytes<E>  multiple of 16; the inverse with one workgroup per frame and a scan of one element per lane
//
// Rule (E = element size, B = block size): the input is cut into the frames of the byte-plane layout (E*B bytes, only the
// last may be shorter; E = 1: one block).  A frame of L bytes holds N = L / E little-endian unsigned elements x[0..N); the
// filter writes d[0] = x[0], d[i] = x[i] - x[i-1] mod 2^(8E); the L - N*E trailing bytes stay as they are; the layout is
// then applied to the d's (none for E = 1).  The inverse undoes the layout and takes the running sum mod 2^(8E) inside
// each frame.  Every frame starts afresh, so the blocks of different frames stay independent.  The sum mod 2^(8E) is
// associative and exact: any scan order gives the same bytes.
//
// Arithmetic is per element: E = 1 and 2 elements share a dword and are added / subtracted with the carry between them cut
// (delta_add / delta_sub), E = 8 is a 64-bit add.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_planes.hpp"

namespace redux {

// what carries a sum of elements: a dword for E <= 4 (taken mod 2^(8E) where it is used), 64 bits for E = 8
template <int E> struct DeltaSum { typedef uint32_t T; };
template <> struct DeltaSum<8> { typedef uint64_t T; };

// a - b and a + b on the 4 / E elements packed in a dword, no borrow or carry from one element into the next
template <int E>
__device__ __forceinline__ uint32_t delta_sub(uint32_t a, uint32_t b)
{
    if (E >= 4)
        return a - b;
    constexpr uint32_t H = E == 2 ? 0x80008000u : 0x80808080u; // the elements' top bits
    return ((a | H) - (b & ~H)) ^ ((a ^ ~b) & H);
}

template <int E>
__device__ __forceinline__ uint32_t delta_add(uint32_t a, uint32_t b)
{
    if (E >= 4)
        return a + b;
    constexpr uint32_t H = E == 2 ? 0x80008000u : 0x80808080u;
    return ((a & ~H) + (b & ~H)) ^ ((a ^ b) & H);
}

// v (16 elements, 4*E dwords) -> their differences; prev = the element before v[0] (0 at a frame start): the element
// itself for E = 8, else the dword that ENDS with it (its top E bytes)
template <int E>
__device__ __forceinline__ void delta_diff(const uint32_t (&v)[4 * E], typename DeltaSum<E>::T prev, uint32_t (&d)[4 * E])
{
    if constexpr (E == 8) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t x = (uint64_t)v[2 * j + 1] << 32 | v[2 * j];
            const uint64_t p = j ? (uint64_t)v[2 * j - 1] << 32 | v[2 * j - 2] : prev;
            const uint64_t r = x - p;
            d[2 * j] = (uint32_t)r; d[2 * j + 1] = (uint32_t)(r >> 32);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * E; j++) {
            // the dword one element earlier in the series: E = 4 the dword before, else the two dwords shifted by one element
            uint32_t p = j ? v[j - 1] : prev;
            if constexpr (E < 4)
                p = v[j] << (8 * E) | p >> (32 - 8 * E);
            d[j] = delta_sub<E>(v[j], p);
        }
    }
}

// the running sum of v's 16 elements in place, from 0; returns their total (E < 4: in the low 8*E bits)
template <int E>
__device__ __forceinline__ typename DeltaSum<E>::T delta_prefix(uint32_t (&v)[4 * E])
{
    if constexpr (E == 8) {
        uint64_t s = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            s += (uint64_t)v[2 * j + 1] << 32 | v[2 * j];
            v[2 * j] = (uint32_t)s; v[2 * j + 1] = (uint32_t)(s >> 32);
        }
        return s;
    } else if constexpr (E == 4) {
#pragma unroll
        for (int j = 1; j < 16; j++)
            v[j] += v[j - 1];
        return v[15];
    } else {
        uint32_t carry = 0; // the last element so far
#pragma unroll
        for (int j = 0; j < 4 * E; j++) {
            uint32_t w = v[j];
            w = delta_add<E>(w, w << (8 * E)); // the running sum inside the dword
            if (E == 1)
                w = delta_add<E>(w, w << 16);
            w     = delta_add<E>(w, carry * (E == 2 ? 0x00010001u : 0x01010101u));
            carry = w >> (32 - 8 * E);
            v[j]  = w;
        }
        return carry;
    }
}

// v's 16 elements += s
template <int E>
__device__ __forceinline__ void delta_offset(uint32_t (&v)[4 * E], typename DeltaSum<E>::T s)
{
    if constexpr (E == 8) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t x = ((uint64_t)v[2 * j + 1] << 32 | v[2 * j]) + s;
            v[2 * j] = (uint32_t)x; v[2 * j + 1] = (uint32_t)(x >> 32);
        }
    } else {
        const uint32_t b = E == 4 ? s : E == 2 ? (s & 0xFFFFu) * 0x00010001u : (s & 0xFFu) * 0x01010101u;
#pragma unroll
        for (int j = 0; j < 4 * E; j++)
            v[j] = delta_add<E>(v[j], b);
    }
}

// inclusive scan of x across the wave's 64 lanes (all of them must call it)
template <typename T>
__device__ __forceinline__ T delta_wave_scan(T x, uint32_t lane)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        T u;
        if constexpr (sizeof(T) == 8)
            u = (T)__shfl_up((unsigned long long)x, s);
        else
            u = (T)__shfl_up((unsigned int)x, s);
        if (lane >= (uint32_t)s)
            x += u;
    }
    return x;
}

// Forward, full frames: planes_group's forward staged form with the subtraction in front of the permutation.  A lane's
// predecessor element is the end of the 16-byte chunk before its own in the wave's staged region; the wave's first lane
// loads it from memory; at a frame start there is none.
template <int E>
__global__ void __launch_bounds__(256) k_delta_planes(PlanesArgs a)
{
    typedef typename DeltaSum<E>::T T;
    __shared__ uint4 lds[4 * 64 * E];
    const uint64_t g     = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane  = threadIdx.x & 63;
    const uint64_t g0    = g - lane;
    const bool     live  = g < a.groups;
    const uint64_t f     = live ? g / a.frame_groups : 0;
    const uint64_t i     = live ? g - f * a.frame_groups : 0;
    const uint64_t fbase = f * (uint64_t)E * a.block_size;
    const uint64_t left  = g0 < a.groups ? a.groups - g0 : 0;
    const uint32_t wave_chunks = (uint32_t)((left < 64 ? left : 64) * E);
    uint4 *wl = lds + (threadIdx.x >> 6) * 64 * E;

    T prev = 0;
    if (live && i != 0 && lane == 0) // (i != 0: the bytes before the wave's region belong to the same frame)
        prev = *(const T *)(a.src + g * 16 * E - sizeof(T));
    const uint4 *s = (const uint4 *)(a.src + g0 * 16 * E);
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint32_t c = k * 64 + lane;
        if (c < wave_chunks)
            wl[planes_lds_slot<E>(c)] = s[c];
    }
    __syncthreads();
    if (!live)
        return;
    uint32_t in[4 * E], d[4 * E], out[4 * E];
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint4 v = wl[planes_lds_slot<E>(lane * E + k)];
        in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w;
    }
    if (i != 0 && lane != 0) {
        const uint4 *c = &wl[planes_lds_slot<E>(lane * E - 1)];
        if constexpr (E == 8)
            prev = ((const uint64_t *)c)[1];
        else
            prev = ((const uint32_t *)c)[3];
    }
    delta_diff<E>(in, prev, d);
    planes_permute<E, false>(d, out);
#pragma unroll
    for (int p = 0; p < E; p++)
        *(uint4 *)(a.dst + fbase + (uint64_t)p * a.block_size + i * 16) = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
}

// Inverse, full frames: workgroup w walks frames w, w + gridDim.x, ...; an iteration takes 256 groups of 16 elements.
// The plane loads of the next iteration are issued before this one's scan, so the dependency chain along the frame (scan,
// two barriers) overlaps the memory latency.  The wave totals alternate between two LDS rows, so one barrier per
// iteration orders them.
template <int E>
__global__ void __launch_bounds__(256) k_delta_unplanes(PlanesArgs a)
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
        if (threadIdx.x < a.frame_groups) {
#pragma unroll
            for (int p = 0; p < E; p++) {
                const uint4 v = *(const uint4 *)(a.src + fbase + (uint64_t)p * a.block_size + (uint64_t)threadIdx.x * 16);
                nxt[4 * p] = v.x; nxt[4 * p + 1] = v.y; nxt[4 * p + 2] = v.z; nxt[4 * p + 3] = v.w;
            }
        }
        for (uint32_t i0 = 0; i0 < a.frame_groups; i0 += 256, row ^= 1) {
            const uint32_t i    = i0 + threadIdx.x;
            const bool     live = i < a.frame_groups;
            uint32_t in[4 * E], v[4 * E];
#pragma unroll
            for (int q = 0; q < 4 * E; q++)
                in[q] = nxt[q];
            if ((uint64_t)i + 256 < a.frame_groups) {
#pragma unroll
                for (int p = 0; p < E; p++) {
                    const uint4 x = *(const uint4 *)(a.src + fbase + (uint64_t)p * a.block_size + ((uint64_t)i + 256) * 16);
                    nxt[4 * p] = x.x; nxt[4 * p + 1] = x.y; nxt[4 * p + 2] = x.z; nxt[4 * p + 3] = x.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    nxt[q] = 0;
            }
            planes_permute<E, true>(in, v); // (lanes past the frame: zeros, a total of 0)
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
#pragma unroll
                for (int k = 0; k < E; k++)
                    wl[planes_lds_slot<E>(lane * E + k)] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
            __syncthreads();
            const uint32_t w0 = i0 + wave * 64; // the wave's first group of the frame
            if (w0 < a.frame_groups) {
                const uint32_t left = a.frame_groups - w0, wave_chunks = (left < 64 ? left : 64) * E;
                uint4 *d = (uint4 *)(a.dst + fbase + (uint64_t)w0 * 16 * E);
#pragma unroll
                for (int k = 0; k < E; k++) {
                    const uint32_t c = k * 64 + lane;
                    if (c < wave_chunks)
                        d[c] = wl[planes_lds_slot<E>(c)];
                }
            }
        }
    }
}

// Forward, any alignment and block size: source bytes [first, len) of the whole buffer, the thread of an element's first
// byte does the element, the threads of a frame's trailing bytes copy them.
template <int E>
__global__ void __launch_bounds__(256) k_delta_planes_bytes(PlanesArgs a)
{
    const uint64_t frame = (uint64_t)E * a.block_size;
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
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
#pragma unroll
        for (int k = 0; k < E; k++) {
            x |= (uint64_t)a.src[o + k] << (8 * k);
            if (i)
                p |= (uint64_t)a.src[o - E + k] << (8 * k);
        }
        const uint64_t d = x - p;
#pragma unroll
        for (int k = 0; k < E; k++)
            a.dst[base + (uint64_t)k * n + i] = (uint8_t)(d >> (8 * k));
    }
}

// Inverse, any alignment and block size: workgroup w takes frames w, w + gridDim.x, ... of [first, len), 256 elements per
// iteration, one per lane, summed in 64 bits (congruent mod 2^(8E)) by a wave scan and the wave totals in LDS.
template <int E>
__global__ void __launch_bounds__(256) k_delta_unplanes_bytes(PlanesArgs a)
{
    __shared__ uint64_t wtot[2][4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t frame = (uint64_t)E * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    uint32_t row = 0;
    for (uint64_t fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
        const uint64_t base = a.first + fi * frame;
        const uint64_t L = a.len - base < frame ? a.len - base : frame;
        const uint64_t n = L / E;
        if (n * E + threadIdx.x < L) // (at most E - 1 trailing bytes)
            a.dst[base + n * E + threadIdx.x] = a.src[base + n * E + threadIdx.x];
        uint64_t carry = 0;
        for (uint64_t i0 = 0; i0 < n; i0 += 256, row ^= 1) {
            const uint64_t i = i0 + threadIdx.x;
            uint64_t d = 0;
            if (i < n)
#pragma unroll
                for (int k = 0; k < E; k++)
                    d |= (uint64_t)a.src[base + (uint64_t)k * n + i] << (8 * k);
            const uint64_t incl = delta_wave_scan<uint64_t>(d, lane);
            if (lane == 63)
                wtot[row][wave] = incl;
            __syncthreads();
            uint64_t x = carry + incl;
#pragma unroll
            for (uint32_t w = 0; w < 4; w++) {
                const uint64_t t = wtot[row][w];
                x += w < wave ? t : 0;
                carry += t;
            }
            if (i < n)
#pragma unroll
                for (int k = 0; k < E; k++)
                    a.dst[base + i * E + k] = (uint8_t)(x >> (8 * k));
        }
    }
}

} // namespace redux
