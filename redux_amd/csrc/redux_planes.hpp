// redux_planes.hpp -- the byte-plane layout of typed data ("shuffle" filter), a byte transform in front of the coder, and
// the pieces every layout transform is put together from (redux_delta.hpp, redux_zigzag.hpp, redux_base.hpp, redux_mixed.hpp).
//
//   k_planes<E, INVERSE>        full frames: the forward tile / the plain inverse tile, one row of 256 groups per workgroup
//   k_planes_bytes<E, INVERSE>  one byte per thread under the frame index rule: the short last frame, unaligned buffers,
//                               blocks not a multiple of 16
//
// Layout (E = element size, B = block size): the input is cut into frames of E*B bytes (only the last may be shorter); a
// frame of L bytes holds N = L / E elements, byte p of element i moves to frame offset p*N + i, and the L - N*E trailing
// bytes stay where they are.  A full frame thus becomes E blocks, block j of the frame being plane j of B elements.  The
// adaptive model's cost of a block does not depend on the order of its bytes, so the layout only pays because each BLOCK
// holds one plane ("Byte planes").
//
// The frame tile (full frames, block size and pointers 16-byte multiples): a lane holds one group of 16 elements, 16*E
// bytes in 4*E registers.  The planes side is read / written straight from / to memory, E 16-byte accesses per lane, a
// wave's 64 lanes covering 1 KiB of each plane.  The interleaved side is moved by the wave, its 1024*E contiguous bytes
// with coalesced 16-byte accesses, and the lanes exchange them with the wave's row of LDS (the lane-strided form without
// LDS measured up to 14 % slower at E = 8 and never faster: DESIGN.md, "Byte planes", profiles/r05_planes_ab.txt).
// Between the two sits planes_permute, and in front of it (forward) or behind it (inverse) whatever a filter adds.
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
    uint64_t       first, len;   // byte kernels: bytes [first, len) of the whole buffer
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

// ---- the frame-tile pieces ---------------------------------------------------------------------------------------------
// 16-byte chunks a wave owns whose first group is g0, of `groups` in all
template <int E, typename I>
__device__ __forceinline__ uint32_t tile_wave_chunks(I groups, I g0)
{
    const I left = g0 < groups ? groups - g0 : 0;
    return (uint32_t)((left < 64 ? left : 64) * E);
}

// What a wave applies to a chunk on its way between memory and LDS: hook(chunk, k, c) for the wave's chunk c = 64*k + lane.
struct TileNoHook {
    __device__ __forceinline__ uint4 operator()(uint4 v, int, uint32_t) const { return v; }
};

// Wave stage-in / stage-out: the wave's wave_chunks contiguous chunks at `mem` to / from its LDS row.
template <int E, typename H>
__device__ __forceinline__ void tile_stage_in(uint4 *row, const uint4 *mem, uint32_t wave_chunks, uint32_t lane, H hook)
{
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint32_t c = k * 64 + lane;
        if (c < wave_chunks)
            row[planes_lds_slot<E>(c)] = hook(mem[c], k, c);
    }
}

template <int E, typename H>
__device__ __forceinline__ void tile_stage_out(const uint4 *row, uint4 *mem, uint32_t wave_chunks, uint32_t lane, H hook)
{
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint32_t c = k * 64 + lane;
        if (c < wave_chunks)
            mem[c] = hook(row[planes_lds_slot<E>(c)], k, c);
    }
}

// Lane get / put: the lane's E chunks of the wave's LDS row.
template <int E>
__device__ __forceinline__ void tile_get(const uint4 *row, uint32_t lane, uint32_t (&v)[4 * E])
{
#pragma unroll
    for (int k = 0; k < E; k++) {
        const uint4 x = row[planes_lds_slot<E>(lane * E + k)];
        v[4 * k] = x.x; v[4 * k + 1] = x.y; v[4 * k + 2] = x.z; v[4 * k + 3] = x.w;
    }
}

template <int E>
__device__ __forceinline__ void tile_put(uint4 *row, uint32_t lane, const uint32_t (&v)[4 * E])
{
#pragma unroll
    for (int k = 0; k < E; k++)
        row[planes_lds_slot<E>(lane * E + k)] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}

// Plane load / store: group i of a frame at fbase, the 16 bytes at fbase + p*block_size + i*16 of every plane p.
template <int E>
__device__ __forceinline__ void plane_load(const uint8_t *fbase, uint32_t block_size, uint64_t i, uint32_t (&v)[4 * E])
{
#pragma unroll
    for (int p = 0; p < E; p++) {
        const uint4 x = *(const uint4 *)(fbase + (uint64_t)p * block_size + i * 16);
        v[4 * p] = x.x; v[4 * p + 1] = x.y; v[4 * p + 2] = x.z; v[4 * p + 3] = x.w;
    }
}

template <int E>
__device__ __forceinline__ void plane_store(uint8_t *fbase, uint32_t block_size, uint64_t i, const uint32_t (&v)[4 * E])
{
#pragma unroll
    for (int p = 0; p < E; p++)
        *(uint4 *)(fbase + (uint64_t)p * block_size + i * 16) = make_uint4(v[4 * p], v[4 * p + 1], v[4 * p + 2], v[4 * p + 3]);
}

// What a filter on the elements does in the forward tile: `before` runs ahead of the barrier and its result crosses it,
// `apply` works on the lane's 16 elements in front of the permutation.  This one is no filter; DeltaForward
// (redux_delta.hpp), with or without the fold, is the other.
template <int E>
struct PlainForward {
    struct Pred {};
    __device__ __forceinline__ static Pred before(const uint8_t *, uint64_t, bool, uint32_t) { return Pred(); }
    __device__ __forceinline__ static void apply(const uint4 *, uint32_t, bool, Pred, uint32_t (&)[4 * E]) {}
};

// The forward tile: R rows of 256 groups, groups t0 + 256*r + threadIdx.x of `groups` (src, dst: group 0's frame), under
// one pair of barriers; the caller puts the second one where another tile follows.  Every thread of the workgroup calls it.
// lds: 4 waves x R rows x 64*E chunks.  I: what holds a group index (64 bits over a whole buffer).
template <int E, typename F, int R, typename I, typename H>
__device__ __forceinline__ void tile_forward(const uint8_t *src, uint8_t *dst, I groups, I t0, uint32_t frame_groups, uint32_t block_size,
                                             uint4 *lds, H hook)
{
    const uint32_t lane = threadIdx.x & 63;
    uint4         *wl   = lds + (threadIdx.x >> 6) * 64 * E * R;
    typename F::Pred pred[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const I g = t0 + r * 256 + threadIdx.x, g0 = g - lane;
        pred[r] = F::before(src, g, g < groups && g % frame_groups != 0, lane); // (!= 0: the bytes before are the frame's)
        tile_stage_in<E>(wl + r * 64 * E, (const uint4 *)(src + (uint64_t)g0 * 16 * E), tile_wave_chunks<E, I>(groups, g0), lane, hook);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; r++) {
        const I g = t0 + r * 256 + threadIdx.x;
        if (g < groups) {
            const I f = g / frame_groups, i = g - f * frame_groups;
            uint32_t in[4 * E], out[4 * E];
            tile_get<E>(wl + r * 64 * E, lane, in);
            F::apply(wl + r * 64 * E, lane, i != 0, pred[r], in);
            planes_permute<E, false>(in, out);
            plane_store<E>(dst + (uint64_t)f * E * block_size, block_size, i, out);
        }
    }
}

// The plain inverse tile: one row of 256 groups, groups t0 + threadIdx.x of `groups`; barriers and lds as above (R = 1).
template <int E, typename I, typename H>
__device__ __forceinline__ void tile_inverse(const uint8_t *src, uint8_t *dst, I groups, I t0, uint32_t frame_groups, uint32_t block_size,
                                             uint4 *lds, H hook)
{
    const uint32_t lane = threadIdx.x & 63;
    uint4         *wl   = lds + (threadIdx.x >> 6) * 64 * E;
    const I        g = t0 + threadIdx.x, g0 = g - lane;
    if (g < groups) {
        const I f = g / frame_groups, i = g - f * frame_groups;
        uint32_t in[4 * E], out[4 * E];
        plane_load<E>(src + (uint64_t)f * E * block_size, block_size, i, in);
        planes_permute<E, true>(in, out);
        tile_put<E>(wl, lane, out);
    }
    __syncthreads();
    tile_stage_out<E>(wl, (uint4 *)(dst + (uint64_t)g0 * 16 * E), tile_wave_chunks<E, I>(groups, g0), lane, hook);
}

template <int E, bool INVERSE>
__global__ void __launch_bounds__(256) k_planes(PlanesArgs a)
{
    __shared__ uint4 lds[4 * 64 * E];
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x;
    if (INVERSE)
        tile_inverse<E>(a.src, a.dst, a.groups, t0, a.frame_groups, a.block_size, lds, TileNoHook());
    else
        tile_forward<E, PlainForward<E>, 1>(a.src, a.dst, a.groups, t0, a.frame_groups, a.block_size, lds, TileNoHook());
}

// ---- the byte path -----------------------------------------------------------------------------------------------------
// Byte o of a buffer of len bytes in its frame (E: a constant where the kernel has one): the frame's first byte, o's offset
// in it, the frame's elements.
struct FramePos {
    uint64_t base, r, n;
};

__device__ __forceinline__ FramePos frame_pos(uint64_t o, uint64_t len, uint32_t E, uint32_t block_size)
{
    const uint64_t frame = (uint64_t)E * block_size;
    FramePos p;
    p.base = o / frame * frame;
    p.r    = o - p.base;
    p.n    = (len - p.base < frame ? len - p.base : frame) / E;
    return p;
}

// The frame index rule: the offset in its frame that destination offset p.r is read from.
template <bool INVERSE>
__device__ __forceinline__ uint64_t frame_src(const FramePos &p, uint32_t E)
{
    if (p.r >= p.n * E) // trailing bytes: in place
        return p.r;
    return INVERSE ? (p.r % E) * p.n + p.r / E  // interleaved byte r = byte r%E of element r/E <- plane r%E
                   : (p.r % p.n) * E + p.r / p.n; // plane r/n, element r%n <- byte r/n of element r%n
}

// Forward with or without the differences, for the thread of source byte o: the thread of an element's first byte does
// the element, the threads of a frame's trailing bytes copy them.  fold (with delta): the zigzag fold of the difference
// (redux_zigzag.hpp).
__device__ __forceinline__ void bytes_forward(const uint8_t *src, uint8_t *dst, uint64_t o, uint64_t len, uint32_t E, uint32_t block_size,
                                              bool delta, bool fold = false)
{
    const FramePos f = frame_pos(o, len, E, block_size);
    if (f.r >= f.n * E) {
        dst[o] = src[o];
        return;
    }
    if (f.r % E)
        return;
    const uint64_t i = f.r / E;
    uint64_t x = 0, p = 0;
    for (uint32_t q = 0; q < E; q++) {
        x |= (uint64_t)src[o + q] << (8 * q);
        if (delta && i)
            p |= (uint64_t)src[o - E + q] << (8 * q);
    }
    uint64_t d = x - p;
    if (fold) // (the bits above the element's 8*E are dropped below)
        d = d << 1 ^ (0 - (d >> (8 * E - 1) & 1));
    for (uint32_t q = 0; q < E; q++)
        dst[f.base + (uint64_t)q * f.n + i] = (uint8_t)(d >> (8 * q));
}

// Destination bytes [first, len) of the whole buffer, one per thread: any alignment, any block size.
template <int E, bool INVERSE>
__global__ void __launch_bounds__(256) k_planes_bytes(PlanesArgs a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
        const FramePos f = frame_pos(o, a.len, E, a.block_size);
        a.dst[o] = a.src[f.base + frame_src<INVERSE>(f, E)];
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
