// redux_delta.hpp -- the delta filter for integer series, fused with the byte-plane layout (redux_planes.hpp): a byte
// transform in front of the coder, next to k_planes.
//
//   k_delta_planes<E, FOLD>          forward, full frames: the forward tile (redux_planes.hpp) with DeltaForward in front of
//                                    the permutation: the predecessor rule and one subtraction; one read and one write
//   k_delta_unplanes<E, FOLD>        inverse, full frames: one workgroup per frame, one row of 256 groups per iteration: the
//                                    walk of delta_inverse_walk (which the mixed kernel runs with 8 / E rows) with its own
//                                    prefetch
//   k_delta_planes_bytes<E, FOLD>    the byte path, one element per thread: the short last frame, unaligned buffers, blocks
//   k_delta_unplanes_bytes<E, FOLD>  not a multiple of 16; bytes_forward (redux_planes.hpp), and bytes_inverse_frame with
//                                    one workgroup per frame
//
// FOLD: the zigzag-folded delta filter for signed series (redux_zigzag.hpp: its rule and its reasons): the fold of the
// lane's 16 differences in registers behind the subtraction, the unfold between the permutation and the serial prefix.
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
#include "redux_zigzag.hpp"

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

// The forward predecessor rule, as the forward tile's filter (PlainForward, redux_planes.hpp): a lane's predecessor element
// is the end of the 16-byte chunk before its own in the wave's LDS row; the wave's first lane loads it from memory, ahead of
// the barrier; a group that starts a frame has none (inside = false).  FOLD: the differences are then folded.
template <int E, bool FOLD>
struct DeltaForward {
    typedef typename DeltaSum<E>::T Pred;
    __device__ __forceinline__ static Pred before(const uint8_t *src, uint64_t g, bool inside, uint32_t lane)
    {
        return inside && lane == 0 ? *(const Pred *)(src + g * 16 * E - sizeof(Pred)) : 0;
    }
    __device__ __forceinline__ static void apply(const uint4 *row, uint32_t lane, bool inside, Pred prev, uint32_t (&v)[4 * E])
    {
        if (inside && lane != 0) {
            const uint4 *c = &row[planes_lds_slot<E>(lane * E - 1)];
            if constexpr (E == 8)
                prev = ((const uint64_t *)c)[1];
            else
                prev = ((const uint32_t *)c)[3];
        }
        uint32_t d[4 * E];
        delta_diff<E>(v, prev, d);
#pragma unroll
        for (int q = 0; q < 4 * E; q++)
            v[q] = d[q];
        if constexpr (FOLD)
            zigzag_fold<E>(v);
    }
};

// Forward, full frames: the forward tile with the subtraction (and the fold) in front of the permutation; one read and one
// write.
template <int E, bool FOLD>
__global__ void __launch_bounds__(256) k_delta_planes(PlanesArgs a)
{
    __shared__ uint4 lds[4 * 64 * E];
    tile_forward<E, DeltaForward<E, FOLD>, 1>(a.src, a.dst, a.groups, (uint64_t)blockIdx.x * blockDim.x, a.frame_groups, a.block_size,
                                              lds, TileNoHook());
}

// The frame walk of the inverse: the workgroup walks frames first, first + step, ... below count (src, dst: frame 0), R rows
// of 256 groups per iteration and pair of barriers: the plane loads, planes_permute inverse, a serial prefix over the
// lane's 16 elements in registers, the lane totals scanned across the wave, the wave totals through LDS, a running carry
// along the frame, the interleaved side written through LDS.  The plane loads of the next iteration are issued before this
// one's scan, so the dependency chain along the frame (scan, two barriers) overlaps the memory latency.  The wave totals
// alternate between two LDS rows, so one barrier per iteration orders them.  Row r's running sum starts from the carry
// behind rows 0 .. r - 1: the totals of every row's waves are in LDS after the first barrier.
// lds: 4 waves x R rows x 64*E chunks.
template <int E, int R, typename I>
__device__ __forceinline__ void delta_inverse_walk(const uint8_t *src, uint8_t *dst, uint32_t frame_groups, uint32_t block_size, I first,
                                                   I step, I count, uint4 *lds, typename DeltaSum<E>::T (*wtot)[R][4])
{
    typedef typename DeltaSum<E>::T T;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4 *wl = lds + wave * 64 * E * R;
    uint32_t row = 0;
    for (I f = first; f < count; f += step) {
        const uint64_t fbase = (uint64_t)f * E * block_size;
        T        carry = 0; // the sum of the frame's elements before this iteration
        uint32_t nxt[R][4 * E];
        auto load = [&](uint32_t i0) { // rows i0 / 256 .. of the frame; a lane past the frame's end gets zeros (a total of 0)
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t i = i0 + r * 256 + threadIdx.x;
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    nxt[r][q] = 0;
                if (i < frame_groups)
                    plane_load<E>(src + fbase, block_size, i, nxt[r]);
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
                    tile_put<E>(wl + r * 64 * E, lane, v[r]);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < R; r++) {
                const uint32_t w0 = i0 + r * 256 + threadIdx.x - lane; // the wave's first group of the row
                tile_stage_out<E>(wl + r * 64 * E, (uint4 *)(dst + fbase + (uint64_t)w0 * 16 * E), tile_wave_chunks<E>(frame_groups, w0), lane,
                                  TileNoHook());
            }
        }
    }
}

// Inverse, full frames: workgroup w walks frames w, w + gridDim.x, ..., one row of 256 groups per iteration: the walk above
// with R = 1, written out.  Through delta_inverse_walk<E, 1> the E = 8 instance measured 0.7 % slower (profiles/
// layout_bodies.txt), so this kernel keeps its own loop, whose prefetch is decided per lane and issued ahead of the permutation.
// FOLD: the unfold between the permutation and the prefix.  A lane past the frame's end holds zeros, their unfold is zeros, so
// its total is still 0, which the scan relies on.
template <int E, bool FOLD>
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
            planes_permute<E, true>(in, v); // (lanes past the frame: zeros, a total of 0)
            if constexpr (FOLD)
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
template <int E, bool FOLD>
__global__ void __launch_bounds__(256) k_delta_planes_bytes(PlanesArgs a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x)
        bytes_forward(a.src, a.dst, o, a.len, E, a.block_size, true, FOLD);
}

// The inverse of the byte path: the workgroup walks the frame of L bytes at `base`, 256 elements per iteration, one per
// lane, summed in 64 bits (congruent mod 2^(8E)) by a wave scan and the wave totals in LDS; a plain layout skips the sum.
// E, delta and L are uniform over the workgroup.  The rows of wtot alternate from one barrier to the next, across frames
// too (row), so one barrier per iteration orders them.  fold (with delta): the elements are unfolded first
// (redux_zigzag.hpp), sign-extended to 64 bits, which is congruent too; a lane past the frame's end keeps its 0.
__device__ __forceinline__ void bytes_inverse_frame(const uint8_t *src, uint8_t *dst, uint64_t base, uint64_t L, uint32_t E, bool delta,
                                                    uint64_t (*wtot)[4], uint32_t &row, bool fold = false)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t n = L / E;
    if (n * E + threadIdx.x < L) // (at most E - 1 trailing bytes)
        dst[base + n * E + threadIdx.x] = src[base + n * E + threadIdx.x];
    uint64_t carry = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += 256) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t d = 0;
        if (i < n)
            for (uint32_t q = 0; q < E; q++)
                d |= (uint64_t)src[base + (uint64_t)q * n + i] << (8 * q);
        if (fold)
            d = d >> 1 ^ (0 - (d & 1));
        uint64_t x = d;
        if (delta) {
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
                dst[base + i * E + q] = (uint8_t)(x >> (8 * q));
    }
}

// Inverse, any alignment and block size: workgroup w takes frames w, w + gridDim.x, ... of [first, len).
template <int E, bool FOLD>
__global__ void __launch_bounds__(256) k_delta_unplanes_bytes(PlanesArgs a)
{
    __shared__ uint64_t wtot[2][4];
    const uint64_t frame = (uint64_t)E * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    uint32_t row = 0;
    for (uint64_t fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
        const uint64_t base = a.first + fi * frame;
        bytes_inverse_frame(a.src, a.dst, base, a.len - base < frame ? a.len - base : frame, E, true, wtot, row, FOLD);
    }
}

} // namespace redux
