// redux_stride.hpp -- the snapshot-stride filter for time series of fields: one buffer of T snapshots of the same S elements
// (a trajectory [frame, atom, xyz], a field [time, lat, lon], a stack of sensor frames), each element predicted by the same
// element one snapshot back.  The folded difference of redux_base_sub.hpp with the second operand taken from the source
// itself, S elements back, fused with the byte-plane layout (redux_planes.hpp).
//
//   k_stride_planes<E>         forward, full frames: the forward tile with the stage-in hook subtracting the chunk S*E bytes
//                              back and folding the 16 / E differences in registers; E = 1: a 16-byte stream kernel, no LDS.
//                              S*E need be no 16-byte multiple: the chunk S*E bytes back is then put together from the two
//                              aligned chunks it lies in
//   k_stride_planes_bytes<E>   forward, one element per thread under the frame index rule, any alignment and block size: the
//                              short last frame, and everything when a pointer or the block size is no 16-byte multiple
//   k_stride_sum<E, FORM>      inverse, stage two, in place on the destination behind the inverse of the layout (k_planes):
//                              a thread owns one column of one time segment and walks its snapshots with the carry in
//                              registers.  FORM 0: a column is a 16-byte chunk (S*E and the pointer 16-byte multiples), the
//                              wave's accesses contiguous; FORM 1: one element, E-byte accesses; FORM 2: one element, bytes
//   k_stride_totals<E, FORM>   where the columns alone leave the machine idle (small S), time is cut into segments
//   k_stride_scan<E, FORM>     (redux_stride_host.hpp, stride_plan): the totals of every (segment, column) go to the
//                              workspace, a workgroup per column scans them over the segments, and k_stride_sum starts from
//                              them.  No chain is longer than a segment's snapshots
//   k_stride_sum_tail<E>       the fewer than 16 / E elements behind FORM 0's last whole chunk
//
// Rule (E = element size, B = block size, S >= 1 the stride in elements, x the input of len bytes, n = len / E whole
// little-endian elements counted from byte 0 of the WHOLE buffer, not per frame): z[i] = x[i] for i < S;
// z[i] = fold(x[i] - x[i - S] mod 2^(8E)) for S <= i < n, the fold of redux_zigzag.hpp; the len - n*E trailing bytes stay.
// The byte-plane layout of E is applied to z (none for E = 1).  S >= n is the layout alone.  The inverse undoes the layout,
// then x[i] = unfold(z[i]) + x[i - S] for i from S upward.  The predecessor lies outside the frame: nothing here is local to
// a frame, and the inverse of a block needs every block before it in its columns.
//
// Traffic: forward, one read from memory, one more S*E bytes back (from cache where a snapshot fits it), one write; inverse,
// the layout's read and write, then one read and one write in place, and one read more where time is cut into segments.
//
// All index arithmetic is 64-bit.  Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_base_sub.hpp"
#include "redux_stride_host.hpp"

#include <type_traits>

namespace redux {

struct StrideArgs {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       groups;       // fused kernel: full frames * frame_groups, 16-element groups
    uint32_t       frame_groups; // block_size / 16
    uint32_t       block_size;
    uint64_t       first, len;   // byte kernel: source bytes [first, len) of the whole buffer
    uint64_t       S;            // the stride in elements
    uint64_t       D;            // S*E bytes; ~0 where S >= n (nothing is folded)
};

// bytes [r, r + 16) of the 32 bytes lo : hi, 0 < r < 16 and r a multiple of E (the same for every thread)
template <int E>
__device__ __forceinline__ uint4 stride_bytes_at(uint4 lo, uint4 hi, uint32_t r)
{
    uint32_t a0, a1, a2, a3, a4;
    switch (r >> 2) {
    case 0:  a0 = lo.x; a1 = lo.y; a2 = lo.z; a3 = lo.w; a4 = hi.x; break;
    case 1:  a0 = lo.y; a1 = lo.z; a2 = lo.w; a3 = hi.x; a4 = hi.y; break;
    case 2:  a0 = lo.z; a1 = lo.w; a2 = hi.x; a3 = hi.y; a4 = hi.z; break;
    default: a0 = lo.w; a1 = hi.x; a2 = hi.y; a3 = hi.z; a4 = hi.w; break;
    }
    if constexpr (E >= 4) {
        return make_uint4(a0, a1, a2, a3);
    } else {
        const uint32_t bs = (r & 3) * 8;
        return make_uint4((uint32_t)(((uint64_t)a1 << 32 | a0) >> bs), (uint32_t)(((uint64_t)a2 << 32 | a1) >> bs),
                          (uint32_t)(((uint64_t)a3 << 32 | a2) >> bs), (uint32_t)(((uint64_t)a4 << 32 | a3) >> bs));
    }
}

// the first `keep` bytes (0 < keep < 16) of x, the rest of z
__device__ __forceinline__ uint32_t stride_keep_dword(uint32_t x, uint32_t z, uint32_t keep, uint32_t at)
{
    const uint32_t k = keep > at ? keep - at : 0;
    const uint32_t m = k >= 4 ? ~0u : (1u << (8 * k)) - 1;
    return (x & m) | (z & ~m);
}

__device__ __forceinline__ uint4 stride_keep(uint4 x, uint4 z, uint32_t keep)
{
    return make_uint4(stride_keep_dword(x.x, z.x, keep, 0), stride_keep_dword(x.y, z.y, keep, 4), stride_keep_dword(x.z, z.z, keep, 8),
                      stride_keep_dword(x.w, z.w, keep, 12));
}

// The chunk x at byte `off` (a 16-byte multiple) of src, a 16-byte multiple itself: its elements at or behind byte D folded
// against the elements D bytes back.  No byte before src is read: where the chunk D bytes back begins before src (the chunk the
// boundary falls into), that part is not loaded, and the elements it would predict pass unfolded.
template <int E>
__device__ __forceinline__ uint4 stride_fold_chunk(const uint8_t *src, uint64_t off, uint64_t D, uint4 x)
{
    if (off + 16 <= D) // (D = ~0: never folded)
        return x;
    const int64_t  p = (int64_t)(off - D); // > -16
    const uint32_t r = (uint32_t)p & 15;
    uint4 y;
    if (r == 0) { // (then D is a 16-byte multiple and p >= 0)
        y = *(const uint4 *)(src + p);
    } else {
        const int64_t A  = p - (int64_t)r; // >= -16; A + 16 <= off: the second chunk is at most x's own
        const uint4   lo = A >= 0 ? *(const uint4 *)(src + A) : make_uint4(0, 0, 0, 0);
        const uint4   hi = *(const uint4 *)(src + A + 16);
        y = stride_bytes_at<E>(lo, hi, r);
    }
    const uint4 z = base_sub_fold<E>(x, y);
    return off < D ? stride_keep(x, z, (uint32_t)(D - off)) : z;
}

// Forward, full frames.  The wave's 1024*E contiguous bytes are loaded with coalesced 16-byte accesses and meet the bytes
// D back on the way into LDS.
template <int E>
__global__ void __launch_bounds__(256) k_stride_planes(StrideArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (E == 1) { // no layout: group g is 16 bytes of the stream
        if (g < a.groups)
            ((uint4 *)a.dst)[g] = stride_fold_chunk<1>(a.src, g * 16, a.D, ((const uint4 *)a.src)[g]);
    } else {
        __shared__ uint4 lds[4 * 64 * E];
        const uint8_t *src = a.src;
        const uint64_t w0 = (g - (threadIdx.x & 63)) * 16 * E, D = a.D; // the wave's first byte
        tile_forward<E, PlainForward<E>, 1>(a.src, a.dst, a.groups, (uint64_t)blockIdx.x * blockDim.x, a.frame_groups, a.block_size, lds,
                                            [src, w0, D](uint4 v, int, uint32_t c) { return stride_fold_chunk<E>(src, w0 + (uint64_t)c * 16, D, v); });
    }
}

// Source bytes [first, len) of the whole buffer, one per thread: the thread of an element's first byte does the element, the
// threads of the trailing bytes copy them.
template <int E>
__global__ void __launch_bounds__(256) k_stride_planes_bytes(StrideArgs a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
        const FramePos f = frame_pos(o, a.len, E, a.block_size);
        if (f.r >= f.n * E) { // trailing bytes: in place
            a.dst[o] = a.src[o];
            continue;
        }
        if (f.r % E)
            continue;
        const uint64_t i = f.r / E, p0 = f.base + i; // the element in its frame, and its byte of plane 0
        const bool     folded = o / E >= a.S;        // (o / E: the element in the whole buffer; frames are whole elements)
        uint64_t v = 0, y = 0;
#pragma unroll
        for (uint32_t q = 0; q < E; q++) {
            v |= (uint64_t)a.src[o + q] << (8 * q);
            if (folded)
                y |= (uint64_t)a.src[o - a.D + q] << (8 * q);
        }
        if (folded) { // (the bits above the element's 8*E are dropped below)
            v -= y;
            v = v << 1 ^ (0 - (v >> (8 * E - 1) & 1));
        }
#pragma unroll
        for (uint32_t q = 0; q < E; q++)
            a.dst[p0 + q * f.n] = (uint8_t)(v >> (8 * q));
    }
}

// ---- the inverse's second stage -----------------------------------------------------------------------------------------
struct StrideSumArgs {
    uint8_t *dst;       // x[0 .. head): z on entry, x on return
    void    *ws;        // segs > 1: segs * cols items
    uint64_t cols, rows, segs, steps;
    uint64_t row_bytes; // S*E
    uint64_t head;      // bytes the columns cover
    uint64_t S, n;      // the tail kernel: elements [head / E, n)
};

// What a column holds in a snapshot: FORM 0 a chunk of 16 / E elements, FORM 1 / 2 one element in the low 8*E bits
template <int FORM> struct StrideItem { typedef uint64_t T; };
template <> struct StrideItem<0> { typedef uint4 T; };

template <int E, int FORM>
__device__ __forceinline__ typename StrideItem<FORM>::T stride_load(const uint8_t *p)
{
    if constexpr (FORM == 0) {
        return *(const uint4 *)p;
    } else if constexpr (FORM == 1) {
        if constexpr (E == 1) return *p;
        else if constexpr (E == 2) return *(const uint16_t *)p;
        else if constexpr (E == 4) return *(const uint32_t *)p;
        else return *(const uint64_t *)p;
    } else {
        uint64_t v = 0;
#pragma unroll
        for (uint32_t q = 0; q < E; q++)
            v |= (uint64_t)p[q] << (8 * q);
        return v;
    }
}

template <int E, int FORM>
__device__ __forceinline__ void stride_store(uint8_t *p, typename StrideItem<FORM>::T v)
{
    if constexpr (FORM == 0) {
        *(uint4 *)p = v;
    } else if constexpr (FORM == 1) {
        if constexpr (E == 1) *p = (uint8_t)v;
        else if constexpr (E == 2) *(uint16_t *)p = (uint16_t)v;
        else if constexpr (E == 4) *(uint32_t *)p = (uint32_t)v;
        else *(uint64_t *)p = v;
    } else {
#pragma unroll
        for (uint32_t q = 0; q < E; q++)
            p[q] = (uint8_t)(v >> (8 * q));
    }
}

template <int FORM>
__device__ __forceinline__ typename StrideItem<FORM>::T stride_zero()
{
    if constexpr (FORM == 0) return make_uint4(0, 0, 0, 0);
    else return 0;
}

// a + b, element by element mod 2^(8E)
template <int E, int FORM>
__device__ __forceinline__ typename StrideItem<FORM>::T stride_add(typename StrideItem<FORM>::T a, typename StrideItem<FORM>::T b)
{
    if constexpr (FORM != 0) {
        return (a + b) & (E == 8 ? ~0ull : (1ull << (8 * (E & 7))) - 1);
    } else if constexpr (E == 8) {
        const uint64_t l = ((uint64_t)a.y << 32 | a.x) + ((uint64_t)b.y << 32 | b.x), h = ((uint64_t)a.w << 32 | a.z) + ((uint64_t)b.w << 32 | b.z);
        return make_uint4((uint32_t)l, (uint32_t)(l >> 32), (uint32_t)h, (uint32_t)(h >> 32));
    } else {
        return make_uint4(delta_add<E>(a.x, b.x), delta_add<E>(a.y, b.y), delta_add<E>(a.z, b.z), delta_add<E>(a.w, b.w));
    }
}

// unfold(z) + carry, element by element
template <int E, int FORM>
__device__ __forceinline__ typename StrideItem<FORM>::T stride_unfold_add(typename StrideItem<FORM>::T z, typename StrideItem<FORM>::T carry)
{
    if constexpr (FORM == 0)
        return base_sub_unfold<E>(z, carry);
    else
        return ((z >> 1 ^ (0 - (z & 1))) + carry) & (E == 8 ? ~0ull : (1ull << (8 * (E & 7))) - 1);
}

// Thread (segment g, column j), j fastest: the snapshots [g * steps, (g + 1) * steps) of the column.  WALK: x = unfold(z) +
// carry written in place, the carry starting at the workspace's entry (the sum of the segments before, from k_stride_scan) or
// at zero; else the segment's total goes to the workspace.  Snapshot 0 is x itself.  The loads of z do not depend on the
// carry: four are in flight ahead of the additions.
template <int E, int FORM, bool WALK>
__device__ __forceinline__ void stride_sum_body(const StrideSumArgs &a)
{
    typedef typename StrideItem<FORM>::T T;
    constexpr uint64_t U = FORM == 0 ? 16 : E;
    T *ws = (T *)a.ws;
    const uint64_t total = a.segs * a.cols;
    for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = id / a.cols, j = id - g * a.cols;
        const uint64_t have = a.head >= (j + 1) * U ? (a.head - (j + 1) * U) / a.row_bytes + 1 : 0; // snapshots that hold column j
        uint64_t       t    = g * a.steps;
        const uint64_t t1   = t + a.steps < have ? t + a.steps : have;
        uint8_t       *col  = a.dst + j * U;
        T carry = WALK && a.segs > 1 ? ws[id] : stride_zero<FORM>();
        if (t == 0 && t < t1) {
            carry = stride_add<E, FORM>(carry, stride_load<E, FORM>(col));
            t = 1;
        }
        for (; t + 4 <= t1; t += 4) {
            uint8_t *p = col + t * a.row_bytes;
            const T z0 = stride_load<E, FORM>(p), z1 = stride_load<E, FORM>(p + a.row_bytes);
            const T z2 = stride_load<E, FORM>(p + 2 * a.row_bytes), z3 = stride_load<E, FORM>(p + 3 * a.row_bytes);
            const T x0 = stride_unfold_add<E, FORM>(z0, carry), x1 = stride_unfold_add<E, FORM>(z1, x0);
            const T x2 = stride_unfold_add<E, FORM>(z2, x1), x3 = stride_unfold_add<E, FORM>(z3, x2);
            if (WALK) {
                stride_store<E, FORM>(p, x0);
                stride_store<E, FORM>(p + a.row_bytes, x1);
                stride_store<E, FORM>(p + 2 * a.row_bytes, x2);
                stride_store<E, FORM>(p + 3 * a.row_bytes, x3);
            }
            carry = x3;
        }
        for (; t < t1; t++) {
            uint8_t *p = col + t * a.row_bytes;
            carry = stride_unfold_add<E, FORM>(stride_load<E, FORM>(p), carry);
            if (WALK)
                stride_store<E, FORM>(p, carry);
        }
        if (!WALK)
            ws[id] = carry;
    }
}

template <int E, int FORM>
__global__ void __launch_bounds__(256) k_stride_totals(StrideSumArgs a)
{
    stride_sum_body<E, FORM, false>(a);
}

template <int E, int FORM>
__global__ void __launch_bounds__(256) k_stride_sum(StrideSumArgs a)
{
    stride_sum_body<E, FORM, true>(a);
}

// The totals of a column over the segments -> the sums of the segments before each: a workgroup per column, a thread per
// run of ceil(segs / 256) segments, the 256 runs' totals scanned in LDS.
template <int E, int FORM>
__global__ void __launch_bounds__(256) k_stride_scan(StrideSumArgs a)
{
    typedef typename StrideItem<FORM>::T T;
    __shared__ T part[256];
    T *ws = (T *)a.ws;
    const uint64_t q = (a.segs + 255) / 256, s0 = threadIdx.x * q, s1 = s0 + q < a.segs ? s0 + q : a.segs;
    for (uint64_t j = blockIdx.x; j < a.cols; j += gridDim.x) {
        T acc = stride_zero<FORM>();
        for (uint64_t s = s0; s < s1; s++)
            acc = stride_add<E, FORM>(acc, ws[s * a.cols + j]);
        part[threadIdx.x] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            T run = stride_zero<FORM>();
            for (int k = 0; k < 256; k++) {
                const T v = part[k];
                part[k]   = run;
                run       = stride_add<E, FORM>(run, v);
            }
        }
        __syncthreads();
        T carry = part[threadIdx.x];
        for (uint64_t s = s0; s < s1; s++) {
            const T v          = ws[s * a.cols + j];
            ws[s * a.cols + j] = carry;
            carry              = stride_add<E, FORM>(carry, v);
        }
        __syncthreads(); // (part is written again for the next column)
    }
}

// elements [head / E, n), fewer than 16 / E of them, behind FORM 0's chunks: one thread, in order
template <int E>
__global__ void __launch_bounds__(64) k_stride_sum_tail(StrideSumArgs a)
{
    if (blockIdx.x || threadIdx.x)
        return;
    for (uint64_t i = a.head / E; i < a.n; i++) {
        if (i < a.S)
            continue;
        uint8_t *p = a.dst + i * E;
        stride_store<E, 2>(p, stride_unfold_add<E, 2>(stride_load<E, 2>(p), stride_load<E, 2>(p - a.row_bytes)));
    }
}

} // namespace redux
