// redux_range.hpp -- range reads: the plan of the granules a set of byte ranges covers, and the segmented byte copy that
// gathers covered streams and scatters requested bytes (gfx950 only).
//
// The rule (include/redux_hip.h, "range reads"): granule j of an input of total bytes in blocks of B is blocks
// [j g, min((j + 1) g, nblocks)), bytes [j g B, min((j + 1) g B, total)).  The union of the granules a set of ranges covers,
// as ascending disjoint runs, concatenated, is the virtual input: a valid smaller input of every decode entry point.
//
//   range_plan       host: ranges -> runs, the virtual input's length, each range's place in it (no device call)
//   segment_tiles    host: segments (src, dst, len) -> tiles of at most 64 KiB that never straddle a segment; every tile but a
//                    segment's first starts at a 16-byte boundary of the destination
//   k_segment_copy   a workgroup per tile, grid-stride: head and tail of at most 15 bytes bytewise, the body in 16-byte stores
//                    to aligned addresses.  The source of a body chunk sits at any of 16 phases against it: phase 0 is a plain
//                    uint4 copy; the others load the two ALIGNED 16-byte chunks that hold the 16 source bytes and shift them
//                    together with v_alignbyte_b32 (phase / 4 picks the dwords, a wave-uniform choice made outside the loop;
//                    phase % 4 is the byte shift).  Both aligned chunks hold at least one byte of the tile's source, so nothing
//                    is read from a 16-byte chunk that holds no source byte.  No LDS, no atomics.
//
// Included by redux_hip.hip (one translation unit), after redux_mixed.hpp.
#pragma once

#include "../../include/redux_hip.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace redux {

constexpr uint64_t kSegmentTile = 65536; // bytes of a tile at most

// ======================================================================================
// host: the plan
// ======================================================================================
// bytes of a granule: g B, saturated (a granule that long is the whole input)
static inline uint64_t granule_bytes(uint32_t block_size, uint64_t g)
{
    return g > UINT64_MAX / block_size ? UINT64_MAX : g * block_size;
}

// where granule j begins, for j <= total / gb + 1, clipped to the input
static inline uint64_t granule_start(uint64_t j, uint64_t gb, uint64_t total)
{
    return j > total / gb ? total : j * gb;
}

static int range_plan(uint64_t total, uint32_t block_size, uint64_t g, const uint64_t *starts, const uint64_t *lens, uint64_t n,
                      uint64_t *run_first, uint64_t *run_count, uint64_t *nruns, uint64_t *virt_off, uint64_t *virt_len)
{
    if (block_size == 0 || g == 0 || !nruns || !virt_len || (n && (!starts || !lens || !run_first || !run_count || !virt_off)))
        return REDUX_INVALID_INPUT;
    for (uint64_t i = 0; i < n; i++)
        if (starts[i] > total || lens[i] > total - starts[i]) // (no sum: it cannot overflow)
            return REDUX_INVALID_INPUT;
    const uint64_t gb = granule_bytes(block_size, g);
    std::vector<std::pair<uint64_t, uint64_t>> iv; // [first, last] granule of every range with bytes
    iv.reserve(n);
    for (uint64_t i = 0; i < n; i++)
        if (lens[i])
            iv.push_back({starts[i] / gb, (starts[i] + lens[i] - 1) / gb});
    std::sort(iv.begin(), iv.end());
    uint64_t r = 0;
    for (const auto &v : iv) {
        if (r && v.first <= run_first[r - 1] + run_count[r - 1]) { // overlaps or touches the run before
            if (v.second + 1 > run_first[r - 1] + run_count[r - 1])
                run_count[r - 1] = v.second + 1 - run_first[r - 1];
        } else {
            run_first[r] = v.first;
            run_count[r] = v.second - v.first + 1;
            r++;
        }
    }
    std::vector<uint64_t> at(r + 1, 0); // where each run begins in the virtual input
    for (uint64_t k = 0; k < r; k++)
        at[k + 1] = at[k] + granule_start(run_first[k] + run_count[k], gb, total) - granule_start(run_first[k], gb, total);
    for (uint64_t i = 0; i < n; i++) {
        virt_off[i] = 0;
        if (lens[i] == 0)
            continue;
        const uint64_t j = starts[i] / gb;
        const uint64_t k = (uint64_t)(std::upper_bound(run_first, run_first + r, j) - run_first) - 1; // the run that holds granule j
        virt_off[i]      = at[k] + starts[i] - granule_start(run_first[k], gb, total);
    }
    *nruns    = r;
    *virt_len = at[r];
    return REDUX_OK;
}

// ======================================================================================
// host: the tiles
// ======================================================================================
// tiles of the segments in order; `tiles` may be null (the count alone).  A segment without bytes has no tile.
static uint64_t segment_tiles(const redux_segment *segs, uint64_t nsegs, redux_segment *tiles)
{
    uint64_t n = 0;
    for (uint64_t i = 0; i < nsegs; i++) {
        uint64_t src = segs[i].src, dst = segs[i].dst, left = segs[i].len;
        // the first tile ends at the last 16-byte boundary of the destination it can reach, the others are whole
        uint64_t len = left <= kSegmentTile ? left : kSegmentTile - (dst & 15);
        while (left) {
            if (tiles)
                tiles[n] = redux_segment{src, dst, len};
            n++;
            src += len;
            dst += len;
            left -= len;
            len = left < kSegmentTile ? left : kSegmentTile;
        }
    }
    return n;
}

// what redux_segment_copy_dev refuses before any device call: a segment outside its buffer (overflow included), destination
// segments that overlap each other, buffers that overlap
static int segment_table_check(const void *d_src, uint64_t src_bytes, const void *d_dst, uint64_t dst_bytes, const redux_segment *segs,
                               uint64_t nsegs)
{
    if (nsegs && !segs)
        return REDUX_INVALID_INPUT;
    std::vector<std::pair<uint64_t, uint64_t>> d; // (dst, len) of the segments with bytes
    d.reserve(nsegs);
    for (uint64_t i = 0; i < nsegs; i++) {
        const redux_segment &s = segs[i];
        if (s.src > src_bytes || s.len > src_bytes - s.src || s.dst > dst_bytes || s.len > dst_bytes - s.dst)
            return REDUX_INVALID_INPUT;
        if (s.len)
            d.push_back({s.dst, s.len});
    }
    std::sort(d.begin(), d.end());
    for (size_t i = 1; i < d.size(); i++)
        if (d[i - 1].first + d[i - 1].second > d[i].first)
            return REDUX_INVALID_INPUT;
    if (d.empty())
        return REDUX_OK;
    if (!d_src || !d_dst)
        return REDUX_INVALID_INPUT;
    const uintptr_t s0 = (uintptr_t)d_src, d0 = (uintptr_t)d_dst;
    if (src_bytes > UINTPTR_MAX - s0 || dst_bytes > UINTPTR_MAX - d0 || (s0 < d0 + dst_bytes && d0 < s0 + src_bytes))
        return REDUX_INVALID_INPUT;
    return REDUX_OK;
}

// ======================================================================================
// device: the copy
// ======================================================================================
struct SegmentCopyArgs {
    const uint8_t       *src;
    uint8_t             *dst;
    const redux_segment *tiles; // byte offsets into src / dst, len <= kSegmentTile
    uint64_t             ntiles;
};

constexpr uint32_t kSegmentThreads = 256;
constexpr uint32_t kSegmentUnroll  = 4; // 16-byte chunks a lane has in flight

// 16 bytes from byte 4 W + shift of the 32 bytes (lo, hi), shift 0 .. 3
template <int W>
__device__ __forceinline__ uint4 shifted_chunk(const uint4 lo, const uint4 hi, const uint32_t shift)
{
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    return make_uint4(__builtin_amdgcn_alignbyte(w[W + 1], w[W], shift), __builtin_amdgcn_alignbyte(w[W + 2], w[W + 1], shift),
                      __builtin_amdgcn_alignbyte(w[W + 3], w[W + 2], shift), __builtin_amdgcn_alignbyte(w[W + 4], w[W + 3], shift));
}

// the body of a tile whose source is `phase` bytes, 1 .. 15, past the 16-byte boundary s16: d16[i] = bytes
// [16 i + phase, 16 i + phase + 16) of s16.  Chunk i + 1 of s16 holds byte 16 i + phase + 15 of it: a source byte.
#ifdef REDUX_SEGMENT_UNALIGNED_LOADS
// The form that was measured against it (tools/measure_range.py under a library built with this macro; DESIGN.md 6o: 1.5
// times slower at relative phases 1, 4 and 8): one 16-byte load per chunk at the source's own alignment, which the hardware
// splits.
template <int W>
__device__ __forceinline__ void shifted_body(uint4 *d16, const uint4 *s16, const uint32_t nchunks, const uint32_t shift, const uint32_t tid)
{
    const uint8_t *s = reinterpret_cast<const uint8_t *>(s16) + 4 * W + shift;
    for (uint32_t base = 0; base < nchunks; base += kSegmentThreads * kSegmentUnroll) {
        uint4 q[kSegmentUnroll];
#pragma unroll
        for (uint32_t k = 0; k < kSegmentUnroll; k++) {
            const uint32_t i = base + kSegmentThreads * k + tid;
            if (i < nchunks)
                __builtin_memcpy(&q[k], s + 16 * (uint64_t)i, 16);
        }
#pragma unroll
        for (uint32_t k = 0; k < kSegmentUnroll; k++) {
            const uint32_t i = base + kSegmentThreads * k + tid;
            if (i < nchunks)
                d16[i] = q[k];
        }
    }
}
#else
template <int W>
__device__ __forceinline__ void shifted_body(uint4 *d16, const uint4 *s16, const uint32_t nchunks, const uint32_t shift, const uint32_t tid)
{
    for (uint32_t base = 0; base < nchunks; base += kSegmentThreads * kSegmentUnroll) {
        uint4 lo[kSegmentUnroll], hi[kSegmentUnroll];
#pragma unroll
        for (uint32_t k = 0; k < kSegmentUnroll; k++) {
            const uint32_t i = base + kSegmentThreads * k + tid;
            if (i < nchunks) {
                lo[k] = s16[i];
                hi[k] = s16[i + 1];
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kSegmentUnroll; k++) {
            const uint32_t i = base + kSegmentThreads * k + tid;
            if (i < nchunks)
                d16[i] = shifted_chunk<W>(lo[k], hi[k], shift);
        }
    }
}
#endif

__global__ void __launch_bounds__(kSegmentThreads) k_segment_copy(SegmentCopyArgs a)
{
    const uint32_t tid = threadIdx.x;
    for (uint64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const redux_segment T   = a.tiles[t];
        const uint8_t      *s   = a.src + T.src;
        uint8_t            *d   = a.dst + T.dst;
        const uint32_t      len = (uint32_t)T.len;
        uint32_t            head = (uint32_t)((16 - ((uintptr_t)d & 15)) & 15);
        if (head > len)
            head = len;
        if (tid < head)
            d[tid] = s[tid];
        const uint32_t nchunks = (len - head) >> 4;
        uint4         *d16     = reinterpret_cast<uint4 *>(d + head);
        const uint32_t phase   = (uint32_t)((uintptr_t)(s + head) & 15);
        const uint4   *s16     = reinterpret_cast<const uint4 *>(s + head - phase);
        if (phase == 0) {
            for (uint32_t base = 0; base < nchunks; base += kSegmentThreads * kSegmentUnroll) {
                uint4 q[kSegmentUnroll];
#pragma unroll
                for (uint32_t k = 0; k < kSegmentUnroll; k++) {
                    const uint32_t i = base + kSegmentThreads * k + tid;
                    if (i < nchunks)
                        q[k] = s16[i];
                }
#pragma unroll
                for (uint32_t k = 0; k < kSegmentUnroll; k++) {
                    const uint32_t i = base + kSegmentThreads * k + tid;
                    if (i < nchunks)
                        d16[i] = q[k];
                }
            }
        } else {
            switch (phase >> 2) { // (uniform over the workgroup)
            case 0: shifted_body<0>(d16, s16, nchunks, phase & 3, tid); break;
            case 1: shifted_body<1>(d16, s16, nchunks, phase & 3, tid); break;
            case 2: shifted_body<2>(d16, s16, nchunks, phase & 3, tid); break;
            default: shifted_body<3>(d16, s16, nchunks, phase & 3, tid); break;
            }
        }
        const uint32_t done = head + (nchunks << 4);
        if (tid < len - done)
            d[done + tid] = s[done + tid];
    }
}

} // namespace redux
