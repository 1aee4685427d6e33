// redux_stride_host.hpp -- the host side of the snapshot-stride filter (redux_stride.hpp): the argument check, the shape of
// the inverse's second stage (columns, time segments, workspace) and the container's stride record.  Plain C++ with no device
// code and no runtime call, so that a stand-alone program can run it under a sanitizer (tests/cpp/stride_plan_test.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace redux {

// redux_stride_check's rule: element size 1, 2, 4 or 8 and a stride of at least one element
inline bool stride_args_ok(uint32_t element_size, uint64_t stride)
{
    return (element_size == 1 || element_size == 2 || element_size == 4 || element_size == 8) && stride >= 1;
}

// Threads the second stage wants in flight before it stops cutting time into segments, and the fewest snapshots a segment
// holds.  Constants, not properties of a device: the workspace size must not depend on where the call runs.
constexpr uint64_t kStrideThreads  = 1ull << 18;
constexpr uint64_t kStrideMinSteps = 32;

// The second stage of the inverse over n = len / E elements: x[i] = unfold(z[i]) + x[i - S] for i >= S, in place.
//   chunks = true:  a column is a 16-byte chunk of the S*E bytes of a snapshot (S*E and the pointer 16-byte multiples); the
//                   chunk kernels take bytes [0, head) and the tail kernel the fewer than 16 / E elements behind them
//   chunks = false: a column is one element
// A thread owns one column of one time segment: `cols` columns, `rows` snapshots, `segs` segments of `steps` snapshots.
// segs > 1: the totals of every (segment, column) go to the workspace (item_bytes each), are scanned over the segments, and
// the walk starts from them, so no thread's chain is longer than `steps` and the scan's is segs / 256.
struct StridePlan {
    bool     run;    // false: S >= n, nothing to add
    bool     chunks;
    uint64_t n, cols, rows, segs, steps, head;
    uint64_t item_bytes, ws_bytes;
};

inline StridePlan stride_plan(uint64_t len, uint32_t E, uint64_t S, bool aligned16)
{
    StridePlan p = {false, false, 0, 0, 0, 1, 0, 0, 0, 0};
    if (!stride_args_ok(E, S))
        return p;
    p.n = len / E;
    if (S >= p.n)
        return p;
    p.run = true;
    const uint64_t row_bytes = S * E; // (S < n <= 2^64 / E: no overflow)
    p.chunks = aligned16 && row_bytes % 16 == 0;
    if (p.chunks) {
        p.head       = p.n * E / 16 * 16;
        p.cols       = row_bytes / 16;
        p.rows       = p.head / row_bytes + (p.head % row_bytes ? 1 : 0);
        p.item_bytes = 16;
    } else {
        p.head       = p.n * E;
        p.cols       = S;
        p.rows       = p.n / S + (p.n % S ? 1 : 0);
        p.item_bytes = 8;
    }
    if (p.rows < 2) { // (the chunk form's head can end inside the first snapshot)
        p.segs  = 1;
        p.steps = p.rows;
        return p;
    }
    uint64_t segs = p.cols >= kStrideThreads ? 1 : kStrideThreads / p.cols;
    if (segs > p.rows / kStrideMinSteps)
        segs = p.rows / kStrideMinSteps;
    if (segs < 2)
        segs = 1;
    p.steps = p.rows / segs + (p.rows % segs ? 1 : 0);
    p.segs  = p.rows / p.steps + (p.rows % p.steps ? 1 : 0);
    if (p.segs > 1) // (by the count before the rounding, which never falls as len grows; segs * cols <= kStrideThreads)
        p.ws_bytes = segs * p.cols * p.item_bytes;
    return p;
}

// room for either form: the caller of the size does not say how its pointers are aligned
inline uint64_t stride_workspace_bytes(uint64_t len, uint32_t E, uint64_t S)
{
    const uint64_t a = stride_plan(len, E, S, true).ws_bytes, b = stride_plan(len, E, S, false).ws_bytes;
    const uint64_t m = a > b ? a : b;
    return m ? (m + 16 + 255) / 256 * 256 : 0; // (16: the items are aligned inside whatever the caller hands over)
}

// ---- the container's record (redux_amd/container.py, version 15 kind 2) -------------------------------------------------
// The kind-2 word is 0xF0000000 | 2 << 24 | E with every other bit zero; the stride follows the header as a little-endian
// u64.  0 = fine, 1 = malformed (InvalidInput), 2 = the record is cut short (Eof).
constexpr uint32_t kStrideWordBase = 0xF2000000u;

inline uint32_t stride_record_word(uint32_t E) { return kStrideWordBase | E; }

inline void stride_record_pack(uint64_t S, uint8_t out[8])
{
    for (int q = 0; q < 8; q++)
        out[q] = (uint8_t)(S >> (8 * q));
}

inline int stride_record_parse(uint32_t word, const uint8_t *rec, size_t avail, uint32_t *E, uint64_t *S)
{
    if ((word & 0xFFFFFFF0u) != kStrideWordBase || !stride_args_ok(word & 15, 1))
        return 1;
    if (!rec || avail < 8)
        return 2;
    uint64_t s = 0;
    for (int q = 0; q < 8; q++)
        s |= (uint64_t)rec[q] << (8 * q);
    if (s == 0)
        return 1;
    *E = word & 15;
    *S = s;
    return 0;
}

} // namespace redux
