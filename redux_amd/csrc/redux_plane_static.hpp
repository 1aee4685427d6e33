// redux_plane_static.hpp -- plane-static coding: the static coder with one table per byte plane (gfx950 only).
//
// The rule (include/redux_hip.h, "plane-static coding"): x' is the byte-plane layout of the input for element size E and
// block size B; table t, 0 <= t < E, is the semi-static table of the bytes of all blocks b of x' with b mod E == t, and
// block b is coded under table b mod E by the static coder of redux_static.hpp.
//
//   k_plane_hist   counts x' into u64[E][256] (added to).  k_byte_hist's design (per-lane packed u16 counters in LDS, folded
//                  before 65,536, one global u64 atomic per nonzero bin); a workgroup is bound to one t and walks the blocks
//                  t, t + E, t + 2E, ... as contiguous B-byte runs
//
// The coders are those of redux_segment_static.hpp with a single segment (SegmentTables::k == 0); what they share with this
// file is the description of the tables and their device-side check.  The tables are read from device memory (u32[E][258]:
// eight tables are 8,256 bytes, more than a kernel's arguments should carry) and are checked by the workgroup that loads
// them: a table that is not strictly increasing from 0 to the launch's total makes every block of that workgroup
// INVALID_INPUT, so a table no host code has seen cannot break the coder's invariants.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_hist.hpp"
#include "redux_static.hpp"

namespace redux {

// ---- per-plane histogram ---------------------------------------------------------------------------------------------
struct PlaneHistArgs {
    const uint8_t      *in;     // x'
    uint64_t            in_len;
    uint64_t            nfull;  // full blocks: in_len / block_size
    uint32_t            block_size;
    uint32_t            E;
    uint32_t            wgs;    // workgroups per table: the grid is E * wgs, workgroup g serves t = g % E as number g / E
    uint32_t            vec;    // in and block_size are 16-byte multiples: full blocks are read as 16-byte vectors
    uint32_t            vshift; // log2(block_size / 16) if that is a power of two, else 0xFFFFFFFF
    unsigned long long *counts; // u64[E][256]
};

constexpr uint32_t kHistLaneMax = 65535; // what one packed u16 counter holds

// n bytes at p, lane-strided; `since` = the most any counter of a lane can have gained since the last flush
__device__ __forceinline__ void hist_run_bytes(uint32_t *lds, uint32_t lane, unsigned long long (&acc)[4], uint32_t &since,
                                               const uint8_t *p, uint64_t n)
{
    constexpr uint64_t kPiece = 64ull * 32768; // 32,768 bytes per lane
    for (uint64_t o = 0; o < n; o += kPiece) { // (wave-uniform: the flush reads other lanes' counters)
        const uint64_t m   = n - o < kPiece ? n - o : kPiece;
        const uint32_t per = (uint32_t)((m + 63) / 64);
        if (since + per > kHistLaneMax) {
            hist_flush(lds, lane, acc);
            since = 0;
        }
        for (uint64_t i = lane; i < m; i += 64)
            hist_byte(lds + lane, p[o + i]);
        since += per;
    }
}

__global__ void __launch_bounds__(64) k_plane_hist(PlaneHistArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const uint32_t t = blockIdx.x % a.E, k = blockIdx.x / a.E;
    const uint64_t B = a.block_size;
    unsigned long long acc[4] = {0, 0, 0, 0};
    uint32_t           since  = 0;
    // full blocks of table t: t, t + E, ...: nft of them
    const uint64_t nft = a.nfull > t ? (a.nfull - t + a.E - 1) / a.E : 0;
    if (a.vec) {
        // as k_byte_hist, over the virtual buffer "the full blocks of table t back to back": vector i is vector i % V of
        // block t + (i / V) E.  Rows of 64 vectors, workgroup k takes rows k, k + G, ... kHistUnroll at a time.
        const uint64_t V = B / 16, nvec = nft * V, G = a.wgs;
        auto at = [&](uint64_t i) {
            const uint64_t j = a.vshift != 0xFFFFFFFFu ? i >> a.vshift : i / V;
            return (const uint4 *)(a.in + (j * a.E + t) * B + (i - j * V) * 16);
        };
        uint64_t r = k;
        uint4    x[kHistUnroll];
        bool     ok[kHistUnroll];
        auto load = [&](uint64_t r0) {
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; u++) {
                const uint64_t i = (r0 + u * G) * 64 + lane;
                ok[u] = i < nvec;
                if (ok[u])
                    x[u] = *at(i);
            }
        };
        if (r * 64 < nvec)
            load(r);
        while (r * 64 < nvec) {
            uint4 cur[kHistUnroll];
            bool  cok[kHistUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; u++) {
                cur[u] = x[u];
                cok[u] = ok[u];
            }
            const uint64_t next = r + kHistUnroll * G;
            if (next * 64 < nvec) // the next step's loads are in flight while this step counts
                load(next);
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; u++)
                if (cok[u]) {
                    hist_word(col, cur[u].x);
                    hist_word(col, cur[u].y);
                    hist_word(col, cur[u].z);
                    hist_word(col, cur[u].w);
                }
            since += 16 * kHistUnroll;
            if (since + 16 * kHistUnroll > kHistLaneMax) {
                hist_flush(lds, lane, acc);
                since = 0;
            }
            r = next;
        }
    } else {
        // byte-wise: block sizes that are not 16-byte multiples, unaligned buffers
        for (uint64_t j = k; j < nft; j += a.wgs)
            hist_run_bytes(lds, lane, acc, since, a.in + (j * a.E + t) * B, B);
    }
    // the short last block is counted by its index like any other, by the first workgroup of its table
    if (k == 0 && a.nfull * B < a.in_len && a.nfull % a.E == t)
        hist_run_bytes(lds, lane, acc, since, a.in + a.nfull * B, a.in_len - a.nfull * B);
    hist_flush(lds, lane, acc);
    unsigned long long *counts = a.counts + 256 * t;
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
        if (acc[i])
            atomicAdd(counts + 2 * lane + 128 * (i >> 1) + (i & 1), acc[i]);
}

// ---- the tables of the coders ---------------------------------------------------------------------------------------
struct PlaneTables {
    const uint32_t *cum;   // u32[E][258], device memory
    uint32_t        E;
    uint32_t        total; // every table's cum[257] ...
    double          rc257; // ... but for the table of a t that owns no bytes: all ones, total 257 (static_rc(257))
};

// Every thread of the workgroup calls this (a barrier).  True if table `cum` is one the coders can run under: strictly
// increasing from 0 to the launch's total, or to 257 (then it is all ones: an empty input's one block is coded under it).
__device__ __forceinline__ bool plane_table_ok(const uint32_t *cum, uint32_t total)
{
    bool bad = false;
    for (uint32_t i = threadIdx.x; i < kStaticEntries; i += blockDim.x) {
        const uint32_t v = cum[i];
        bad |= i == 0 ? v != 0 : v <= cum[i - 1];
        bad |= i == kStaticEntries - 1 && v != total && v != kStaticEntries - 1;
    }
    return __syncthreads_or(bad) == 0;
}

// the reciprocal that goes with table `cum` (wave-uniform)
__device__ __forceinline__ double plane_table_rc(const uint32_t *cum, const PlaneTables &t, double rc)
{
    return cum[kStaticEntries - 1] == t.total ? rc : t.rc257;
}

// the blocks of a workgroup whose table failed the check: WAVES waves of 64 blocks from wave slot w0 of table t
__device__ __forceinline__ void plane_static_refuse(const DecArgs &d, const PlaneTables &pt, uint64_t w0, uint32_t t)
{
    const uint64_t blk = (w0 * 64 + threadIdx.x) * pt.E + t;
    if (blk < d.nblocks) {
        d.out_sizes[blk] = 0;
        d.status[blk]    = REDUX_INVALID_INPUT;
    }
}

} // namespace redux
