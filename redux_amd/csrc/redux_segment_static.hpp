// redux_segment_static.hpp -- segment-static coding: the static coder with E tables per block range (gfx950 only).
//
// The rule (include/redux_hip.h, "segment-static coding"): x' is the byte-plane layout of the input for element size E and
// block size B; a segment is G = 64 E k consecutive blocks of x'; table (s, t) is the semi-static table of the bytes of the
// blocks b of segment s with b mod E == t, and block b is coded under table (b / G) E + b mod E by the static coder.
//
//   k_segment_hist                 counts x' into u64[nseg][E][256] (added to).  k_plane_hist's design; a workgroup is bound
//                                  to one (s, t) at a time and walks that pair's blocks s G + t, s G + t + E, ...
//   k_static_tables                k_static_table's body (static_table_build, redux_hist.hpp), one workgroup per table
//   k_encode_segment_static        k_encode_static / k_decode_static / k_decode_static_lock / k_decode_static_lut with their
//   k_decode_segment_static        bodies unchanged; what differs is which block a lane owns and which table a workgroup
//   k_decode_segment_static_lock   loads: workgroup g serves plane t = g mod E, and wave slot w of that t owns the blocks
//   k_decode_segment_static_lut    (64 w + lane) E + t, which all lie in segment w / k, so it loads table (w / k) E + t.
//                                  Slots, sizes, status and offsets stay indexed by the real block number, so the scan /
//                                  compact kernels and the output addressing are untouched.  The lookup decoder shares one
//                                  table among WAVES wave slots: it is launched only where k is a multiple of WAVES, so
//                                  that those slots share a segment.  These are plane-static's coders too (k == 0, below).
//
// The tables are read from device memory and checked by the workgroup that loads them (plane_table_ok): a bad table makes
// only that workgroup's blocks INVALID_INPUT.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_plane_static.hpp"

namespace redux {

// ---- per-(segment, plane) histogram -------------------------------------------------------------------------------------
struct SegmentHistArgs {
    const uint8_t      *in;     // x'
    uint64_t            in_len;
    uint64_t            nfull;  // full blocks: in_len / block_size
    uint64_t            npairs; // nseg * E
    uint64_t            pstep;  // pairs in flight: the grid is pstep * wgs, workgroup g starts at pair g / wgs as number g % wgs
    uint32_t            block_size;
    uint32_t            E;
    uint32_t            G;      // blocks per segment: 64 E k
    uint32_t            wgs;    // workgroups per pair
    uint32_t            vec;    // in and block_size are 16-byte multiples: full blocks are read as 16-byte vectors
    uint32_t            vshift; // log2(block_size / 16) if that is a power of two, else 0xFFFFFFFF
    unsigned long long *counts; // u64[nseg][E][256]
};

__global__ void __launch_bounds__(64) k_segment_hist(SegmentHistArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const uint32_t k = blockIdx.x % a.wgs;
    const uint64_t B = a.block_size;
    for (uint64_t pair = blockIdx.x / a.wgs; pair < a.npairs; pair += a.pstep) { // (every flush leaves the counters zero)
        const uint64_t s  = pair / a.E;
        const uint32_t t  = (uint32_t)(pair % a.E);
        const uint64_t b0 = s * a.G + t; // the pair's first block; its blocks are b0 + j E, j < nft, inside the segment
        const uint64_t hi = (s + 1) * a.G < a.nfull ? (s + 1) * a.G : a.nfull;
        const uint64_t nft = hi > b0 ? (hi - b0 + a.E - 1) / a.E : 0; // full blocks of the pair
        unsigned long long acc[4] = {0, 0, 0, 0};
        uint32_t           since  = 0;
        if (a.vec) {
            // as k_plane_hist, over the virtual buffer "the full blocks of the pair back to back"
            const uint64_t V = B / 16, nvec = nft * V, W = a.wgs;
            auto at = [&](uint64_t i) {
                const uint64_t j = a.vshift != 0xFFFFFFFFu ? i >> a.vshift : i / V;
                return (const uint4 *)(a.in + (b0 + j * a.E) * B + (i - j * V) * 16);
            };
            uint64_t r = k;
            uint4    x[kHistUnroll];
            bool     ok[kHistUnroll];
            auto load = [&](uint64_t r0) {
#pragma unroll
                for (uint32_t u = 0; u < kHistUnroll; u++) {
                    const uint64_t i = (r0 + u * W) * 64 + lane;
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
                const uint64_t next = r + kHistUnroll * W;
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
                hist_run_bytes(lds, lane, acc, since, a.in + (b0 + j * a.E) * B, B);
        }
        // the short last block is counted by its index like any other, by the first workgroup of its pair
        if (k == 0 && a.nfull * B < a.in_len && a.nfull / a.G == s && a.nfull % a.E == t)
            hist_run_bytes(lds, lane, acc, since, a.in + a.nfull * B, a.in_len - a.nfull * B);
        hist_flush(lds, lane, acc);
        unsigned long long *counts = a.counts + 256 * pair;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (acc[i])
                atomicAdd(counts + 2 * lane + 128 * (i >> 1) + (i & 1), acc[i]);
    }
}

// ---- the rule for a batch of tables: workgroup g turns counts + 256 g into cum + 258 g -------------------------------
__global__ void __launch_bounds__(256) k_static_tables(const unsigned long long *counts, uint32_t total, uint32_t *cum)
{
    static_table_build(counts + 256ull * blockIdx.x, total, cum + (uint64_t)kStaticEntries * blockIdx.x);
}

// ---- the coders with nseg * E tables -------------------------------------------------------------------------------------
// k == 0 stands for "one segment that holds every block": E tables, table t for every wave slot of plane t, which is
// plane-static coding (redux_plane_static.hpp).  Nothing is divided by such a k, and the launch code's "k a multiple of
// WAVES" holds for it, as it should: all wave slots of a plane share the one table.
struct SegmentTables {
    PlaneTables p; // p.cum: u32[nseg][E][258], device memory
    uint32_t    k; // wave slots of a plane per segment: G = 64 E k; 0: a single segment
};

// the table of wave slot w of plane t (w: wave-uniform)
__device__ __forceinline__ const uint32_t *segment_cum(const SegmentTables &s, uint64_t w, uint32_t t)
{
    return s.p.cum + (uint64_t)kStaticEntries * ((s.k ? w / s.k : 0) * s.p.E + t);
}

struct SegmentStaticEncArgs {
    StaticEncCore c;
    SegmentTables t;
};

template <bool FIXUP, bool CB32, bool SOLO = false>
__global__ void __launch_bounds__(64) k_encode_segment_static(SegmentStaticEncArgs a)
{
    __shared__ uint32_t tab[kStaticEntries + 2];
    claim_the_simd<SOLO>();
    const uint32_t E    = a.t.p.E, t = blockIdx.x % E;
    const uint64_t w    = blockIdx.x / E;
    const uint64_t blk0 = w * 64 * E + t; // lane 0's block
    if (blk0 >= a.c.nblocks)
        return;
    const uint32_t *cum = segment_cum(a.t, w, t);
    if (!plane_table_ok(cum, a.t.p.total)) {
        const uint64_t blk = blk0 + (uint64_t)threadIdx.x * E;
        if (blk < a.c.nblocks) {
            a.c.sizes[blk]  = 0;
            a.c.status[blk] = REDUX_INVALID_INPUT;
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < kStaticEntries; i += 64)
        tab[i] = cum[i];
    __syncthreads();
    StaticEncCore c = a.c;
    c.rc            = plane_table_rc(cum, a.t.p, a.c.rc);
    TableModel m{tab};
    static_encode_body<FIXUP, CB32>(c, m, blk0, threadIdx.x, E);
}

struct SegmentStaticDecArgs {
    StaticDecCore c;
    SegmentTables t;
};

template <bool FIXUP>
__global__ void __launch_bounds__(64) k_decode_segment_static(SegmentStaticDecArgs a)
{
    __shared__ uint32_t tab[kStaticEntries + 2];
    const uint32_t  E   = a.t.p.E, t = blockIdx.x % E;
    const uint64_t  w   = blockIdx.x / E;
    const uint64_t  blk = (w * 64 + threadIdx.x) * E + t;
    const uint32_t *cum = segment_cum(a.t, w, t);
    if (!plane_table_ok(cum, a.t.p.total)) {
        if (blk < a.c.nblocks) {
            a.c.out_sizes[blk] = 0;
            a.c.status[blk]    = REDUX_INVALID_INPUT;
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < kStaticEntries; i += 64)
        tab[i] = cum[i];
    __syncthreads();
    StaticDecCore c = a.c;
    c.rc            = plane_table_rc(cum, a.t.p, a.c.rc);
    TableModel m{tab};
    static_decode_body<FIXUP>(c, m, blk);
}

struct SegmentStaticLockArgs {
    DecArgs       d;
    double        rc;
    SegmentTables t;
};

template <bool CB32, bool SOLO>
__global__ void __launch_bounds__(64) k_decode_segment_static_lock(SegmentStaticLockArgs a)
{
    __shared__ uint32_t lds[kStaticTreeDwords + 32 * 64];
    claim_the_simd<SOLO>();
    const uint32_t  t   = blockIdx.x % a.t.p.E;
    const uint64_t  w   = blockIdx.x / a.t.p.E;
    const uint32_t *cum = segment_cum(a.t, w, t);
    if (!plane_table_ok(cum, a.t.p.total)) {
        plane_static_refuse(a.d, a.t.p, w, t);
        return;
    }
    decode_lock_body<CB32, 1>(a.d, lds, cum, plane_table_rc(cum, a.t.p, a.rc), threadIdx.x, w, nullptr, nullptr, a.t.p.E, t);
}

// k % WAVES == 0 (the launch code's condition): the slots g WAVES .. g WAVES + WAVES - 1 lie in segment g WAVES / k
template <bool CB32, int WAVES>
__global__ void __launch_bounds__(64 * WAVES) k_decode_segment_static_lut(SegmentStaticLockArgs a)
{
    __shared__ uint32_t lds[65536 / 4 + 260 + WAVES * 32 * 64];
    const uint32_t  t   = blockIdx.x % a.t.p.E;
    const uint64_t  g   = blockIdx.x / a.t.p.E;
    const uint32_t *cum = segment_cum(a.t, g * WAVES, t);
    if (!plane_table_ok(cum, a.t.p.total)) {
        plane_static_refuse(a.d, a.t.p, g * WAVES, t); // (threadIdx.x runs over the workgroup's WAVES * 64 blocks)
        return;
    }
    static_lut_body<CB32, WAVES>(a.d, plane_table_rc(cum, a.t.p, a.rc), cum, lds, g, a.t.p.E, t);
}

} // namespace redux
