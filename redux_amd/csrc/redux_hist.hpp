// redux_hist.hpp -- semi-static coding: the byte histogram of a device buffer and the static table built from it.
//
//   k_byte_hist     counts the bytes of a buffer into u64[256] (added to).  One wave per workgroup; every lane keeps its
//                   own packed u16 counters in LDS, dword [bin/2][lane] (32 KiB per wave): lane l's counter of bin b is
//                   dword 64 (b/2) + l, so the 64 lanes of a ds_add always address 64 consecutive dwords, one per bank
//                   of gfx950's 64, whatever the data: a buffer of one byte value costs what iid bytes cost.  The counters are
//                   folded into 64-bit registers before any of them can reach 65,536, and each workgroup ends with one
//                   global u64 atomic add per nonzero bin (integer adds: the result does not depend on their order).
//   k_static_table  one workgroup of 256 threads (static_table_build): the counts -> cum[0..=257] by the rule of include/redux_hip.h
//                   ("semi-static coding"), bit for bit what redux_static_table_from_counts computes on the host.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace redux {

constexpr uint32_t kHistPairs  = 128;  // dword rows of the per-lane counters: bins 2p (low half) and 2p+1 (high half)
#ifndef REDUX_HIST_UNROLL
#define REDUX_HIST_UNROLL 4 // (variant builds: tools/ab/hist_variants.sh)
#endif
#ifndef REDUX_HIST_WGS_PER_CU
#define REDUX_HIST_WGS_PER_CU 4
#endif
constexpr uint32_t kHistUnroll = REDUX_HIST_UNROLL; // 16-byte vectors a lane loads per step (and as many prefetched for the next)
constexpr uint32_t kHistWgsPerCu = REDUX_HIST_WGS_PER_CU; // one-wave workgroups per CU (32 KiB of LDS each)
constexpr uint32_t kHistFlush  = 4095; // vectors a lane may count between flushes: 16 * 4095 = 65,520 < 65,536

struct HistArgs {
    const uint8_t      *in;
    uint64_t            head;   // bytes before the first 16-byte boundary (< 16)
    uint64_t            nvec;   // 16-byte vectors of the aligned body, which starts at in + head
    uint64_t            tail;   // bytes after it (< 16)
    unsigned long long *counts; // u64[256]
};

__device__ __forceinline__ void hist_byte(uint32_t *col, uint32_t b) // col = the lane's column of the counters
{
    atomicAdd(col + (b >> 1) * 64, 1u << ((b & 1) << 4)); // ds_add_u32, no return
}

__device__ __forceinline__ void hist_word(uint32_t *col, uint32_t w)
{
    hist_byte(col, w & 0xFF);
    hist_byte(col, (w >> 8) & 0xFF);
    hist_byte(col, (w >> 16) & 0xFF);
    hist_byte(col, w >> 24);
}

// every lane's counters -> acc (lane l owns bins 2l, 2l+1, 2l+128, 2l+129), the counters back to zero.  Lane l reads row l
// (and l+64) starting at column l: at step k lane l reads dword 64 row + (l + k) mod 64, so the 64 lanes address 64
// different banks.
__device__ __forceinline__ void hist_flush(uint32_t *lds, uint32_t lane, unsigned long long (&acc)[4])
{
    __syncthreads(); // (one wave: orders the adds of every lane before the reads)
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        uint32_t *row = lds + (lane + 64 * h) * 64;
        uint32_t  lo = 0, hi = 0; // 64 lanes * 65,535 < 2^32
        for (uint32_t k = 0; k < 64; k++) {
            const uint32_t j = (lane + k) & 63, v = row[j];
            row[j] = 0;
            lo += v & 0xFFFF;
            hi += v >> 16;
        }
        acc[2 * h] += lo;
        acc[2 * h + 1] += hi;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(64) k_byte_hist(HistArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    unsigned long long acc[4] = {0, 0, 0, 0};
    if (blockIdx.x == 0) { // the unaligned head and tail, a byte per lane
        if (lane < a.head)
            hist_byte(col, a.in[lane]);
        if (lane < a.tail)
            hist_byte(col, a.in[a.head + a.nvec * 16 + lane]);
    }
    // rows of 64 vectors: row r is vectors [64 r, 64 r + 64); workgroup g takes rows g, g + G, g + 2G, ... kHistUnroll at a
    // time.  The loop is wave-uniform (the flush reads other lanes' counters); a lane past the end loads nothing.
    const uint4   *v     = (const uint4 *)(a.in + a.head);
    const uint64_t G     = gridDim.x;
    uint64_t       r     = blockIdx.x;
    uint4          x[kHistUnroll];
    bool           ok[kHistUnroll];
    auto load = [&](uint64_t r0) {
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; u++) {
            const uint64_t i = (r0 + u * G) * 64 + lane;
            ok[u] = i < a.nvec;
            if (ok[u])
                x[u] = v[i];
        }
    };
    uint32_t since = 0;
    if (r * 64 < a.nvec)
        load(r);
    while (r * 64 < a.nvec) {
        uint4 cur[kHistUnroll];
        bool  cok[kHistUnroll];
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; u++) {
            cur[u] = x[u];
            cok[u] = ok[u];
        }
        const uint64_t next = r + kHistUnroll * G;
        if (next * 64 < a.nvec) // the next step's loads are in flight while this step counts
            load(next);
#ifdef REDUX_HIST_LOADS_ONLY // variant: the loads without the counting (what the memory side alone allows)
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; u++)
            if (cok[u])
                acc[0] += cur[u].x ^ cur[u].y ^ cur[u].z ^ cur[u].w;
#else
#pragma unroll
        for (uint32_t u = 0; u < kHistUnroll; u++)
            if (cok[u]) {
                hist_word(col, cur[u].x);
                hist_word(col, cur[u].y);
                hist_word(col, cur[u].z);
                hist_word(col, cur[u].w);
            }
#endif
        since += kHistUnroll;
        if (since + kHistUnroll > kHistFlush) {
            hist_flush(lds, lane, acc);
            since = 0;
        }
        r = next;
    }
    hist_flush(lds, lane, acc);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
        if (acc[k])
            atomicAdd(a.counts + 2 * lane + 128 * (k >> 1) + (k & 1), acc[k]);
}

// ---- the rule (include/redux_hip.h, "semi-static coding") ----------------------------------------------------------
// thread s: byte s.  N = sum c, R = total - 257; f[s] = 1 + floor(c[s] R / N), r[s] = c[s] R mod N; the D = total - sum f
// bytes with the largest r (ties: lower index first) get one more; EOF = 1.  N = 0: every frequency 1.  N R >= 2^64 (or
// N itself >= 2^64): the table is all zeros, which redux_static_table_check rejects.
// (every thread of a 256-thread workgroup calls this: barriers)
__device__ __forceinline__ void static_table_build(const unsigned long long *counts, uint32_t total, uint32_t *cum)
{
    __shared__ unsigned long long s_lo[256], s_hi[256], s_r[256];
    __shared__ uint32_t           s_f[256];
    const uint32_t s = threadIdx.x;
    const unsigned long long c = counts[s];
    s_lo[s] = c;
    s_hi[s] = 0;
    __syncthreads();
    for (uint32_t w = 128; w; w >>= 1) { // N as a 128-bit sum
        if (s < w) {
            const unsigned long long lo = s_lo[s] + s_lo[s + w];
            s_hi[s] += s_hi[s + w] + (lo < s_lo[s] ? 1 : 0);
            s_lo[s] = lo;
        }
        __syncthreads();
    }
    const unsigned long long N = s_lo[0], R = total - 257ull;
    if (s_hi[0] || __umul64hi(N, R)) { // unsupported: a table no coder accepts
        cum[s] = 0;
        if (s < 2)
            cum[256 + s] = 0;
        return;
    }
    uint32_t           f = 1;
    unsigned long long r = 0;
    if (N) {
        const unsigned long long cr = c * R;
        f += (uint32_t)(cr / N);
        r = cr % N;
    }
    s_r[s] = r;
    s_f[s] = f;
    __syncthreads();
    for (uint32_t w = 128; w; w >>= 1) { // sum f (< 2^32: at most total)
        const uint32_t add = s < w ? s_f[s + w] : 0;
        __syncthreads();
        if (s < w)
            s_f[s] += add;
        __syncthreads();
    }
    const uint32_t D = total - 1 - s_f[0]; // (N = 0: nothing is handed out, the total stays 257)
    uint32_t rank = 0;
    for (uint32_t j = 0; j < 256; j++) {
        const unsigned long long o = s_r[j];
        rank += (o > r || (o == r && j < s)) ? 1 : 0;
    }
    if (N && rank < D)
        f++;
    __syncthreads();
    s_f[s] = f;
    __syncthreads();
    for (uint32_t w = 1; w < 256; w <<= 1) { // inclusive scan
        const uint32_t add = s >= w ? s_f[s - w] : 0;
        __syncthreads();
        s_f[s] += add;
        __syncthreads();
    }
    cum[s + 1] = s_f[s];
    if (s == 0)
        cum[0] = 0;
    if (s == 255)
        cum[257] = s_f[255] + 1;
}

__global__ void __launch_bounds__(256) k_static_table(const unsigned long long *counts, uint32_t total, uint32_t *cum)
{
    static_table_build(counts, total, cum);
}

} // namespace redux
