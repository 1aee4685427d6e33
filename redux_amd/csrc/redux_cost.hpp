// redux_cost.hpp -- size estimates: what a block would cost under a model, from counts alone (gfx950 only).
//
// Every model of the project is exchangeable inside a block: the ideal code length of a block is a
// function of its byte counts, not of the order of its bytes.
//
//   k_block_cost   the adaptive model.  A block starts at total 257 (256 bytes + EOF, one each) and every coded symbol adds
//                  one, so a block with histogram h and n bytes costs, EOF included,
//                      A(h, n) = log2 G(n + 258) - log2 G(257) - sum_s log2 G(h[s] + 1)        (G = the gamma function)
//                  bits.  One wave per workgroup walks blocks g, g + G, ...: the block is counted as k_byte_hist counts a
//                  buffer (redux_hist.hpp: lane-private packed u16 counters, 32 KiB of LDS, no bank conflict whatever the
//                  data; 16-byte loads, the next step's in flight while this one counts; a fold before any counter can pass
//                  65,535), the fold leaves each lane 4 bins, the lane takes lgamma of each in f64, one wave reduction, and
//                  lane 0 stores the block's f64.  A block far smaller than a wave's worth pays the whole fold: right, not fast.
//   k_table_cost   a static table.  Row r: sum_s c[s] (log2 T - log2(cum[s+1] - cum[s])), T = cum[257], the cross-entropy of
//                  the counts under the table, EOF not included.  c[s] == 0 terms are 0; +inf when T == 0 or a frequency
//                  that is not positive meets a nonzero count.  Nothing is indexed by table contents.  One wave per row.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_hist.hpp"

#include <math.h>

namespace redux {

constexpr double kInvLn2 = 1.4426950408889634074; // 1 / ln 2

struct BlockCostArgs {
    const uint8_t *in;
    uint64_t       in_len;
    uint64_t       nblocks;    // redux_block_count(in_len, block_size)
    uint32_t       block_size;
    double        *bits;       // f64[nblocks]
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (uint32_t w = 32; w; w >>= 1)
        v += __shfl_xor(v, w);
    return v;
}

__global__ void __launch_bounds__(64) k_block_cost(BlockCostArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const double lg257 = lgamma(257.0);
    for (uint64_t b = blockIdx.x; b < a.nblocks; b += gridDim.x) { // (wave-uniform)
        const uint64_t at   = b * a.block_size;
        const uint64_t n    = a.in_len - at < a.block_size ? a.in_len - at : a.block_size; // (in_len == 0: block 0, n = 0)
        const uint8_t *base = a.in + at;
        // the block as k_byte_hist sees a buffer: a head of < 16 bytes, 16-byte vectors, a tail of < 16 bytes
        const uint64_t lead = (16 - ((uintptr_t)base & 15)) & 15;
        const uint64_t head = lead < n ? lead : n;
        const uint64_t nvec = (n - head) / 16;
        const uint64_t tail = n - head - nvec * 16;
        unsigned long long acc[4] = {0, 0, 0, 0};
        if (lane < head)
            hist_byte(col, base[lane]);
        if (lane < tail)
            hist_byte(col, base[head + nvec * 16 + lane]);
        uint32_t since = 2; // the most one counter of a lane can hold since the last fold
        // rows of 64 vectors, kHistUnroll at a time; a lane past the end loads nothing
        const uint4 *v = (const uint4 *)(base + head);
        uint4        x[kHistUnroll];
        bool         ok[kHistUnroll];
        auto load = [&](uint64_t r0) {
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; u++) {
                const uint64_t i = (r0 + u) * 64 + lane;
                ok[u] = i < nvec;
                if (ok[u])
                    x[u] = v[i];
            }
        };
        uint64_t r = 0;
        if (nvec)
            load(0);
        while (r * 64 < nvec) {
            uint4 cur[kHistUnroll];
            bool  cok[kHistUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kHistUnroll; u++) {
                cur[u] = x[u];
                cok[u] = ok[u];
            }
            const uint64_t next = r + kHistUnroll;
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
            if (since + 16 * kHistUnroll > 65535) {
                hist_flush(lds, lane, acc);
                since = 0;
            }
            r = next;
        }
        hist_flush(lds, lane, acc); // (leaves the counters zero for the next block)
        double s = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (acc[k] > 1) // (lgamma(1) = lgamma(2) = 0)
                s += lgamma((double)acc[k] + 1.0);
        s = wave_sum(s);
        if (lane == 0)
            a.bits[b] = (lgamma((double)n + 258.0) - lg257 - s) * kInvLn2;
    }
}

// one term of the table cost: c (log2 T - log2 f); +inf for a frequency that is not positive under a nonzero count
__host__ __device__ inline double table_cost_term(unsigned long long c, uint32_t lo, uint32_t hi, double log2T)
{
    if (c == 0)
        return 0.0;
    if (hi <= lo)
        return INFINITY;
    return (double)c * (log2T - log2((double)(hi - lo)));
}

__global__ void __launch_bounds__(64) k_table_cost(const unsigned long long *counts, const uint32_t *cum, uint64_t n, double *bits)
{
    const uint32_t lane = threadIdx.x;
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const unsigned long long *c = counts + 256 * r;
        const uint32_t           *t = cum + 258 * r;
        const uint32_t            T = t[257];
        const double              log2T = T ? log2((double)T) : 0.0;
        double s = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            const uint32_t sym = lane + 64 * k;
            s += table_cost_term(c[sym], t[sym], t[sym + 1], log2T);
        }
        s = wave_sum(s);
        if (lane == 0)
            bits[r] = T ? s : INFINITY;
    }
}

} // namespace redux
