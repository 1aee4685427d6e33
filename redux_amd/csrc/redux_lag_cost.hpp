// redux_lag_cost.hpp -- lag and order estimates: the adaptive model's cost of every block of the input behind the lagged
// delta filter and its higher orders, for a list of lags or of (lag, order) candidates, counted from the untransformed bytes
// (gfx950 only).
//
// Rule: bits[c][b] is k_block_cost's value (redux_cost.hpp) for block b of what k_lag_order_planes /
// k_lag_order_planes_bytes (redux_lag.hpp) write for candidate c = (S, K) -- the fresh start of every frame, terms before
// the frame zero, the fold always on, S >= N (only folds), the short last frame and its trailing bytes included -- and
// nothing else defines it.  A block's adaptive cost depends on its byte counts alone, and the counts of the transformed
// frame can be taken from the frame as it lies: no transformed copy is written.
//
// Frame sampling: with frame_step T only frames 0, T, 2T, ... are costed, and a row of the output holds the blocks of the
// selected frames in order (selected frame k -> blocks k E ...; only the last selected frame can be the short one).
//
// The lag estimates (k_lag_cost, k_lag_cost_bytes) take every candidate at order 1 and leave the list of orders unread; K = 1
// of the order estimates (k_lag_order_cost, k_lag_order_cost_bytes) is k_lag_cost's row for S.  Both share the argument
// struct, the predecessor rule and the difference (lag_pred, lag_diff: redux_lag.hpp), and the byte kernels one body,
// templated on KMAX as the transforms' are.  k_lag_cost and k_lag_order_cost stay two bodies: they run one wave a SIMD at
// the edge of the register file, and the order body reached through a shared function spilled to scratch at E = 2
// (96 bytes a lane; 0 as a kernel of its own) -- profiles/lag_bodies.txt.
//
//   k_lag_cost<E>               full frames, block size and buffer 16-byte multiples.  A job is (selected frame, four
//   k_lag_order_cost<E>         consecutive candidates); a wave counts one candidate, the E blocks of the frame at once, as
//                               a wave of k_layout_cost does (redux_layout_cost.hpp: R rows of 64 x 16 elements per step
//                               with the next step's loads in flight, planes_permute, the exchange through LDS so that
//                               lane group p counts plane p into k_block_cost's lane-private packed u16 counters,
//                               layout_fold before a counter can pass 65,535 -- the kLayoutFoldRows bound: a lane adds at
//                               most 16 E to one counter per row -- lgamma in f64 and one wave reduction per plane).  The
//                               kLagCostWaves waves of a workgroup take consecutive candidates of the SAME frame: the frame
//                               comes from HBM once per workgroup and the other waves, and the workgroups that count
//                               further candidates of the frame at the same time, are served by the caches.  A wave reads
//                               its own 16-byte chunks and K predecessor chunks S E, 2 S E and 3 S E bytes back, bytes the
//                               workgroup reads anyway, each masked on its own by lag_pred's three-way rule against j S: no
//                               byte before a frame's first is read.  It forms d as LagForwardHook does (lag_diff) and
//                               counts it.  The order is wave-uniform: a wave of order 1 issues one predecessor load per
//                               chunk, not three.  The waves of a workgroup meet at every step's barriers (E = 1: at the
//                               fold that ends a frame), so a workgroup moves at the pace of its highest order: callers
//                               that care order the list by ORDER first (measured on 4 GiB and 12 candidates: 0.82 to 0.95
//                               of the time of the same list by lag first).
//   k_lag_cost_bytes<E>         everything else -- the short last frame, unaligned buffers, block sizes that are no multiple
//   k_lag_order_cost_bytes<E>   of 16: one wave per output block and candidate maps each transformed offset back to its
//                               source, as k_layout_cost_bytes does, with the binomial form of the K-fold difference
//                               (lag_order_bytes_forward's).  Right, not fast.
//
// LDS: a wave has 40 KiB (E = 1: 32), so the four waves of a workgroup fill a CU's 160 KiB, the occupancy k_block_cost and
// k_layout_cost run at, and every SIMD holds one wave, which may use the whole register file: the loads in flight are a
// step's 128 bytes of the frame and up to three times as many predecessors.  k_lag_order_cost<1> takes steps of 64 bytes: the
// chunk that j S falls into has 16 elements to mask for each of three predecessors, and with eight rows in flight the
// kernel spilled 28 bytes a lane to scratch; with four it uses none, as every other instance.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_lag.hpp"
#include "redux_layout_cost.hpp"

namespace redux {

constexpr int kLagCostWaves = 4; // waves of a workgroup of k_lag_cost: candidates of one frame counted side by side

struct LagCostArgs {
    const uint8_t *in;
    uint64_t       in_len;
    uint64_t       nblocks;     // redux_block_count(in_len, block_size)
    uint64_t       row_blocks;  // blocks of a row of bits: redux_lag_cost_block_count
    uint64_t       nsel_fast;   // selected frames the fast kernel takes; the byte kernel takes row blocks nsel_fast * E ...
    double        *bits;        // f64[ncand][row_blocks]
    uint32_t       block_size;
    uint32_t       frame_step;
    uint32_t       ncand;
    uint16_t       lags[REDUX_LAG_ORDER_COST_MAX];   // (a lag is at most REDUX_LAG_MAX = 256)
    uint8_t        orders[REDUX_LAG_ORDER_COST_MAX]; // (an order is at most REDUX_LAG_ORDER_MAX = 3; the lag estimates leave it unread)
};
static_assert(REDUX_LAG_ORDER_COST_MAX >= REDUX_LAG_MAX, "a list of lags may name every lag");

// v's 16 elements less p's, folded, in place: k_lag_cost's own form of lag_fold(lag_sub()) on its dword arrays.  Written
// through the two helpers the kernel compiled to other instructions at every E (E = 1: 159 AGPRs for 157), so it stays,
// as the kernel does
template <int E>
__device__ __forceinline__ void lag_cost_diff(uint32_t (&v)[4 * E], const uint32_t (&p)[4 * E])
{
    if constexpr (E == 8) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t d = ((uint64_t)v[2 * j + 1] << 32 | v[2 * j]) - ((uint64_t)p[2 * j + 1] << 32 | p[2 * j]);
            const uint64_t z = d << 1 ^ (uint64_t)((int64_t)d >> 63);
            v[2 * j] = (uint32_t)z; v[2 * j + 1] = (uint32_t)(z >> 32);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4 * E; j++)
            v[j] = zigzag_fold_dword<E>(delta_sub<E>(v[j], p[j]));
    }
}

template <int E>
__global__ void __launch_bounds__(64 * kLagCostWaves) k_lag_cost(LagCostArgs a)
{
    constexpr int      NW = kLagCostWaves;
    constexpr uint32_t W = 64 / E;
    constexpr int      R = 8 / E; // rows per step: a lane loads 128 bytes (and their predecessors) per step
    __shared__ uint32_t counters[NW][kHistPairs * 64];
    __shared__ uint4    exchange[NW][E > 1 ? 64 * 8 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t      *lds = counters[wave], *col = lds + lane;
    uint4         *xl  = exchange[wave];
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const uint32_t frame_groups = a.block_size / 16;         // 16-element groups of a frame
    const uint32_t rows  = (frame_groups + 63) / 64;
    const double   top   = lgamma((double)a.block_size + 258.0) - lgamma(257.0);
    const uint32_t group = lane / W, member = lane % W;
    const uint32_t cand_groups = (a.ncand + NW - 1) / NW;
    // every loop below is uniform over the workgroup: its waves walk the same frame and meet at the same barriers
    for (uint64_t job = blockIdx.x; job < a.nsel_fast * cand_groups; job += gridDim.x) {
        const uint64_t k  = job / cand_groups;                           // the selected frame
        const uint32_t j  = (uint32_t)(job - k * cand_groups) * NW + wave; // the wave's lag (wave-uniform)
        const bool     on = j < a.ncand;                                // a wave past the list counts the last lag, and stores nothing
        const uint32_t S  = a.lags[on ? j : a.ncand - 1];
        const uint8_t *frame = a.in + k * a.frame_step * (uint64_t)E * a.block_size;
        uint32_t acc[2][E][2];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < E; q++)
                acc[h][q][0] = acc[h][q][1] = 0;
        uint32_t nxt[R][4 * E], pnx[R][4 * E];
        auto load = [&](uint32_t row0) { // rows row0 .. row0 + R - 1; a lane past the frame's end loads nothing
#pragma unroll
            for (int u = 0; u < R; u++) {
                const uint32_t i = (row0 + u) * 64 + lane;
#pragma unroll
                for (int c = 0; c < E; c++) {
                    uint4 v = make_uint4(0, 0, 0, 0), p = make_uint4(0, 0, 0, 0);
                    if (i < frame_groups) {
                        const uint8_t *at = frame + ((uint64_t)i * E + c) * 16;
                        v = *(const uint4 *)at;
                        p = lag_pred<E>(at - (uint64_t)S * E, i * 16 + c * (16 / E), S);
                    }
                    nxt[u][4 * c] = v.x; nxt[u][4 * c + 1] = v.y; nxt[u][4 * c + 2] = v.z; nxt[u][4 * c + 3] = v.w;
                    pnx[u][4 * c] = p.x; pnx[u][4 * c + 1] = p.y; pnx[u][4 * c + 2] = p.z; pnx[u][4 * c + 3] = p.w;
                }
            }
        };
        load(0);
        uint32_t since = 0; // rows since the last fold
        for (uint32_t row0 = 0; row0 < rows; row0 += R) {
            uint32_t d[R][4 * E];
#pragma unroll
            for (int u = 0; u < R; u++) { // (rows past the frame's end hold zeros: they are not counted)
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    d[u][q] = nxt[u][q];
                lag_cost_diff<E>(d[u], pnx[u]);
            }
            if (row0 + R < rows) // the next step's loads are in flight while this step counts
                load(row0 + R);
            // live groups of each of the step's rows (0 past the frame's end)
            uint32_t nlive[R];
#pragma unroll
            for (int u = 0; u < R; u++) {
                const uint32_t g0 = (row0 + u) * 64;
                nlive[u] = g0 >= frame_groups ? 0 : frame_groups - g0 < 64 ? frame_groups - g0 : 64;
            }
            if constexpr (E == 1) {
#pragma unroll
                for (int u = 0; u < R; u++)
                    if (lane < nlive[u]) {
                        hist_word(col, d[u][0]);
                        hist_word(col, d[u][1]);
                        hist_word(col, d[u][2]);
                        hist_word(col, d[u][3]);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < R; u++) {
                    uint32_t out[4 * E];
                    planes_permute<E, false>(d[u], out);
                    if (lane < nlive[u])
#pragma unroll
                        for (int p = 0; p < E; p++)
                            xl[u * 64 * E + p * 64 + lane] = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
                }
                __syncthreads();
                // group g takes plane g: chunk pos of the plane came from lane pos; the groups start W chunks apart
#pragma unroll
                for (int u = 0; u < R; u++)
#pragma unroll
                    for (int c = 0; c < E; c++) {
                        const uint32_t pos = ((c + group) & (E - 1)) * W + member;
                        if (pos < nlive[u]) {
                            const uint4 v = xl[u * 64 * E + group * 64 + pos];
                            hist_word(col, v.x);
                            hist_word(col, v.y);
                            hist_word(col, v.z);
                            hist_word(col, v.w);
                        }
                    }
                __syncthreads(); // (the next step overwrites the exchange)
            }
            since += R;
            if (since + R > kLayoutFoldRows<E>) { // the next step's rows would pass the bound
                layout_fold<E>(lds, lane, acc);
                since = 0;
            }
        }
        layout_fold<E>(lds, lane, acc); // (leaves the counters zero for the next job)
        double t[E];
#pragma unroll
        for (int q = 0; q < E; q++) {
            double s = 0;
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int x = 0; x < 2; x++)
                    if (acc[h][q][x] > 1) // (lgamma(1) = lgamma(2) = 0)
                        s += lgamma((double)acc[h][q][x] + 1.0);
            t[q] = s;
        }
#pragma unroll
        for (int g = 0; g < E; g++) { // plane g: the lane's t[q] with (q + lane) mod E == g
            double v = 0;
#pragma unroll
            for (int q = 0; q < E; q++)
                if (((q + lane) & (E - 1)) == (uint32_t)g)
                    v = t[q];
            v = wave_sum(v);
            if (lane == 0 && on)
                a.bits[(uint64_t)j * a.row_blocks + k * E + g] = (top - v) * kInvLn2;
        }
    }
}

template <int E>
__global__ void __launch_bounds__(64 * kLagCostWaves) k_lag_order_cost(LagCostArgs a)
{
    constexpr int      NW = kLagCostWaves;
    constexpr uint32_t W = 64 / E;
    constexpr int      R = E == 1 ? 4 : 8 / E; // rows per step: a lane loads 128 bytes (E = 1: 64) and their predecessors per step
    __shared__ uint32_t counters[NW][kHistPairs * 64];
    __shared__ uint4    exchange[NW][E > 1 ? 64 * 8 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t      *lds = counters[wave], *col = lds + lane;
    uint4         *xl  = exchange[wave];
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const uint32_t frame_groups = a.block_size / 16;         // 16-element groups of a frame
    const uint32_t rows  = (frame_groups + 63) / 64;
    const double   top   = lgamma((double)a.block_size + 258.0) - lgamma(257.0);
    const uint32_t group = lane / W, member = lane % W;
    const uint32_t cand_groups = (a.ncand + NW - 1) / NW;
    // every loop below is uniform over the workgroup: its waves walk the same frame and meet at the same barriers
    for (uint64_t job = blockIdx.x; job < a.nsel_fast * cand_groups; job += gridDim.x) {
        const uint64_t k  = job / cand_groups;                            // the selected frame
        const uint32_t j  = (uint32_t)(job - k * cand_groups) * NW + wave; // the wave's candidate (wave-uniform)
        const bool     on = j < a.ncand;                                  // a wave past the list counts the last one, and stores nothing
        const uint32_t S  = a.lags[on ? j : a.ncand - 1];
        const uint32_t K  = __builtin_amdgcn_readfirstlane((uint32_t)a.orders[on ? j : a.ncand - 1]);
        const uint64_t step = (uint64_t)S * E;                            // bytes from a chunk to its predecessor
        const uint8_t *frame = a.in + k * a.frame_step * (uint64_t)E * a.block_size;
        uint32_t acc[2][E][2];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < E; q++)
                acc[h][q][0] = acc[h][q][1] = 0;
        uint4 nxt[R][E], pn1[R][E], pn2[R][E], pn3[R][E];
        auto load = [&](uint32_t row0) { // rows row0 .. row0 + R - 1; a lane past the frame's end loads nothing
#pragma unroll
            for (int u = 0; u < R; u++) {
                const uint32_t i = (row0 + u) * 64 + lane;
#pragma unroll
                for (int c = 0; c < E; c++) {
                    const uint4 zero = make_uint4(0, 0, 0, 0);
                    nxt[u][c] = pn1[u][c] = pn2[u][c] = pn3[u][c] = zero;
                    if (i < frame_groups) {
                        const uint8_t *at = frame + ((uint64_t)i * E + c) * 16;
                        const uint32_t e0 = i * 16 + c * (16 / E); // the chunk's first element in its frame
                        nxt[u][c] = *(const uint4 *)at;
                        pn1[u][c] = lag_pred<E>(at - step, e0, S);
                        if (K >= 2)
                            pn2[u][c] = lag_pred<E>(at - 2 * step, e0, 2 * S);
                        if (K >= 3)
                            pn3[u][c] = lag_pred<E>(at - 3 * step, e0, 3 * S);
                    }
                }
            }
        };
        load(0);
        uint32_t since = 0; // rows since the last fold
        for (uint32_t row0 = 0; row0 < rows; row0 += R) {
            uint32_t d[R][4 * E];
#pragma unroll
            for (int u = 0; u < R; u++) // (rows past the frame's end hold zeros: they are not counted)
#pragma unroll
                for (int c = 0; c < E; c++) {
                    const uint4 z = lag_diff<E>(nxt[u][c], pn1[u][c], pn2[u][c], pn3[u][c], K);
                    d[u][4 * c] = z.x; d[u][4 * c + 1] = z.y; d[u][4 * c + 2] = z.z; d[u][4 * c + 3] = z.w;
                }
            if (row0 + R < rows) // the next step's loads are in flight while this step counts
                load(row0 + R);
            // live groups of each of the step's rows (0 past the frame's end)
            uint32_t nlive[R];
#pragma unroll
            for (int u = 0; u < R; u++) {
                const uint32_t g0 = (row0 + u) * 64;
                nlive[u] = g0 >= frame_groups ? 0 : frame_groups - g0 < 64 ? frame_groups - g0 : 64;
            }
            if constexpr (E == 1) {
#pragma unroll
                for (int u = 0; u < R; u++)
                    if (lane < nlive[u]) {
                        hist_word(col, d[u][0]);
                        hist_word(col, d[u][1]);
                        hist_word(col, d[u][2]);
                        hist_word(col, d[u][3]);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < R; u++) {
                    uint32_t out[4 * E];
                    planes_permute<E, false>(d[u], out);
                    if (lane < nlive[u])
#pragma unroll
                        for (int p = 0; p < E; p++)
                            xl[u * 64 * E + p * 64 + lane] = make_uint4(out[4 * p], out[4 * p + 1], out[4 * p + 2], out[4 * p + 3]);
                }
                __syncthreads();
                // group g takes plane g: chunk pos of the plane came from lane pos; the groups start W chunks apart
#pragma unroll
                for (int u = 0; u < R; u++)
#pragma unroll
                    for (int c = 0; c < E; c++) {
                        const uint32_t pos = ((c + group) & (E - 1)) * W + member;
                        if (pos < nlive[u]) {
                            const uint4 v = xl[u * 64 * E + group * 64 + pos];
                            hist_word(col, v.x);
                            hist_word(col, v.y);
                            hist_word(col, v.z);
                            hist_word(col, v.w);
                        }
                    }
                __syncthreads(); // (the next step overwrites the exchange)
            }
            since += R;
            if (since + R > kLayoutFoldRows<E>) { // the next step's rows would pass the bound
                layout_fold<E>(lds, lane, acc);
                since = 0;
            }
        }
        layout_fold<E>(lds, lane, acc); // (leaves the counters zero for the next job)
        double t[E];
#pragma unroll
        for (int q = 0; q < E; q++) {
            double s = 0;
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int x = 0; x < 2; x++)
                    if (acc[h][q][x] > 1) // (lgamma(1) = lgamma(2) = 0)
                        s += lgamma((double)acc[h][q][x] + 1.0);
            t[q] = s;
        }
#pragma unroll
        for (int g = 0; g < E; g++) { // plane g: the lane's t[q] with (q + lane) mod E == g
            double v = 0;
#pragma unroll
            for (int q = 0; q < E; q++)
                if (((q + lane) & (E - 1)) == (uint32_t)g)
                    v = t[q];
            v = wave_sum(v);
            if (lane == 0 && on)
                a.bits[(uint64_t)j * a.row_blocks + k * E + g] = (top - v) * kInvLn2;
        }
    }
}

// the byte at offset r of the transformed frame that starts at `frame` and has L bytes, under lag S and order K: the
// binomial form, a term j S back counted where it lies in the frame (lag_order_bytes_forward's)
template <int E>
__device__ __forceinline__ uint32_t lag_cost_byte(const uint8_t *frame, uint64_t L, uint64_t r, uint32_t S, uint32_t K)
{
    const uint64_t N = L / E;
    if (r >= N * E) // trailing bytes (all of a frame shorter than an element)
        return frame[r];
    const uint64_t p = r / N, i = r - p * N;
    uint64_t d = 0;
    int64_t  coef = 1; // (-1)^j C(K, j)
    for (uint32_t j = 0; j <= K && i >= (uint64_t)j * S; j++) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < E; k++)
            x |= (uint64_t)frame[(i - (uint64_t)j * S) * E + k] << (8 * k);
        d += (uint64_t)coef * x;
        coef = -coef * (int64_t)(K - j) / (int64_t)(j + 1);
    }
    d = d << 1 ^ (0 - (d >> (8 * E - 1) & 1)); // (the bits above the element's 8 E are dropped below)
    return (uint32_t)(d >> (8 * p)) & 0xFF;
}

template <int E, int KMAX>
__device__ __forceinline__ void lag_cost_bytes_body(const LagCostArgs &a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const double   lg257 = lgamma(257.0);
    const uint64_t frame = (uint64_t)E * a.block_size, first = a.nsel_fast * E, nrest = a.row_blocks - first;
    for (uint64_t w = blockIdx.x; w < nrest * a.ncand; w += gridDim.x) { // (wave-uniform)
        const uint32_t j     = (uint32_t)(w / nrest);
        const uint64_t c     = first + (w - j * nrest);               // the block's place in its row
        const uint64_t b     = c / E * a.frame_step * E + c % E;      // the block of the input
        const uint32_t S     = a.lags[j], K = KMAX == 1 ? 1 : a.orders[j];
        const uint64_t at    = b * a.block_size;
        const uint64_t n     = a.in_len > at ? (a.in_len - at < a.block_size ? a.in_len - at : a.block_size) : 0;
        const uint64_t fbase = at / frame * frame; // (a block lies inside one frame)
        const uint64_t L     = a.in_len - fbase < frame ? a.in_len - fbase : frame;
        unsigned long long acc[4] = {0, 0, 0, 0};
        uint32_t since = 0;
        for (uint64_t o = 0; o < n; o += 64) {
            if (o + lane < n)
                hist_byte(col, lag_cost_byte<E>(a.in + fbase, L, at - fbase + o + lane, S, K));
            if (++since == 65535) { // a lane adds one byte per step
                hist_flush(lds, lane, acc);
                since = 0;
            }
        }
        hist_flush(lds, lane, acc);
        double s = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (acc[k] > 1)
                s += lgamma((double)acc[k] + 1.0);
        s = wave_sum(s);
        if (lane == 0)
            a.bits[(uint64_t)j * a.row_blocks + c] = (lgamma((double)n + 258.0) - lg257 - s) * kInvLn2;
    }
}

template <int E>
__global__ void __launch_bounds__(64) k_lag_cost_bytes(LagCostArgs a)
{
    lag_cost_bytes_body<E, 1>(a);
}

template <int E>
__global__ void __launch_bounds__(64) k_lag_order_cost_bytes(LagCostArgs a)
{
    lag_cost_bytes_body<E, REDUX_LAG_ORDER_MAX>(a);
}

} // namespace redux
