// redux_layout_cost.hpp -- layout estimates: the adaptive model's cost of every block of every transformed input, counted
// from the untransformed bytes (gfx950 only).
//
// Layout k = 4 F + log2 E: the byte-plane layout for elements of E = 1, 2, 4, 8 bytes (redux_planes.hpp), behind the delta
// filter when F = 1 (redux_delta.hpp).  A block's adaptive cost A(h, n) depends on its byte counts alone (redux_cost.hpp),
// and the counts of block b of transform_k(input) can be taken from the input: no transformed copy is written.
//
//   k_layout_cost<E, NW>      full frames (E*B bytes -> blocks f*E .. f*E + E - 1), block size and buffer 16-byte multiples.
//                             A workgroup of NW waves walks frames g, g + G, ...; wave w counts filter a.filt[w] (NW = 2:
//                             plain and delta of one frame side by side, so that both read the frame at the same time and the
//                             second read is served by the CU's cache; NW = 1: one of them).  A row is 64 x 16 elements, and a
//                             wave takes 8 / E rows per step (128 bytes per lane, as at E = 8: with one row per step the
//                             loop's fixed cost made E = 1 four times slower than k_block_cost): lane l loads its 16
//                             elements of each row (E 16-byte loads, the next step's in flight while this one counts),
//                             subtracts its predecessor (delta_diff; the element before a lane's
//                             first comes from the lane below, the wave's from the row before, none at a frame start), and
//                             planes_permute leaves it 16 bytes of each plane.  The lanes are E groups of W = 64 / E: through
//                             8 KiB of LDS, group p receives each row's 1 KiB of plane p, 16 E bytes per lane, and counts them
//                             into k_block_cost's lane-private packed u16 counters (32 KiB per wave).  layout_fold sums each
//                             group's W columns apart: lane l ends with bins 2l, 2l+1, 2l+128, 2l+129 of every plane, takes
//                             lgamma of each, and one wave reduction per plane gives the block's f64.
//                             A lane counts 16 E bytes per row, all of which may be one value: the counters are folded
//                             before a step that could carry one past 65,535: at most floor(65535 / (16 E)) rows lie between
//                             two folds -- 4095, 2047, 1023, 511 rows for E = 1, 2, 4, 8 (kLayoutFoldRows), E times sooner
//                             than k_block_cost.
//   k_layout_cost_bytes<E>    everything else -- the short last frame, unaligned buffers, block sizes that are no multiple
//                             of 16: one wave per output block and filter maps each transformed offset t back to its source
//                             (frame of L bytes, N = L / E: p = t / N, i = t % N, byte p of x[i] or of x[i] - x[i-1]; the
//                             L - N E trailing bytes as they are) and counts as k_block_cost does.  Right, not fast.
//
// LDS: a workgroup has NW 40 KiB (E = 1: NW 32), so two workgroups of two waves or four of one -- four waves -- share a CU's
// 160 KiB, the occupancy k_block_cost runs at.  One wave holding both counter sets (64 KiB) would leave two waves per CU.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_cost.hpp"
#include "redux_delta.hpp"

namespace redux {

struct LayoutCostArgs {
    const uint8_t *in;
    uint64_t       in_len;
    uint64_t       nblocks;    // redux_block_count(in_len, block_size)
    uint64_t       nfull;      // frames the fast kernel takes; the byte kernel takes blocks nfull * E ... nblocks
    uint32_t       block_size;
    uint32_t       nfilt;      // filters of this launch: 1 or 2
    uint32_t       filt[2];    // 0 plain, 1 delta
    double        *bits[2];    // f64[nblocks] of each filter's layout
};

// rows (64 lanes x 16 elements) a wave may count between folds: a lane adds at most 16 E to one counter per row
template <int E> constexpr uint32_t kLayoutFoldRows = 65535 / (16 * E);

// every lane's counters -> acc, group by group, the counters back to zero.  Lane l reads rows l and l + 64 (bins 2l, 2l+1 and
// 2l+128, 2l+129); at step (q, k) it reads column ((q + l) mod E) W + (k + l / E) mod W, so the 64 lanes address 64 different
// columns: acc[h][q] belongs to plane (q + l) mod E.
template <int E>
__device__ __forceinline__ void layout_fold(uint32_t *lds, uint32_t lane, uint32_t (&acc)[2][E][2])
{
    constexpr uint32_t W = 64 / E;
    __syncthreads(); // (orders the adds of every lane before the reads)
#pragma unroll
    for (uint32_t h = 0; h < 2; h++) {
        uint32_t *row = lds + (lane + 64 * h) * 64;
#pragma unroll
        for (uint32_t q = 0; q < (uint32_t)E; q++) {
            const uint32_t g = (q + lane) & (E - 1);
            uint32_t       lo = 0, hi = 0; // W lanes * 65,535 < 2^32
            for (uint32_t k = 0; k < W; k++) {
                const uint32_t j = g * W + ((k + lane / E) & (W - 1)), v = row[j];
                row[j] = 0;
                lo += v & 0xFFFF;
                hi += v >> 16;
            }
            acc[h][q][0] += lo; // (a block has at most 2^30 bytes)
            acc[h][q][1] += hi;
        }
    }
    __syncthreads();
}

template <int E, int NW>
__global__ void __launch_bounds__(64 * NW) k_layout_cost(LayoutCostArgs a)
{
    typedef typename DeltaSum<E>::T T;
    constexpr uint32_t W = 64 / E;
    constexpr int      R = 8 / E; // rows per step: a lane loads 128 bytes per step whatever the element size
    __shared__ uint32_t counters[NW][kHistPairs * 64];
    __shared__ uint4    exchange[NW][E > 1 ? 64 * 8 : 1];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool     delta = a.filt[wave] != 0; // (wave-uniform)
    uint32_t      *lds = counters[wave], *col = lds + lane;
    uint4         *xl  = exchange[wave];
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const uint32_t frame_groups = a.block_size / 16;         // 16-element groups of a frame
    const uint32_t rows  = (frame_groups + 63) / 64;
    const double   top   = lgamma((double)a.block_size + 258.0) - lgamma(257.0);
    const uint32_t group = lane / W, member = lane % W;
    // every loop below is uniform over the workgroup: its waves walk the same frame and meet at the same barriers
    for (uint64_t f = blockIdx.x; f < a.nfull; f += gridDim.x) {
        const uint4 *src = (const uint4 *)(a.in + f * (uint64_t)E * a.block_size);
        uint32_t acc[2][E][2];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int q = 0; q < E; q++)
                acc[h][q][0] = acc[h][q][1] = 0;
        uint32_t nxt[R][4 * E];
        auto load = [&](uint32_t row0) { // rows row0 .. row0 + R - 1; a lane past the frame's end loads nothing
#pragma unroll
            for (int u = 0; u < R; u++) {
                const uint32_t i = (row0 + u) * 64 + lane;
#pragma unroll
                for (int k = 0; k < E; k++) {
                    uint4 v = make_uint4(0, 0, 0, 0);
                    if (i < frame_groups)
                        v = src[(uint64_t)i * E + k];
                    nxt[u][4 * k] = v.x; nxt[u][4 * k + 1] = v.y; nxt[u][4 * k + 2] = v.z; nxt[u][4 * k + 3] = v.w;
                }
            }
        };
        load(0);
        T        carry = 0; // the element before the row's first (delta_diff's prev), 0 at the frame's start
        uint32_t since = 0; // rows since the last fold
        for (uint32_t row0 = 0; row0 < rows; row0 += R) {
            uint32_t d[R][4 * E];
#pragma unroll
            for (int u = 0; u < R; u++)
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    d[u][q] = nxt[u][q];
            if (row0 + R < rows) // the next step's loads are in flight while this step counts
                load(row0 + R);
            if (delta) {
#pragma unroll
                for (int u = 0; u < R; u++) { // (rows past the frame's end hold zeros: their differences are not counted)
                    uint32_t cur[4 * E];
#pragma unroll
                    for (int q = 0; q < 4 * E; q++)
                        cur[q] = d[u][q];
                    T last, prev;
                    if constexpr (E == 8) {
                        last  = (uint64_t)cur[4 * E - 1] << 32 | cur[4 * E - 2];
                        prev  = (T)__shfl_up((unsigned long long)last, 1);
                        last  = (T)__shfl((unsigned long long)last, 63);
                    } else {
                        last  = cur[4 * E - 1];
                        prev  = (T)__shfl_up((unsigned int)last, 1);
                        last  = (T)__shfl((unsigned int)last, 63);
                    }
                    if (lane == 0)
                        prev = carry;
                    carry = last;
                    delta_diff<E>(cur, prev, d[u]);
                }
            }
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
                    for (int k = 0; k < E; k++) {
                        const uint32_t pos = ((k + group) & (E - 1)) * W + member;
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
        layout_fold<E>(lds, lane, acc); // (leaves the counters zero for the next frame)
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
            if (lane == 0)
                a.bits[wave][f * E + g] = (top - v) * kInvLn2;
        }
    }
}

// the byte at offset r of the transformed frame that starts at `frame` and has L bytes
template <int E>
__device__ __forceinline__ uint32_t layout_byte(const uint8_t *frame, uint64_t L, uint64_t r, bool delta)
{
    const uint64_t N = L / E;
    if (r >= N * E) // trailing bytes (all of a frame shorter than an element)
        return frame[r];
    const uint64_t p = r / N, i = r - p * N;
    if (!delta)
        return frame[i * E + p];
    uint64_t x = 0, y = 0;
#pragma unroll
    for (int k = 0; k < E; k++) {
        x |= (uint64_t)frame[i * E + k] << (8 * k);
        if (i)
            y |= (uint64_t)frame[(i - 1) * E + k] << (8 * k);
    }
    return (uint32_t)((x - y) >> (8 * p)) & 0xFF;
}

template <int E>
__global__ void __launch_bounds__(64) k_layout_cost_bytes(LayoutCostArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const double   lg257 = lgamma(257.0);
    const uint64_t frame = (uint64_t)E * a.block_size, first = a.nfull * E, nrest = a.nblocks - first;
    for (uint64_t w = blockIdx.x; w < nrest * a.nfilt; w += gridDim.x) { // (wave-uniform)
        const uint32_t fi    = (uint32_t)(w / nrest);
        const uint64_t b     = first + (w - fi * nrest);
        const bool     delta = a.filt[fi] != 0;
        const uint64_t at    = b * a.block_size;
        const uint64_t n     = a.in_len > at ? (a.in_len - at < a.block_size ? a.in_len - at : a.block_size) : 0;
        const uint64_t fbase = at / frame * frame; // (a block lies inside one frame)
        const uint64_t L     = a.in_len - fbase < frame ? a.in_len - fbase : frame;
        unsigned long long acc[4] = {0, 0, 0, 0};
        uint32_t since = 0;
        for (uint64_t o = 0; o < n; o += 64) {
            if (o + lane < n)
                hist_byte(col, layout_byte<E>(a.in + fbase, L, at - fbase + o + lane, delta));
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
            a.bits[fi][b] = (lgamma((double)n + 258.0) - lg257 - s) * kInvLn2;
    }
}

} // namespace redux
