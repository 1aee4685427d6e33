// redux_record_cost.hpp -- record estimates: the adaptive model's cost of every block of the input behind the record layout,
// for a list of (record size, byte delta) candidates, counted from the untransformed bytes (gfx950 only).
//
// Rule: bits[c][b] is k_block_cost's value (redux_cost.hpp) for block b of what k_record_planes / k_record_planes_bytes
// (redux_record.hpp) write for candidate c = (R, F) -- the fresh start of every frame of R B bytes with the first record
// undifferenced, the short last frame of L bytes with its N = L / R records and L - N R trailing bytes included -- and
// nothing else defines it.  A block's adaptive cost depends on its byte counts alone, and in a full frame block p of the
// transformed frame is byte column p of its records: no transformed copy is written.
//
// Frame sampling (redux_record_cost_list.hpp, record_cost_sample): with sample_blocks Q > 0 a candidate costs frames
// 0, T, 2T, ... for its own T, and its row holds the blocks of the selected frames in order.
//
//   k_record_cost        full frames, block size and buffer 16-byte multiples.  A workgroup takes a job (candidate, selected
//                        frame, range of byte columns) and walks the frame alone, as k_record_unplanes does.  The counters
//                        are kRecordCostSlots shared histograms of 256 u32 in LDS (no counter can overflow: a block has at
//                        most 2^30 bytes), 257 dwords apart so that the same byte value of neighbouring columns lies in
//                        neighbouring banks.
//                          R <= 32: the range is all R columns, the frame is read as it lies in aligned 16-byte chunks,
//                          chunk c's byte e belongs to column (16 c + e) mod R, and every column has floor(32 / R) copies
//                          of its histogram, a thread counting into copy (thread mod copies): a constant column at R = 3
//                          spreads over 10 addresses.
//                          R > 32: ranges of 32 columns; an item is (record, 16 bytes of the range), loaded at any
//                          alignment; the last piece of a range of W bytes with W mod 16 != 0 is loaded so that it ENDS with
//                          the range, and its first bytes, which belong to the piece before, are not counted: no byte past
//                          the frame is read.
//                        With F = 1 the 16 bytes R back are read a second time (cache) and subtracted bytewise, masked at the
//                        frame's start as k_record_planes masks them: no byte before the frame is read.  A lane counts its 16
//                        bytes in an order rotated by its lane number, so that the lanes of a wave that hold the same columns
//                        (a table whose every record is the same) add to different columns at the same time.  The job ends
//                        as k_layout_cost does: the copies are summed, lgamma in f64, one wave reduction per column.
//   k_record_cost_bytes  everything else -- the short last frame, unaligned buffers, block sizes that are no multiple of 16:
//                        one wave per (candidate, row block) maps each transformed offset back to its source, as
//                        k_layout_cost_bytes and k_lag_cost_bytes do.  Right, not fast.
//
// The jobs of the candidates of a list differ in number (frames, ranges), so the host passes their running count in the
// kernels' arguments next to the list, and a workgroup finds its candidate by bisection.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_cost.hpp"
#include "redux_record.hpp"
#include "redux_record_cost_list.hpp"

namespace redux {

constexpr uint32_t kRecordCostSlots  = 32;  // shared histograms of a workgroup of k_record_cost
constexpr uint32_t kRecordCostStride = 257; // dwords from one to the next: 256 counters and one dword of padding
constexpr uint32_t kRecordCostPC     = 32;  // byte columns of a range; R <= kRecordCostPC: one range of R columns
constexpr uint32_t kRecordCostWgsPerCu = 4; // resident workgroups of k_record_cost per CU (32.1 KiB of LDS each)

struct RecordCostArgs {
    const uint8_t *in;
    uint64_t       in_len;
    uint64_t       stride;        // f64 from one row of bits to the next: redux_block_count(in_len, block_size)
    double        *bits;          // f64[ncand][stride]
    uint32_t       block_size;
    uint32_t       sample_blocks;
    uint32_t       ncand;
    uint32_t       fast;          // full frames go to k_record_cost (block size and buffer are 16-byte multiples)
    uint64_t       jobs[REDUX_RECORD_COST_MAX + 1]; // of the launched kernel: candidate c has jobs [jobs[c], jobs[c + 1])
    uint16_t       records[REDUX_RECORD_COST_MAX];
    uint8_t        deltas[REDUX_RECORD_COST_MAX];
};
static_assert(sizeof(RecordCostArgs) <= 4096, "the list and the job counts travel in the kernel's arguments");

// the selected frames of candidate R that k_record_cost takes: the full ones (a short frame is the last, and selected last)
REDUX_RECORD_COST_HD inline uint64_t record_cost_fast_frames(uint64_t in_len, uint32_t B, uint32_t R, uint32_t fast,
                                                             const RecordCostSample &sm)
{
    const uint64_t nfull = fast ? in_len / ((uint64_t)R * B) : 0;
    return (nfull + sm.step - 1) / sm.step;
}

// the candidate whose jobs hold `job` (< jobs[ncand]); candidates without jobs are passed over
__device__ __forceinline__ uint32_t record_cost_find(const RecordCostArgs &a, uint64_t job)
{
    uint32_t lo = 0, hi = a.ncand; // jobs[lo] <= job < jobs[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.jobs[mid] <= job)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ln n! = lgamma(n + 1) for a count n >= 2.  Below 16 the log of the exact product; from 16 on Stirling's series to 1 / x^7,
// whose first dropped term is 1 / (1188 x^9) < 2e-14.  k_record_cost ends its jobs with this and not with lgamma: the
// library function's coefficients stayed in registers across the counting loops, 180 VGPRs and two waves a SIMD
__device__ __forceinline__ double record_cost_lnfact(uint32_t n)
{
    double f = 1.0;
    if (n < 16)
        for (uint32_t i = 2; i <= n; i++)
            f *= (double)i;
    const double x = (double)n, l = log(n < 16 ? f : x);
    if (n < 16)
        return l;
    const double r = 1.0 / x, r2 = r * r;
    return (x + 0.5) * l - x + 0.91893853320467274178 + r * (1.0 / 12.0 - r2 * (1.0 / 360.0 - r2 * (1.0 / 1260.0 - r2 * (1.0 / 1680.0))));
}

__global__ void __launch_bounds__(256) k_record_cost(RecordCostArgs a)
{
    __shared__ uint32_t hist[kRecordCostSlots * kRecordCostStride];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t i = tid; i < kRecordCostSlots * kRecordCostStride; i += 256)
        hist[i] = 0;
    __syncthreads();
    const uint32_t B   = a.block_size;
    const double   top = lgamma((double)B + 258.0) - lgamma(257.0);
    const uint32_t rd = (lane >> 2) & 3, rb = lane & 3; // the lane's rotation: dwords of a chunk, bytes of a dword
    // every loop bound below is uniform over the workgroup
    for (uint64_t job = blockIdx.x; job < a.jobs[a.ncand]; job += gridDim.x) {
        const uint32_t c = record_cost_find(a, job);
        const uint32_t R = __builtin_amdgcn_readfirstlane((uint32_t)a.records[c]); // (uniform: the job's values stay scalar)
        const uint32_t F = __builtin_amdgcn_readfirstlane((uint32_t)a.deltas[c]);
        const RecordCostSample sm = record_cost_sample(a.in_len, B, R, a.sample_blocks);
        const bool     split = R > kRecordCostPC;
        const uint32_t nr = split ? (R + kRecordCostPC - 1) / kRecordCostPC : 1;
        const uint64_t local = job - a.jobs[c], k = local / nr;
        const uint32_t p0 = (uint32_t)(local - k * nr) * kRecordCostPC;
        const uint32_t W  = !split ? R : R - p0 < kRecordCostPC ? R - p0 : kRecordCostPC;
        const uint32_t copies  = kRecordCostSlots / W;
        const uint32_t cstride = copies * kRecordCostStride; // dwords from a column's histogram to the next column's
        uint32_t      *mine    = hist + (tid % copies) * kRecordCostStride;
        const uint8_t *frame   = a.in + k * sm.step * (uint64_t)R * B;
        const uint32_t mR = split ? 0 : record_magic(R), dR = split ? 0 : R; // column = n mod R, or n itself in a range

        // counts chunk bytes [lo, 16) of v less p; byte e belongs to column (col0 + e) mod R (a range: col0 + e)
        auto count = [&](uint4 v, uint4 p, uint32_t col0, uint32_t lo) {
            if (F)
                v = record_sub(v, p);
            uint32_t w0 = v.x, w1 = v.y, w2 = v.z, w3 = v.w, t;
            if (rd & 1) { t = w0; w0 = w1; w1 = w2; w2 = w3; w3 = t; }
            if (rd & 2) { t = w0; w0 = w2; w2 = t; t = w1; w1 = w3; w3 = t; }
            const uint32_t w[4] = {w0, w1, w2, w3};
#pragma unroll
            for (uint32_t d = 0; d < 4; d++)
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) {
                    const uint32_t bb = (b + rb) & 3, e = ((d + rd) & 3) * 4 + bb, x = w[d] >> (8 * bb) & 0xFF;
                    const uint32_t n = col0 + e, col = n - __umulhi(n, mR) * dR;
                    if (e >= lo)
                        atomicAdd(mine + col * cstride + x, 1u); // ds_add_u32, no return
                }
        };
        const uint4 zero = make_uint4(0, 0, 0, 0);
        if (!split) { // the frame as it lies: R B / 16 <= 2^31 chunks
            const uint32_t nch = (uint32_t)((uint64_t)R * B / 16), dc = 4096 % R;
            uint32_t col0 = 16 * tid % R;
#pragma unroll 1
            for (uint32_t ch = tid; ch < nch; ch += 256) {
                const uint64_t o  = 16ull * ch;
                const uint8_t *at = frame + o;
                const uint4    v  = *(const uint4 *)at;
                uint4          p  = zero;
                if (F) {
                    if (o >= R) {
                        const LagChunk x = *(const LagChunk *)(at - R);
                        p = make_uint4(x.x, x.y, x.z, x.w);
                    } else if (o + 16 > R) { // the frame's chunk that R falls into: no byte before the frame is read
                        union {
                            uint4   q;
                            uint8_t e[16];
                        } u;
                        u.q = zero;
#pragma unroll
                        for (uint32_t e = 0; e < 16; e++)
                            if (o + e >= R)
                                u.e[e] = at[(int32_t)e - (int32_t)R];
                        p = u.q;
                    }
                }
                count(v, p, col0, 0);
                col0 += dc;
                col0 -= col0 >= R ? R : 0;
            }
        } else { // W bytes of every record in pieces of 16: B npc <= 2^31 items
            const uint32_t npc = (W + 15) >> 4, lgn = npc - 1, nit = B << lgn; // (npc is 1 or 2)
#pragma unroll 1
            for (uint32_t it = tid; it < nit; it += 256) {
                const uint32_t i = it >> lgn, q = it & lgn, nb = W - 16 * q < 16 ? W - 16 * q : 16, lo = 16 - nb;
                const uint8_t *at = frame + (uint64_t)i * R + p0 + 16 * q - lo; // (p0 >= 32: inside the record)
                const LagChunk x  = *(const LagChunk *)at;
                uint4          p  = zero;
                if (F && i) {
                    const LagChunk y = *(const LagChunk *)(at - R);
                    p = make_uint4(y.x, y.y, y.z, y.w);
                }
                count(make_uint4(x.x, x.y, x.z, x.w), p, 16 * q - lo, lo); // (col0 wraps below 0 only for bytes not counted)
            }
        }
        __syncthreads();
        // wave w takes columns w, w + 4, ...; lane l byte values l, l + 64, l + 128, l + 192.  Leaves the counters zero.
        for (uint32_t p = wave; p < W; p += 4) {
            double s = 0;
#pragma unroll 1
            for (uint32_t j = 0; j < 4; j++) {
                uint32_t n = 0;
                for (uint32_t cp = 0; cp < copies; cp++) {
                    uint32_t *at = hist + (p * copies + cp) * kRecordCostStride + lane + 64 * j;
                    n += *at;
                    *at = 0;
                }
                if (n > 1) // (ln 0! = ln 1! = 0)
                    s += record_cost_lnfact(n);
            }
            s = wave_sum(s);
            if (lane == 0)
                a.bits[(uint64_t)c * a.stride + k * R + p0 + p] = (top - s) * kInvLn2;
        }
        __syncthreads();
    }
}

// the byte at offset r of the transformed frame that starts at `frame` and has L bytes (k_record_planes_bytes' rule)
__device__ __forceinline__ uint32_t record_cost_byte(const uint8_t *frame, uint64_t L, uint64_t r, uint32_t R, uint32_t F)
{
    const uint64_t N = L / R;
    if (r >= N * R) // trailing bytes (all of a frame shorter than a record)
        return frame[r];
    const uint64_t p = r / N, i = r - p * N;
    return (uint8_t)(frame[i * R + p] - (F && i ? frame[(i - 1) * R + p] : 0));
}

__global__ void __launch_bounds__(64) k_record_cost_bytes(RecordCostArgs a)
{
    __shared__ uint32_t lds[kHistPairs * 64];
    const uint32_t lane = threadIdx.x;
    uint32_t      *col  = lds + lane;
    for (uint32_t p = 0; p < kHistPairs; p++)
        col[p * 64] = 0;
    __syncthreads();
    const double lg257 = lgamma(257.0);
    for (uint64_t w = blockIdx.x; w < a.jobs[a.ncand]; w += gridDim.x) { // (wave-uniform)
        const uint32_t c = record_cost_find(a, w);
        const uint32_t R = __builtin_amdgcn_readfirstlane((uint32_t)a.records[c]); // (uniform: the job's values stay scalar)
        const uint32_t F = __builtin_amdgcn_readfirstlane((uint32_t)a.deltas[c]);
        const RecordCostSample sm = record_cost_sample(a.in_len, a.block_size, R, a.sample_blocks);
        const uint64_t cc    = record_cost_fast_frames(a.in_len, a.block_size, R, a.fast, sm) * R + (w - a.jobs[c]); // place in the row
        const uint64_t b     = cc / R * sm.step * R + cc % R;                                                        // block of the input
        const uint64_t at    = b * a.block_size;
        const uint64_t n     = a.in_len > at ? (a.in_len - at < a.block_size ? a.in_len - at : a.block_size) : 0;
        const uint64_t frame = (uint64_t)R * a.block_size, fbase = at / frame * frame; // (a block lies inside one frame)
        const uint64_t L     = a.in_len - fbase < frame ? a.in_len - fbase : frame;
        unsigned long long acc[4] = {0, 0, 0, 0};
        uint32_t since = 0;
        for (uint64_t o = 0; o < n; o += 64) {
            if (o + lane < n)
                hist_byte(col, record_cost_byte(a.in + fbase, L, at - fbase + o + lane, R, F));
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
            a.bits[(uint64_t)c * a.stride + cc] = (lgamma((double)n + 258.0) - lg257 - s) * kInvLn2;
    }
}

} // namespace redux
