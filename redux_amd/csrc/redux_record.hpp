// redux_record.hpp -- the record layout for fixed-width structs: the byte-plane layout for a record of R bytes, 2 <= R <=
// REDUX_RECORD_MAX, with an optional byte delta against the record before.  R and the filter flag are kernel arguments.
//
//   k_record_planes          forward, full frames: a tile of T records goes through LDS in interleaved order (16-byte
//                            accesses, the 16 bytes R back read a second time from cache for the delta, masked at the frame's
//                            start); a work item gathers 16 records of one byte column from LDS and writes them to the plane
//   k_record_unplanes        inverse, full frames: a workgroup owns a range of byte columns of a frame and walks the frame's
//                            records tile by tile; a work item loads 16 records of a column from the plane, takes their
//                            running sum in registers, the items' totals are scanned along the column in LDS, the column's
//                            carry from the tile before is added, and the bytes are scattered into the LDS tile in
//                            interleaved order, which leaves in 16-byte accesses
//   k_record_planes_bytes    the byte path under the frame index rule: the short last frame, unaligned buffers, blocks not a
//   k_record_unplanes_bytes  multiple of 16; the inverse sums with one thread per (frame, column)
//
// Rule (B = block size): frames of R*B bytes, only the last may be shorter; a frame of L bytes holds N = L / R records;
// with the delta d[i][p] = x[i][p] - x[i-1][p] mod 256 for i >= 1, d[0][p] = x[0][p], without it d = x; byte p of record i
// moves to frame offset p*N + i; the L - N*R trailing bytes stay where they are.  Every frame starts afresh.  Without the
// delta and for R = 2, 4, 8 this is what k_planes<R> writes.
//
// The LDS tile holds records in interleaved order, 16 records (16*W bytes, W the tile's row width) a group.  A column
// access has lanes 16 records apart: 4*W dwords, which for even W is a multiple of 8 dwords and lands the lanes of a wave
// on few banks.  So for even W every group is followed by 16 bytes of padding: the stride is 4*(W + 1) dwords, 4 times an
// odd number, and 8 neighbouring groups lie on 8 different sets of 4 banks (16 with 64 banks).  Chunks of 16 bytes never
// straddle a group, so the interleaved side keeps its aligned 16-byte LDS accesses.
//
// The inverse's decomposition.  A frame's R column sums are independent, so a workgroup takes (frame, column range) and
// walks the frame alone: no workspace, no second pass, one read and one write per byte.  With many frames the range is all R
// columns and the interleaved side leaves as one contiguous run per tile.  With few frames (R*B large) the host cuts the
// columns into ranges of PC, a multiple of 16 that is at least 64, so that every CU has work; a range's rows then leave in
// pieces of 16 bytes, PC contiguous bytes per record.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_lag.hpp"

namespace redux {

constexpr uint32_t kRecordLdsBytes = 33792; // the tile: T records of W bytes and their padding
constexpr uint32_t kRecordItems    = 2048;  // work items (16 records of a column) of an inverse tile: 8 per thread

struct RecordArgs {
    const uint8_t *src;
    uint8_t       *dst;
    uint64_t       nfull;      // full frames of the fast path
    uint32_t       block_size;
    uint32_t       R;
    uint32_t       delta;
    uint32_t       lgT;        // fast kernels: a tile is 1 << lgT records (>= 16)
    uint32_t       PC;         // inverse: byte columns of a workgroup, R or a multiple of 16
    uint64_t       first, len; // byte kernels: bytes [first, len) of the whole buffer
};

// n / d for n < 2^24 and 1 <= d <= 2^8 by the reciprocal m = record_magic(d): m*d - 2^32 <= d, so the error stays below 1
__device__ __forceinline__ uint32_t record_magic(uint32_t d) { return d > 1 ? 0xFFFFFFFFu / d + 1 : 0; }
__device__ __forceinline__ uint32_t record_div(uint32_t n, uint32_t d, uint32_t m) { return d > 1 ? __umulhi(n, m) : n; }

__device__ __forceinline__ uint4 record_sub(uint4 a, uint4 b)
{
    return make_uint4(delta_sub<1>(a.x, b.x), delta_sub<1>(a.y, b.y), delta_sub<1>(a.z, b.z), delta_sub<1>(a.w, b.w));
}

// Forward, full frames: workgroup w takes tiles w, w + gridDim.x, ... of nfull * ceil(B / T).
__global__ void __launch_bounds__(256) k_record_planes(RecordArgs a)
{
    __shared__ uint4 lds[kRecordLdsBytes / 16];
    uint8_t *tile = (uint8_t *)lds;
    const uint32_t R = a.R, B = a.block_size, T = 1u << a.lgT, lgG = a.lgT - 4, G = 1u << lgG;
    const uint32_t tpf = (B + T - 1) >> a.lgT, pad = R & 1 ? 0 : 16, mR = record_magic(R);
    const uint64_t ntiles = a.nfull * tpf;
    for (uint64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const uint64_t f  = t / tpf;
        const uint32_t i0 = (uint32_t)(t - f * tpf) << a.lgT, Tn = B - i0 < T ? B - i0 : T, Gn = Tn >> 4;
        const uint64_t fbase = f * (uint64_t)R * B;
        const uint8_t *in = a.src + fbase + (uint64_t)i0 * R;
        const uint32_t nch = Gn * R; // the tile's 16-byte chunks
        for (uint32_t c = threadIdx.x; c < nch; c += 256) {
            const uint8_t *at = in + 16 * c;
            uint4 v = *(const uint4 *)at;
            if (a.delta) {
                union {
                    uint4   q;
                    uint8_t e[16];
                } p;
                p.q = make_uint4(0, 0, 0, 0);
                if (i0 || 16 * c >= R) {
                    const LagChunk x = *(const LagChunk *)(at - R);
                    p.q = make_uint4(x.x, x.y, x.z, x.w);
                } else if (16 * c + 16 > R) { // the frame's chunk that R falls into: no byte before the frame is read
#pragma unroll
                    for (uint32_t e = 0; e < 16; e++)
                        if (16 * c + e >= R)
                            p.e[e] = at[(int32_t)e - (int32_t)R];
                }
                v = record_sub(v, p.q);
            }
            *(uint4 *)(tile + 16 * c + pad * record_div(c, R, mR)) = v;
        }
        __syncthreads();
        const uint32_t nit = R << lgG;
        for (uint32_t w = threadIdx.x; w < nit; w += 256) {
            const uint32_t p = w >> lgG, j = w & (G - 1);
            if (j >= Gn)
                continue;
            const uint8_t *at = tile + j * (16 * R + pad) + p;
            uint32_t o[4];
#pragma unroll
            for (uint32_t d = 0; d < 4; d++)
                o[d] = (uint32_t)at[4 * d * R] | (uint32_t)at[(4 * d + 1) * R] << 8 | (uint32_t)at[(4 * d + 2) * R] << 16 |
                       (uint32_t)at[(4 * d + 3) * R] << 24;
            *(uint4 *)(a.dst + fbase + (uint64_t)p * B + i0 + 16 * j) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
    }
}

// Inverse, full frames: gridDim.x is a multiple of the column ranges nr = ceil(R / PC); workgroup w takes range w % nr of
// frames w / nr, w / nr + gridDim.x / nr, ...  Work item w of a tile is 16 records of one column: column w >> lgG of the
// range, group w & (G - 1) of the tile; a thread holds up to 8 of them across the scan.
__global__ void __launch_bounds__(256) k_record_unplanes(RecordArgs a)
{
    __shared__ uint4   lds[kRecordLdsBytes / 16];
    __shared__ uint8_t tot[2][kRecordItems];
    __shared__ uint8_t carry[2][REDUX_RECORD_MAX];
    uint8_t *tile = (uint8_t *)lds;
    const uint32_t R = a.R, B = a.block_size, T = 1u << a.lgT, lgG = a.lgT - 4, G = 1u << lgG;
    const uint32_t nr = (R + a.PC - 1) / a.PC, p0 = blockIdx.x % nr * a.PC, W = R - p0 < a.PC ? R - p0 : a.PC;
    const bool     split = nr > 1;
    const uint32_t Wl = split ? (W + 15) & ~15u : W, pad = Wl & 1 ? 0 : 16; // the tile's row width
    const uint32_t npc = Wl >> 4, mW = record_magic(Wl), mN = record_magic(npc);
    uint32_t par = 0;
    for (uint64_t f = blockIdx.x / nr; f < a.nfull; f += gridDim.x / nr) {
        const uint64_t fbase = f * (uint64_t)R * B;
        for (uint32_t i0 = 0; i0 < B; i0 += T) {
            const uint32_t Tn = B - i0 < T ? B - i0 : T, Gn = Tn >> 4, nit = W << lgG;
            uint32_t v[8][4], incl[8];
            // item u of the thread: is it one of the tile's (the last tile of a frame may hold fewer groups)
            const auto ok = [&](int u) { return threadIdx.x + 256 * u < nit && ((threadIdx.x + 256 * u) & (G - 1)) < Gn; };
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t w = threadIdx.x + 256 * u, p = w >> lgG, j = w & (G - 1);
                uint4 x = make_uint4(0, 0, 0, 0);
                if (ok(u))
                    x = *(const uint4 *)(a.src + fbase + (uint64_t)(p0 + p) * B + i0 + 16 * j);
                v[u][0] = x.x; v[u][1] = x.y; v[u][2] = x.z; v[u][3] = x.w;
            }
            if (a.delta) {
#pragma unroll
                for (int u = 0; u < 8; u++)
                    incl[u] = delta_prefix<1>(v[u]); // (the items' totals stay in their last bytes)
                uint32_t cur = 0;
                for (uint32_t off = 1; off < Gn; off <<= 1, cur ^= 1) {
#pragma unroll
                    for (int u = 0; u < 8; u++)
                        if (ok(u))
                            tot[cur][threadIdx.x + 256 * u] = (uint8_t)incl[u];
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        const uint32_t w = threadIdx.x + 256 * u;
                        if (ok(u) && (w & (G - 1)) >= off)
                            incl[u] += tot[cur][w - off];
                    }
                }
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const uint32_t w = threadIdx.x + 256 * u, p = w >> lgG, j = w & (G - 1);
                    if (!ok(u))
                        continue;
                    delta_offset<1>(v[u], incl[u] - (v[u][3] >> 24) + (i0 ? carry[par][p] : 0u));
                    if (j == Gn - 1) // the column's last record of the tile: the next tile's carry
                        carry[par ^ 1][p] = (uint8_t)(v[u][3] >> 24);
                }
                par ^= 1;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const uint32_t w = threadIdx.x + 256 * u, p = w >> lgG, j = w & (G - 1);
                if (!ok(u))
                    continue;
                uint8_t *at = tile + j * (16 * Wl + pad) + p;
#pragma unroll
                for (uint32_t k = 0; k < 16; k++)
                    at[k * Wl] = (uint8_t)(v[u][k >> 2] >> (8 * (k & 3)));
            }
            __syncthreads();
            uint8_t *out = a.dst + fbase + (uint64_t)i0 * R + p0;
            if (!split) { // the tile's rows are one contiguous run
                const uint32_t nch = Gn * R;
                for (uint32_t c = threadIdx.x; c < nch; c += 256)
                    *(uint4 *)(out + 16 * c) = *(const uint4 *)(tile + 16 * c + pad * record_div(c, Wl, mW));
            } else { // W bytes of every record, in pieces of 16
                const uint32_t nps = Tn * npc;
                for (uint32_t it = threadIdx.x; it < nps; it += 256) {
                    const uint32_t i = record_div(it, npc, mN), q = it - i * npc, nb = W - 16 * q < 16 ? W - 16 * q : 16;
                    const uint8_t *at = tile + i * Wl + (i >> 4) * pad + 16 * q;
                    uint8_t       *o  = out + (uint64_t)i * R + 16 * q;
                    if (nb == 16) {
                        const uint4 x = *(const uint4 *)at;
                        *(LagChunk *)o = LagChunk{x.x, x.y, x.z, x.w};
                    } else {
                        for (uint32_t e = 0; e < nb; e++)
                            o[e] = at[e];
                    }
                }
            }
            __syncthreads();
        }
    }
}

// ---- the byte path -----------------------------------------------------------------------------------------------------
// Forward, one thread per source byte of [first, len): any alignment, any block size.
__global__ void __launch_bounds__(256) k_record_planes_bytes(RecordArgs a)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x) {
        const FramePos f = frame_pos(o, a.len, a.R, a.block_size);
        if (f.r >= f.n * a.R) {
            a.dst[o] = a.src[o];
            continue;
        }
        const uint64_t i = f.r / a.R, p = f.r - i * a.R;
        a.dst[f.base + p * f.n + i] = (uint8_t)(a.src[o] - (a.delta && i ? a.src[o - a.R] : 0));
    }
}

// Inverse: without the delta one thread per destination byte; with it one thread per (frame, column) of [first, len), which
// walks the column's running sum, and one per frame for the trailing bytes.
__global__ void __launch_bounds__(256) k_record_unplanes_bytes(RecordArgs a)
{
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    if (!a.delta) {
        for (uint64_t o = a.first + t0; o < a.len; o += step) {
            const FramePos f = frame_pos(o, a.len, a.R, a.block_size);
            a.dst[o] = a.src[f.base + frame_src<true>(f, a.R)];
        }
        return;
    }
    const uint64_t frame = (uint64_t)a.R * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    for (uint64_t w = t0; w < nframes * a.R; w += step) {
        const uint64_t fi = w / a.R, p = w - fi * a.R, base = a.first + fi * frame;
        const uint64_t L = a.len - base < frame ? a.len - base : frame, n = L / a.R;
        uint8_t x = 0;
        for (uint64_t i = 0; i < n; i++) {
            x = (uint8_t)(x + a.src[base + p * n + i]);
            a.dst[base + i * a.R + p] = x;
        }
        if (p == 0)
            for (uint64_t o = base + n * a.R; o < base + L; o++)
                a.dst[o] = a.src[o];
    }
}

} // namespace redux
