// redux_lag.hpp -- the lagged delta filter for interleaved channels and fixed-width records, fused with the byte-plane
// layout: the zigzag-folded delta filter (redux_delta.hpp, redux_zigzag.hpp) with the predecessor S elements back.
//
//   k_lag_planes<E>          forward, full frames: the forward tile (redux_planes.hpp) with LagForwardHook on the way into
//                            LDS: a chunk's predecessors are the 16 bytes S elements before it, read from memory a second
//                            time (a cache hit), masked at the frame's start; one read, one cached read and one write
//   k_lag_unplanes<E>        inverse, full frames: one workgroup per frame, one row of 256 groups (4096 elements) per
//                            iteration with the next row's plane loads in flight; the row's S running sums are taken in LDS
//                            (below)
//   k_lag_planes_bytes<E>    the byte path, one element per thread: the short last frame, unaligned buffers, blocks not a
//   k_lag_unplanes_bytes<E>  multiple of 16; the inverse one workgroup per frame, 256 elements per iteration
//
// Rule (E, B and the frames as for the delta filter; 1 <= S <= REDUX_LAG_MAX): d[i] = x[i] for i < S,
// d[i] = x[i] - x[i-S] mod 2^(8E) for i >= S; z[i] = the zigzag fold of d[i], always; the L - N*E trailing bytes of a frame
// stay as they are; the layout is applied to the z's (none for E = 1).  The inverse undoes the layout, unfolds and takes
// x[i] = d[i] + x[i-S]: S independent running sums per frame.  Every frame starts afresh.  S >= N folds every element and
// subtracts nothing.  S = 1 is the zigzag filter byte for byte.
//
// The inverse row.  The unfolded row lies in LDS in interleaved order (tile_put).  It is cut into strips: strip s = m*S + q
// (q < S) holds the 16 row elements m*16*S + q + j*S, j < 16, consecutive members of the chain q.  A thread reads its strip
// (16 reads S elements apart; the lanes of a wave read neighbouring elements), takes the prefix in registers, and the
// strips' totals are scanned along their chains: strip s follows strip s - S, so a Hillis-Steele scan with offsets S, 2S,
// 4S ... over the <= 256 + S totals in LDS, one barrier per step (two buffers), no step at all for S >= 256.  The strip's
// offset and the chain's carry are added and the strip written back; the row leaves through tile_stage_out.  The carry is
// the row's last S elements: element q of the next row follows element 4096 - S + q of this one, so the chain's phase
// never has to be worked out.  Wave 3 owns those elements' part of the tile and copies them, in program order with its own
// next tile_put.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include "redux_delta.hpp"

namespace redux {

template <int E> struct LagElem { typedef uint32_t T; };
template <> struct LagElem<1> { typedef uint8_t T; };
template <> struct LagElem<2> { typedef uint16_t T; };
template <> struct LagElem<8> { typedef uint64_t T; };

// 16 bytes at any alignment
struct __attribute__((packed, aligned(1))) LagChunk {
    uint32_t x, y, z, w;
};

// The forward predecessor rule, as the forward tile's stage-in hook: chunk c of the wave's region holds 16 / E elements;
// their predecessors are the 16 bytes lag*E before the chunk, as far as they lie in the chunk's frame.  wsrc: the wave's
// first chunk in memory, r0: the wave's first group in its frame.
template <int E>
struct LagForwardHook {
    const uint8_t *wsrc;
    uint32_t       r0, frame_groups, lag;
    __device__ __forceinline__ uint4 operator()(uint4 v, int, uint32_t c) const
    {
        typedef typename LagElem<E>::T U;
        constexpr uint32_t PER = 16 / E; // elements of a chunk
        uint32_t gi = r0 + c / E;        // the chunk's group in its frame
        if (gi >= frame_groups)
            gi = frame_groups >= 64 ? gi - frame_groups : gi % frame_groups;
        const uint32_t e0 = gi * 16 + c % E * PER; // the chunk's first element in its frame
        const uint8_t *at = wsrc + (uint64_t)c * 16 - (uint64_t)lag * E;
        union {
            uint4 q;
            U     e[PER];
        } p;
        p.q = make_uint4(0, 0, 0, 0);
        if (e0 >= lag) {
            const LagChunk t = *(const LagChunk *)at;
            p.q = make_uint4(t.x, t.y, t.z, t.w);
        } else if (e0 + PER > lag) { // the frame's chunk that S falls into: no byte before the frame is read
#pragma unroll
            for (uint32_t e = 0; e < PER; e++)
                if (e0 + e >= lag)
                    p.e[e] = ((const U *)at)[e];
        }
        if constexpr (E == 8) {
            const uint64_t d0 = ((uint64_t)v.y << 32 | v.x) - ((uint64_t)p.q.y << 32 | p.q.x);
            const uint64_t d1 = ((uint64_t)v.w << 32 | v.z) - ((uint64_t)p.q.w << 32 | p.q.z);
            const uint64_t z0 = d0 << 1 ^ (uint64_t)((int64_t)d0 >> 63), z1 = d1 << 1 ^ (uint64_t)((int64_t)d1 >> 63);
            return make_uint4((uint32_t)z0, (uint32_t)(z0 >> 32), (uint32_t)z1, (uint32_t)(z1 >> 32));
        } else {
            return make_uint4(zigzag_fold_dword<E>(delta_sub<E>(v.x, p.q.x)), zigzag_fold_dword<E>(delta_sub<E>(v.y, p.q.y)),
                              zigzag_fold_dword<E>(delta_sub<E>(v.z, p.q.z)), zigzag_fold_dword<E>(delta_sub<E>(v.w, p.q.w)));
        }
    }
};

// Forward, full frames: the forward tile with the lagged difference and the fold on the way into LDS.
template <int E>
__global__ void __launch_bounds__(256) k_lag_planes(PlanesArgs a, uint32_t lag)
{
    __shared__ uint4 lds[4 * 64 * E];
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x, g0 = t0 + threadIdx.x - (threadIdx.x & 63);
    const LagForwardHook<E> hook = {a.src + g0 * 16 * E, (uint32_t)(g0 % a.frame_groups), a.frame_groups, lag};
    tile_forward<E, PlainForward<E>, 1>(a.src, a.dst, a.groups, t0, a.frame_groups, a.block_size, lds, hook);
}

// Where element p of a row (4 waves x 64 groups x 16 elements) sits in the workgroup's LDS tile, in bytes: tile_put's
// place for it (planes_lds_slot; a wave's 64 groups are a multiple of E, so the rotation by the lane is one by the group).
template <int E>
__device__ __forceinline__ uint32_t lag_lds_byte(uint32_t p)
{
    const uint32_t g = p >> 4, b = (p & 15) * E;
    return ((g * E + (((b >> 4) + g) & (E - 1))) << 4) + (b & 15);
}

// Inverse, full frames: workgroup w walks frames w, w + gridDim.x, ..., one row of 256 groups per iteration (the scheme
// at the head of this file).  A lane past the frame's end holds zeros, their unfold is zeros: the tile is zero there, what
// the sums write there is never staged out, and no row follows a short one.
template <int E>
__global__ void __launch_bounds__(256) k_lag_unplanes(PlanesArgs a, uint32_t lag)
{
    typedef typename LagElem<E>::T U;
    typedef U __attribute__((may_alias)) UA;
    __shared__ uint4 lds[4 * 64 * E];
    __shared__ U     tot[2][512];
    __shared__ U     carry[REDUX_LAG_MAX];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint4   *wl   = lds + wave * 64 * E;
    uint8_t *tile = (uint8_t *)lds;
    const uint32_t S = lag, nstr = (255 + S) / S * S; // strips of a row: <= 256 + S - 1
    uint32_t sq[2], sp[2];                            // the thread's strips tid and tid + 256: chain, first element
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const uint32_t s = threadIdx.x + 256 * u, m = s / S;
        sq[u] = s - m * S;
        sp[u] = s < nstr ? m * 16 * S + sq[u] : 4096;
    }
    const uint64_t nframes = a.groups / a.frame_groups;
    for (uint64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
        const uint64_t fbase = f * (uint64_t)E * a.block_size;
        uint32_t nxt[4 * E];
#pragma unroll
        for (int q = 0; q < 4 * E; q++)
            nxt[q] = 0;
        if (threadIdx.x < a.frame_groups)
            plane_load<E>(a.src + fbase, a.block_size, threadIdx.x, nxt);
        for (uint32_t i0 = 0; i0 < a.frame_groups; i0 += 256) {
            const uint32_t i = i0 + threadIdx.x;
            uint32_t in[4 * E], v[4 * E];
#pragma unroll
            for (int q = 0; q < 4 * E; q++)
                in[q] = nxt[q];
            if ((uint64_t)i + 256 < a.frame_groups) {
                plane_load<E>(a.src + fbase, a.block_size, (uint64_t)i + 256, nxt);
            } else {
#pragma unroll
                for (int q = 0; q < 4 * E; q++)
                    nxt[q] = 0;
            }
            planes_permute<E, true>(in, v);
            zigzag_unfold<E>(v);
            tile_put<E>(wl, lane, v);
            __syncthreads();
            U x[2][16], total[2], incl[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t p = sp[u] + j * S;
                    x[u][j] = p < 4096 ? *(const UA *)(tile + lag_lds_byte<E>(p)) : (U)0;
                }
#pragma unroll
                for (int j = 1; j < 16; j++)
                    x[u][j] = (U)(x[u][j] + x[u][j - 1]);
                total[u] = incl[u] = x[u][15];
            }
            uint32_t cur = 0;
            for (uint32_t off = S; off < nstr; off <<= 1, cur ^= 1) {
#pragma unroll
                for (int u = 0; u < 2; u++)
                    if (threadIdx.x + 256 * u < nstr)
                        tot[cur][threadIdx.x + 256 * u] = incl[u];
                __syncthreads();
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t s = threadIdx.x + 256 * u;
                    if (s >= off && s < nstr)
                        incl[u] = (U)(incl[u] + tot[cur][s - off]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (sp[u] >= 4096)
                    continue;
                const U before = (U)(incl[u] - total[u] + (i0 ? carry[sq[u]] : (U)0));
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    const uint32_t p = sp[u] + j * S;
                    if (p < 4096)
                        *(UA *)(tile + lag_lds_byte<E>(p)) = (U)(x[u][j] + before);
                }
            }
            __syncthreads();
            const uint32_t w0 = i0 + wave * 64; // the wave's first group of the frame
            if (w0 < a.frame_groups) {
                const uint32_t left = a.frame_groups - w0;
                tile_stage_out<E>(wl, (uint4 *)(a.dst + fbase + (uint64_t)w0 * 16 * E), (left < 64 ? left : 64) * E, lane, TileNoHook());
            }
            if (wave == 3) // the row's last S elements lie in wave 3's part of the tile (S <= 256 <= 1024)
                for (uint32_t c = lane; c < S; c += 64)
                    carry[c] = *(const UA *)(tile + lag_lds_byte<E>(4096 - S + c));
        }
    }
}

// ---- the byte path (bytes_forward, bytes_inverse_frame: redux_planes.hpp, redux_delta.hpp) ---------------------------------
// Forward for the thread of source byte o: the thread of an element's first byte does the element, the threads of a frame's
// trailing bytes copy them.
__device__ __forceinline__ void lag_bytes_forward(const uint8_t *src, uint8_t *dst, uint64_t o, uint64_t len, uint32_t E, uint32_t block_size,
                                                  uint32_t lag)
{
    const FramePos f = frame_pos(o, len, E, block_size);
    if (f.r >= f.n * E) {
        dst[o] = src[o];
        return;
    }
    if (f.r % E)
        return;
    const uint64_t i = f.r / E;
    uint64_t x = 0, p = 0;
    for (uint32_t q = 0; q < E; q++) {
        x |= (uint64_t)src[o + q] << (8 * q);
        if (i >= lag)
            p |= (uint64_t)src[o - (uint64_t)lag * E + q] << (8 * q);
    }
    uint64_t d = x - p;
    d = d << 1 ^ (0 - (d >> (8 * E - 1) & 1)); // (the bits above the element's 8*E are dropped below)
    for (uint32_t q = 0; q < E; q++)
        dst[f.base + (uint64_t)q * f.n + i] = (uint8_t)(d >> (8 * q));
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_planes_bytes(PlanesArgs a, uint32_t lag)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x)
        lag_bytes_forward(a.src, a.dst, o, a.len, E, a.block_size, lag);
}

// The inverse of the byte path: the workgroup walks the frame of L bytes at `base`, 256 elements per iteration, one per
// lane, in 64 bits (congruent mod 2^(8E)): a Hillis-Steele scan with offsets S, 2S, ... < 256 through LDS (two buffers, one
// barrier per step), then the chain's carry: element t of an iteration is in the chain of t % S, whose predecessor is
// element 256 - S + t % S of the iteration before (last, two rows alternating by par).  E, S and L are uniform over the
// workgroup, so are the barriers.
__device__ __forceinline__ void lag_bytes_inverse_frame(const uint8_t *src, uint8_t *dst, uint64_t base, uint64_t L, uint32_t E, uint32_t S,
                                                        uint64_t (*buf)[256], uint64_t (*last)[256], uint32_t &par)
{
    const uint64_t n = L / E;
    if (n * E + threadIdx.x < L) // (at most E - 1 trailing bytes)
        dst[base + n * E + threadIdx.x] = src[base + n * E + threadIdx.x];
    const uint32_t from = 256 - S + threadIdx.x % S;
    for (uint64_t i0 = 0; i0 < n; i0 += 256) {
        const uint64_t i = i0 + threadIdx.x;
        uint64_t d = 0;
        if (i < n)
            for (uint32_t q = 0; q < E; q++)
                d |= (uint64_t)src[base + (uint64_t)q * n + i] << (8 * q);
        uint64_t x = d >> 1 ^ (0 - (d & 1));
        uint32_t cur = 0;
        for (uint32_t off = S; off < 256; off <<= 1, cur ^= 1) {
            buf[cur][threadIdx.x] = x;
            __syncthreads();
            if (threadIdx.x >= off)
                x += buf[cur][threadIdx.x - off];
        }
        if (i0)
            x += last[par][from];
        last[par ^ 1][threadIdx.x] = x;
        __syncthreads();
        par ^= 1;
        if (i < n)
            for (uint32_t q = 0; q < E; q++)
                dst[base + i * E + q] = (uint8_t)(x >> (8 * q));
    }
}

// Inverse, any alignment and block size: workgroup w takes frames w, w + gridDim.x, ... of [first, len).
template <int E>
__global__ void __launch_bounds__(256) k_lag_unplanes_bytes(PlanesArgs a, uint32_t lag)
{
    __shared__ uint64_t buf[2][256], last[2][256];
    const uint64_t frame = (uint64_t)E * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    uint32_t par = 0;
    for (uint64_t fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
        const uint64_t base = a.first + fi * frame;
        lag_bytes_inverse_frame(a.src, a.dst, base, a.len - base < frame ? a.len - base : frame, E, lag, buf, last, par);
    }
}

} // namespace redux
