// redux_lag.hpp -- the lagged delta filter for interleaved channels and fixed-width records, and its higher orders, fused
// with the byte-plane layout: the zigzag-folded delta filter (redux_delta.hpp, redux_zigzag.hpp) with the predecessor S
// elements back, applied K times, K the order, 1 <= K <= REDUX_LAG_ORDER_MAX.  A sampled, band-limited signal is locally a
// low-degree polynomial, and the K-th difference removes one of degree K - 1 (FLAC's fixed predictors of order 2 and 3).
//
//   k_lag_planes<E>          forward, full frames: the forward tile (redux_planes.hpp) with LagForwardHook on the way into
//   k_lag_order_planes<E>    LDS: a chunk's K predecessors are the 16 bytes S, 2S .. KS elements before it, read from memory
//                            a second time (cache hits), each masked on its own at the frame's start
//   k_lag_unplanes<E>        inverse, full frames: one workgroup per frame, one row of 256 groups (4096 elements) per
//   k_lag_order_unplanes<E>  iteration with the next row's plane loads in flight; the stage that takes the row's S running
//                            sums in LDS (below) runs K times
//   k_lag_[order_]planes_bytes<E>    the byte path, one element per thread: the short last frame, unaligned buffers, blocks
//   k_lag_[order_]unplanes_bytes<E>  not a multiple of 16; the inverse one workgroup per frame, K passes of a 256-element
//                                    scan per iteration
//
// Both families share the predecessor rule, the subtract and the fold (lag_pred, lag_sub, lag_fold), and one body each for
// the forward tile (with LagForwardHook) and for the inverse byte path, templated on KMAX, the highest order the instance can
// run: the k_lag_* kernels are the bodies at KMAX = 1 and take no order, the k_lag_order_* kernels at KMAX =
// REDUX_LAG_ORDER_MAX.  A body reads KMAX in one line, K = KMAX == 1 ? 1 : order, and in the size of its per-level arrays:
// at KMAX = 1 the level loop and the further predecessors fold away.  Two roles keep a body per family, because the shared
// one was slower on the GPU than the parent's (profiles/lag_bodies.txt): the inverse row (k_lag_unplanes,
// k_lag_order_unplanes: 1.4 to 2.2 % at E = 4 and 8) and the forward byte path (lag_bytes_forward, lag_order_bytes_forward:
// 1.2 to 1.7 times).
//
// Rule (E, B and the frames as for the delta filter; 1 <= S <= REDUX_LAG_MAX), with x[j] = 0 for j < 0:
//   d[i] = sum over j = 0 .. K of (-1)^j C(K, j) x[i - j S]  mod 2^(8E)
// which is the lag-S difference d[i] = x[i] - x[i-S] (d[i] = x[i] for i < S) applied K times, each application leaving its
// first S elements as they are.  z[i] is the zigzag fold of d[i], always; the L - N*E trailing bytes of a frame stay as they
// are; the layout is applied to the z's (none for E = 1).  The inverse undoes the layout, unfolds and takes the S running
// sums of the frame, x[i] = d[i] + x[i-S], K times.  Every frame starts afresh; terms before the frame are zero, so any S
// and K are legal for any N.  S >= N folds every element and subtracts nothing.  S = 1, K = 1 is the zigzag filter byte for
// byte.
//
// Forward.  With p1, p2, p3 the masked predecessors (zero where they lie before the frame): t0 = v - p1, t1 = p1 - p2,
// t2 = p2 - p3; d = t0 for K = 1, t0 - t1 for K = 2 and (t0 - t1) - (t1 - t2) for K = 3, all with the packed subtract of
// the delta filter.
//
// The inverse row.  The unfolded row lies in LDS in interleaved order (tile_put).  It is cut into strips: strip s = m*S + q
// (q < S) holds the 16 row elements m*16*S + q + j*S, j < 16, consecutive members of the chain q.  A thread reads its strip
// (16 reads S elements apart; the lanes of a wave read neighbouring elements), takes the prefix in registers, and the
// strips' totals are scanned along their chains: strip s follows strip s - S, so a Hillis-Steele scan with offsets S, 2S,
// 4S ... over the <= 256 + S totals in LDS, one barrier per step (two buffers), no step at all for S >= 256.  The strip's
// offset and the chain's carry are added and the strip written back.  Level l = 0 .. K - 1 does this on the tile as level
// l - 1 left it; the row leaves through tile_stage_out.  carry[l] is the row's last S elements as level l leaves them:
// element q of the next row follows element 4096 - S + q of this one, so the chain's phase never has to be worked out.  An
// intermediate level's tile is overwritten by the next level, so its carry is copied between two barriers of its own; the
// last level's stays in the tile until wave 3's next tile_put: wave 3 owns those elements' part of the tile and copies
// them, in program order with its own next tile_put.
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

// The predecessor rule: the 16 bytes `back` elements before a chunk whose first element in its frame is e0, `at` their
// address: the whole chunk, nothing (zeros), or element by element in the frame's one chunk that `back` falls into.  No byte
// before the frame is read.
template <int E>
__device__ __forceinline__ uint4 lag_pred(const uint8_t *at, uint32_t e0, uint32_t back)
{
    typedef typename LagElem<E>::T U;
    constexpr uint32_t PER = 16 / E; // elements of a chunk
    union {
        uint4 q;
        U     e[PER];
    } p;
    p.q = make_uint4(0, 0, 0, 0);
    if (e0 >= back) {
        const LagChunk t = *(const LagChunk *)at;
        p.q = make_uint4(t.x, t.y, t.z, t.w);
    } else if (e0 + PER > back) {
#pragma unroll
        for (uint32_t e = 0; e < PER; e++)
            if (e0 + e >= back)
                p.e[e] = ((const U *)at)[e];
    }
    return p.q;
}

// a - b element by element
template <int E>
__device__ __forceinline__ uint4 lag_sub(uint4 a, uint4 b)
{
    if constexpr (E == 8) {
        const uint64_t d0 = ((uint64_t)a.y << 32 | a.x) - ((uint64_t)b.y << 32 | b.x);
        const uint64_t d1 = ((uint64_t)a.w << 32 | a.z) - ((uint64_t)b.w << 32 | b.z);
        return make_uint4((uint32_t)d0, (uint32_t)(d0 >> 32), (uint32_t)d1, (uint32_t)(d1 >> 32));
    } else {
        return make_uint4(delta_sub<E>(a.x, b.x), delta_sub<E>(a.y, b.y), delta_sub<E>(a.z, b.z), delta_sub<E>(a.w, b.w));
    }
}

// the zigzag fold of a chunk's elements
template <int E>
__device__ __forceinline__ uint4 lag_fold(uint4 d)
{
    if constexpr (E == 8) {
        const uint64_t d0 = (uint64_t)d.y << 32 | d.x, d1 = (uint64_t)d.w << 32 | d.z;
        const uint64_t z0 = d0 << 1 ^ (uint64_t)((int64_t)d0 >> 63), z1 = d1 << 1 ^ (uint64_t)((int64_t)d1 >> 63);
        return make_uint4((uint32_t)z0, (uint32_t)(z0 >> 32), (uint32_t)z1, (uint32_t)(z1 >> 32));
    } else {
        return make_uint4(zigzag_fold_dword<E>(d.x), zigzag_fold_dword<E>(d.y), zigzag_fold_dword<E>(d.z), zigzag_fold_dword<E>(d.w));
    }
}

// the folded K-th lagged difference of a chunk v with its masked predecessors p1, p2, p3 already loaded (the forward scheme
// at the head of this file, as LagForwardHook forms it; p2 and p3 are not looked at below their order): the estimates, whose
// loads are a step ahead (redux_lag_cost.hpp)
template <int E>
__device__ __forceinline__ uint4 lag_diff(uint4 v, uint4 p1, uint4 p2, uint4 p3, uint32_t K)
{
    uint4 d = lag_sub<E>(v, p1);
    if (K >= 2) {
        const uint4 t1 = lag_sub<E>(p1, p2);
        d = lag_sub<E>(d, t1);
        if (K >= 3)
            d = lag_sub<E>(d, lag_sub<E>(t1, lag_sub<E>(p2, p3)));
    }
    return lag_fold<E>(d);
}

// The forward rule as the forward tile's stage-in hook: chunk c of the wave's region holds 16 / E elements; predecessor j
// is the 16 bytes j*lag*E before the chunk, as far as they lie in the chunk's frame.  wsrc: the wave's first chunk in
// memory, r0: the wave's first group in its frame.
template <int E, int KMAX>
struct LagForwardHook {
    const uint8_t *wsrc;
    uint32_t       r0, frame_groups, lag, order;
    __device__ __forceinline__ uint4 operator()(uint4 v, int, uint32_t c) const
    {
        const uint32_t K = KMAX == 1 ? 1 : order;
        constexpr uint32_t PER = 16 / E; // elements of a chunk
        uint32_t gi = r0 + c / E;        // the chunk's group in its frame
        if (gi >= frame_groups)
            gi = frame_groups >= 64 ? gi - frame_groups : gi % frame_groups;
        const uint32_t e0 = gi * 16 + c % E * PER; // the chunk's first element in its frame
        const uint8_t *at = wsrc + (uint64_t)c * 16;
        const uint64_t step = (uint64_t)lag * E;
        const uint4 p1 = lag_pred<E>(at - step, e0, lag);
        uint4 d = lag_sub<E>(v, p1);
        // lag_diff's chain with each further predecessor loaded only at its order.  (Through lag_diff with p2 and p3 loaded
        // ahead, k_lag_order_planes<2, 4, 8> took 36 SGPRs for 32 and 0.5 to 1.6 % longer; through a lag_diff that fetches
        // them by callback, k_lag_order_cost<1, 2, 8> lost the parent's instructions.)
        if (K >= 2) {
            const uint4 p2 = lag_pred<E>(at - 2 * step, e0, 2 * lag);
            const uint4 t1 = lag_sub<E>(p1, p2);
            d = lag_sub<E>(d, t1);
            if (K >= 3) {
                const uint4 p3 = lag_pred<E>(at - 3 * step, e0, 3 * lag);
                d = lag_sub<E>(d, lag_sub<E>(t1, lag_sub<E>(p2, p3)));
            }
        }
        return lag_fold<E>(d);
    }
};

// Forward, full frames: the forward tile with the K-th lagged difference and the fold on the way into LDS.
template <int E, int KMAX>
__device__ __forceinline__ void lag_planes_body(PlanesArgs a, uint32_t lag, uint32_t order)
{
    __shared__ uint4 lds[4 * 64 * E];
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x, g0 = t0 + threadIdx.x - (threadIdx.x & 63);
    const LagForwardHook<E, KMAX> hook = {a.src + g0 * 16 * E, (uint32_t)(g0 % a.frame_groups), a.frame_groups, lag, order};
    tile_forward<E, PlainForward<E>, 1>(a.src, a.dst, a.groups, t0, a.frame_groups, a.block_size, lds, hook);
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_planes(PlanesArgs a, uint32_t lag)
{
    lag_planes_body<E, 1>(a, lag, 1);
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_order_planes(PlanesArgs a, uint32_t lag, uint32_t order)
{
    lag_planes_body<E, REDUX_LAG_ORDER_MAX>(a, lag, order);
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

// (k_lag_unplanes with its stage in a loop over the levels and a carry per level: a body of its own, see the head of this
// file.)
// Inverse, full frames: workgroup w walks frames w, w + gridDim.x, ..., one row of 256 groups per iteration, K levels per
// row (the scheme at the head of this file).  A lane past the frame's end holds zeros, their unfold is zeros: the tile is
// zero there, what the sums write there is never staged out, and no row follows a short one.
template <int E>
__global__ void __launch_bounds__(256) k_lag_order_unplanes(PlanesArgs a, uint32_t lag, uint32_t order)
{
    typedef typename LagElem<E>::T U;
    typedef U __attribute__((may_alias)) UA;
    __shared__ uint4 lds[4 * 64 * E];
    __shared__ U     tot[2][512];
    __shared__ U     carry[REDUX_LAG_ORDER_MAX][REDUX_LAG_MAX];
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
            {
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
            }
            __syncthreads();
#pragma unroll 1
            for (uint32_t l = 0; l < order; l++) {
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
                    const U before = (U)(incl[u] - total[u] + (i0 ? carry[l][sq[u]] : (U)0));
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        const uint32_t p = sp[u] + j * S;
                        if (p < 4096)
                            *(UA *)(tile + lag_lds_byte<E>(p)) = (U)(x[u][j] + before);
                    }
                }
                __syncthreads(); // the level's row is whole, and every read of carry[l] is done
                if (l + 1 < order) {
                    // the next level overwrites the tile: the level's carry leaves it now, and before the next write-back
                    for (uint32_t c = threadIdx.x; c < S; c += 256)
                        carry[l][c] = *(const UA *)(tile + lag_lds_byte<E>(4096 - S + c));
                    __syncthreads();
                }
            }
            const uint32_t w0 = i0 + wave * 64; // the wave's first group of the frame
            if (w0 < a.frame_groups) {
                const uint32_t left = a.frame_groups - w0;
                tile_stage_out<E>(wl, (uint4 *)(a.dst + fbase + (uint64_t)w0 * 16 * E), (left < 64 ? left : 64) * E, lane, TileNoHook());
            }
            if (wave == 3) // the row's last S elements lie in wave 3's part of the tile (S <= 256 <= 1024)
                for (uint32_t c = lane; c < S; c += 64)
                    carry[order - 1][c] = *(const UA *)(tile + lag_lds_byte<E>(4096 - S + c));
        }
    }
}

// ---- the byte path (bytes_forward, bytes_inverse_frame: redux_planes.hpp, redux_delta.hpp) ---------------------------------
// (Two forward functions: the order's binomial loop at K = 1 took 1.3 to 1.7 times the lag filter's own form on the GPU at
// E = 1, and without its early exit the higher orders took 1.2 to 1.3 times theirs at E = 4: profiles/lag_bodies.txt.)
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

// Forward for the thread of source byte o: the thread of an element's first byte does the element in 64 bits (congruent
// mod 2^(8E)), the threads of a frame's trailing bytes copy them.
__device__ __forceinline__ void lag_order_bytes_forward(const uint8_t *src, uint8_t *dst, uint64_t o, uint64_t len, uint32_t E,
                                                        uint32_t block_size, uint32_t lag, uint32_t order)
{
    const FramePos f = frame_pos(o, len, E, block_size);
    if (f.r >= f.n * E) {
        dst[o] = src[o];
        return;
    }
    if (f.r % E)
        return;
    const uint64_t i = f.r / E;
    uint64_t d = 0;
    int64_t  coef = 1; // (-1)^j C(K, j)
    for (uint32_t j = 0; j <= order && i >= (uint64_t)j * lag; j++) {
        uint64_t x = 0;
        for (uint32_t q = 0; q < E; q++)
            x |= (uint64_t)src[o - (uint64_t)j * lag * E + q] << (8 * q);
        d += (uint64_t)coef * x;
        coef = -coef * (int64_t)(order - j) / (int64_t)(j + 1);
    }
    d = d << 1 ^ (0 - (d >> (8 * E - 1) & 1)); // (the bits above the element's 8*E are dropped below)
    for (uint32_t q = 0; q < E; q++)
        dst[f.base + (uint64_t)q * f.n + i] = (uint8_t)(d >> (8 * q));
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_order_planes_bytes(PlanesArgs a, uint32_t lag, uint32_t order)
{
    for (uint64_t o = a.first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; o < a.len; o += (uint64_t)gridDim.x * blockDim.x)
        lag_order_bytes_forward(a.src, a.dst, o, a.len, E, a.block_size, lag, order);
}

// The inverse of the byte path: the workgroup walks the frame of L bytes at `base`, 256 elements per iteration, one per
// lane, in 64 bits (congruent mod 2^(8E)).  Level l < K: a Hillis-Steele scan with offsets S, 2S, ... < 256 through LDS (two
// buffers, one barrier per step), then the chain's carry: element t of an iteration is in the chain of t % S, whose
// predecessor is element 256 - S + t % S of the iteration before as level l left it (last[l], two rows alternating by par).
// E, S, K and L are uniform over the workgroup, so are the barriers.
__device__ __forceinline__ void lag_bytes_inverse_frame(const uint8_t *src, uint8_t *dst, uint64_t base, uint64_t L, uint32_t E, uint32_t S,
                                                        uint32_t K, uint64_t (*buf)[256], uint64_t (*last)[2][256], uint32_t &par)
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
        for (uint32_t l = 0; l < K; l++) {
            uint32_t cur = 0;
            for (uint32_t off = S; off < 256; off <<= 1, cur ^= 1) {
                buf[cur][threadIdx.x] = x;
                __syncthreads();
                if (threadIdx.x >= off)
                    x += buf[cur][threadIdx.x - off];
            }
            if (i0)
                x += last[l][par][from];
            last[l][par ^ 1][threadIdx.x] = x;
            __syncthreads();
        }
        par ^= 1;
        if (i < n)
            for (uint32_t q = 0; q < E; q++)
                dst[base + i * E + q] = (uint8_t)(x >> (8 * q));
    }
}

// Inverse, any alignment and block size: workgroup w takes frames w, w + gridDim.x, ... of [first, len).
template <int E, int KMAX>
__device__ __forceinline__ void lag_unplanes_bytes_body(PlanesArgs a, uint32_t lag, uint32_t order)
{
    __shared__ uint64_t buf[2][256], last[KMAX][2][256];
    const uint32_t K = KMAX == 1 ? 1 : order;
    const uint64_t frame = (uint64_t)E * a.block_size, nframes = (a.len - a.first + frame - 1) / frame;
    uint32_t par = 0;
    for (uint64_t fi = blockIdx.x; fi < nframes; fi += gridDim.x) {
        const uint64_t base = a.first + fi * frame;
        lag_bytes_inverse_frame(a.src, a.dst, base, a.len - base < frame ? a.len - base : frame, E, lag, K, buf, last, par);
    }
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_unplanes_bytes(PlanesArgs a, uint32_t lag)
{
    lag_unplanes_bytes_body<E, 1>(a, lag, 1);
}

template <int E>
__global__ void __launch_bounds__(256) k_lag_order_unplanes_bytes(PlanesArgs a, uint32_t lag, uint32_t order)
{
    lag_unplanes_bytes_body<E, REDUX_LAG_ORDER_MAX>(a, lag, order);
}

} // namespace redux
