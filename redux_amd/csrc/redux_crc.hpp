// redux_crc.hpp -- CRC-32 (ISO-HDLC: the zlib / gzip / PNG CRC) of every block of a device buffer.
//
// The checksum of block b is zlib.crc32 of the ORIGINAL bytes x[b*B .. min((b+1)*B, len)); an empty block has CRC 0.
// Reflected polynomial 0xEDB88320, init and xorout 0xFFFFFFFF.  gfx950 has no CRC or carry-less-multiply instruction, so
// the kernel uses the linearity of CRC over GF(2):
//
//   Z_n(r)      = the register r advanced through n zero bytes = r * x^(8n) mod P, a linear map (crc_mulmod by the constant
//                 x^(8n); n may be negative: x is invertible mod P);
//   raw(M)      = the register after M from 0, no init, no xorout;
//   crc32(M)    = raw(M) ^ Z_|M|(~0) ^ ~0;     raw(A || B) = Z_|B|(raw(A)) ^ raw(B).
//
// So a block's CRC is the XOR of independent terms Z_(bytes after piece)(raw(piece)), in any order, and the init term is
// carried by the lane that reads the block's first byte: its register starts at Z_-h(~0), h = the zero bytes it reads in
// front of that byte (the 16-byte-aligned chunk that holds it), so the register is ~0 where the block begins.
//
// k_crc32: a GROUP of G lanes (G = 1 .. 64, a power of two) takes one piece of a block at a time: [s, e), the whole block or
// (blocks above kCrcSeg bytes) one segment of kCrcSeg bytes.  The piece is read in rows of W = 16 G bytes from a0 = s
// rounded down to 16: lane q reads 16-byte chunk q of each row, so a wave load is one coalesced 1 KiB (G = 64) or 64/G
// runs of 16 G bytes.  Bytes outside [s, e) are masked to zero; every chunk read holds at least one byte of [s, e), so no
// read leaves the 16-byte-aligned range of the piece.  Each chunk costs 16 table reads (slicing-by-16): chunk k of a lane
// is followed, in the lane's own stream, by the W - 16 bytes of the other lanes, which are zeros to it, so every chunk
// but the lane's last uses the gap-folded tables T'_j = Z_(W-16) o T_j and the last one the plain T_j.  A lane's
// register then stands at the end of its last chunk, p; its term is Z_(e - p)(r), -15 <= e - p < W, one crc_mulmod by a
// constant of kCrc.c.  The terms are XOR-reduced over the group; a segment's sum is advanced to the block end by the
// wave-uniform Z_(block end - e) and XORed into the (zeroed) output with a vector atomicXor, a whole block's is stored.
// LDS: T (16 KiB) and T'_G (16 KiB), copied from the tables below, shared by the workgroup's waves.
//
// Included by redux_hip.hip (one translation unit).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace redux {

constexpr uint32_t kCrcPoly   = 0xEDB88320u;
constexpr uint32_t kCrcThreads = 256;               // 4 waves per workgroup
constexpr uint64_t kCrcSeg    = 256ull << 10;       // blocks above this are split into segments of this many bytes
constexpr uint32_t kCrcCOff   = 15;                 // kCrc.c[n + 15] = x^(8n) mod P, n = -15 .. 1024

// ---- GF(2) arithmetic modulo P, reflected (bit 31 = x^0): the same for host and device --------------------------------
__host__ __device__ constexpr uint32_t crc_mulx(uint32_t b) { return (b >> 1) ^ (kCrcPoly & (0u - (b & 1u))); }
__host__ __device__ constexpr uint32_t crc_divx(uint32_t b) // b * x^-1
{
    return (b & 0x80000000u) ? (((b ^ kCrcPoly) << 1) | 1u) : (b << 1);
}
// a * b mod P (zlib's multmodp, branch-free)
__host__ __device__ constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = crc_mulx(b);
    }
    return p;
}

struct alignas(16) CrcTables {
    uint32_t t[16][256];         // t[j][v] = Z_j(raw(byte v)): slicing-by-16
    uint32_t gap[7][16][256];    // gap[g][j] = Z_(16 (2^g - 1)) o t[j]: the tables of a group of G = 2^g lanes
    uint32_t c[1040];            // c[n + 15] = x^(8n) mod P, n = -15 .. 1024
    uint32_t init[16];           // init[h] = Z_-h(~0)
    uint32_t x2n[32];            // x2n[k] = x^(8 * 2^k) mod P
};

constexpr CrcTables make_crc_tables()
{
    CrcTables T{};
    for (uint32_t v = 0; v < 256; v++) {
        uint32_t r = v;
        for (int i = 0; i < 8; i++)
            r = crc_mulx(r);
        T.t[0][v] = r;
    }
    for (int j = 1; j < 16; j++)
        for (uint32_t v = 0; v < 256; v++)
            T.t[j][v] = (T.t[j - 1][v] >> 8) ^ T.t[0][T.t[j - 1][v] & 0xFF];
    // x^(8n), n >= 0: one zero byte at a time; n < 0: eight divisions by x at a time
    T.c[kCrcCOff] = 0x80000000u;
    for (uint32_t n = 1; n + kCrcCOff < 1040; n++) {
        const uint32_t p = T.c[kCrcCOff + n - 1];
        T.c[kCrcCOff + n] = (p >> 8) ^ T.t[0][p & 0xFF];
    }
    for (uint32_t n = 1; n <= kCrcCOff; n++) {
        uint32_t p = T.c[kCrcCOff - n + 1];
        for (int i = 0; i < 8; i++)
            p = crc_divx(p);
        T.c[kCrcCOff - n] = p;
    }
    for (uint32_t h = 0; h < 16; h++)
        T.init[h] = crc_mulmod(T.c[kCrcCOff - h], 0xFFFFFFFFu);
    T.x2n[0] = T.c[kCrcCOff + 1];
    for (int k = 1; k < 32; k++)
        T.x2n[k] = crc_mulmod(T.x2n[k - 1], T.x2n[k - 1]);
    // gap[g][j][v] = Z_n(t[j][v]), n = 16 (2^g - 1), by the linearity of Z_n: z[i][u] = Z_n(byte u at byte i of the register)
    for (int g = 0; g < 7; g++) {
        const uint32_t x8n = T.c[kCrcCOff + 16 * ((1u << g) - 1)];
        uint32_t       z[4][256] = {};
        for (int i = 0; i < 4; i++)
            for (uint32_t u = 1; u < 256; u++)
                z[i][u] = (u & (u - 1)) ? z[i][u & (u - 1)] ^ z[i][u & (0u - u)] : crc_mulmod(x8n, u << (8 * i));
        for (int j = 0; j < 16; j++)
            for (uint32_t v = 0; v < 256; v++) {
                const uint32_t r = T.t[j][v];
                T.gap[g][j][v] = z[0][r & 0xFF] ^ z[1][(r >> 8) & 0xFF] ^ z[2][(r >> 16) & 0xFF] ^ z[3][r >> 24];
            }
    }
    return T;
}

__device__ constexpr CrcTables kCrc = make_crc_tables();

// x^(8n) mod P for 0 <= n < 2^32 (wave-uniform n: scalar work)
__device__ __forceinline__ uint32_t crc_x8n(uint64_t n)
{
    uint32_t p = 0x80000000u;
    for (int k = 0; n; k++, n >>= 1)
        if (n & 1)
            p = crc_mulmod(kCrc.x2n[k], p);
    return p;
}

struct CrcArgs {
    const uint8_t  *in;
    uint64_t        in_len;     // blocks form: block b = in[b B .. min((b+1) B, in_len))
    const uint32_t *sizes;      // sizes form (non-null): block b = in[b B .. b B + min(sizes[b], B))
    uint64_t        nblocks;
    uint32_t        block_size; // B
    uint32_t        nseg;       // pieces per block: 1, or ceil(B / kCrcSeg) (then crc is zeroed first and XORed into)
    uint64_t        nitems;     // nblocks * nseg
    uint32_t       *crc;        // u32[nblocks]
};

// bytes of the 16-byte chunk at c that lie in [s, e) -- the others read as zero
__device__ __forceinline__ uint4 crc_mask(uint4 v, uint64_t c, uint64_t s, uint64_t e)
{
    const int64_t lo = (int64_t)s - (int64_t)c, hi = (int64_t)e - (int64_t)c; // keep bytes i with lo <= i < hi
    uint32_t      w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            m |= (4 * k + i >= lo && 4 * k + i < hi) ? (0xFFu << (8 * i)) : 0u;
        w[k] &= m;
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// slicing-by-16 step through one chunk: table j of t applies to byte 15 - j
__device__ __forceinline__ uint32_t crc_step(uint32_t r, uint4 v, const uint32_t *t)
{
    const uint32_t w0 = v.x ^ r;
    return t[15 * 256 + (w0 & 0xFF)] ^ t[14 * 256 + ((w0 >> 8) & 0xFF)] ^ t[13 * 256 + ((w0 >> 16) & 0xFF)] ^
           t[12 * 256 + (w0 >> 24)] ^ t[11 * 256 + (v.y & 0xFF)] ^ t[10 * 256 + ((v.y >> 8) & 0xFF)] ^
           t[9 * 256 + ((v.y >> 16) & 0xFF)] ^ t[8 * 256 + (v.y >> 24)] ^ t[7 * 256 + (v.z & 0xFF)] ^
           t[6 * 256 + ((v.z >> 8) & 0xFF)] ^ t[5 * 256 + ((v.z >> 16) & 0xFF)] ^ t[4 * 256 + (v.z >> 24)] ^
           t[3 * 256 + (v.w & 0xFF)] ^ t[2 * 256 + ((v.w >> 8) & 0xFF)] ^ t[1 * 256 + ((v.w >> 16) & 0xFF)] ^
           t[0 * 256 + (v.w >> 24)];
}

template <int G>
__device__ __forceinline__ uint32_t crc_group_xor(uint32_t v)
{
#pragma unroll
    for (int d = 1; d < G; d <<= 1)
        v ^= __shfl_xor(v, d, 64);
    return v;
}

template <int G>
__global__ void __launch_bounds__(kCrcThreads) k_crc32(CrcArgs a)
{
    constexpr int      LG = G == 1 ? 0 : G == 2 ? 1 : G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6;
    constexpr uint64_t W  = 16 * G;
    __shared__ uint32_t lds[2 * 16 * 256]; // [0, 4096): T, [4096, 8192): T'_G
    {
        const uint4 *t  = (const uint4 *)&kCrc.t[0][0];
        const uint4 *tg = (const uint4 *)&kCrc.gap[LG][0][0];
        uint4       *l  = (uint4 *)lds;
        for (uint32_t i = threadIdx.x; i < 1024; i += kCrcThreads) {
            l[i]        = t[i];
            l[1024 + i] = tg[i];
        }
    }
    __syncthreads();
    const uint32_t *T  = lds;
    const uint32_t *TG = lds + 4096;

    const uint32_t q      = threadIdx.x % G;                  // lane within the group
    const uint64_t groups = (uint64_t)gridDim.x * (kCrcThreads / G);
    const uint64_t B      = a.block_size;
    // (every lane of a group runs the same trip count, so the group reduction sees all its lanes)
    for (uint64_t it = (uint64_t)blockIdx.x * (kCrcThreads / G) + threadIdx.x / G; it < a.nitems; it += groups) {
        const uint64_t b = a.nseg == 1 ? it : it / a.nseg, j = a.nseg == 1 ? 0 : it % a.nseg;
        uint64_t       len;
        if (a.sizes)
            len = a.sizes[b] < B ? a.sizes[b] : B;
        else
            len = a.in_len - b * B < B ? a.in_len - b * B : B;
        const uint64_t o0 = j * kCrcSeg, o1 = a.nseg == 1 ? len : (o0 + kCrcSeg < len ? o0 + kCrcSeg : len);
        const uint64_t base = (uint64_t)(uintptr_t)a.in + b * B;
        uint32_t       term = 0;
        if (o0 < o1) {
            const uint64_t s = base + o0, e = base + o1, h = s & 15, a0 = s - h;
            const uint64_t R = (e - a0) / W, rem = (e - a0) % W, n = R + (16 * q < rem ? 1 : 0); // chunks of this lane
            uint32_t       r = (q == 0 && j == 0) ? kCrc.init[h] : 0u;
            if (n) {
                const uint64_t c0 = a0 + 16 * q;
                // first chunk: may begin before s, and (R == 0) pass e
                r = crc_step(r, crc_mask(*(const uint4 *)c0, c0, s, e), n > 1 ? TG : T);
                uint64_t i = 1;
                for (; i + 4 < n; i += 4) { // whole chunks, all followed by more of this lane's chunks
                    const uint4 v0 = *(const uint4 *)(c0 + i * W), v1 = *(const uint4 *)(c0 + (i + 1) * W);
                    const uint4 v2 = *(const uint4 *)(c0 + (i + 2) * W), v3 = *(const uint4 *)(c0 + (i + 3) * W);
                    r = crc_step(r, v0, TG);
                    r = crc_step(r, v1, TG);
                    r = crc_step(r, v2, TG);
                    r = crc_step(r, v3, TG);
                }
                for (; i + 1 < n; i++)
                    r = crc_step(r, *(const uint4 *)(c0 + i * W), TG);
                if (n > 1) { // last chunk: the tail row may pass e
                    const uint64_t c = c0 + (n - 1) * W;
                    r = crc_step(r, crc_mask(*(const uint4 *)c, c, s, e), T);
                }
                const uint64_t p = c0 + (n - 1) * W + 16; // where the register stands
                term = crc_mulmod(kCrc.c[(int64_t)e - (int64_t)p + kCrcCOff], r);
            }
            term = crc_group_xor<G>(term);
            if (a.nseg > 1) // a segment: advanced to the end of its block
                term = crc_mulmod(crc_x8n(len - o1), term);
        } else {
            term = 0;
        }
        if (q == 0) {
            if (a.nseg == 1)
                a.crc[b] = len ? term ^ 0xFFFFFFFFu : 0u;
            else if (o0 < o1)
                atomicXor(a.crc + b, j == 0 ? term ^ 0xFFFFFFFFu : term);
        }
    }
}

} // namespace redux
