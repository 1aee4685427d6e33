// planes_ab.hip -- the two ways of filling the lanes of k_planes (redux_amd/csrc/redux_planes.hpp), side by side:
// lane-strided 16-byte accesses to the interleaved side (direct) against coalesced accesses staged through LDS (staged).
// Both forms run on the same 4 GiB (default) for E = 2, 4, 8, forward and inverse; prints the effective rate
// 2 * len / kernel time (hipEvent, median of 20 after 5 warm-up launches) and checks that both forms wrote the same bytes.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ab/planes_ab.hip -o tools/ubench/bin/planes_ab && tools/ubench/bin/planes_ab [GiB]
#include "../../redux_amd/csrc/redux_planes.hpp"

#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace redux;

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);       \
            exit(1);                                                                          \
        }                                                                                     \
    } while (0)

template <int E, bool INVERSE, bool STAGED>
__global__ void __launch_bounds__(256) k_ab(PlanesArgs a)
{
    __shared__ uint4 lds[STAGED ? 4 * 64 * E : 1];
    planes_group<E, INVERSE, STAGED>(a, lds);
}

__global__ void k_fill(uint64_t *p, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        p[i] = (i * 0x9E3779B97F4A7C15ull) ^ (i >> 7);
}

__global__ void k_diff(const uint64_t *a, const uint64_t *b, uint64_t n, unsigned long long *bad)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        if (a[i] != b[i])
            atomicAdd(bad, 1ull);
}

template <int E, bool INVERSE, bool STAGED>
static double run(const uint8_t *src, uint8_t *dst, uint64_t len, uint32_t block)
{
    PlanesArgs a{};
    a.src = src; a.dst = dst; a.block_size = block; a.frame_groups = block / 16; a.len = len;
    a.groups = len / ((uint64_t)E * block) * a.frame_groups;
    const uint32_t wgs = (uint32_t)((a.groups + 255) / 256);
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int it = 0; it < 25; it++) {
        CK(hipEventRecord(e0, 0));
        k_ab<E, INVERSE, STAGED><<<wgs, 256>>>(a);
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float t = 0;
        CK(hipEventElapsedTime(&t, e0, e1));
        if (it >= 5)
            ms.push_back(t);
    }
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

template <int E>
static void one(uint8_t *src, uint8_t *d1, uint8_t *d2, uint64_t len, uint32_t block, unsigned long long *bad)
{
    const uint64_t used = len / ((uint64_t)E * block) * E * block; // the fast kernel's full frames
    for (int inv = 0; inv < 2; inv++) {
        const double td = inv ? run<E, true, false>(src, d1, len, block) : run<E, false, false>(src, d1, len, block);
        const double ts = inv ? run<E, true, true>(src, d2, len, block) : run<E, false, true>(src, d2, len, block);
        CK(hipMemset(bad, 0, 8));
        k_diff<<<4096, 256>>>((const uint64_t *)d1, (const uint64_t *)d2, used / 8, bad);
        unsigned long long nbad = 0;
        CK(hipMemcpy(&nbad, bad, 8, hipMemcpyDeviceToHost));
        printf("E=%d %-7s direct %.3f ms %.2f TB/s   staged %.3f ms %.2f TB/s   %s\n", E, inv ? "inverse" : "forward", td,
               2.0 * len / td / 1e9, ts, 2.0 * len / ts / 1e9, nbad ? "OUTPUTS DIFFER" : "same bytes");
    }
}

int main(int argc, char **argv)
{
    const uint64_t len   = (uint64_t)(argc > 1 ? atof(argv[1]) : 4.0) * (1ull << 30);
    const uint32_t block = 65536;
    uint8_t *src, *d1, *d2;
    unsigned long long *bad;
    CK(hipMalloc(&src, len));
    CK(hipMalloc(&d1, len));
    CK(hipMalloc(&d2, len));
    CK(hipMalloc(&bad, 8));
    k_fill<<<4096, 256>>>((uint64_t *)src, len / 8);
    CK(hipDeviceSynchronize());
    printf("len %llu bytes, block %u\n", (unsigned long long)len, block);
    one<2>(src, d1, d2, len, block, bad);
    one<4>(src, d1, d2, len, block, bad);
    one<8>(src, d1, d2, len, block, bad);
    CK(hipFree(src));
    CK(hipFree(d1));
    CK(hipFree(d2));
    CK(hipFree(bad));
    return 0;
}
