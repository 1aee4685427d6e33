// The copy yardstick of the encoder's row gather (k_compact_rows): a grid-stride uint4 copy of n bytes between two device
// buffers, nothing else.  Timed per launch with events; prints the median of `reps` launches after `warmup` launches.
// hipcc --offload-arch=gfx950 -O3 -o copy_rate tools/ubench/copy_rate.hip && ./copy_rate [bytes [warmup [reps [blocks per CU]]]]
// (tools/copy_rate.py builds and runs it with the bytes the gather moves at the headline shape.)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define TRY(x)                                                                              \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                         \
            return 1;                                                                       \
        }                                                                                   \
    } while (0)
__global__ void __launch_bounds__(256) k_copy(const uint4 *__restrict__ src, uint4 *__restrict__ dst, uint64_t n16)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride)
        dst[i] = src[i];
}
int main(int argc, char **argv)
{
    const uint64_t n      = (argc > 1 ? strtoull(argv[1], nullptr, 0) : 4300000000ull) / 16 * 16;
    const int      warmup = argc > 2 ? atoi(argv[2]) : 10, reps = argc > 3 ? atoi(argv[3]) : 10;
    const int      per_cu = argc > 4 ? atoi(argv[4]) : 8;
    if (n == 0 || warmup < 0 || reps < 1 || per_cu < 1)
        return 2;
    hipDeviceProp_t prop;
    TRY(hipGetDeviceProperties(&prop, 0));
    uint4 *a = nullptr, *b = nullptr;
    TRY(hipMalloc(&a, n));
    TRY(hipMalloc(&b, n));
    TRY(hipMemset(a, 0x5A, n));
    TRY(hipMemset(b, 0, n));
    const uint32_t grid = (uint32_t)std::min<uint64_t>((uint64_t)prop.multiProcessorCount * per_cu, (n / 16 + 255) / 256);
    hipEvent_t     e0, e1;
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int i = 0; i < warmup + reps; i++) {
        TRY(hipEventRecord(e0));
        k_copy<<<grid, 256>>>(a, b, n / 16);
        TRY(hipEventRecord(e1));
        TRY(hipEventSynchronize(e1));
        float t;
        TRY(hipEventElapsedTime(&t, e0, e1));
        if (i >= warmup)
            ms.push_back(t);
    }
    TRY(hipGetLastError());
    std::sort(ms.begin(), ms.end());
    const double med = reps & 1 ? ms[reps / 2] : 0.5 * (ms[reps / 2 - 1] + ms[reps / 2]);
    uint8_t      last = 0;
    TRY(hipMemcpy(&last, (const uint8_t *)b + n - 1, 1, hipMemcpyDeviceToHost));
    printf("copy_rate: %llu bytes, grid %u x 256 (%d per CU), %d warm-up + %d launches: median %.4f ms (min %.4f, max %.4f) = %.3f TB/s "
           "read+write%s\n",
           (unsigned long long)n, grid, per_cu, warmup, reps, med, ms.front(), ms.back(), 2.0 * n / med / 1e9,
           last == 0x5A ? "" : "  COPY WRONG");
    TRY(hipFree(a));
    TRY(hipFree(b));
    return last == 0x5A ? 0 : 1;
}
