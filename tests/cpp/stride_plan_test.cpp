// The host side of the snapshot-stride filter (redux_amd/csrc/redux_stride_host.hpp) as a stand-alone program, for a run
// under -fsanitize=address,undefined: the argument check, the shape of the inverse's second stage at its extremes (lengths
// and strides up to 2^64 - 1, where an overflow would be reported) checked against the rules the kernels rely on, and the
// container's record parsed from heap buffers of exactly the bytes on offer, so that a read past them is reported.  No
// device call.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined stride_plan_test.cpp -o t && ./t
#include "../../redux_amd/csrc/redux_stride_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);           \
            failures++;                                                  \
        }                                                                \
    } while (0)

// what the kernels rely on, for one plan
static void check_plan(uint64_t len, uint32_t E, uint64_t S, bool aligned)
{
    const redux::StridePlan p = redux::stride_plan(len, E, S, aligned);
    const uint64_t n = len / E;
    EXPECT(p.run == (S < n));
    if (!p.run) {
        EXPECT(p.ws_bytes == 0);
        return;
    }
    EXPECT(p.n == n);
    EXPECT(p.chunks == (aligned && S * E % 16 == 0));
    const uint64_t unit = p.chunks ? 16 : E;
    EXPECT(p.cols * unit == S * E);                        // the columns tile a snapshot
    EXPECT(p.head % unit == 0 && p.head <= n * E && n * E - p.head < unit);
    EXPECT(p.rows >= 1 && p.rows == p.head / (S * E) + (p.head % (S * E) != 0));          // the snapshots cover the head
    EXPECT(p.segs >= 1 && p.steps >= 1);
    EXPECT(p.segs == p.rows / p.steps + (p.rows % p.steps != 0));                         // the segments tile the snapshots
    if (p.segs > 1) {
        EXPECT(p.steps >= redux::kStrideMinSteps);                                       // no segment is a sliver
        EXPECT(p.segs * p.cols <= redux::kStrideThreads);                                // the workspace is bounded
        EXPECT(p.ws_bytes >= p.segs * p.cols * p.item_bytes && p.ws_bytes <= redux::kStrideThreads * 16);
        EXPECT(p.item_bytes == (p.chunks ? 16u : 8u));
    } else {
        EXPECT(p.ws_bytes == 0);
        // one segment only where the columns fill the machine or the snapshots are few
        EXPECT(p.cols > redux::kStrideThreads / 2 || p.rows < 2 * redux::kStrideMinSteps);
    }
    EXPECT(redux::stride_workspace_bytes(len, E, S) >= p.ws_bytes + (p.ws_bytes ? 16 : 0));
    EXPECT(redux::stride_workspace_bytes(len, E, S) % 256 == 0);
}

int main()
{
    // the check
    const uint32_t sizes[] = {1, 2, 4, 8}, bad_sizes[] = {0, 3, 5, 6, 7, 9, 16, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t E : sizes) {
        EXPECT(redux::stride_args_ok(E, 1) && redux::stride_args_ok(E, ~0ull) && !redux::stride_args_ok(E, 0));
        EXPECT(redux::stride_plan(1000, E, 0, true).run == false && redux::stride_workspace_bytes(1000, E, 0) == 0);
    }
    for (uint32_t E : bad_sizes) {
        EXPECT(!redux::stride_args_ok(E, 1));
        EXPECT(redux::stride_plan(1000, E, 1, true).run == false && redux::stride_workspace_bytes(1000, E, 1) == 0);
    }
    // the plan
    const uint64_t lens[] = {0, 1, 7, 8, 15, 16, 17, 1000, 4096, 100003 * 8ull, (1ull << 24) + 3, (1ull << 32) + (1ull << 20) + 3,
                             (1ull << 40) + 12345, (1ull << 63) - 1, 1ull << 63, ~0ull - 8, ~0ull};
    for (uint32_t E : sizes)
        for (uint64_t len : lens) {
            const uint64_t n = len / E;
            const uint64_t strides[] = {1, 2, 3, 4, 5, 15, 16, 17, 64, 1024, 1025, 30000, (1ull << 18) - 1, 1ull << 18, (1ull << 18) + 1,
                                        (1ull << 28) + 5, n / 40 + 1, n / 3 + 1, n / 2, n - 1, n, n + 7, ~0ull};
            for (uint64_t S : strides) {
                if (S == 0)
                    continue;
                check_plan(len, E, S, true);
                check_plan(len, E, S, false);
            }
        }
    { // S = 1 over 2^32 bytes of E = 4: a column, 2^30 snapshots, 2^18 segments of 4096
        const redux::StridePlan p = redux::stride_plan(1ull << 32, 4, 1, true);
        EXPECT(p.run && !p.chunks && p.cols == 1 && p.rows == 1ull << 30 && p.segs == 1ull << 18 && p.steps == 4096);
        EXPECT(p.ws_bytes == (1ull << 18) * 8);
    }
    { // S = 64 over 2^22 elements of E = 4: 16 chunk columns, 65536 snapshots, 2048 segments of 32
        const redux::StridePlan p = redux::stride_plan(1ull << 24, 4, 64, true);
        EXPECT(p.run && p.chunks && p.cols == 16 && p.rows == 65536 && p.segs == 2048 && p.steps == 32 && p.head == 1ull << 24);
        const redux::StridePlan q = redux::stride_plan(1ull << 24, 4, 64, false); // the pointer is not aligned: elements
        EXPECT(q.run && !q.chunks && q.cols == 64 && q.rows == 65536 && q.segs == 2048);
    }
    { // the workspace never falls as the length grows (a decoder sized for its largest input)
        for (uint32_t E : sizes)
            for (uint64_t S : {1ull, 3ull, 64ull, 1000ull}) {
                uint64_t last = 0;
                for (uint64_t len = 0; len < 3000000; len += 9973) {
                    const uint64_t ws = redux::stride_workspace_bytes(len, E, S);
                    EXPECT(ws >= last);
                    last = ws;
                }
            }
    }
    // the container's record, from heap buffers of exactly `avail` bytes
    for (uint32_t E : sizes) {
        const uint32_t word = redux::stride_record_word(E);
        EXPECT(word == (0xF0000000u | 2u << 24 | E));
        for (uint64_t S : {1ull, 30000ull, 1ull << 32, ~0ull}) {
            for (size_t avail = 0; avail <= 9; avail++) {
                uint8_t full[8];
                redux::stride_record_pack(S, full);
                uint8_t *rec = (uint8_t *)std::malloc(avail ? avail : 1);
                std::memcpy(rec, full, avail < 8 ? avail : 8);
                uint32_t e = 99;
                uint64_t s = 99;
                const int rc = redux::stride_record_parse(word, rec, avail, &e, &s);
                if (avail < 8)
                    EXPECT(rc == 2 && e == 99 && s == 99);
                else
                    EXPECT(rc == 0 && e == E && s == S);
                std::free(rec);
            }
        }
        uint8_t zero[8] = {0};
        uint32_t e = 99;
        uint64_t s = 99;
        EXPECT(redux::stride_record_parse(word, zero, 8, &e, &s) == 1 && e == 99 && s == 99);
        EXPECT(redux::stride_record_parse(word, nullptr, 0, &e, &s) == 2);
    }
    const uint32_t bad_words[] = {0xF2000017u, 0xF3000017u, 0xFF000017u, 0xF2000000u, 0xF2000003u, 0xF2000014u, 0xF2000104u,
                                  0xF2800004u, 0xF1000004u, 0xF3000004u, 0xF0000004u, 0x02000004u, 0xE2000004u, 0u, ~0u};
    for (uint32_t word : bad_words) {
        uint8_t rec[8] = {1, 0, 0, 0, 0, 0, 0, 0};
        uint32_t e = 99;
        uint64_t s = 99;
        EXPECT(redux::stride_record_parse(word, rec, 8, &e, &s) == 1 && e == 99 && s == 99);
    }
    if (failures)
        return 1;
    std::printf("stride plan checks ok\n");
    return 0;
}
