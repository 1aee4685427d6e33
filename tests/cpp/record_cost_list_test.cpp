// The host side of redux_record_cost_dev (redux_amd/csrc/redux_record_cost_list.hpp) as a stand-alone program, for a run under
// -fsanitize=address,undefined: the candidate lists live on the heap with exactly ncand entries, so a read past either, or a
// write past the argument arrays, is reported; the sampling arithmetic runs at its extremes (lengths past 2^32, the largest
// frame, one byte), where an overflow would be reported.  No device call.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined record_cost_list_test.cpp -o t && ./t
#include "../../redux_amd/csrc/redux_record_cost_list.hpp"
#include "../../include/redux_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// redux_record_check's rule (include/redux_hip.h), restated: the library is not linked here
static int check(uint32_t R, int delta)
{
    return R >= 2 && R <= REDUX_RECORD_MAX && (delta == 0 || delta == 1) ? 0 : 1;
}

static int failures = 0;
#define EXPECT(c)                                                        \
    do {                                                                 \
        if (!(c)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);           \
            failures++;                                                  \
        }                                                                \
    } while (0)

// the call on heap copies of exactly n entries, into heap arrays of exactly cap entries
static bool run(const std::vector<uint32_t> &records, const std::vector<uint8_t> &deltas, uint32_t n, std::vector<uint16_t> &orr,
                std::vector<uint8_t> &od, bool null_records = false, bool null_deltas = false)
{
    const uint32_t cap = REDUX_RECORD_COST_MAX;
    uint32_t *hr = (uint32_t *)std::malloc(records.size() * 4 + 1);
    uint8_t  *hd = (uint8_t *)std::malloc(deltas.size() + 1);
    std::memcpy(hr, records.data(), records.size() * 4);
    std::memcpy(hd, deltas.data(), deltas.size());
    orr.assign(cap, 0xAAAA);
    od.assign(cap, 0xAA);
    const bool ok = redux::record_cost_list(null_records ? nullptr : hr, null_deltas ? nullptr : hd, n, cap, orr.data(), od.data(), check);
    std::free(hr);
    std::free(hd);
    return ok;
}

static bool untouched(const std::vector<uint16_t> &orr, const std::vector<uint8_t> &od)
{
    for (size_t c = 0; c < orr.size(); c++)
        if (orr[c] != 0xAAAA || od[c] != 0xAA)
            return false;
    return true;
}

// the sampling rule, restated with a loop over the selected frames where that is affordable
static void sample_by_walking(uint64_t len, uint32_t B, uint32_t R, uint32_t Q)
{
    const redux::RecordCostSample s = redux::record_cost_sample(len, B, R, Q);
    const uint64_t frame = (uint64_t)R * B, nframes = len ? len / frame + (len % frame != 0) : 1, nblocks = len ? len / B + (len % B != 0) : 1;
    uint64_t T = 1;
    if (Q) {
        const uint64_t want = ((uint64_t)Q + R - 1) / R;
        if (nframes > want)
            T = nframes / want + (nframes % want != 0);
    }
    EXPECT(s.nframes == nframes && s.step == T);
    if (nframes / T > 100000)
        return;
    uint64_t nsel = 0, row = 0;
    for (uint64_t f = 0; f < nframes; f += T) {
        const uint64_t left = nblocks - f * R;
        nsel++;
        row += left < R ? left : R;
    }
    EXPECT(s.nsel == nsel && s.row_blocks == row);
}

int main()
{
    std::vector<uint16_t> orr;
    std::vector<uint8_t>  od;
    // a short list: packed in order, zeros behind it
    EXPECT(run({2, 23, 23, 256}, {0, 1, 1, 0}, 4, orr, od));
    EXPECT(orr[0] == 2 && orr[1] == 23 && orr[2] == 23 && orr[3] == 256 && od[0] == 0 && od[1] == 1 && od[2] == 1 && od[3] == 0);
    for (uint32_t c = 4; c < REDUX_RECORD_COST_MAX; c++)
        EXPECT(orr[c] == 0 && od[c] == 0);
    // one candidate, and a full list of 256
    EXPECT(run({256}, {1}, 1, orr, od) && orr[0] == 256 && od[0] == 1 && orr[1] == 0);
    std::vector<uint32_t> fr(REDUX_RECORD_COST_MAX);
    std::vector<uint8_t>  fd(REDUX_RECORD_COST_MAX);
    for (uint32_t c = 0; c < REDUX_RECORD_COST_MAX; c++) {
        fr[c] = 2 + c / 2;
        fd[c] = c & 1;
    }
    EXPECT(run(fr, fd, REDUX_RECORD_COST_MAX, orr, od));
    for (uint32_t c = 0; c < REDUX_RECORD_COST_MAX; c++)
        EXPECT(orr[c] == 2 + c / 2 && od[c] == (c & 1));
    // refusals write nothing; a count above the cap is refused before either list is read (they hold one entry here)
    EXPECT(!run({2}, {0}, 0, orr, od) && untouched(orr, od));
    EXPECT(!run({2}, {0}, REDUX_RECORD_COST_MAX + 1, orr, od) && untouched(orr, od));
    EXPECT(!run({2}, {0}, 0xFFFFFFFFu, orr, od) && untouched(orr, od));
    EXPECT(!run({2}, {0}, 1, orr, od, true, false) && untouched(orr, od));
    EXPECT(!run({2}, {0}, 1, orr, od, false, true) && untouched(orr, od));
    const uint32_t bad_records[] = {0, 1, 257, 1u << 16, 0xFFFFFFFFu};
    const uint8_t  bad_deltas[]  = {2, 128, 255};
    for (uint32_t at = 0; at < 4; at++) {
        for (uint32_t bad : bad_records) {
            std::vector<uint32_t> r = {2, 3, 23, 256};
            r[at] = bad;
            EXPECT(!run(r, {0, 1, 0, 1}, 4, orr, od) && untouched(orr, od));
        }
        for (uint8_t bad : bad_deltas) {
            std::vector<uint8_t> d = {0, 1, 0, 1};
            d[at] = bad;
            EXPECT(!run({2, 3, 23, 256}, d, 4, orr, od) && untouched(orr, od));
        }
    }
    // the sampling arithmetic
    const uint32_t Rs[] = {2, 3, 23, 255, 256}, Bs[] = {1, 16, 4096, 65536, 1u << 30}, Qs[] = {0, 1, 64, 1000, 0xFFFFFFFFu};
    for (uint32_t R : Rs)
        for (uint32_t B : Bs)
            for (uint32_t Q : Qs) {
                const uint64_t frame = (uint64_t)R * B;
                const uint64_t lens[] = {0, 1, R - 1, frame - 1, frame, frame + 1, 100 * frame, 100 * frame + B + 1, (1ull << 33) + 5,
                                         (1ull << 40) + 12345, ~0ull};
                for (uint64_t len : lens)
                    sample_by_walking(len, B, R, Q);
            }
    EXPECT(redux::record_cost_sample(100, 0, 2, 0).step == 0 && redux::record_cost_sample(100, 16, 0, 0).step == 0);
    { // one frame plus one byte at R = 3, B = 16: two frames, the second of one block
        const redux::RecordCostSample s = redux::record_cost_sample(49, 16, 3, 0);
        EXPECT(s.nframes == 2 && s.nsel == 2 && s.step == 1 && s.row_blocks == 4);
        const redux::RecordCostSample q = redux::record_cost_sample(49, 16, 3, 1); // want = 1 frame: T = 2, frame 0 alone
        EXPECT(q.step == 2 && q.nsel == 1 && q.row_blocks == 3);
    }
    { // 2^33 + 5 bytes at R = 23, B = 65536, Q = 64: want = 3 of 5699 frames
        const redux::RecordCostSample s = redux::record_cost_sample((1ull << 33) + 5, 65536, 23, 64);
        EXPECT(s.nframes == 5699 && s.step == 1900 && s.nsel == 3 && s.row_blocks == 69);
    }
    if (failures)
        return 1;
    std::printf("record cost list checks ok\n");
    return 0;
}
