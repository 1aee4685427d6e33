// redux_record_cost_list.hpp -- the host side of redux_record_cost_dev: the frame sampling arithmetic, the checks of the
// candidate list and its packing into the kernels' argument arrays.  Plain C++ with no device code and no runtime call, so
// that a stand-alone program can run it under a sanitizer (tests/cpp/record_cost_list_test.cpp).  The kernels of
// redux_record_cost.hpp call the same sampling functions, which is all REDUX_RECORD_COST_HD is for.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define REDUX_RECORD_COST_HD __host__ __device__
#else
#define REDUX_RECORD_COST_HD
#endif

namespace redux {

// What a candidate of record size R costs under sample_blocks Q: frames 0, T, 2T, ... of the nframes frames of R * B bytes
// (only the last may be short; an empty input is one empty frame), nsel of them, and the blocks of its compact row.
struct RecordCostSample {
    uint64_t nframes, nsel, row_blocks;
    uint64_t step; // T; 0: bad arguments
};

// Q == 0: every frame.  Q > 0: want = ceil(Q / R) frames; T = 1 if nframes <= want, else ceil(nframes / want).
// R >= 1 and B >= 1 are the caller's to check (R * B stays below 2^38: no overflow).
REDUX_RECORD_COST_HD inline RecordCostSample record_cost_sample(uint64_t in_len, uint32_t B, uint32_t R, uint32_t Q)
{
    RecordCostSample s = {0, 0, 0, 0};
    if (B == 0 || R == 0)
        return s;
    const uint64_t frame   = (uint64_t)R * B;
    const uint64_t nblocks = in_len ? in_len / B + (in_len % B ? 1 : 0) : 1; // redux_block_count
    s.nframes = in_len ? in_len / frame + (in_len % frame ? 1 : 0) : 1;
    s.step    = 1;
    if (Q) {
        const uint64_t want = ((uint64_t)Q + R - 1) / R;
        if (s.nframes > want)
            s.step = s.nframes / want + (s.nframes % want ? 1 : 0);
    }
    s.nsel = (s.nframes - 1) / s.step + 1;
    const uint64_t left = nblocks - (s.nsel - 1) * s.step * R; // blocks from the last selected frame on (>= 1)
    s.row_blocks = (s.nsel - 1) * R + (left < R ? left : R);
    return s;
}

// ncand candidates (records[c], deltas[c]) -> out_records[cap], out_deltas[cap], zero past the list.  false, with nothing
// written, for a null list, ncand == 0 or above cap, or a pair that check(record, delta) refuses (0 = fine).  Neither list
// is read past ncand entries, and neither before ncand is known to be in range.
template <class Check>
inline bool record_cost_list(const uint32_t *records, const uint8_t *deltas, uint32_t ncand, uint32_t cap, uint16_t *out_records,
                             uint8_t *out_deltas, Check check)
{
    if (!records || !deltas || ncand == 0 || ncand > cap)
        return false;
    for (uint32_t c = 0; c < ncand; c++)
        if (check(records[c], (int)deltas[c]) != 0)
            return false;
    for (uint32_t c = 0; c < cap; c++) {
        out_records[c] = (uint16_t)(c < ncand ? records[c] : 0);
        out_deltas[c]  = (uint8_t)(c < ncand ? deltas[c] : 0);
    }
    return true;
}

} // namespace redux
