// The host side of redux_lag_order_cost_dev's candidate list (redux_amd/csrc/redux_lag_order_cost_list.hpp) as a stand-alone
// program, for a run under -fsanitize=address,undefined: the lists live on the heap with exactly ncand entries, so a read past
// either, or a write past the argument arrays, is reported.  No device call.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined lag_order_cost_list_test.cpp -o t && ./t
#include "../../redux_amd/csrc/redux_lag_order_cost_list.hpp"
#include "../../include/redux_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// redux_lag_order_check's rule (include/redux_hip.h), restated: the library is not linked here
static int check(uint32_t E, uint32_t lag, uint32_t order)
{
    return (E == 1 || E == 2 || E == 4 || E == 8) && lag >= 1 && lag <= REDUX_LAG_MAX && order >= 1 && order <= REDUX_LAG_ORDER_MAX ? 0 : 1;
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
static bool run(uint32_t E, const std::vector<uint32_t> &lags, const std::vector<uint32_t> &orders, uint32_t n,
                std::vector<uint16_t> &ol, std::vector<uint8_t> &oo, bool null_lags = false, bool null_orders = false)
{
    const uint32_t cap = REDUX_LAG_ORDER_COST_MAX;
    uint32_t *hl = (uint32_t *)std::malloc(lags.size() * 4 + 1), *ho = (uint32_t *)std::malloc(orders.size() * 4 + 1);
    std::memcpy(hl, lags.data(), lags.size() * 4);
    std::memcpy(ho, orders.data(), orders.size() * 4);
    ol.assign(cap, 0xAAAA);
    oo.assign(cap, 0xAA);
    const bool ok = redux::lag_order_cost_list(E, null_lags ? nullptr : hl, null_orders ? nullptr : ho, n, cap, ol.data(), oo.data(), check);
    std::free(hl);
    std::free(ho);
    return ok;
}

static bool untouched(const std::vector<uint16_t> &ol, const std::vector<uint8_t> &oo)
{
    for (size_t c = 0; c < ol.size(); c++)
        if (ol[c] != 0xAAAA || oo[c] != 0xAA)
            return false;
    return true;
}

int main()
{
    std::vector<uint16_t> ol;
    std::vector<uint8_t>  oo;
    // a short list: packed in order, zeros behind it
    EXPECT(run(2, {1, 3, 3, 256}, {1, 2, 2, 3}, 4, ol, oo));
    EXPECT(ol[0] == 1 && ol[1] == 3 && ol[2] == 3 && ol[3] == 256 && oo[0] == 1 && oo[1] == 2 && oo[2] == 2 && oo[3] == 3);
    for (uint32_t c = 4; c < REDUX_LAG_ORDER_COST_MAX; c++)
        EXPECT(ol[c] == 0 && oo[c] == 0);
    // one candidate, and a full list of 256
    EXPECT(run(8, {256}, {3}, 1, ol, oo) && ol[0] == 256 && oo[0] == 3 && ol[1] == 0);
    std::vector<uint32_t> fl(REDUX_LAG_ORDER_COST_MAX), fo(REDUX_LAG_ORDER_COST_MAX);
    for (uint32_t c = 0; c < REDUX_LAG_ORDER_COST_MAX; c++) {
        fl[c] = c + 1;
        fo[c] = c % 3 + 1;
    }
    EXPECT(run(1, fl, fo, REDUX_LAG_ORDER_COST_MAX, ol, oo));
    for (uint32_t c = 0; c < REDUX_LAG_ORDER_COST_MAX; c++)
        EXPECT(ol[c] == c + 1 && oo[c] == c % 3 + 1);
    // refusals write nothing; a count above the cap is refused before either list is read (they hold one entry here)
    EXPECT(!run(2, {1}, {1}, 0, ol, oo) && untouched(ol, oo));
    EXPECT(!run(2, {1}, {1}, REDUX_LAG_ORDER_COST_MAX + 1, ol, oo) && untouched(ol, oo));
    EXPECT(!run(2, {1}, {1}, 0xFFFFFFFFu, ol, oo) && untouched(ol, oo));
    EXPECT(!run(2, {1}, {1}, 1, ol, oo, true, false) && untouched(ol, oo));
    EXPECT(!run(2, {1}, {1}, 1, ol, oo, false, true) && untouched(ol, oo));
    const uint32_t bad_lags[] = {0, 257, 1u << 16, 0xFFFFFFFFu}, bad_orders[] = {0, 4, 256, 0xFFFFFFFFu};
    for (uint32_t at = 0; at < 4; at++) {
        for (uint32_t bad : bad_lags) {
            std::vector<uint32_t> l = {1, 2, 3, 256};
            l[at] = bad;
            EXPECT(!run(2, l, {1, 2, 3, 3}, 4, ol, oo) && untouched(ol, oo));
        }
        for (uint32_t bad : bad_orders) {
            std::vector<uint32_t> o = {1, 2, 3, 3};
            o[at] = bad;
            EXPECT(!run(2, {1, 2, 3, 256}, o, 4, ol, oo) && untouched(ol, oo));
        }
    }
    for (uint32_t E : {0u, 3u, 16u})
        EXPECT(!run(E, {1}, {1}, 1, ol, oo) && untouched(ol, oo));
    if (failures)
        return 1;
    std::printf("lag order cost list checks ok\n");
    return 0;
}
