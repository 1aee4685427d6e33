// redux_lag_order_cost_list.hpp -- the host side of redux_lag_order_cost_dev's candidate list: the checks, and the packing
// into the kernels' argument arrays.  Plain C++ with no device code and no runtime call, so that a stand-alone program can
// run it under a sanitizer (tests/cpp/lag_order_cost_list_test.cpp).
#pragma once

#include <cstdint>

namespace redux {

// ncand candidates (lags[c], orders[c]) -> out_lags[cap], out_orders[cap], zero past the list.  false, with nothing
// written, for a null list, ncand == 0 or above cap, or a pair that check(element_size, lag, order) refuses (0 = fine).
// Neither list is read past ncand entries, and neither before ncand is known to be in range.
template <class Check>
inline bool lag_order_cost_list(uint32_t element_size, const uint32_t *lags, const uint32_t *orders, uint32_t ncand, uint32_t cap,
                                uint16_t *out_lags, uint8_t *out_orders, Check check)
{
    if (!lags || !orders || ncand == 0 || ncand > cap)
        return false;
    for (uint32_t c = 0; c < ncand; c++)
        if (check(element_size, lags[c], orders[c]) != 0)
            return false;
    for (uint32_t c = 0; c < cap; c++) {
        out_lags[c]   = (uint16_t)(c < ncand ? lags[c] : 0);
        out_orders[c] = (uint8_t)(c < ncand ? orders[c] : 0);
    }
    return true;
}

} // namespace redux
