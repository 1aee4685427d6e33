// Higher-order lagged differences through the C++ mirror (redux_amd/host/redux.hpp): two interleaved int16 tones coded behind
// the lagged delta filter at lag 2 and behind its orders 2 and 3, decoded again; order 1 against the lag filter's streams; and
// the refusals that come before any device call.  `lag_order_mirror_test --gpu` (or `--no-gpu`: the refusals alone); prints
// "lag order mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cmath>
#include <cstdio>
#include <cstring>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 8; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_lag_order(x, 8, 0, 2, 3, 2, P); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_lag_order(x, 8, 4, 3, 3, 2, P); // element size 3
            else if (which == 2)
                redux::hip::compress_blocks_lag_order(x, 8, 4, 2, 0, 2, P); // lag 0
            else if (which == 3)
                redux::hip::compress_blocks_lag_order(x, 8, 4, 2, REDUX_LAG_MAX + 1, 2, P); // lag above the maximum
            else if (which == 4)
                redux::hip::compress_blocks_lag_order(x, 8, 4, 2, 3, 0, P); // order 0
            else if (which == 5)
                redux::hip::compress_blocks_lag_order(x, 8, 4, 2, 3, REDUX_LAG_ORDER_MAX + 1, P); // order above the maximum
            else if (which == 6)
                redux::hip::decompress_blocks_lag_order(none, 4, 4, 2, 3, 4, P); // the same on the way back
            else
                redux::hip::decompress_blocks_lag_order(none, 8, 4, 2, 3, 2, P); // one stream for two blocks
            std::fprintf(stderr, "refusal %d was accepted\n", which);
            return 1;
        } catch (const redux::Error &e) {
            if (e.kind() != redux::Error::InvalidInput) {
                std::fprintf(stderr, "refusal %d: another error\n", which);
                return 1;
            }
        }
    }
    for (std::uint32_t K = 1; K <= REDUX_LAG_ORDER_MAX; K++)
        if (redux_lag_order_check(4, 1, K) != REDUX_OK || redux_lag_order_check(4, REDUX_LAG_MAX, K) != REDUX_OK) {
            std::fprintf(stderr, "a legal order was refused\n");
            return 1;
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2 || (std::strcmp(argv[1], "--no-gpu") && std::strcmp(argv[1], "--gpu"))) {
        std::fprintf(stderr, "usage: %s --gpu | --no-gpu\n", argv[0]);
        return 2;
    }
    if (refusals())
        return 1;
    if (!std::strcmp(argv[1], "--no-gpu")) {
        std::printf("lag order mirror host-side checks ok\n");
        return 0;
    }
    // two interleaved int16 channels, each three sinusoids plus noise of a few counts: three frames of 4096 elements and 100
    // more, plus one trailing byte
    const std::uint32_t block = 4096, E = 2, C = 2;
    const std::size_t   n = 3 * block + 100;
    std::vector<std::uint8_t> data(n * E + 1, 0x5A);
    std::uint64_t lcg = 20261020;
    for (std::size_t i = 0; i < n; i++) {
        const double t = (double)(i / C), c = (double)(i % C);
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        const double noise = (double)((lcg >> 33) % 13) - 6.0;
        const double v = 6000 * std::sin(6.283185307179586 * 0.003 * (c + 1) * t + c) + 2500 * std::sin(6.283185307179586 * 0.011 * t) +
                         900 * std::sin(6.283185307179586 * 0.031 * t + 1.0) + noise;
        const std::int16_t s = (std::int16_t)std::lround(v);
        std::memcpy(&data[i * E], &s, E);
    }
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const redux::hip::Blocks lag = redux::hip::compress_blocks_lag(data.data(), data.size(), block, E, C, P);
    const redux::hip::Blocks one = redux::hip::compress_blocks_lag_order(data.data(), data.size(), block, E, C, 1, P);
    if (one.data != lag.data || one.offsets != lag.offsets) {
        std::fprintf(stderr, "order 1 is not the lagged delta filter\n");
        return 1;
    }
    std::size_t bytes[4] = {0, lag.data.size(), 0, 0};
    for (std::uint32_t K = 1; K <= 3; K++) {
        const redux::hip::Blocks b = redux::hip::compress_blocks_lag_order(data.data(), data.size(), block, E, C, K, P);
        if (redux::hip::decompress_blocks_lag_order(b, data.size(), block, E, C, K, P) != data) {
            std::fprintf(stderr, "the round trip at order %u differs\n", K);
            return 1;
        }
        bytes[K] = b.data.size();
    }
    // (the first difference of a slow sinusoid is a slow sinusoid again; the second is a few counts plus the noise)
    if (bytes[2] * 10 > bytes[1] * 9) {
        std::fprintf(stderr, "order 2 did not pay: %zu against %zu bytes\n", bytes[2], bytes[1]);
        return 1;
    }
    std::printf("lag order mirror ok: %zu bytes -> %zu / %zu / %zu bytes at order 1 / 2 / 3\n", data.size(), bytes[1], bytes[2], bytes[3]);
    return 0;
}
