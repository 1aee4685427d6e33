// The lagged delta filter through the C++ mirror (redux_amd/host/redux.hpp): three interleaved int32 random walks coded
// behind the zigzag filter and behind the lagged one with lag 3, decoded again; and the refusals that come before any device
// call.  `lag_mirror_test --gpu` (or `--no-gpu`: the refusals alone); prints "lag mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <cstring>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 6; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_lag(x, 8, 0, 2, 3, P); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_lag(x, 8, 4, 3, 3, P); // element size 3
            else if (which == 2)
                redux::hip::compress_blocks_lag(x, 8, 4, 2, 0, P); // lag 0
            else if (which == 3)
                redux::hip::compress_blocks_lag(x, 8, 4, 2, REDUX_LAG_MAX + 1, P); // lag above the maximum
            else if (which == 4)
                redux::hip::decompress_blocks_lag(none, 4, 4, 2, 257, P); // the same on the way back
            else
                redux::hip::decompress_blocks_lag(none, 8, 4, 2, 3, P); // one stream for two blocks
            std::fprintf(stderr, "refusal %d was accepted\n", which);
            return 1;
        } catch (const redux::Error &e) {
            if (e.kind() != redux::Error::InvalidInput) {
                std::fprintf(stderr, "refusal %d: another error\n", which);
                return 1;
            }
        }
    }
    if (redux_lag_check(4, 1) != REDUX_OK || redux_lag_check(4, REDUX_LAG_MAX) != REDUX_OK) {
        std::fprintf(stderr, "a legal lag was refused\n");
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
        std::printf("lag mirror host-side checks ok\n");
        return 0;
    }
    // three interleaved int32 walks with steps -50 .. 50 around levels 10,000 apart: three frames of 4096 elements and 100
    // more, plus three trailing bytes
    const std::uint32_t block = 4096, E = 4, C = 3;
    const std::size_t   n = 3 * block + 100;
    std::vector<std::uint8_t> data(n * E + 3, 0x5A);
    std::uint64_t lcg = 20261020;
    std::int32_t  v[C] = {0, 10000, -10000};
    for (std::size_t i = 0; i < n; i++) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v[i % C] += (std::int32_t)((lcg >> 33) % 101) - 50;
        std::memcpy(&data[i * E], &v[i % C], E);
    }
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const redux::hip::Blocks zz = redux::hip::compress_blocks_zigzag(data.data(), data.size(), block, E, P);
    const redux::hip::Blocks lag = redux::hip::compress_blocks_lag(data.data(), data.size(), block, E, C, P);
    const redux::hip::Blocks one = redux::hip::compress_blocks_lag(data.data(), data.size(), block, E, 1, P);
    if (redux::hip::decompress_blocks_lag(lag, data.size(), block, E, C, P) != data) {
        std::fprintf(stderr, "the round trip differs\n");
        return 1;
    }
    if (one.data != zz.data || one.offsets != zz.offsets) {
        std::fprintf(stderr, "lag 1 is not the zigzag filter\n");
        return 1;
    }
    // (the neighbour is another channel, 10,000 or 20,000 away: its difference fills two planes; the difference to the
    // element three back is a step of at most 50)
    if (lag.data.size() * 10 > zz.data.size() * 8) {
        std::fprintf(stderr, "the lag did not pay: %zu against %zu bytes\n", lag.data.size(), zz.data.size());
        return 1;
    }
    std::printf("lag mirror ok: %zu bytes -> %zu bytes (%zu behind the zigzag filter)\n", data.size(), lag.data.size(), zz.data.size());
    return 0;
}
