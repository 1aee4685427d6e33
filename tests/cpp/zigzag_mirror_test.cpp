// The zigzag-folded delta filter through the C++ mirror (redux_amd/host/redux.hpp): a generated int32 random walk coded
// behind the delta filter and behind the folded one, decoded again; and the refusals that come before any device call.
// `zigzag_mirror_test --gpu` (or `--no-gpu`: the refusals alone); prints "zigzag mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <cstring>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 3; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_zigzag(x, 8, 0, 2, P); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_zigzag(x, 8, 4, 3, P); // element size 3
            else
                redux::hip::decompress_blocks_zigzag(none, 8, 4, 2, P); // one stream for two blocks
            std::fprintf(stderr, "refusal %d was accepted\n", which);
            return 1;
        } catch (const redux::Error &e) {
            if (e.kind() != redux::Error::InvalidInput) {
                std::fprintf(stderr, "refusal %d: another error\n", which);
                return 1;
            }
        }
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
        std::printf("zigzag mirror host-side checks ok\n");
        return 0;
    }
    // an int32 walk with steps -50 .. 50, three frames of 4096 elements and 100 more, plus three trailing bytes
    const std::uint32_t block = 4096, E = 4;
    const std::size_t   n = 3 * block + 100;
    std::vector<std::uint8_t> data(n * E + 3, 0x5A);
    std::uint64_t lcg = 20261020;
    std::int32_t  v = 0;
    for (std::size_t i = 0; i < n; i++) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v += (std::int32_t)((lcg >> 33) % 101) - 50;
        std::memcpy(&data[i * E], &v, E);
    }
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const redux::hip::Blocks delta = redux::hip::compress_blocks_delta(data.data(), data.size(), block, E, P);
    const redux::hip::Blocks zz = redux::hip::compress_blocks_zigzag(data.data(), data.size(), block, E, P);
    if (redux::hip::decompress_blocks_zigzag(zz, data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the round trip differs\n");
        return 1;
    }
    if (redux::hip::decompress_blocks_delta(delta, data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the delta round trip differs\n");
        return 1;
    }
    // (the three upper planes of the differences are an even mix of 0x00 and 0xFF, about a bit per element each; folded
    // they are zeros: the CPU oracle gives 0.75 of delta's size on such a walk)
    if (zz.data.size() * 10 > delta.data.size() * 8) {
        std::fprintf(stderr, "the fold did not pay: %zu against %zu bytes\n", zz.data.size(), delta.data.size());
        return 1;
    }
    std::printf("zigzag mirror ok: %zu bytes -> %zu bytes (%zu behind the delta filter)\n", data.size(), zz.data.size(), delta.data.size());
    return 0;
}
