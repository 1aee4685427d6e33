// The folded difference against a base through the C++ mirror (redux_amd/host/redux.hpp): a file coded against a base that
// is the file with a byte changed here and there and its last third cut off, decoded again with the same base; the file
// against itself; and the refusals that come before any device call.  `base_sub_mirror_test <file>` (or `--no-gpu`: the
// refusals alone); prints "base sub mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 4; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_base_sub(x, 8, x, 8, 0, 2, P); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_base_sub(x, 8, x, 8, 4, 3, P); // element size 3
            else if (which == 2)
                redux::hip::compress_blocks_base_sub(x, 8, nullptr, 8, 4, 2, P); // no base, but a length
            else
                redux::hip::decompress_blocks_base_sub(none, x, 8, 8, 4, 2, P); // one stream for two blocks
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
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <file> | --no-gpu\n", argv[0]);
        return 2;
    }
    if (refusals())
        return 1;
    if (!std::strcmp(argv[1], "--no-gpu")) {
        std::printf("base sub mirror host-side checks ok\n");
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint32_t block = 4096, E = 2;
    std::vector<std::uint8_t> base(data.begin(), data.begin() + data.size() * 2 / 3 + 1);
    for (std::size_t i = 0; i < base.size(); i += 97)
        base[i] ^= (std::uint8_t)(1 + i % 7);
    const redux::hip::Blocks plain = redux::hip::compress_blocks_planes(data.data(), data.size(), block, E, P);
    const redux::hip::Blocks s = redux::hip::compress_blocks_base_sub(data.data(), data.size(), base.data(), base.size(), block, E, P);
    if (redux::hip::decompress_blocks_base_sub(s, base.data(), base.size(), data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the round trip with the base differs\n");
        return 1;
    }
    if (s.data.size() >= plain.data.size()) {
        std::fprintf(stderr, "a related base did not pay: %zu against %zu bytes\n", s.data.size(), plain.data.size());
        return 1;
    }
    // the file against itself: all-zero coder input; and no base at all: the byte-plane layout's streams
    const redux::hip::Blocks self = redux::hip::compress_blocks_base_sub(data.data(), data.size(), data.data(), data.size(), block, E, P);
    if (self.data.size() * 10 > data.size() || // (a block of 4096 zeros costs about 175 bytes under (8, 30, 32))
        redux::hip::decompress_blocks_base_sub(self, data.data(), data.size(), data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the file against itself: %zu bytes, or a differing round trip\n", self.data.size());
        return 1;
    }
    const redux::hip::Blocks nobase = redux::hip::compress_blocks_base_sub(data.data(), data.size(), nullptr, 0, block, E, P);
    if (nobase.data != plain.data || nobase.offsets != plain.offsets) {
        std::fprintf(stderr, "an empty base does not give the byte-plane layout's streams\n");
        return 1;
    }
    std::printf("base sub mirror ok: %zu bytes -> %zu bytes (%zu without the base)\n", data.size(), s.data.size(), plain.data.size());
    return 0;
}
