// Constant blocks through the C++ mirror (redux_amd/host/redux.hpp): a file with a run of zeros in its middle coded against
// a base that equals its first third, decoded again with the flags and the same base; the file against itself, where no
// block is left for the coder; and the refusals that come before any device call.  `const_mirror_test <file>` (or
// `--no-gpu`: the refusals alone); prints "const mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    std::vector<std::uint8_t> flags;
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 5; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_const(x, 8, nullptr, 0, 0, 2, P, flags); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_const(x, 8, nullptr, 0, 4, 3, P, flags); // element size 3
            else if (which == 2)
                redux::hip::compress_blocks_const(x, 8, nullptr, 8, 4, 2, P, flags); // no base, but a length
            else if (which == 3)
                redux::hip::decompress_blocks_const(none, {0}, nullptr, 0, 8, 4, 2, P); // one stream for two blocks
            else
                redux::hip::decompress_blocks_const(none, {0, 0}, nullptr, 0, 4, 4, 2, P); // two flags for one block
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
        std::printf("const mirror host-side checks ok\n");
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint32_t block = 4096, E = 2;
    const std::size_t third = data.size() / 3;
    std::fill(data.begin() + third, data.begin() + 2 * third, 0); // constant without a base
    const std::vector<std::uint8_t> base(data.begin(), data.begin() + third); // and unchanged against one
    std::vector<std::uint8_t> flags, noflags;
    const redux::hip::Blocks plain = redux::hip::compress_blocks_base(data.data(), data.size(), base.data(), base.size(), block, E, P);
    const redux::hip::Blocks s = redux::hip::compress_blocks_const(data.data(), data.size(), base.data(), base.size(), block, E, P, flags);
    if (redux::hip::decompress_blocks_const(s, flags, base.data(), base.size(), data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the round trip differs\n");
        return 1;
    }
    std::size_t nconst = 0, saved = 0;
    for (std::size_t b = 0; b < flags.size(); b++) {
        const std::uint64_t size = s.offsets[b + 1] - s.offsets[b], was = plain.offsets[b + 1] - plain.offsets[b];
        if (flags[b] > 1 || (flags[b] == 1 && size != 1) || (flags[b] == 0 && size != was)) {
            std::fprintf(stderr, "block %zu: flag %u, %llu bytes (%llu without the option)\n", b, flags[b], (unsigned long long)size,
                         (unsigned long long)was);
            return 1;
        }
        nconst += flags[b];
        saved += flags[b] ? was - 1 : 0;
    }
    // every frame that lies wholly inside the first two thirds is constant
    if (nconst + 2 * E < 2 * third / block || s.data.size() + saved != plain.data.size()) {
        std::fprintf(stderr, "%zu constant blocks of %zu, %zu bytes against %zu\n", nconst, flags.size(), s.data.size(), plain.data.size());
        return 1;
    }
    // the file against itself: no block is left for the coder; and without a base
    const redux::hip::Blocks self = redux::hip::compress_blocks_const(data.data(), data.size(), data.data(), data.size(), block, E, P, flags);
    if (self.data.size() != flags.size() || redux::hip::decompress_blocks_const(self, flags, data.data(), data.size(), data.size(), block, E, P) != data) {
        std::fprintf(stderr, "the file against itself: %zu bytes for %zu blocks, or a differing round trip\n", self.data.size(), flags.size());
        return 1;
    }
    const redux::hip::Blocks nobase = redux::hip::compress_blocks_const(data.data(), data.size(), nullptr, 0, block, E, P, noflags);
    if (redux::hip::decompress_blocks_const(nobase, noflags, nullptr, 0, data.size(), block, E, P) != data) {
        std::fprintf(stderr, "without a base: a differing round trip\n");
        return 1;
    }
    std::printf("const mirror ok: %zu bytes -> %zu bytes (%zu without the option), %zu of %zu blocks constant\n", data.size(), s.data.size(),
                plain.data.size(), nconst, flags.size());
    return 0;
}
