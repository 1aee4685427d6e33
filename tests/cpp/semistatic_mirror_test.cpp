// Semi-static coding through the C++ mirror (redux_amd/host/redux.hpp): the table of a file, every block coded under it,
// decoded again.  `semistatic_mirror_test <file>`; prints "semistatic mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <fstream>
#include <iterator>

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <file>\n", argv[0]);
        return 2;
    }
    std::ifstream f(argv[1], std::ios::binary);
    const std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint32_t block = 4096;
    const std::vector<std::uint32_t> cum = redux::hip::static_table(data.data(), data.size(), P);
    if (cum.size() != 258 || cum[0] != 0 || cum[257] != 65536) {
        std::fprintf(stderr, "unexpected table total %u\n", cum.empty() ? 0u : cum[257]);
        return 1;
    }
    const redux::hip::Blocks s = redux::hip::compress_blocks_static(data.data(), data.size(), block, P, cum);
    std::vector<std::uint32_t> sizes;
    const std::vector<std::uint8_t> back = redux::hip::decompress_blocks_static(s, block, P, cum, &sizes);
    std::uint64_t pos = 0;
    for (std::size_t b = 0; b < sizes.size(); b++) {
        for (std::uint32_t i = 0; i < sizes[b]; i++)
            if (back[b * (std::uint64_t)block + i] != data[pos + i]) {
                std::fprintf(stderr, "block %zu differs\n", b);
                return 1;
            }
        pos += sizes[b];
    }
    if (pos != data.size()) {
        std::fprintf(stderr, "decoded %llu of %zu bytes\n", (unsigned long long)pos, data.size());
        return 1;
    }
    std::vector<std::uint32_t> bad = cum;
    bad[1] = 0; // a zero frequency: rejected before any device call
    try {
        redux::hip::compress_blocks_static(data.data(), data.size(), block, P, bad);
        std::fprintf(stderr, "a bad table was accepted\n");
        return 1;
    } catch (const redux::Error &e) {
        if (e.kind() != redux::Error::InvalidInput)
            return 1;
    }
    std::printf("semistatic mirror ok: %zu bytes -> %zu bytes\n", data.size(), s.data.size());
    return 0;
}
