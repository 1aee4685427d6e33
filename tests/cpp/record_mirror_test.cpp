// The record layout through the C++ mirror (redux_amd/host/redux.hpp): a table of 20-byte structs coded plain, behind the
// record layout and behind the layout with the byte delta, decoded again; and the refusals that come before any device call.
// `record_mirror_test --gpu` (or `--no-gpu`: the refusals alone); prints "record mirror ok" on success.
#include "../../redux_amd/host/redux.hpp"

#include <cstdio>
#include <cstring>

static int refusals()
{
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const std::uint8_t x[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    redux::hip::Blocks none;
    none.offsets = {0, 0};
    for (int which = 0; which < 7; which++) {
        try {
            if (which == 0)
                redux::hip::compress_blocks_record(x, 8, 0, 3, true, P); // block size 0
            else if (which == 1)
                redux::hip::compress_blocks_record(x, 8, 4, 0, true, P); // record size 0
            else if (which == 2)
                redux::hip::compress_blocks_record(x, 8, 4, 1, false, P); // record size 1
            else if (which == 3)
                redux::hip::compress_blocks_record(x, 8, 4, REDUX_RECORD_MAX + 1, false, P); // above the maximum
            else if (which == 4)
                redux::hip::decompress_blocks_record(none, 4, 4, 1, true, P); // the same on the way back
            else if (which == 5)
                redux::hip::decompress_blocks_record(none, 4, 0, 3, true, P);
            else
                redux::hip::decompress_blocks_record(none, 8, 4, 3, true, P); // one stream for two blocks
            std::fprintf(stderr, "refusal %d was accepted\n", which);
            return 1;
        } catch (const redux::Error &e) {
            if (e.kind() != redux::Error::InvalidInput) {
                std::fprintf(stderr, "refusal %d: another error\n", which);
                return 1;
            }
        }
    }
    for (std::uint32_t R = 2; R <= REDUX_RECORD_MAX; R++)
        if (redux_record_check(R, 0) != REDUX_OK || redux_record_check(R, 1) != REDUX_OK) {
            std::fprintf(stderr, "a legal record size was refused\n");
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
        std::printf("record mirror host-side checks ok\n");
        return 0;
    }
    // records of {u32 id; i32 px; u16 qty; u8 side; u8 pad; u64 ts}: two frames of 4096 records and 100 more, plus 7 trailing bytes
    const std::uint32_t block = 4096, R = 20;
    const std::size_t   n = 2 * block + 100;
    std::vector<std::uint8_t> data(n * R + 7, 0x5A);
    std::uint64_t lcg = 20261021, ts = 1700000000000ull;
    std::int32_t  px = 100000;
    for (std::size_t i = 0; i < n; i++) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        const std::uint32_t r = (std::uint32_t)(lcg >> 33);
        const std::uint32_t id = (std::uint32_t)i + r % 3;
        px += (std::int32_t)(r / 3 % 11) - 5;
        const std::uint16_t qty = (std::uint16_t)(1 + r / 33 % 40);
        const std::uint8_t  side = (std::uint8_t)(r >> 20 & 1), padb = 0;
        ts += r >> 22 & 31;
        std::uint8_t *o = &data[i * R];
        std::memcpy(o, &id, 4); std::memcpy(o + 4, &px, 4); std::memcpy(o + 8, &qty, 2);
        o[10] = side; o[11] = padb; std::memcpy(o + 12, &ts, 8);
    }
    const auto P = redux::model::Parameters::make(8, 30, 32);
    const redux::hip::Blocks plain = redux::hip::compress_blocks(data.data(), data.size(), block, P);
    std::size_t bytes[2];
    for (int delta = 0; delta < 2; delta++) {
        const redux::hip::Blocks b = redux::hip::compress_blocks_record(data.data(), data.size(), block, R, delta != 0, P);
        if (redux::hip::decompress_blocks_record(b, data.size(), block, R, delta != 0, P) != data) {
            std::fprintf(stderr, "the round trip with delta %d differs\n", delta);
            return 1;
        }
        bytes[delta] = b.data.size();
    }
    if (bytes[1] * 10 > plain.data.size() * 9) {
        std::fprintf(stderr, "the layout with the delta did not pay: %zu against %zu bytes\n", bytes[1], plain.data.size());
        return 1;
    }
    std::printf("record mirror ok: %zu bytes -> %zu plain / %zu record layout / %zu with the delta\n", data.size(), plain.data.size(),
                bytes[0], bytes[1]);
    return 0;
}
