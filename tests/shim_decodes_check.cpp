// Compile-only check of cwslgpu::Context::fetchDecodes and the cwslg_decode layout against the C ABI (C++17, stand-alone).
#include "../include/cwsl_gpu_shim.hpp"
#include <cstddef>
static_assert(sizeof(cwslg_decode) == 40, "cwslg_decode is 40 bytes");
static_assert(offsetof(cwslg_decode, entry) == 4 && offsetof(cwslg_decode, by_osd) == 6 && offsetof(cwslg_decode, set) == 7, "head");
static_assert(offsetof(cwslg_decode, bits) == 8 && offsetof(cwslg_decode, freq_hz) == 20 && offsetof(cwslg_decode, dmin) == 32, "body");
static_assert(offsetof(cwslg_decode, nharderr) == 36 && offsetof(cwslg_decode, ndup) == 38, "tail");
int shim_decodes_check()
{
    cwslgpu::Context ctx(0);
    std::vector<cwslg_decode> words;
    std::uint64_t epoch = 0;
    int channels = 0;
    const int total = ctx.fetchDecodes(CWSLG_GROUP_FT8, words, epoch, 100, &channels);
    std::uint64_t again = epoch;
    const int total4 = ctx.fetchDecodes(CWSLG_GROUP_FT4, words, again);
    int osd = 0;
    for (const cwslg_decode &w : words) osd += w.by_osd + w.ndup + w.bits[0];
    return total + total4 + channels + osd + static_cast<int>(words.size());
}
