// Compile-only check (tests/test_shim_decode_reports.py): cwslgpu::Context::fetchDecodeReports / ft8Tones and the layout of cwslg_decode_report
// are self-contained C++17 against the C ABI.
#include "../include/cwsl_gpu_shim.hpp"

#include <cstddef>

static_assert(sizeof(cwslg_decode_report) == 16, "cwslg_decode_report is 16 bytes");
static_assert(offsetof(cwslg_decode_report, snr_db) == 0 && offsetof(cwslg_decode_report, xsig) == 4 && offsetof(cwslg_decode_report, xnoise) == 8, "layout");
static_assert(offsetof(cwslg_decode_report, nsync) == 12 && offsetof(cwslg_decode_report, nsymerr) == 14, "layout");
static_assert(sizeof(cwslg_decode) == 40, "cwslg_decode stays 40 bytes");

int spot_path(cwslgpu::Context &ctx)
{
    std::vector<cwslg_decode> dec;
    std::vector<cwslg_decode_report> rep;
    std::uint64_t epoch = 0;
    int channels = 0;
    const int total = ctx.fetchDecodeReports(CWSLG_GROUP_FT8, dec, rep, epoch, 4096, &channels);
    int good = 0;
    for (std::size_t p = 0; p < dec.size(); ++p) {
        const std::array<std::uint8_t, 79> tones = ctx.ft8Tones(dec[p].bits);
        if (rep[p].nsymerr <= 20 && rep[p].snr_db >= -24.0f && tones[0] == 3) ++good;
    }
    return total - good + channels;
}
