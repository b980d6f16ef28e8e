// Compile-only check (tests/test_shim_ft4_decode_reports.py): cwslgpu::Context::fetchFt4DecodeReports / ft4Tones are self-contained C++17 against
// the C ABI, and the FT4 call reuses cwslg_decode_report as it is.
#include "../include/cwsl_gpu_shim.hpp"

#include <cstddef>

static_assert(sizeof(cwslg_decode_report) == 16, "cwslg_decode_report is 16 bytes");
static_assert(offsetof(cwslg_decode_report, nsync) == 12 && offsetof(cwslg_decode_report, nsymerr) == 14, "layout");
static_assert(sizeof(cwslg_decode) == 40, "cwslg_decode stays 40 bytes");
static_assert(CWSLG_ABI_VERSION == 5, "two exports are added, the ABI version stays");

int ft4_spot_path(cwslgpu::Context &ctx)
{
    std::vector<cwslg_decode> dec;
    std::vector<cwslg_decode_report> rep;
    std::uint64_t epoch = 0;
    int channels = 0;
    const int total = ctx.fetchFt4DecodeReports(dec, rep, epoch, 4096, &channels);
    int good = 0;
    for (std::size_t p = 0; p < dec.size(); ++p) {
        const std::array<std::uint8_t, 103> tones = ctx.ft4Tones(dec[p].bits);
        if (rep[p].nsymerr <= 30 && rep[p].nsync >= 8 && rep[p].snr_db >= -21.0f && tones[0] == 0 && tones[102] == 1) ++good;
    }
    return total - good + channels;
}
