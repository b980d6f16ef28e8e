// Compiled with -fsyntax-only -Wall -Werror by tests/test_ft4_osd_inputs.py: the shim's FT4 OSD surface and the record layout as C++ sees them.
#include "../include/cwsl_gpu_shim.hpp"

static_assert(sizeof(cwslg_ft4_osd) == 72 && sizeof(cwslg_osd_msg) == 24, "cwslg_ft4_osd is three cwslg_osd_msg");

int shim_ft4_osd_check(cwslgpu::Context &ctx, cwslgpu::SsbChannel &ch)
{
    ctx.enableFt4Osd();
    ctx.enableFt4Osd(true, 1, 8, 20);
    std::vector<cwslg_ft4_msg> msg;
    std::vector<cwslg_ft4_osd> osd;
    std::uint64_t t0 = 0;
    const int n = ch.fetchFt4Osd(osd, 1800, &t0);
    int words = 0;
    if (ch.fetchFt4Decode(msg) == n)
        for (int q = 0; q < n; ++q) {
            bool byOsd = false;
            const int s = cwslgpu::ft4BestWord(msg[q], osd[q], &byOsd);
            if (s >= 0 && (byOsd ? osd[q].set[s].crc_ok : msg[q].set[s].crc_ok)) ++words;
            if (cwslgpu::ft4BestWord(msg[q], osd[q]) != s) return -1;
        }
    ctx.enableFt4Osd(false);
    return words;
}
