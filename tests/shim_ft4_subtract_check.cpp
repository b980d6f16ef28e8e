// Compile-only check (tests/test_shim_ft4_subtract.py): cwslgpu::Context::subtractFt4 / ft4Residual / ft4ResidualDevice / ft4SubtractFlat and the
// layouts of cwslg_subtract_report and cwslg_ft4_sub_item are self-contained C++17 against the C ABI.
#include "../include/cwsl_gpu_shim.hpp"

#include <cstddef>

static_assert(sizeof(cwslg_subtract_report) == 28, "cwslg_subtract_report is 28 bytes");
static_assert(offsetof(cwslg_subtract_report, n_inside) == 20 && offsetof(cwslg_subtract_report, df_steps) == 24 && offsetof(cwslg_subtract_report, dt_steps) == 26, "layout");
static_assert(sizeof(cwslg_ft4_sub_item) == 24 && offsetof(cwslg_ft4_sub_item, frame) == 0 && offsetof(cwslg_ft4_sub_item, bits) == 4, "layout");
static_assert(offsetof(cwslg_ft4_sub_item, freq_hz) == 16 && offsetof(cwslg_ft4_sub_item, dt_s) == 20, "layout");
static_assert(sizeof(cwslg_ft4_sub_item) == sizeof(cwslg_ft8_sub_item), "the FT8 item's layout");
static_assert(CWSLG_FT4_FRAME_SAMPLES == 72576 && CWSLG_FT4_FRAME_SAMPLES % 4 == 0, "the decoder's frame");
static_assert(CWSLG_ABI_VERSION == 5, "exports only added");

int residual_path(cwslgpu::Context &ctx)
{
    std::vector<cwslg_decode> dec;
    std::vector<cwslg_subtract_report> sub;
    std::uint64_t epoch = 0;
    int channels = 0;
    const int total = ctx.subtractFt4(dec, sub, epoch, 4096, &channels);
    int handed = 0;
    std::vector<float> residual;
    for (std::size_t p = 0; p < dec.size(); ++p) {
        const float *d = nullptr;
        std::uint64_t e = 0;
        if (sub[p].p_removed > 0.0f && sub[p].n_inside > 0 && ctx.ft4Residual(dec[p].ch_id, residual, &e) && ctx.ft4ResidualDevice(dec[p].ch_id, d) && e == epoch) ++handed;
    }
    std::vector<cwslg_ft4_sub_item> items(1);
    std::vector<float> audio(CWSLG_FT4_FRAME_SAMPLES), out;
    ctx.ft4SubtractFlat(audio.data(), 1, items, sub, &out);
    return total - handed + channels + static_cast<int>(out.size());
}
