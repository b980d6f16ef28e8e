// Compile-only check of the shim's FT8 OSD wrappers (Context::enableFt8Osd, Context::osdDecode, SsbChannel::fetchFt8Osd) against the C ABI.
#include <cstddef>
#include "../include/cwsl_gpu_shim.hpp"
int shim_ft8_osd_check(const std::uint8_t *nm, const float *llr)
{
    static_assert(sizeof(cwslg_osd_msg) == 24, "cwslg_osd_msg is 24 bytes");
    static_assert(offsetof(cwslg_osd_msg, dmin) == 12 && offsetof(cwslg_osd_msg, nharderr) == 16 && offsetof(cwslg_osd_msg, nskip) == 18, "record layout");
    static_assert(offsetof(cwslg_osd_msg, crc_ok) == 20 && offsetof(cwslg_osd_msg, how) == 21 && offsetof(cwslg_osd_msg, flip) == 22, "record layout");
    static_assert(CWSLG_ABI_VERSION == 5, "exports are only added");
    cwslgpu::Context ctx(0);
    ctx.setLdpcCode(nm);
    ctx.enableFt8Softbits();
    ctx.enableFt8Decode();
    ctx.enableFt8Osd();
    ctx.enableFt8Osd(true, 1, 10);
    std::vector<cwslg_osd_msg> flat;
    ctx.osdDecode(llr, 3, flat);
    ctx.osdDecode(llr, 3, flat, 0);
    cwslgpu::ReceiverPort rx(ctx, 48000, 1024, 14000000);
    cwslgpu::SsbChannel ch(rx, 7000.0, true, "FT8");
    std::vector<cwslg_osd_msg> msg;
    std::uint64_t t0 = 0;
    const int n = ch.fetchFt8Osd(msg, 300, &t0);
    ctx.enableFt8Osd(false);
    return n > 0 ? msg[0].how : (int)flat.size();
}
