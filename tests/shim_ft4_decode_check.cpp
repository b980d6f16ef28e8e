// Compile-only check of the shim's FT4 decode wrappers (Context::enableFt4Decode, SsbChannel::fetchFt4Decode, ft4BestSet) against the C ABI.
#include "../include/cwsl_gpu_shim.hpp"
int shim_ft4_decode_check(const std::uint8_t *nm)
{
    static_assert(sizeof(cwslg_ft4_msg) == 60, "cwslg_ft4_msg is 60 bytes");
    static_assert(sizeof(cwslg_ft4_msg) == 3 * sizeof(cwslg_ft8_msg), "three cwslg_ft8_msg");
    static_assert(CWSLG_ABI_VERSION == 5, "exports are only added");
    cwslgpu::Context ctx(0);
    ctx.setLdpcCode(nm);
    ctx.enableFt4Softbits();
    ctx.enableFt4Decode();
    ctx.enableFt4Decode(true, 30, 8, 20);
    cwslgpu::ReceiverPort rx(ctx, 48000, 1024, 14000000);
    cwslgpu::SsbChannel ch(rx, 7000.0, true, "FT4");
    std::vector<cwslg_ft4_msg> msg;
    std::uint64_t t0 = 0;
    const int n = ch.fetchFt4Decode(msg, 300, &t0);
    ctx.enableFt4Decode(false);
    return n > 0 ? cwslgpu::ft4BestSet(msg[0]) : -1;
}
