// Compile-only check of the shim's FT4 soft-bit wrappers (Context::enableFt4Softbits, SsbChannel::fetchFt4Softbits) against the C ABI.
#include "../include/cwsl_gpu_shim.hpp"
int shim_ft4_softbits_check()
{
    static_assert(sizeof(cwslg_ft4_soft) == 2112, "cwslg_ft4_soft is 2112 bytes");
    cwslgpu::Context ctx(0);
    ctx.enableFt4Softbits();
    cwslgpu::ReceiverPort rx(ctx, 48000, 1024, 14000000);
    cwslgpu::SsbChannel ch(rx, 7000.0, true, "FT4");
    std::vector<cwslg_ft4_soft> soft;
    std::uint64_t t0 = 0;
    const int n = ch.fetchFt4Softbits(soft, 300, &t0);
    ctx.enableFt4Softbits(false);
    return n > 0 ? soft[0].nsync + soft[0].nqual : 0;
}
