// Check of the shim's FT4 a-priori wrappers against the C ABI.  Compiled -fsyntax-only for the wrappers (Context::setFt4Ap,
// Context::fetchFt4Ap); with -DSHIM_FT4_AP_CHECK_MAIN it is a program that needs no library and no GPU: apSetSplit of every byte value, one
// "set metric-set pattern" line each (tests/test_shim_ft4_ap.py compares them with api.ap_set_split).
#include <cstddef>
#include <cstdio>
#include "../include/cwsl_gpu_shim.hpp"

static_assert(sizeof(cwslg_ap_pattern) == 24 && sizeof(cwslg_decode) == 40 && offsetof(cwslg_decode, set) == 7, "record layouts");
static_assert(CWSLG_ABI_VERSION == 5, "exports are only added");

#ifndef SHIM_FT4_AP_CHECK_MAIN
int shim_ft4_ap_check(const std::uint8_t *nm)
{
    cwslgpu::Context ctx(0);
    ctx.setLdpcCode(nm);
    std::vector<cwslg_ap_pattern> pat(2);
    pat[0].mask[0] = 0xff; pat[0].value[0] = 0x5a;
    ctx.setFt4Ap(pat);
    ctx.setFt4Ap(pat.data(), 1, 50, 10, 22);
    std::vector<cwslg_decode> dec, ap;
    std::uint64_t t0 = 0;
    int nch = 0;
    const int total = ctx.fetchDecodes(CWSLG_GROUP_FT4, dec, t0);
    const int total_ap = ctx.fetchFt4Ap(ap, t0, 100, &nch);
    ctx.setFt4Ap(std::vector<cwslg_ap_pattern>());
    const std::array<int, 2> sp = ap.empty() ? std::array<int, 2>{0, 0} : cwslgpu::apSetSplit(ap[0].set);
    return (int)cwslgpu::mergeApDecodes(dec, ap).size() + total + total_ap + sp[0] + sp[1];
}
#else
int main()
{
    for (int v = 0; v < 256; ++v) {
        const std::array<int, 2> sp = cwslgpu::apSetSplit((std::uint8_t)v);
        std::printf("%d %d %d\n", v, sp[0], sp[1]);
    }
    return 0;
}
#endif
