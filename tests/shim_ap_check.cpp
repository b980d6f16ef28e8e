// Check of the shim's FT8 a-priori wrappers against the C ABI.  Compiled -fsyntax-only for the wrappers (Context::setFt8Ap, Context::apDecode,
// Context::fetchFt8Ap); with -DSHIM_AP_CHECK_MAIN it is a program that needs no library and no GPU: mergeApDecodes on records read from stdin,
// the merged records written to stdout (tests/test_shim_ap.py compares them with api.merge_ap_decodes).
#include <cstddef>
#include <cstdio>
#include "../include/cwsl_gpu_shim.hpp"

static_assert(sizeof(cwslg_ap_pattern) == 24 && offsetof(cwslg_ap_pattern, value) == 12, "cwslg_ap_pattern is 24 bytes");
static_assert(sizeof(cwslg_ap_msg) == 24 && offsetof(cwslg_ap_msg, dmin) == 20, "cwslg_ap_msg is 24 bytes");
static_assert(sizeof(cwslg_decode) == 40, "cwslg_decode is 40 bytes");
static_assert(CWSLG_ABI_VERSION == 5, "exports are only added");

#ifndef SHIM_AP_CHECK_MAIN
int shim_ap_check(const std::uint8_t *nm, const float *llr)
{
    cwslgpu::Context ctx(0);
    ctx.setLdpcCode(nm);
    std::vector<cwslg_ap_pattern> pat(2);
    pat[0].mask[0] = 0xff; pat[0].value[0] = 0x5a;
    ctx.setFt8Ap(pat);
    ctx.setFt8Ap(pat.data(), 1, 50, 10);
    std::vector<cwslg_ap_msg> flat;
    ctx.apDecode(llr, 3, flat);
    std::vector<cwslg_decode> dec, ap;
    std::uint64_t t0 = 0;
    int nch = 0;
    const int total = ctx.fetchDecodes(CWSLG_GROUP_FT8, dec, t0);
    const int total_ap = ctx.fetchFt8Ap(ap, t0, 100, &nch);
    ctx.setFt8Ap(std::vector<cwslg_ap_pattern>());
    return (int)cwslgpu::mergeApDecodes(dec, ap).size() + total + total_ap + (flat.empty() ? 0 : flat[0].msg.pad_);
}
#else
// stdin: uint32 n_dec, uint32 n_ap, then the records; stdout: the merged records
int main()
{
    std::uint32_t n[2] = {0, 0};
    if (std::fread(n, 4, 2, stdin) != 2) return 2;
    std::vector<cwslg_decode> dec(n[0]), ap(n[1]);
    if (n[0] && std::fread(dec.data(), sizeof(cwslg_decode), n[0], stdin) != n[0]) return 2;
    if (n[1] && std::fread(ap.data(), sizeof(cwslg_decode), n[1], stdin) != n[1]) return 2;
    const std::vector<cwslg_decode> out = cwslgpu::mergeApDecodes(dec, ap);
    if (!out.empty() && std::fwrite(out.data(), sizeof(cwslg_decode), out.size(), stdout) != out.size()) return 2;
    return 0;
}
#endif
