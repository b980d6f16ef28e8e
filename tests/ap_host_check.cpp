// ap_host_check.cpp -- stand-alone host program over csrc/ap_host.hpp: the validation of AP patterns and the block the kernel reads.
//   ap_host_check in.bin out.bin
// in:  uint32 n_sets; per set: int32 n_pat, uint32 n_given, n_given x 24 bytes (cwslg_ap_pattern)
// out: per set: int32 reason (ap_pack's), then 192 bytes of block -- the packed block on success, 0xEE bytes otherwise (ap_pack must not touch it)
// tests/test_ap_ref.py compares both with tests/ap_ref.py, plain and under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../cwsl_digi_amd/csrc/ap_host.hpp"

using namespace cwslg;

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::perror("open"); return 2; }
    uint32_t n_sets = 0;
    if (std::fread(&n_sets, 4, 1, in) != 1) return 2;
    for (uint32_t s = 0; s < n_sets; ++s) {
        int32_t n_pat = 0;
        uint32_t n_given = 0;
        if (std::fread(&n_pat, 4, 1, in) != 1 || std::fread(&n_given, 4, 1, in) != 1) return 2;
        std::vector<ApPattern> pat(n_given);                 // exactly as many as given: a read beyond them is the sanitizer's to find
        if (n_given && std::fread(pat.data(), sizeof(ApPattern), n_given, in) != n_given) return 2;
        ApBlock b;
        std::memset(&b, 0xEE, sizeof(b));
        const int32_t why = ap_pack(n_given ? pat.data() : nullptr, n_pat, &b);
        std::fwrite(&why, 4, 1, out);
        std::fwrite(&b, sizeof(b), 1, out);
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 2;
}
