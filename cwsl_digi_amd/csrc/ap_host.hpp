// ap_host.hpp -- the parts of FT8 a-priori decoding that are plain C++: the validation of a caller's patterns and the block the kernel reads.
// The library (ap_kernels.hpp, sync_host.inc) and a stand-alone host program (tests/ap_host_check.cpp) both compile this file;
// include/cwsl_gpu.h states the contract (cwslg_ap_pattern) and tests/ap_ref.py restates it in numpy.
#pragma once
#include <stdint.h>
#include <string.h>

namespace cwslg {

constexpr int AP_MAXPAT = 8, AP_PAT_BYTES = 12, AP_PAT_WORDS = 6;

// What the kernel reads (device copy: one 192-byte block).  Pattern p is six dwords in BALLOT order -- codeword bit t at bit t & 31 of word t >> 5,
// the order in which a wave's ballot over "lane l owns bit l / l + 64" holds a codeword -- so that a lane's own mask and value bits are one shift
// away and "the word agrees with the pattern" is three ANDs:  w[p][0..2] = mask bits 0..31, 32..63, 64..90;  w[p][3..5] = value, likewise.
struct ApBlock { uint32_t w[AP_MAXPAT][AP_PAT_WORDS]; };
static_assert(sizeof(ApBlock) == 192, "pattern block");

// One caller's pattern as the header lays it out: codeword bit t at byte[t >> 3] & (0x80 >> (t & 7)), mask then value.
struct ApPattern { uint8_t mask[AP_PAT_BYTES]; uint8_t value[AP_PAT_BYTES]; };
static_assert(sizeof(ApPattern) == 24, "cwslg_ap_pattern is 24 bytes");

inline unsigned ap_bit(const uint8_t *b, int t) { return (unsigned)(b[t >> 3] >> (7 - (t & 7))) & 1u; }

// Validate n_pat patterns and pack them.  Returns 0, or a reason 1..3: 1 n_pat outside 0..8 (or a null array with n_pat > 0), 2 a mask or value
// bit at position 91..95, 3 a value bit outside its mask.  Patterns are read in order, positions in order, and the first finding is returned;
// *out is written only on success (patterns n_pat..7 are zero).
inline int ap_pack(const ApPattern *pat, int n_pat, ApBlock *out)
{
    if (n_pat < 0 || n_pat > AP_MAXPAT || (n_pat > 0 && !pat)) return 1;
    ApBlock b;
    memset(&b, 0, sizeof(b));
    for (int p = 0; p < n_pat; ++p)
        for (int t = 0; t < 8 * AP_PAT_BYTES; ++t) {
            const unsigned m = ap_bit(pat[p].mask, t), v = ap_bit(pat[p].value, t);
            if (t >= 91 && (m | v)) return 2;
            if (v && !m) return 3;
            b.w[p][t >> 5] |= m << (t & 31);
            b.w[p][3 + (t >> 5)] |= v << (t & 31);
        }
    if (out) *out = b;
    return 0;
}

} // namespace cwslg
