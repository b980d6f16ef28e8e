// ldpc_host.hpp -- the parts of the LDPC(174,91) decode that are plain C++: the two scalar functions of the message update (T, A), the CRC-14,
// the validation of a caller's parity-check table and the tables derived from it.  The library (ldpc_kernels.hpp, sync_host.inc) and a stand-alone
// host program (tests/ldpc_host_check.cpp, g++ -ffp-contract=off) both compile this file; include/cwsl_gpu.h states the contract and
// tests/ldpc_ref.py restates it in numpy.  Every operation is ONE float32 operation: the including translation unit is built -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LDPC_HD __host__ __device__ __forceinline__
#else
#define LDPC_HD inline
#endif

namespace cwslg {

constexpr int LDPC_N = 174, LDPC_K = 91, LDPC_M = 83, LDPC_ROWMAX = 7, LDPC_EDGES = 522;
constexpr int LDPC_EPITCH = 8;             // an edge's position in the message arrays: 8 m + e
constexpr int LDPC_ABSENT = 255;           // rowbit entry of an edge that does not exist (e = 6 of a weight-6 row, rows 83..127)

// T(x): tanh(x) as the [5/4] Pade form, 1 from |x| = 4.97 on
LDPC_HD float ldpc_T(float x)
{
    const float a = fabsf(x);
    float r = 1.0f;
    if (!(a >= 4.97f)) {
        const float x2 = a * a;
        const float num = a * (945.0f + x2 * (105.0f + x2));
        const float den = 945.0f + x2 * (420.0f + x2 * 15.0f);
        r = fminf(num / den, 1.0f);
    }
    return copysignf(r, x);
}

// A(y): atanh(y) in four straight pieces (upstream platanh), 7 beyond 0.9998
LDPC_HD float ldpc_A(float y)
{
    const float z = fabsf(y);
    float r;
    if (z <= 0.664f) r = z / 0.83f;
    else if (z <= 0.9217f) r = (z - 0.4064f) / 0.322f;
    else if (z <= 0.9951f) r = (z - 0.8378f) / 0.0524f;
    else if (z <= 0.9998f) r = (z - 0.9914f) / 0.0012f;
    else r = 7.0f;
    return copysignf(r, y);
}

// CRC-14 (polynomial 0x2757, x^14 implicit; bit-serial, MSB first, initial remainder 0) of codeword bits 0..76 followed by 5 zero bits and the 14
// augmenting zero bits: the remainder of M(x) x^14 for the 82-bit M.  Codeword bit t is bit t of lo (t < 64) or bit t - 64 of hi.
LDPC_HD unsigned ldpc_cw_bit(uint64_t lo, uint64_t hi, int t) { return (unsigned)((t < 64 ? lo >> t : hi >> (t - 64)) & 1u); }
LDPC_HD unsigned ldpc_crc14(uint64_t lo, uint64_t hi)
{
    unsigned rem = 0;
    for (int i = 0; i < 77 + 5 + 14; ++i) {
        rem = (rem << 1) | (i < 77 ? ldpc_cw_bit(lo, hi, i) : 0u);
        if (rem & 0x4000u) rem ^= 0x6757u;
    }
    return rem;
}
// bits 77..90, MSB first
LDPC_HD unsigned ldpc_crc_field(uint64_t lo, uint64_t hi)
{
    unsigned v = 0;
    for (int i = 0; i < 14; ++i) v = (v << 1) | ldpc_cw_bit(lo, hi, 77 + i);
    return v;
}

// What the kernel reads (device copy: one 2560-byte block).  rowbit[m][e]: the 0-based bit of edge e of row m, LDPC_ABSENT where there is none
// (rows 83..127 are all absent: a wave's lanes 19..63 read them for their second row).  epos[n][k]: the position 8 m + e of bit n's edge to its
// k-th check in ascending row order (bits 174..191: 0, never used); epos[n][3] = 0.
struct LdpcTables {
    uint8_t rowbit[128][LDPC_EPITCH];
    uint16_t epos[192][4];
};
static_assert(sizeof(LdpcTables) == 2560, "table block");

// Validate nm[83][7] (1-based positions, a weight-6 row ends in one 0) and derive the tables.  Returns 0, or a reason 1..4:
// 1 a position out of range, 2 a zero that is not the last entry of its row (row weight below 6 included), 3 a position twice in one row,
// 4 a position that does not occur exactly three times.
inline int ldpc_derive(const uint8_t *nm, LdpcTables *out)
{
    LdpcTables t;
    memset(&t, 0, sizeof(t));
    memset(t.rowbit, LDPC_ABSENT, sizeof(t.rowbit));
    int count[LDPC_N] = {0};
    for (int m = 0; m < LDPC_M; ++m) {
        for (int e = 0; e < LDPC_ROWMAX; ++e) {
            const int v = nm[m * LDPC_ROWMAX + e];
            if (v > LDPC_N) return 1;
            if (v == 0) {
                if (e != LDPC_ROWMAX - 1) return 2;
                continue;
            }
            for (int f = 0; f < e; ++f) if (nm[m * LDPC_ROWMAX + f] == v) return 3;
            const int n = v - 1;
            if (count[n] >= 3) return 4;
            t.rowbit[m][e] = (uint8_t)n;
            t.epos[n][count[n]++] = (uint16_t)(LDPC_EPITCH * m + e);       // rows are visited in ascending order: c(n,0) < c(n,1) < c(n,2)
        }
    }
    for (int n = 0; n < LDPC_N; ++n) if (count[n] != 3) return 4;
    if (out) *out = t;
    return 0;
}

} // namespace cwslg
