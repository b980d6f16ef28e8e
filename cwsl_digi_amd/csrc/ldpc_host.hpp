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

// ---- ordered-statistics decoding (cwslg_osd_msg in include/cwsl_gpu.h; tests/osd_ref.py restates it) ----------------------------------------------
// A generator of the code: 91 rows of 174 bits, 6 dwords per row (codeword bit t at row[t >> 5] bit t & 31; bits 174..191 are 0) -- one 2184-byte
// device block.  Which basis of the null space it is does not matter to the result (the most reliable basis is reduced from whatever it starts with).
constexpr int OSD_GW = 6, OSD_NPAIR = LDPC_K * (LDPC_K - 1) / 2;
struct OsdGen { uint32_t row[LDPC_K][OSD_GW]; };
static_assert(sizeof(OsdGen) == 2184, "generator block");
struct OsdRec { uint8_t bits[12]; float dmin; int16_t nharderr, nskip; uint8_t crc_ok, how, flip[2]; };    // = cwslg_osd_msg
static_assert(sizeof(OsdRec) == 24, "cwslg_osd_msg is 24 bytes");

// Rank of H over GF(2), and -- when it is 83 and gen != nullptr -- the generator whose row k carries free column f_k (ascending) alone among the
// free columns: bit f_k, and at pivot column c_r the entry of reduced row r in column f_k.
inline int ldpc_generator(const LdpcTables &t, OsdGen *gen)
{
    uint32_t h[LDPC_M][OSD_GW];
    memset(h, 0, sizeof(h));
    for (int m = 0; m < LDPC_M; ++m)
        for (int e = 0; e < LDPC_ROWMAX; ++e)
            if (t.rowbit[m][e] != LDPC_ABSENT) h[m][t.rowbit[m][e] >> 5] ^= 1u << (t.rowbit[m][e] & 31);
    int pivcol[LDPC_M], rank = 0;
    bool is_piv[LDPC_N] = {false};
    for (int c = 0; c < LDPC_N && rank < LDPC_M; ++c) {
        int r = rank;
        while (r < LDPC_M && !((h[r][c >> 5] >> (c & 31)) & 1u)) ++r;
        if (r == LDPC_M) continue;
        for (int w = 0; w < OSD_GW; ++w) { const uint32_t x = h[r][w]; h[r][w] = h[rank][w]; h[rank][w] = x; }
        for (int i = 0; i < LDPC_M; ++i)
            if (i != rank && ((h[i][c >> 5] >> (c & 31)) & 1u))
                for (int w = 0; w < OSD_GW; ++w) h[i][w] ^= h[rank][w];
        pivcol[rank++] = c;
        is_piv[c] = true;
    }
    if (rank != LDPC_M || !gen) return rank;
    memset(gen, 0, sizeof(*gen));
    int k = 0;
    for (int f = 0; f < LDPC_N; ++f) {
        if (is_piv[f]) continue;
        gen->row[k][f >> 5] |= 1u << (f & 31);
        for (int r = 0; r < LDPC_M; ++r)
            if ((h[r][f >> 5] >> (f & 31)) & 1u) gen->row[k][pivcol[r] >> 5] |= 1u << (pivcol[r] & 31);
        ++k;
    }
    return rank;
}

// ---- re-encoding (cwslg_decode_report in include/cwsl_gpu.h; tests/decode_reports_ref.py restates it) ----------------------------------------------
// The systematic encoder of the loaded code in the OsdGen layout: row k (k = 0..90) is the codeword of the unit message e_k -- bit k, and the parity
// bits 91..173 that H demands.  H is reduced taking pivots in columns 91..173 only; false (and *enc untouched) when those 83 columns are singular:
// such a table is still a code the decoders take, but a 91-bit word then has no codeword that merely continues it.
inline bool ldpc_encoder(const LdpcTables &t, OsdGen *enc)
{
    uint32_t h[LDPC_M][OSD_GW];
    memset(h, 0, sizeof(h));
    for (int m = 0; m < LDPC_M; ++m)
        for (int e = 0; e < LDPC_ROWMAX; ++e)
            if (t.rowbit[m][e] != LDPC_ABSENT) h[m][t.rowbit[m][e] >> 5] ^= 1u << (t.rowbit[m][e] & 31);
    for (int r = 0; r < LDPC_M; ++r) {                         // reduced row r ends up with column 91 + r alone among the parity columns
        const int c = LDPC_K + r;
        int p = r;
        while (p < LDPC_M && !((h[p][c >> 5] >> (c & 31)) & 1u)) ++p;
        if (p == LDPC_M) return false;
        for (int w = 0; w < OSD_GW; ++w) { const uint32_t x = h[p][w]; h[p][w] = h[r][w]; h[r][w] = x; }
        for (int i = 0; i < LDPC_M; ++i)
            if (i != r && ((h[i][c >> 5] >> (c & 31)) & 1u))
                for (int w = 0; w < OSD_GW; ++w) h[i][w] ^= h[r][w];
    }
    if (!enc) return true;
    memset(enc, 0, sizeof(*enc));
    for (int k = 0; k < LDPC_K; ++k) {
        enc->row[k][k >> 5] |= 1u << (k & 31);
        for (int r = 0; r < LDPC_M; ++r)                       // parity bit 91 + r of e_k: the entry of reduced row r in column k
            if ((h[r][k >> 5] >> (k & 31)) & 1u) enc->row[k][(LDPC_K + r) >> 5] |= 1u << ((LDPC_K + r) & 31);
    }
    return true;
}

// The 174-bit codeword (OsdGen bit layout) of the 91 message bits of bits[12] (MSB first, as cwslg_ft8_msg.bits; the last 5 bits are ignored)
inline void ldpc_encode(const OsdGen &enc, const uint8_t *bits, uint32_t *cw)
{
    for (int w = 0; w < OSD_GW; ++w) cw[w] = 0;
    for (int k = 0; k < LDPC_K; ++k)
        if ((bits[k >> 3] >> (7 - (k & 7))) & 1)
            for (int w = 0; w < OSD_GW; ++w) cw[w] ^= enc.row[k][w];
}

// The 79 channel tones of a codeword: Costas 3,1,4,0,6,5,2 at symbols 0..6, 36..42, 72..78; data symbol d (0..57) at n = d + 7 (d < 29) or
// d + 14, its tone graymap[4 cw[3d] + 2 cw[3d+1] + cw[3d+2]] -- the inverse of what ft8_softbits_kernel reads.
inline void ft8_tones_of(const uint32_t *cw, uint8_t *tones)
{
    static const uint8_t icos7[7] = {3, 1, 4, 0, 6, 5, 2}, graymap[8] = {0, 1, 3, 2, 5, 6, 4, 7};
    for (int r = 0; r < 7; ++r) tones[r] = tones[36 + r] = tones[72 + r] = icos7[r];
    for (int d = 0; d < 58; ++d) {
        unsigned v = 0;
        for (int b = 0; b < 3; ++b) v = (v << 1) | ((cw[(3 * d + b) >> 5] >> ((3 * d + b) & 31)) & 1u);
        tones[d + (d < 29 ? 7 : 14)] = graymap[v];
    }
}

// The 103 FT4 channel tones of a codeword (no rvec: descrambling stays with the consumer): Costas blocks 0132 1023 2310 3201 at symbols 0..3,
// 33..36, 66..69, 99..102; data symbol d (0..86) at n = d + 4 (d < 29), d + 8 (d < 58) or d + 12, its tone graymap[2 cw[2d] + cw[2d+1]],
// graymap = 0,1,3,2 -- the inverse of what ft4_softbits_kernel reads.
inline void ft4_tones_of(const uint32_t *cw, uint8_t *tones)
{
    static const uint8_t icos4[16] = {0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1}, graymap[4] = {0, 1, 3, 2};
    for (int b = 0; b < 4; ++b)
        for (int s = 0; s < 4; ++s) tones[33 * b + s] = icos4[4 * b + s];
    for (int d = 0; d < 87; ++d) {
        unsigned v = 0;
        for (int b = 0; b < 2; ++b) v = (v << 1) | ((cw[(2 * d + b) >> 5] >> ((2 * d + b) & 31)) & 1u);
        tones[d + (d < 29 ? 4 : d < 58 ? 8 : 12)] = graymap[v];
    }
}

// d(c) of the contract: float32 adds of a[t] over the set bits of the error pattern, ascending t
inline float osd_distance(const uint32_t *e, const float *a)
{
    float d = 0.0f;
    for (int t = 0; t < LDPC_N; ++t)
        if ((e[t >> 5] >> (t & 31)) & 1u) d = d + a[t];
    return d;
}

// The whole contract on the host, one set of metrics: what osd_decode_kernel computes (tests/osd_host_check.cpp prints it).
inline void osd_host(const OsdGen &gen, const float *llr, int order, OsdRec *out)
{
    memset(out, 0, sizeof(*out));
    out->nharderr = out->nskip = -1;
    out->how = out->flip[0] = out->flip[1] = 0xff;
    float a[LDPC_N];
    uint32_t hard[OSD_GW] = {0};
    for (int t = 0; t < LDPC_N; ++t) {
        a[t] = fabsf(llr[t]);
        if (!(a[t] < INFINITY)) return;                        // not attempted
        if (llr[t] > 0.0f) hard[t >> 5] |= 1u << (t & 31);
    }
    int perm[LDPC_N];
    for (int t = 0; t < LDPC_N; ++t) {
        int r = 0;
        for (int u = 0; u < LDPC_N; ++u) r += (a[u] > a[t]) || (a[u] == a[t] && u < t);
        perm[r] = t;
    }
    OsdGen g = gen;
    int rowof[LDPC_K], pos[LDPC_K], npiv = 0, k = 0;           // rowof[i]: the row that became g_i; pos[i] = p_i
    bool used[LDPC_K] = {false};
    uint32_t c0[OSD_GW] = {0};
    for (; k < LDPC_N && npiv < LDPC_K; ++k) {
        const int t = perm[k], w = t >> 5;
        const uint32_t bm = 1u << (t & 31);
        int r = 0;
        while (r < LDPC_K && (used[r] || !(g.row[r][w] & bm))) ++r;
        if (r == LDPC_K) continue;
        for (int i = 0; i < LDPC_K; ++i)
            if (i != r && (g.row[i][w] & bm))
                for (int x = 0; x < OSD_GW; ++x) g.row[i][x] ^= g.row[r][x];
        used[r] = true;
        pos[npiv] = t;
        rowof[npiv++] = r;
    }
    if (npiv != LDPC_K) return;
    for (int i = 0; i < LDPC_K; ++i)
        if ((hard[pos[i] >> 5] >> (pos[i] & 31)) & 1u)
            for (int x = 0; x < OSD_GW; ++x) c0[x] ^= g.row[rowof[i]][x];
    uint32_t e[OSD_GW], best[OSD_GW];
    for (int x = 0; x < OSD_GW; ++x) best[x] = e[x] = c0[x] ^ hard[x];
    float dmin = osd_distance(e, a);
    int how = 0, fi = 0xff, fj = 0xff;
    if (order >= 1)
        for (int i = 0; i < LDPC_K; ++i) {
            uint32_t c[OSD_GW];
            for (int x = 0; x < OSD_GW; ++x) c[x] = e[x] ^ g.row[rowof[i]][x];
            const float d = osd_distance(c, a);
            if (d < dmin) { dmin = d; how = 1; fi = i; fj = 0xff; memcpy(best, c, sizeof(c)); }
        }
    if (order >= 2)
        for (int i = 0; i < LDPC_K; ++i)
            for (int j = i + 1; j < LDPC_K; ++j) {
                uint32_t c[OSD_GW];
                for (int x = 0; x < OSD_GW; ++x) c[x] = e[x] ^ g.row[rowof[i]][x] ^ g.row[rowof[j]][x];
                const float d = osd_distance(c, a);
                if (d < dmin) { dmin = d; how = 2; fi = i; fj = j; memcpy(best, c, sizeof(c)); }
            }
    int nh = 0;
    for (int t = 0; t < LDPC_N; ++t) nh += (best[t >> 5] >> (t & 31)) & 1u;
    uint32_t cw[OSD_GW];
    for (int x = 0; x < OSD_GW; ++x) cw[x] = best[x] ^ hard[x];
    const uint64_t lo = cw[0] | ((uint64_t)cw[1] << 32), hi = (cw[2] | ((uint64_t)cw[3] << 32)) & ((1ull << (LDPC_K - 64)) - 1);
    for (int t = 0; t < LDPC_K; ++t) if (ldpc_cw_bit(lo, hi, t)) out->bits[t >> 3] |= (uint8_t)(0x80 >> (t & 7));
    out->dmin = dmin;
    out->nharderr = (int16_t)nh;
    out->nskip = (int16_t)(k - LDPC_K);
    out->crc_ok = ldpc_crc14(lo, hi) == ldpc_crc_field(lo, hi);
    out->how = (uint8_t)how;
    out->flip[0] = (uint8_t)fi;
    out->flip[1] = (uint8_t)fj;
}

} // namespace cwslg
