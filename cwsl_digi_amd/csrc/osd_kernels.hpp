// osd_kernels.hpp -- ordered-statistics decoding (order 0, 1 or 2) of the (174, 91) code on gfx950: per FT8 sync candidate that belief propagation
// gave up on, the codeword nearest to the metrics among c0, c0 + g_i and c0 + g_i + g_j of the most reliable basis, as a 24-byte cwslg_osd_msg.
//
// *** PARITY UNPINNED by the reference *** like ldpc_kernels.hpp: the contract is the one include/cwsl_gpu.h states for cwslg_osd_msg and
// tests/osd_ref.py restates in numpy, BIT FOR BIT -- integers throughout except one float32 quantity, the distance, whose summation order is fixed
// (ascending position, one add per term).  It is not upstream osd174_91 (which takes reliabilities summed over BP iterations and its own
// thresholds).  The generator is DATA derived on the host from the caller's table (ldpc_host.hpp: OsdGen); nothing here depends on which basis of
// the code it is.  This translation unit is built -ffp-contract=off.
//
// One wave per candidate, four per workgroup, grid (ceil(max_cand / 4), FT8 channels); the count is read from d_ncand on the device.
//   order      lane l owns positions l, l + 64, l + 128 and ranks them by counting (174 broadcast reads of |llr| from the wave's LDS image)
//   basis      lane l owns generator rows l and l + 64 (rows 64..90: lanes 0..26), 6 dwords each in registers.  One elimination step per walked
//              position: a ballot finds the unused rows that have the bit, the first such lane's row is read with lane reads and XORed into
//              every other row that has the bit.  After the 91st pivot the rows are the reduced basis g_i (i = joining order).
//   search     the rows go to the wave's LDS image (91 x 24 B); c0 + hard (the error pattern) is wave-uniform; lane l evaluates words
//              l, l + 64, ... of the 1 / 92 / 4187, each distance a walk over the set bits of its error pattern in ascending position
//   winner     min over (distance bits, word index): the index order IS the tie rule (c0, singles by i, pairs by (i, j)); six lane exchanges
// Nothing is shared between waves, hence no workgroup barrier (ldpc_wave_sync fences); every exit is wave-uniform.
// The same kernel serves cwslg_osd_decode: works == nullptr, n_flat sets of 174 metrics from llr_flat, no gates.
// And the FT4 chain (cwslg_enable_ft4_osd), a third way of finding llr, out and the gate in front of the same code: works4 != nullptr, one wave per
// (record slot, metric set) of ft4_softbits_kernel's slot array, grid (ceil(9 max_cand / 4), FT4 channels), addressed as ldpc_decode_kernel's
// works4 branch addresses it: slot = q / 3, set s = q % 3, cand = slot / 3, r = slot % 3; the wave leaves if q >= 9 max_cand,
// cand >= min(*ncand, max_cand) or r >= nrec[cand].  It writes set[s] of the slot's cwslg_ft4_osd (record q of the channel's array).  The gate is
// per RECORD: set s is attempted iff its decode record was attempted, NO set of the slot has BP crc_ok, and nsync / nqual pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ldpc_kernels.hpp"

namespace cwslg {

constexpr int OSD_WAVES = 4;
constexpr int OSD_NSINGLE = 1 + LDPC_K;                // c0 and the 91 single flips: word indices 0..91; pairs follow in (i, j) order
struct Ft4OsdRec { OsdRec set[3]; };                   // = cwslg_ft4_osd
static_assert(sizeof(Ft4OsdRec) == 72, "cwslg_ft4_osd is 72 bytes");

// "the row has the bit": bm[] holds the position's bit in its word and 0 in the others (wave-uniform), so no register is indexed
__device__ __forceinline__ bool osd_has(const uint32_t (&r)[OSD_GW], const uint32_t (&bm)[OSD_GW])
{
    uint32_t x = 0u;
#pragma unroll
    for (int k = 0; k < OSD_GW; ++k) x |= r[k] & bm[k];
    return x != 0u;
}

__device__ __forceinline__ void osd_row_load(uint32_t (&r)[OSD_GW], const CWSLG_GLOBAL OsdGen *gen, int row)
{
    const CWSLG_GLOBAL v2u *p = reinterpret_cast<const CWSLG_GLOBAL v2u *>(&gen->row[row][0]);
#pragma unroll
    for (int k = 0; k < OSD_GW / 2; ++k) { const v2u v = p[k]; r[2 * k] = v.x; r[2 * k + 1] = v.y; }
}

__device__ __forceinline__ void osd_lds_row(uint32_t (&r)[OSD_GW], const uint32_t *s_g, int i)
{
    const v2u *p = reinterpret_cast<const v2u *>(s_g + OSD_GW * i);
#pragma unroll
    for (int k = 0; k < OSD_GW / 2; ++k) { const v2u v = p[k]; r[2 * k] = v.x; r[2 * k + 1] = v.y; }
}

// d(c): float32 adds of a[t] over the set bits of the error pattern in ascending t (a skipped term and an added +0 give the same bits)
__device__ __forceinline__ float osd_dist(const uint32_t (&e)[OSD_GW], const float *s_a)
{
    float d = 0.0f;
#pragma unroll
    for (int w = 0; w < OSD_GW; ++w) {
        uint32_t m = e[w];
        while (m) {
            d = d + s_a[32 * w + __builtin_ctz(m)];
            m &= m - 1;
        }
    }
    return d;
}

__device__ __forceinline__ uint64_t osd_key(float d, int k) { return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)k; }   // d >= +0: its bits order like its value

__global__ __launch_bounds__(64 * OSD_WAVES) void osd_decode_kernel(const SyncWork *__restrict__ works, Ft8SoftRec *const *__restrict__ soft,
                                                                    Ft8MsgRec *const *__restrict__ msg, OsdRec *const *__restrict__ osd,
                                                                    const float *__restrict__ llr_flat, OsdRec *__restrict__ out_flat, int n_flat, int maxcand,
                                                                    int order, int min_nsync, const OsdGen *__restrict__ gen,
                                                                    const Ft4Work *__restrict__ works4, Ft4SoftRec *const *__restrict__ soft4,
                                                                    Ft4MsgRec *const *__restrict__ msg4, Ft4OsdRec *const *__restrict__ osd4, int min_nqual)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_gall[OSD_WAVES][LDPC_K * OSD_GW];
    __shared__ __attribute__((aligned(16))) float s_aall[OSD_WAVES][192];
    __shared__ __attribute__((aligned(16))) int s_pall[OSD_WAVES][192];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * OSD_WAVES + wv;
    const CWSLG_GLOBAL float *llr;
    CWSLG_GLOBAL OsdRec *out;
    bool attempt = true;
    if (works) {
        const SyncWork *w = works + blockIdx.y;
        const int ncand = min(*as_global(w->ncand), maxcand);
        if (q >= ncand) return;                                // wave-uniform
        const CWSLG_GLOBAL Ft8SoftRec *rec = as_global(soft[blockIdx.y]) + q;
        const CWSLG_GLOBAL Ft8MsgRec *m = as_global(msg[blockIdx.y]) + q;
        llr = rec->llr;
        out = as_global_rw(osd[blockIdx.y]) + q;
        attempt = m->iters >= 0 && m->crc_ok == 0 && rec->nsync >= min_nsync;
    } else if (works4) {
        const Ft4Work *w = works4 + blockIdx.y;
        if (q >= 9 * maxcand) return;                          // wave-uniform, all three
        const int slot = q / 3, s = q - 3 * slot, cand = slot / 3, r = slot - 3 * cand;
        if (cand >= min(*as_global(w->ncand), maxcand)) return;
        if (r >= as_global(w->nrec)[cand]) return;
        const CWSLG_GLOBAL Ft4SoftRec *rec = as_global(soft4[blockIdx.y]) + slot;
        const CWSLG_GLOBAL Ft8MsgRec *m = as_global(&msg4[blockIdx.y]->set[0]) + 3 * slot;     // the slot's three decode records
        llr = rec->llr[s];
        out = as_global_rw(&osd4[blockIdx.y]->set[0]) + q;     // set s of slot q / 3
        attempt = m[s].iters >= 0 && (m[0].crc_ok | m[1].crc_ok | m[2].crc_ok) == 0 && rec->nsync >= min_nsync && rec->nqual >= min_nqual;
    } else {
        if (q >= n_flat) return;
        llr = as_global(llr_flat) + (size_t)q * LDPC_N;
        out = as_global_rw(out_flat) + q;
    }
    CWSLG_GLOBAL uint32_t *ow = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(out);
    const bool third = lane + 128 < LDPC_N;
    float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f;
    if (attempt) {                                             // wave-uniform
        l0 = llr[lane]; l1 = llr[lane + 64]; l2 = third ? llr[lane + 128] : 0.0f;
    }
    const float a0 = fabsf(l0), a1 = fabsf(l1), a2 = fabsf(l2);
    if (__ballot(!(a0 < INFINITY) || !(a1 < INFINITY) || !(a2 < INFINITY)) != 0ull) attempt = false;
    int npiv = 0, kw = 0;
    uint32_t ra[OSD_GW], rb[OSD_GW];
    int ia = -1, ib = -1;                                      // the rows' joining index i (-1: not in the basis yet)
    bool sa = false, sb = false;                               // hard[p_i] of the rows' pivot positions
    const uint64_t h0 = __ballot(l0 > 0.0f), h1 = __ballot(l1 > 0.0f), h2 = __ballot(third && l2 > 0.0f);
    const uint32_t hard[OSD_GW] = {(uint32_t)h0, (uint32_t)(h0 >> 32), (uint32_t)h1, (uint32_t)(h1 >> 32), (uint32_t)h2, (uint32_t)(h2 >> 32)};
    float *s_a = s_aall[wv];
    int *s_p = s_pall[wv];
    uint32_t *s_g = s_gall[wv];
    if (attempt) {
        // ---- reliability order: rank by counting
        s_a[lane] = a0;
        s_a[lane + 64] = a1;
        s_a[lane + 128] = a2;                                  // (174..191: +0, never read)
        ldpc_wave_sync();
        int r0 = 0, r1 = 0, r2 = 0;
        for (int u = 0; u < LDPC_N; ++u) {
            const float au = s_a[u];
            r0 += (au > a0) || (au == a0 && u < lane);
            r1 += (au > a1) || (au == a1 && u < lane + 64);
            r2 += (au > a2) || (au == a2 && u < lane + 128);
        }
        s_p[r0] = lane;
        s_p[r1] = lane + 64;
        if (third) s_p[r2] = lane + 128;
        ldpc_wave_sync();
        // ---- most reliable basis, reduced
        const CWSLG_GLOBAL OsdGen *g = as_global(gen);
        osd_row_load(ra, g, lane);
#pragma unroll
        for (int k = 0; k < OSD_GW; ++k) rb[k] = 0u;           // (a row that does not exist never has the bit)
        if (lane + 64 < LDPC_K) osd_row_load(rb, g, lane + 64);
        for (; kw < LDPC_N && npiv < LDPC_K; ++kw) {
            const int t = __builtin_amdgcn_readfirstlane(s_p[kw]);
            uint32_t bm[OSD_GW];
#pragma unroll
            for (int k = 0; k < OSD_GW; ++k) bm[k] = (t >> 5) == k ? 1u << (t & 31) : 0u;
            const bool ha = osd_has(ra, bm), hb = osd_has(rb, bm);
            const uint64_t ma = __ballot(ha && ia < 0), mb = __ballot(hb && ib < 0);
            if ((ma | mb) == 0ull) continue;                   // dependent on the columns taken: passed over (wave-uniform)
            uint32_t p[OSD_GW];
            const bool from_a = ma != 0ull;
            const int src = __builtin_amdgcn_readfirstlane(__builtin_ctzll(from_a ? ma : mb));
            if (from_a) {
#pragma unroll
                for (int k = 0; k < OSD_GW; ++k) p[k] = (uint32_t)__builtin_amdgcn_readlane((int)ra[k], src);
            } else {
#pragma unroll
                for (int k = 0; k < OSD_GW; ++k) p[k] = (uint32_t)__builtin_amdgcn_readlane((int)rb[k], src);
            }
            const bool piv_a = from_a && lane == src, piv_b = !from_a && lane == src;
#pragma unroll
            for (int k = 0; k < OSD_GW; ++k) {
                ra[k] ^= (ha && !piv_a) ? p[k] : 0u;
                rb[k] ^= (hb && !piv_b) ? p[k] : 0u;
            }
            const bool ht = osd_has(hard, bm);
            if (piv_a) { ia = npiv; sa = ht; }
            if (piv_b) { ib = npiv; sb = ht; }
            ++npiv;
        }
        if (npiv < LDPC_K) attempt = false;                    // (cannot happen with a generator of rank 91; wave-uniform)
    }
    if (!attempt) {                                            // zero bits, dmin +0, nharderr = nskip = -1, crc_ok 0, how = flip[] = 0xff
        if (lane < 6) ow[lane] = lane < 4 ? 0u : lane == 4 ? 0xffffffffu : 0xffffff00u;
        return;
    }
    const int nskip = kw - LDPC_K;
    // ---- the rows to LDS by joining index; c0 = sum of the g_i whose pivot position has hard = 1
    uint32_t x[OSD_GW];
#pragma unroll
    for (int k = 0; k < OSD_GW; ++k) x[k] = (sa ? ra[k] : 0u) ^ (sb ? rb[k] : 0u);
    if (ia >= 0) {
        v2u *d = reinterpret_cast<v2u *>(s_g + OSD_GW * ia);
        d[0] = v2u{ra[0], ra[1]}; d[1] = v2u{ra[2], ra[3]}; d[2] = v2u{ra[4], ra[5]};
    }
    if (ib >= 0) {
        v2u *d = reinterpret_cast<v2u *>(s_g + OSD_GW * ib);
        d[0] = v2u{rb[0], rb[1]}; d[1] = v2u{rb[2], rb[3]}; d[2] = v2u{rb[4], rb[5]};
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < OSD_GW; ++k) x[k] ^= (uint32_t)__shfl_xor((int)x[k], off, 64);
    }
    uint32_t c0[OSD_GW], e0[OSD_GW];
#pragma unroll
    for (int k = 0; k < OSD_GW; ++k) {
        c0[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)x[k]);
        e0[k] = c0[k] ^ hard[k];
    }
    ldpc_wave_sync();
    // ---- the search
    uint64_t best = ~0ull;
    const int nsingle = order >= 1 ? OSD_NSINGLE : 1;
    for (int k = lane; k < nsingle; k += 64) {
        uint32_t e[OSD_GW], gi[OSD_GW];
        osd_lds_row(gi, s_g, k > 0 ? k - 1 : 0);
#pragma unroll
        for (int m = 0; m < OSD_GW; ++m) e[m] = e0[m] ^ (k > 0 ? gi[m] : 0u);
        const uint64_t key = osd_key(osd_dist(e, s_a), k);
        best = key < best ? key : best;
    }
    if (order >= 2) {
        int i = 0, r = lane;                                   // pair number p is (i, j = i + 1 + r): row i holds 90 - i of them
        while (i < LDPC_K - 1 && r >= LDPC_K - 1 - i) { r -= LDPC_K - 1 - i; ++i; }
        for (int p = lane; p < OSD_NPAIR; p += 64) {
            uint32_t e[OSD_GW], gi[OSD_GW], gj[OSD_GW];
            osd_lds_row(gi, s_g, i);
            osd_lds_row(gj, s_g, i + 1 + r);
#pragma unroll
            for (int m = 0; m < OSD_GW; ++m) e[m] = e0[m] ^ gi[m] ^ gj[m];
            const uint64_t key = osd_key(osd_dist(e, s_a), OSD_NSINGLE + p);
            best = key < best ? key : best;
            r += 64;
            while (i < LDPC_K - 1 && r >= LDPC_K - 1 - i) { r -= LDPC_K - 1 - i; ++i; }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t oh = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), off, 64), ol = (uint32_t)__shfl_xor((int)(uint32_t)best, off, 64);
        const uint64_t o = ((uint64_t)oh << 32) | ol;
        best = o < best ? o : best;
    }
    // ---- the winner (every lane holds the same key)
    const uint32_t dbits = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(best >> 32));
    const int kwin = __builtin_amdgcn_readfirstlane((int)(uint32_t)best);
    const int how = kwin == 0 ? 0 : kwin < OSD_NSINGLE ? 1 : 2;
    int fi = kwin - 1, fj = 0;
    if (how == 2) {
        int r = kwin - OSD_NSINGLE;
        fi = 0;
        while (fi < LDPC_K - 1 && r >= LDPC_K - 1 - fi) { r -= LDPC_K - 1 - fi; ++fi; }
        fj = fi + 1 + r;
    }
    uint32_t c[OSD_GW], gi[OSD_GW], gj[OSD_GW];
    osd_lds_row(gi, s_g, how >= 1 ? fi : 0);
    osd_lds_row(gj, s_g, how == 2 ? fj : 0);
    int nharderr = 0;
#pragma unroll
    for (int m = 0; m < OSD_GW; ++m) {
        c[m] = c0[m] ^ (how >= 1 ? gi[m] : 0u) ^ (how == 2 ? gj[m] : 0u);
        nharderr += __popc(c[m] ^ hard[m]);
    }
    const uint64_t b0 = c[0] | ((uint64_t)c[1] << 32);
    const uint64_t hi = (c[2] | ((uint64_t)c[3] << 32)) & ((1ull << (LDPC_K - 64)) - 1);       // codeword bits 64..90
    const bool crc_ok = ldpc_crc14(b0, hi) == ldpc_crc_field(b0, hi);
    const uint64_t r0 = __brevll(b0), r1 = __brevll(hi);       // bits[] as cwslg_ft8_msg packs them
    uint32_t word;
    switch (lane) {
    case 0: word = __builtin_bswap32((uint32_t)(r0 >> 32)); break;
    case 1: word = __builtin_bswap32((uint32_t)r0); break;
    case 2: word = __builtin_bswap32((uint32_t)(r1 >> 32)); break;
    case 3: word = dbits; break;
    case 4: word = ((uint32_t)nharderr & 0xffffu) | ((uint32_t)nskip << 16); break;
    default: word = (crc_ok ? 1u : 0u) | ((uint32_t)how << 8) | ((how >= 1 ? (uint32_t)fi : 0xffu) << 16) | ((how == 2 ? (uint32_t)fj : 0xffu) << 24); break;
    }
    if (lane < 6) ow[lane] = word;
}

} // namespace cwslg
