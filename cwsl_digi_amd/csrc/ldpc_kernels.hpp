// ldpc_kernels.hpp -- LDPC(174,91) flooding sum-product decode on gfx950: per FT8 sync candidate 91 decoded bits, "is a codeword", "CRC-14 matches"
// and an iteration count, from the 174 bit metrics ft8_softbits_kernel has just written.
//
// *** PARITY UNPINNED by the reference *** like the rest of the sync stage.  The arithmetic is the one include/cwsl_gpu.h states for cwslg_ft8_msg
// and tests/ldpc_ref.py restates in numpy, BIT FOR BIT; it is structured like upstream bpdecode174_91 (tanh as a Pade form, platanh's pieces, the
// early stop on a growing count of unsatisfied checks).  The parity-check table is DATA the caller loads (cwslg_set_ldpc_code): nothing here
// depends on which table it is.  This translation unit is built -ffp-contract=off: every product, sum and quotient below is one float32 operation.
//
// One wave per candidate, four candidates per workgroup, grid (ceil(max_cand / 4), FT8 channels): the count is read from d_ncand on the device and
// the waves beyond it leave.  Inside a wave both sides of the graph are lane-owned and every table entry a lane needs is read ONCE, before the
// loop, into registers (23 values per lane from the 2560-byte block LdpcTables: the same block for every wave, so it stays in L2 / the vector L1;
// an LDS copy per workgroup would need the one thing this kernel does without, a workgroup barrier):
//   bit side    lane l owns bits l, l + 64, l + 128: z = ((llr + v0) + v1) + v2 from the three check-to-bit messages it gathers from LDS;
//   check side  lane l owns rows l and l + 64 (rows 64..82: lanes 0..18): it gathers its rows' z, takes the parity, and computes its rows' 7 + 7
//               messages, whose previous values it still holds in registers -- the exclusion product of edge e is the left-to-right product over
//               e' != e, so the products of one row share their prefixes (1, t0, t0 t1, ...) and cost 21 multiplies instead of 42.
// The two sides meet in a wave-private LDS image: v[83][8] (an edge's position is 8 m + e) and z[192], 3.4 KB per wave.  Nothing is shared
// between waves, hence no workgroup barrier; every exit is wave-uniform (nbad comes from ballots).
// The same kernel serves cwslg_ldpc_decode: works == nullptr, n_flat sets of 174 metrics from llr_flat, no nsync filter.
// And the FT4 decode (cwslg_enable_ft4_decode), a third way of finding llr and out in front of the same loop: works4 != nullptr, one wave per
// (record slot, metric set) of ft4_softbits_kernel's slot array, grid (ceil(9 max_cand / 4), FT4 channels).  Wave q of a channel: slot = q / 3,
// set s = q % 3, cand = slot / 3, r = slot % 3; it leaves if q >= 9 max_cand, cand >= min(*ncand, max_cand) or r >= nrec[cand] -- the reads
// ft4_softbits_kernel makes, on the device -- and writes set[s] of the slot's cwslg_ft4_msg (three cwslg_ft8_msg: record q of the channel's array).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ldpc_host.hpp"
#include "ft4soft_kernels.hpp"

namespace cwslg {

constexpr int LDPC_WAVES = 4;
typedef unsigned v2u __attribute__((ext_vector_type(2)));
struct Ft8MsgRec { uint8_t bits[12]; int16_t iters, nbad, nharderr; uint8_t crc_ok, pad_; };    // = cwslg_ft8_msg
static_assert(sizeof(Ft8MsgRec) == 20, "cwslg_ft8_msg is 20 bytes");
struct Ft4MsgRec { Ft8MsgRec set[3]; };                                                          // = cwslg_ft4_msg
static_assert(sizeof(Ft4MsgRec) == 60, "cwslg_ft4_msg is 60 bytes");
constexpr int LDPC_VSIZE = LDPC_M * LDPC_EPITCH;       // 664 message slots
constexpr int LDPC_ZDUMMY = 191;                       // where an absent edge reads its z (a zero nobody writes)

// the hand-over between the two sides: the image is private to this wave, whose LDS operations complete in order
__device__ __forceinline__ void ldpc_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct LdpcRow {            // one row as its lane holds it
    int bit[LDPC_ROWMAX];   // index into z: the edge's bit, LDPC_ZDUMMY for an absent edge
    float v[LDPC_ROWMAX];   // the row's check-to-bit messages
    float z[LDPC_ROWMAX];
    bool has6;              // edge 6 exists (weight 7)
    bool live;              // the row exists
};

__device__ __forceinline__ void ldpc_row_load(LdpcRow &r, const CWSLG_GLOBAL LdpcTables *tab, int m)
{
    const v2u w = *reinterpret_cast<const CWSLG_GLOBAL v2u *>(&tab->rowbit[m][0]);
#pragma unroll
    for (int e = 0; e < LDPC_ROWMAX; ++e) {
        const int b = (int)(((e < 4 ? w.x : w.y) >> (8 * (e & 3))) & 0xffu);
        r.bit[e] = b == LDPC_ABSENT ? LDPC_ZDUMMY : b;
        r.v[e] = 0.0f;
    }
    r.live = r.bit[0] != LDPC_ZDUMMY;
    r.has6 = r.bit[6] != LDPC_ZDUMMY;
}

// steps 1-2 on the check side: gather the row's z, return its parity (an absent edge reads +0: cw = 0)
__device__ __forceinline__ bool ldpc_row_parity(LdpcRow &r, const float *s_z)
{
    bool odd = false;
#pragma unroll
    for (int e = 0; e < LDPC_ROWMAX; ++e) {
        r.z[e] = s_z[r.bit[e]];
        odd ^= r.z[e] > 0.0f;
    }
    return odd;
}

// steps 7-8 for one row: t[e] = T(-0.5 (z - v)), v[e] = 2 A(-prod of t[e'] over e' != e, ascending, from 1.0f); an absent edge contributes no factor
__device__ __forceinline__ void ldpc_row_update(LdpcRow &r, float *s_v, int m)
{
    if (!r.live) return;
    // (a weight-6 row still evaluates t[6] and v[6], from its dummy z, and nobody reads them: rows of both weights share a wave, so a branch on
    // has6 would run both sides anyway and save nothing)
    float t[LDPC_ROWMAX];
#pragma unroll
    for (int e = 0; e < LDPC_ROWMAX; ++e) t[e] = ldpc_T(-0.5f * (r.z[e] - r.v[e]));
    float pre = 1.0f;                                  // 1.0f * t0 * ... * t[e-1], left to right (1.0f * x is x)
#pragma unroll
    for (int e = 0; e < LDPC_ROWMAX; ++e) {
        float p = pre;
#pragma unroll
        for (int f = e + 1; f < LDPC_ROWMAX; ++f) p = (f < 6 || r.has6) ? p * t[f] : p;
        r.v[e] = 2.0f * ldpc_A(-p);
        pre = e == 0 ? t[0] : pre * t[e];
    }
    v4f *dst = reinterpret_cast<v4f *>(s_v + LDPC_EPITCH * m);
    dst[0] = v4f{r.v[0], r.v[1], r.v[2], r.v[3]};
    dst[1] = v4f{r.v[4], r.v[5], r.v[6], 0.0f};       // (slot 6 of a weight-6 row and slot 7 are never read)
}

// The graph as one lane holds it across runs: the message positions of its three bits and its two rows.
struct LdpcGraph {
    int ep[3][3];
    LdpcRow ra, rb;
};

__device__ __forceinline__ void ldpc_graph_load(LdpcGraph &g, const CWSLG_GLOBAL LdpcTables *tab, int lane)
{
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const v2u w = *reinterpret_cast<const CWSLG_GLOBAL v2u *>(&tab->epos[lane + 64 * b][0]);
        g.ep[b][0] = (int)(w.x & 0xffffu); g.ep[b][1] = (int)(w.x >> 16); g.ep[b][2] = (int)(w.y & 0xffffu);
    }
    ldpc_row_load(g.ra, tab, lane);
    ldpc_row_load(g.rb, tab, lane + 64);
}

// The loop of the decode contract (steps 1-8 of cwslg_ft8_msg) on the metrics l0, l1, l2 of the lane's bits, in the wave's LDS image: the ONE
// text of it, called by ldpc_decode_kernel and by ap_decode_kernel (ap_kernels.hpp), which runs it once per pattern.  A run starts from messages
// +0 whatever an earlier run of the wave left; at exit it = iters, nbad, and z0, z1, z2 the lane's z (cw = z > 0).
__device__ __forceinline__ void ldpc_bp_run(LdpcGraph &g, float l0, float l1, float l2, int max_iter, float *s_v, float *s_z, int lane, int &it_out,
                                            int &nbad_out, float &z0, float &z1, float &z2)
{
    const bool third = lane + 128 < LDPC_N;
#pragma unroll
    for (int e = 0; e < LDPC_ROWMAX; ++e) g.ra.v[e] = g.rb.v[e] = 0.0f;
    for (int k = lane; k < LDPC_VSIZE; k += 64) s_v[k] = 0.0f;
    s_z[lane + 128] = 0.0f;                                    // 128..191: bits 128..173 are rewritten below, the rest stays +0
    ldpc_wave_sync();

    int ncnt = 0, nclast = 0, it = 0, nbad = 0;
    for (;;) {
        z0 = ((l0 + s_v[g.ep[0][0]]) + s_v[g.ep[0][1]]) + s_v[g.ep[0][2]];
        z1 = ((l1 + s_v[g.ep[1][0]]) + s_v[g.ep[1][1]]) + s_v[g.ep[1][2]];
        z2 = ((l2 + s_v[g.ep[2][0]]) + s_v[g.ep[2][1]]) + s_v[g.ep[2][2]];
        s_z[lane] = z0;
        s_z[lane + 64] = z1;
        if (third) s_z[lane + 128] = z2;
        ldpc_wave_sync();
        const bool odd_a = ldpc_row_parity(g.ra, s_z), odd_b = ldpc_row_parity(g.rb, s_z);
        nbad = __popcll(__ballot(odd_a)) + __popcll(__ballot(odd_b));
        if (nbad == 0 || it == max_iter) break;
        if (it > 0) {
            ncnt = nbad - nclast < 0 ? 0 : ncnt + 1;
            if (ncnt >= 5 && it >= 10 && nbad > 15) break;
        }
        nclast = nbad;
        ldpc_row_update(g.ra, s_v, lane);
        ldpc_row_update(g.rb, s_v, lane + 64);
        ldpc_wave_sync();
        ++it;
    }
    it_out = it;
    nbad_out = nbad;
}

__global__ __launch_bounds__(64 * LDPC_WAVES) void ldpc_decode_kernel(const SyncWork *__restrict__ works, Ft8SoftRec *const *__restrict__ soft,
                                                                      Ft8MsgRec *const *__restrict__ msg, const float *__restrict__ llr_flat,
                                                                      Ft8MsgRec *__restrict__ out_flat, int n_flat, int maxcand, int max_iter, int min_nsync,
                                                                      const LdpcTables *__restrict__ tables, const Ft4Work *__restrict__ works4,
                                                                      Ft4SoftRec *const *__restrict__ soft4, Ft4MsgRec *const *__restrict__ msg4,
                                                                      int min_nqual)
{
    __shared__ __attribute__((aligned(16))) float s_vall[LDPC_WAVES][LDPC_VSIZE];
    __shared__ __attribute__((aligned(16))) float s_zall[LDPC_WAVES][192];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * LDPC_WAVES + wv;
    const CWSLG_GLOBAL float *llr;
    CWSLG_GLOBAL Ft8MsgRec *out;
    bool attempt = true;
    if (works) {
        const SyncWork *w = works + blockIdx.y;
        const int ncand = min(*as_global(w->ncand), maxcand);
        if (q >= ncand) return;                                // wave-uniform
        const CWSLG_GLOBAL Ft8SoftRec *rec = as_global(soft[blockIdx.y]) + q;
        llr = rec->llr;
        out = as_global_rw(msg[blockIdx.y]) + q;
        attempt = rec->nsync >= min_nsync && rec->sigma != 0.0f;
    } else if (works4) {
        const Ft4Work *w = works4 + blockIdx.y;
        if (q >= 9 * maxcand) return;                          // wave-uniform, all three
        const int slot = q / 3, s = q - 3 * slot, cand = slot / 3, r = slot - 3 * cand;
        if (cand >= min(*as_global(w->ncand), maxcand)) return;
        if (r >= as_global(w->nrec)[cand]) return;
        const CWSLG_GLOBAL Ft4SoftRec *rec = as_global(soft4[blockIdx.y]) + slot;
        llr = rec->llr[s];
        out = as_global_rw(&msg4[blockIdx.y]->set[0]) + q;     // set s of slot q / 3
        attempt = rec->nsync >= min_nsync && rec->nqual >= min_nqual && rec->sigma[s] != 0.0f;
    } else {
        if (q >= n_flat) return;
        llr = as_global(llr_flat) + (size_t)q * LDPC_N;
        out = as_global_rw(out_flat) + q;
    }
    CWSLG_GLOBAL uint32_t *ow = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(out);
    if (!attempt) {                                            // wave-uniform: zero bits, iters = nbad = nharderr = -1, crc_ok = 0
        if (lane < 5) ow[lane] = lane < 3 ? 0u : lane == 3 ? 0xffffffffu : 0x0000ffffu;
        return;
    }
    float *s_v = s_vall[wv], *s_z = s_zall[wv];
    const CWSLG_GLOBAL LdpcTables *tab = as_global(tables);
    const bool third = lane + 128 < LDPC_N;
    const float l0 = llr[lane], l1 = llr[lane + 64], l2 = third ? llr[lane + 128] : 0.0f;
    LdpcGraph g;
    ldpc_graph_load(g, tab, lane);
    int it, nbad;
    float z0, z1, z2;
    ldpc_bp_run(g, l0, l1, l2, max_iter, s_v, s_z, lane, it, nbad, z0, z1, z2);

    const bool c0 = z0 > 0.0f, c1 = z1 > 0.0f, c2 = third && z2 > 0.0f;
    const uint64_t b0 = __ballot(c0), b1 = __ballot(c1);
    const int nharderr = __popcll(__ballot((l0 > 0.0f) != c0)) + __popcll(__ballot((l1 > 0.0f) != c1)) + __popcll(__ballot(third && (l2 > 0.0f) != c2));
    const uint64_t hi = b1 & ((1ull << (LDPC_K - 64)) - 1);   // codeword bits 64..90
    const bool crc_ok = nbad == 0 && ldpc_crc14(b0, hi) == ldpc_crc_field(b0, hi);
    // bits[]: codeword bit t at bits[t >> 3] & (0x80 >> (t & 7)): the ballot reversed as a whole, its bytes then taken from the top
    const uint64_t r0 = __brevll(b0), r1 = __brevll(hi);
    uint32_t word;
    switch (lane) {
    case 0: word = __builtin_bswap32((uint32_t)(r0 >> 32)); break;
    case 1: word = __builtin_bswap32((uint32_t)r0); break;
    case 2: word = __builtin_bswap32((uint32_t)(r1 >> 32)); break;
    case 3: word = ((uint32_t)it & 0xffffu) | ((uint32_t)nbad << 16); break;
    default: word = ((uint32_t)nharderr & 0xffffu) | (crc_ok ? 0x10000u : 0u); break;
    }
    if (lane < 5) ow[lane] = word;
}

} // namespace cwslg
