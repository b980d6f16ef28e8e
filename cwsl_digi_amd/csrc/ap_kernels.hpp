// ap_kernels.hpp -- FT8 and FT4 a-priori decoding on gfx950: the candidates (FT4: sync records) belief propagation and OSD gave up on are decoded again with some of the
// 91 message bits TOLD to the decoder -- a caller's patterns (mask + value, e.g. the bits of "CQ"), tried in the caller's order -- and the first
// pattern under which the loop of the decode contract reaches a CRC-passing codeword that agrees with the pattern is the find.
//
// *** PARITY UNPINNED by the reference *** like ldpc_kernels.hpp.  The arithmetic is the one include/cwsl_gpu.h states for cwslg_ap_msg and
// tests/ap_ref.py restates in numpy, BIT FOR BIT.  The patterns are DATA the caller loads (cwslg_set_ft8_ap): nothing here knows what a message
// packs to.  This translation unit is built -ffp-contract=off: every product and sum below is one float32 operation.
//
// This is a FETCH with a kernel inside, not a stage (cwslg_fetch_ft8_ap, cwslg_fetch_ft4_ap): it reads the records the chain has left on the device and writes only
// the group's staging.  Two kernels, one per job; the decode shares ldpc_decode_kernel's loop (ldpc_bp_run), LDS image and launch shape:
//   ap_decode_kernel    one wave per candidate, four per workgroup, grid (ceil(cap / 4), taking-part channels): the count is read on the device and the
//                surplus waves leave.  The wave loads the graph ONCE (ldpc_graph_load: 23 values per lane, kept in registers across patterns).
//                A pattern's six dwords of the 192-byte block are wave-uniform reads; per pattern the lane replaces the metrics of its bits l and
//                l + 64 where the mask has them (bits 128..173 are never masked) and runs ldpc_bp_run, the ONE text of the loop, in the wave's LDS
//                image.  A = 1.01f * max |llr| comes from a wave max reduction (exact in any order).  On success nharderr and dmin are taken
//                against the ORIGINAL metrics: dmin is OSD's ordered chain (osd_dist over the error pattern, |llr| in the LDS image the loop has
//                left), not a tree.  No cross-wave traffic, no workgroup barrier, every exit wave-uniform.  So that the kernel stays in the decode's
//                register allocation (six waves per SIMD), nothing but the graph stays live across a run: the original metrics of bits l and
//                l + 64 are read again per pattern, A and the pattern words are scalars.
//                Three ways of finding llr and out, chosen by launch-uniform fields of ApArgs: desc != nullptr, candidate q of channel blockIdx.y
//                behind the gate of the contract (its decode record attempted without crc_ok, its OSD record -- where used -- without crc_ok,
//                nsync >= min_nsync), 20-byte record to ap[q] and dmin to dmin[q];  desc == nullptr, cwslg_ap_decode: n_flat sets from llr_flat,
//                no gate, 24-byte cwslg_ap_msg;  desc != nullptr and ft4 (cwslg_fetch_ft4_ap), the FT4 decode's addressing: one wave per (record
//                slot, metric set), grid (ceil(9 cap_max / 4), taking-part channels), wave q: slot = q / 3, s = q % 3, cand = slot / 3,
//                r = slot % 3, gone if q >= 9 cap, cand >= min(*cnt, cap) or r >= nrec[cand]; the gate is PER RECORD -- the three crc_ok bytes of
//                the slot's decode record and, where used, of its OSD record, nsync and nqual of its Ft4SoftRec -- and per set iters >= 0;
//                metrics llr[s] of the slot's soft record, record to set[s] of slot's Ft4MsgRec in the staging (= record q), dmin to dmin[q].
//                All of that addressing is scalar (q goes through readfirstlane); everything behind it is the same text.
//   ap_annotate_kernel  one thread per record decode_harvest_kernel has emitted from the AP records: the record's channel through `offsets` (as
//                decode_report_kernel finds it), then by_osd = 2, set = the pattern index, dmin = the AP record's.  FT4: the metric set s from the set
//                byte the harvest wrote, the entry's slot by a serial walk over nrec (entry e is slot 3 k + (e - prefix(k)), prefix the running
//                sum of min(max(nrec[k], 0), 3)), then set = s | pattern << 2 and dmin[3 slot + s].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ap_host.hpp"
#include "ldpc_kernels.hpp"
#include "osd_kernels.hpp"
#include "harvest_kernels.hpp"

namespace cwslg {

struct ApMsgRec { Ft8MsgRec msg; float dmin; };                                  // = cwslg_ap_msg
static_assert(sizeof(ApMsgRec) == 24, "cwslg_ap_msg is 24 bytes");

// One channel that takes part, built by the host under the context mutex (same index as the call's HarvestDesc array).
struct alignas(16) ApDesc {
    const int *cnt;          // the list's count
    const void *soft;        // Ft8SoftRec[cap]; FT4: Ft4SoftRec[cap][3], the slot layout
    const void *msg;         // Ft8MsgRec[cap]; FT4: Ft4MsgRec[cap][3]
    const void *osd;         // OsdRec[cap]; FT4: Ft4OsdRec[cap][3]; null: the OSD records are not used
    void *ap;                // out: Ft8MsgRec[cap] (FT4: Ft4MsgRec[cap][3]), what the harvest reads as the channel's decode records
    float *dmin;             // out: [cap]; FT4: [cap][3][3], dmin[3 slot + s]
    const int *nrec;         // FT4: records per candidate, [cap]; FT8: null
    int cap;                 // the list limit the arrays were sized for
    int pad_;
};
static_assert(sizeof(ApDesc) == 64, "descriptor layout");

// What the two kernels are told; a field its kernel does not read stays 0 / null.
struct ApArgs {
    int n_pat;
    const void *desc;                  // ApDesc[n_chan], or null: llr_flat / ap_flat
    const void *pats;                  // ApBlock
    void *ap_flat;                     // ApMsgRec[n_flat]
    const unsigned *offsets;           // ap_annotate_kernel: the harvest's offsets and output block
    unsigned *out;
    int n_chan, max_out;
    int ft4;                           // desc names FT4 channels: the slot layout, three sets per record
};

// a wave-uniform pointer, held in scalar registers
template <typename T>
__device__ __forceinline__ T *ap_uniform(T *p)
{
    const uintptr_t v = (uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (T *)(((uintptr_t)hi << 32) | lo);
}

__device__ __forceinline__ void ap_annotate(const ApArgs &ap)
{
    CWSLG_GLOBAL unsigned *g_out = as_global_rw(ap.out);
    const CWSLG_GLOBAL unsigned *g_offsets = as_global(ap.offsets);
    const unsigned n_emit = min(g_out[0], (unsigned)max(ap.max_out, 0));
    const unsigned p = blockIdx.x * (unsigned)(64 * LDPC_WAVES) + threadIdx.x;
    if (p >= n_emit) return;
    // the record's channel: the last c with offsets[c] <= p (offsets[0] = 0; channels without decodes make equal offsets)
    int lo_c = 0, hi_c = ap.n_chan;
    while (hi_c - lo_c > 1) {
        const int mid = (lo_c + hi_c) >> 1;
        if (g_offsets[mid] <= p) lo_c = mid; else hi_c = mid;
    }
    const CWSLG_GLOBAL ApDesc *d = as_global(reinterpret_cast<const ApDesc *>(ap.desc)) + lo_c;
    CWSLG_GLOBAL unsigned *rec = g_out + HARVEST_HEAD_WORDS + (size_t)p * HARVEST_REC_WORDS;
    const unsigned entry = rec[1] & 0xffffu;                   // (< cap: the harvest walked min(count, cap) entries)
    if (ap.ft4) {
        // FT4: the metric set from the byte the harvest wrote; the entry's slot by the harvest's own walk -- slot 3 k + r exists iff r < nrec[k],
        // entries number the existing slots in ascending order.  (The entry exists, so the walk ends inside the list.)
        const unsigned s = rec[1] >> 24 & 3u;
        const CWSLG_GLOBAL int *g_nrec = as_global(d->nrec);
        const int ncand = max(0, min(*as_global(d->cnt), d->cap));
        unsigned prefix = 0u, slot = 0u;
        for (int k = 0; k < ncand; ++k) {
            const unsigned nr = (unsigned)min(max(g_nrec[k], 0), 3);
            if (entry < prefix + nr) { slot = 3u * (unsigned)k + (entry - prefix); break; }
            prefix += nr;
        }
        const unsigned w4 = as_global(reinterpret_cast<const unsigned *>(d->ap))[(size_t)slot * 15u + 5u * s + 4u];
        rec[1] = entry | 2u << 16 | (s | (w4 >> 24) << 2) << 24;
        rec[8] = as_global(reinterpret_cast<const unsigned *>(d->dmin))[3u * slot + s];
        return;
    }
    const unsigned w4 = as_global(reinterpret_cast<const unsigned *>(d->ap))[(size_t)entry * 5u + 4u];      // nharderr | crc_ok << 16 | pad_ << 24
    rec[1] = entry | 2u << 16 | (w4 >> 24) << 24;
    rec[8] = as_global(reinterpret_cast<const unsigned *>(d->dmin))[entry];
}

__global__ __launch_bounds__(64 * LDPC_WAVES) void ap_annotate_kernel(ApArgs ap) { ap_annotate(ap); }

__global__ __launch_bounds__(64 * LDPC_WAVES) void ap_decode_kernel(ApArgs ap, const float *__restrict__ llr_flat, int n_flat, int max_iter, int min_nsync,
                                                                    int min_nqual, const LdpcTables *__restrict__ tables)
{
    __shared__ __attribute__((aligned(16))) float s_vall[LDPC_WAVES][LDPC_VSIZE];
    __shared__ __attribute__((aligned(16))) float s_zall[LDPC_WAVES][192];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float *s_v = s_vall[wv], *s_z = s_zall[wv];               // the wave's LDS image
    const int q = (int)blockIdx.x * LDPC_WAVES + wv;
    const CWSLG_GLOBAL float *llr;
    CWSLG_GLOBAL uint32_t *ow, *od;                            // the 20-byte record, the dmin word
    bool attempt = true;
    if (ap.desc && ap.ft4) {
        // FT4: the decode's third addressing and its exits; wave q is set s of record slot q / 3, all of it scalar
        const CWSLG_GLOBAL ApDesc *d = as_global(reinterpret_cast<const ApDesc *>(ap.desc)) + blockIdx.y;
        const int qs = __builtin_amdgcn_readfirstlane(q), cap = d->cap;
        if (qs >= 9 * cap) return;                             // wave-uniform, all three
        const int slot = qs / 3, s = qs - 3 * slot, cand = slot / 3, r = slot - 3 * cand;
        if (cand >= min(*as_global(d->cnt), cap)) return;
        if (r >= as_global(d->nrec)[cand]) return;
        const CWSLG_GLOBAL Ft4SoftRec *rec = as_global(reinterpret_cast<const Ft4SoftRec *>(d->soft)) + slot;
        const CWSLG_GLOBAL uint32_t *m = reinterpret_cast<const CWSLG_GLOBAL uint32_t *>(as_global(reinterpret_cast<const Ft4MsgRec *>(d->msg)) + slot);
        llr = rec->llr[s];
        ow = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(as_global_rw(reinterpret_cast<Ft8MsgRec *>(d->ap)) + qs);     // set s of slot q / 3
        od = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(as_global_rw(d->dmin) + qs);                                  // dmin[3 slot + s]
        // the record's gate: no set with BP crc_ok (word 4 of a set: nharderr | crc_ok << 16 | pad_ << 24), nor -- where used -- with OSD crc_ok
        // (word 5 of a set: crc_ok | how << 8 | flip << 16); this set attempted by the decode (word 3: iters | nbad << 16)
        attempt = (int16_t)(m[5 * s + 3] & 0xffffu) >= 0 && ((m[4] | m[9] | m[14]) >> 16 & 0xffu) == 0u && rec->nsync >= min_nsync && rec->nqual >= min_nqual;
        if (attempt && d->osd != nullptr) {
            const CWSLG_GLOBAL uint32_t *o = reinterpret_cast<const CWSLG_GLOBAL uint32_t *>(as_global(reinterpret_cast<const Ft4OsdRec *>(d->osd)) + slot);
            attempt = ((o[5] | o[11] | o[17]) & 0xffu) == 0u;
        }
    } else if (ap.desc) {
        const CWSLG_GLOBAL ApDesc *d = as_global(reinterpret_cast<const ApDesc *>(ap.desc)) + blockIdx.y;
        const int ncand = min(*as_global(d->cnt), d->cap);
        if (q >= ncand) return;                                // wave-uniform
        const CWSLG_GLOBAL Ft8SoftRec *rec = as_global(reinterpret_cast<const Ft8SoftRec *>(d->soft)) + q;
        const CWSLG_GLOBAL Ft8MsgRec *m = as_global(reinterpret_cast<const Ft8MsgRec *>(d->msg)) + q;
        llr = rec->llr;
        ow = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(as_global_rw(reinterpret_cast<Ft8MsgRec *>(d->ap)) + q);
        od = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(as_global_rw(d->dmin) + q);
        attempt = m->iters >= 0 && m->crc_ok == 0 && rec->nsync >= min_nsync;
        if (attempt && d->osd != nullptr) attempt = (as_global(reinterpret_cast<const OsdRec *>(d->osd)) + q)->crc_ok == 0;
    } else {
        if (q >= n_flat) return;
        llr = as_global(llr_flat) + (size_t)q * LDPC_N;
        ow = reinterpret_cast<CWSLG_GLOBAL uint32_t *>(as_global_rw(reinterpret_cast<ApMsgRec *>(ap.ap_flat)) + q);
        od = ow + 5;
    }
    llr = ap_uniform(llr); ow = ap_uniform(ow); od = ap_uniform(od);
    const bool third = lane + 128 < LDPC_N;
    float l2 = 0.0f, amax = 0.0f;
    if (attempt) {                                             // wave-uniform
        const float l0 = llr[lane], l1 = llr[lane + 64];
        l2 = third ? llr[lane + 128] : 0.0f;
        const float a0 = fabsf(l0), a1 = fabsf(l1), a2 = fabsf(l2);
        if (__ballot(!(a0 < INFINITY) || !(a1 < INFINITY) || !(a2 < INFINITY)) != 0ull) attempt = false;
        amax = fmaxf(fmaxf(a0, a1), a2);
    }
    if (!attempt) {                                            // the decode record's "not attempted" bytes, pad_ = 0xff, dmin = +0
        if (lane < 5) ow[lane] = lane < 3 ? 0u : lane == 3 ? 0xffffffffu : 0xff00ffffu;
        if (lane == 5) od[0] = 0u;
        return;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) amax = fmaxf(amax, __shfl_xor(amax, off, 64));
    const float A = __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(1.01f * amax)));

    LdpcGraph g;
    ldpc_graph_load(g, as_global(tables), lane);
    const CWSLG_GLOBAL uint32_t *pw = as_global(reinterpret_cast<const uint32_t *>(ap.pats));

    int iters_sum = 0, it = 0, nbad = 0, found = -1;
    uint64_t b0 = 0ull, b1 = 0ull, b2 = 0ull, hi = 0ull;       // the word of the last run as ballots: scalars, nothing per lane outlives a run
    for (int p = 0; p < ap.n_pat; ++p) {                       // wave-uniform
        uint32_t w[AP_PAT_WORDS];
#pragma unroll
        for (int k = 0; k < AP_PAT_WORDS; ++k) w[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)pw[AP_PAT_WORDS * p + k]);
        const uint64_t mlo = w[0] | ((uint64_t)w[1] << 32), mhi = w[2], vlo = w[3] | ((uint64_t)w[4] << 32), vhi = w[5];
        int ln = lane;
        asm volatile("" : "+v"(ln));                           // (the lane's shifts and addresses are made here, per pattern, not kept across the runs)
        const bool m0 = (mlo >> ln) & 1ull, v0 = (vlo >> ln) & 1ull;
        const bool m1 = ln < 32 && ((mhi >> (ln & 31)) & 1ull), v1 = ln < 32 && ((vhi >> (ln & 31)) & 1ull);
        const float p0 = m0 ? (v0 ? A : -A) : llr[ln], p1 = m1 ? (v1 ? A : -A) : llr[ln + 64];
        float z0, z1, z2;
        ldpc_bp_run(g, p0, p1, l2, max_iter, s_v, s_z, lane, it, nbad, z0, z1, z2);
        iters_sum += it;
        b0 = __ballot(z0 > 0.0f);
        b1 = __ballot(z1 > 0.0f);
        b2 = __ballot(third && z2 > 0.0f);
        hi = b1 & ((1ull << (LDPC_K - 64)) - 1);              // codeword bits 64..90
        // success: a codeword, the CRC-14 rule, and the word agrees with the hypothesis it was found under
        if (nbad == 0 && ((b0 ^ vlo) & mlo) == 0ull && ((hi ^ vhi) & mhi) == 0ull && ldpc_crc14(b0, hi) == ldpc_crc_field(b0, hi)) {
            found = p;
            break;
        }
    }
    if (found < 0) {                                           // zero bits, iters = the sum, nbad = the last run's, nharderr -1, crc_ok 0, pad_ 0xff
        if (lane < 5) ow[lane] = lane < 3 ? 0u : lane == 3 ? (((uint32_t)iters_sum & 0xffffu) | ((uint32_t)nbad << 16)) : 0xff00ffffu;
        if (lane == 5) od[0] = 0u;
        return;
    }
    // nharderr and dmin against the ORIGINAL metrics, read once more: the error pattern in OSD's bit layout, |llr| where the loop's z image was
    const float l0 = llr[lane], l1 = llr[lane + 64];
    const uint64_t e0 = __ballot(l0 > 0.0f) ^ b0, e1 = __ballot(l1 > 0.0f) ^ b1, e2 = __ballot(third && l2 > 0.0f) ^ b2;
    const int nharderr = __popcll(e0) + __popcll(e1) + __popcll(e2);
    const uint32_t e[OSD_GW] = {(uint32_t)e0, (uint32_t)(e0 >> 32), (uint32_t)e1, (uint32_t)(e1 >> 32), (uint32_t)e2, (uint32_t)(e2 >> 32)};
    ldpc_wave_sync();                                          // (every lane has read its rows' z)
    s_z[lane] = fabsf(l0);
    s_z[lane + 64] = fabsf(l1);
    s_z[lane + 128] = fabsf(l2);                               // (174..191: +0, never read: the error pattern has no bit there)
    ldpc_wave_sync();
    const float dmin = osd_dist(e, s_z);                       // wave-uniform: every lane walks the same chain
    const uint64_t r0 = __brevll(b0), r1 = __brevll(hi);       // bits[] as cwslg_ft8_msg packs them
    uint32_t word;
    switch (lane) {
    case 0: word = __builtin_bswap32((uint32_t)(r0 >> 32)); break;
    case 1: word = __builtin_bswap32((uint32_t)r0); break;
    case 2: word = __builtin_bswap32((uint32_t)(r1 >> 32)); break;
    case 3: word = (uint32_t)it & 0xffffu; break;             // iters of that run, nbad = 0
    default: word = ((uint32_t)nharderr & 0xffffu) | 0x10000u | ((uint32_t)found << 24); break;
    }
    if (lane < 5) ow[lane] = word;
    if (lane == 5) od[0] = __float_as_uint(dmin);
}

// The launches.  The caller asks hipGetLastError.
//   ap_decode_kernel on the n_chan channels of d_desc (cap_max: the largest cap among them); ft4: a wave per (record slot, metric set), 9 per candidate
inline void ap_launch_chain(hipStream_t s, const ApDesc *d_desc, int n_chan, int cap_max, int max_iter, int min_nsync, const void *tables,
                            const void *pats, int n_pat, bool ft4 = false, int min_nqual = 0)
{
    if (n_chan <= 0 || cap_max <= 0) return;
    ApArgs ap{};
    ap.n_pat = n_pat; ap.desc = d_desc; ap.pats = pats; ap.n_chan = n_chan; ap.ft4 = ft4 ? 1 : 0;
    const int waves = ft4 ? 9 * cap_max : cap_max;
    hipLaunchKernelGGL(ap_decode_kernel, dim3((unsigned)((waves + LDPC_WAVES - 1) / LDPC_WAVES), (unsigned)n_chan), dim3(64 * LDPC_WAVES), 0, s, ap,
                       (const float *)nullptr, 0, max_iter, min_nsync, min_nqual, (const LdpcTables *)tables);
}
//   ap_decode_kernel flat: n sets of 174 metrics, no gate
inline void ap_launch_flat(hipStream_t s, const void *tables, const void *pats, int n_pat, const float *llr, ApMsgRec *out, int n, int max_iter)
{
    if (n <= 0) return;
    ApArgs ap{};
    ap.n_pat = n_pat; ap.pats = pats; ap.ap_flat = out;
    hipLaunchKernelGGL(ap_decode_kernel, dim3((unsigned)((n + LDPC_WAVES - 1) / LDPC_WAVES), 1), dim3(64 * LDPC_WAVES), 0, s, ap, llr, n, max_iter, 0, 0,
                       (const LdpcTables *)tables);
}
//   ap_annotate_kernel behind harvest_launch on the same stream and blocks: a thread per record that emit may have written
inline void ap_launch_annotate(hipStream_t s, const ApDesc *d_desc, const unsigned *d_offsets, unsigned *d_out, int n_chan, int lim, bool ft4 = false)
{
    if (lim <= 0) return;
    ApArgs ap{};
    ap.desc = d_desc; ap.offsets = d_offsets; ap.out = d_out; ap.n_chan = n_chan; ap.max_out = lim; ap.ft4 = ft4 ? 1 : 0;
    hipLaunchKernelGGL(ap_annotate_kernel, dim3((unsigned)((lim + 64 * LDPC_WAVES - 1) / (64 * LDPC_WAVES))), dim3(64 * LDPC_WAVES), 0, s, ap);
}

} // namespace cwslg
