// ft4soft_kernels.hpp -- FT4 soft bits on gfx950: per refined sync record (cwslg_ft4_sync) the last stage of upstream ft4_decode before
// LDPC -- the final downsample at the corrected frequency f1, get_ft4_bitmetrics' three metric sets (single-symbol, two-symbol coherent,
// four-symbol coherent), their normalisation, and the two sync-quality counts nsync / nqual.
//
// *** PARITY UNPINNED by the reference *** like the rest of the sync stage (sync_kernels.hpp).  The arithmetic is the one
// include/cwsl_gpu.h states for cwslg_ft4_soft and tests/ft4_softbits_ref.py restates in numpy, BIT FOR BIT: the baseband is
// ft4_refine_kernel's own (f4_baseband, ft4sync_kernels.hpp) evaluated at f1_hz; symbol k is the 32 samples from ibest + 32 k (+0 outside
// the buffer); its four tone amplitudes are 32-term fmaf chains in ascending sample order; every magnitude is sqrtf(fmaf(re, re, im im));
// the complex sums of sets 1 and 2 are added left to right; maxima are order-free; both 206-term sums of normalizebmet are the fixed tree
// a wave evaluates: lane l holds b[l], b[l+64], b[l+128], b[l+192] (zero beyond 205), adds them left to right, then six halving steps.
// This translation unit is built -ffp-contract=off: every product, sum, quotient and root that is not a written fmaf is one float32
// operation (hipcc's default keeps / and sqrtf correctly rounded).
//
// One 256-thread workgroup per record slot, grid (3 max_cand, FT4 channels): the workgroup of slot (cand, r) reads the candidate count and
// nrec[cand] on the device -- no host round trip -- and leaves if the slot holds no record.  The 412 symbol-spectrum chains are spread over
// the 256 threads; cs[103][4] (32-byte rows: the four tones of a symbol are eight consecutive banks, and a wave's reads of one symbol are
// broadcasts) and the magnitudes stay in LDS.  Set 2's 25 groups go round the four waves, each lane holding four of a group's 256
// magnitudes (index 4 lane + d): the two low index bits are reduced in the lane, the six lane bits by xor butterflies.
//
// cwslg_fetch_ft4_decode_reports adds a kernel of its own, ft4_report_kernel: one workgroup per emitted decode, launched ONCE
// behind decode_harvest_kernel's three launches on a fetch stream.  It finds the decode's channel (binary search of the scan's offsets) and
// record slot (prefix over nrec[]), builds the SAME baseband and cs[103][4] through ft4s_symbol_spectra -- one text for both kernels -- and
// then one wave re-encodes the word (91 bits -> 174 -> 103 tones) and makes the 16-byte cwslg_decode_report.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ft4sync_kernels.hpp"
#include "ft8soft_kernels.hpp"
#include "harvest_kernels.hpp"      // the record layout ft4_report_kernel reads, REPORT_*
#include "ft4_tone_device.hpp"      // FT4S_ICOS4, ft4s_gray, ft4r_tone

namespace cwslg {

constexpr int FT4S_NN = 103, FT4S_NBM = 206, FT4S_NBIT = 174;
struct Ft4SoftRec { float llr[3][FT4S_NBIT]; float sigma[3]; int32_t nsync, nqual, pad_; };       // = cwslg_ft4_soft
static_assert(sizeof(Ft4SoftRec) == 2112, "cwslg_ft4_soft is 2112 bytes");

// (icos4, FT4S_ICOS4: ft4_tone_device.hpp)  the four hard-decision patterns of nqual, one bit per entry [8 block + j]
constexpr unsigned ft4s_pack1(const int (&v)[32]) { unsigned c = 0; for (int i = 0; i < 32; ++i) c |= (unsigned)v[i] << i; return c; }
constexpr int FT4S_QUAL_V[32] = {0, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1};
constexpr unsigned FT4S_QUAL = ft4s_pack1(FT4S_QUAL_V);

// ---- the decode reports (cwslg_fetch_ft4_decode_reports; the contract is the header's, tests/ft4_decode_reports_ref.py restates it) ----
// One channel that takes part in a report call, in an array of its own beside the HarvestDesc array (same index).
struct alignas(16) Ft4ReportDesc {
    const float2 *cx;        // the channel's frame spectrum, [36289] (written by the boundary that made the records)
    const Ft4Rec *rec;       // [cap][3]
    const int *nrec;         // records per candidate, [cap]
    const int *cnt;          // the list's count
    int cap;                 // the list limit the arrays were sized for
    int pad_[3];
};
static_assert(sizeof(Ft4ReportDesc) == 48, "descriptor layout");
struct Ft4ReportArgs {
    int n_chan, max_out;
    const Ft4ReportDesc *rdesc;
    const unsigned *offsets;     // decode_harvest_kernel's scan: the first record of every channel
    const unsigned *out;         // its head and records
    const uint32_t *enc;         // the systematic encoder, 91 x 6 dwords
    unsigned *rep;               // [max_out][4]
};

__device__ __forceinline__ float ft4s_mag(float2 z) { return sqrtf(__builtin_fmaf(z.x, z.x, z.y * z.y)); }
__device__ __forceinline__ float2 ft4s_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// The first two thirds of a record's work, ONE text for the soft bits and for the decode reports: the baseband at f1 from the channel's frame
// spectrum cx, then the 412 symbol-spectrum chains -> s_cs[103][4] and their magnitudes s_mag[103][4].  Called by all 256 threads; ends behind
// a barrier (f4_baseband's barriers also publish s_w32 and whatever the caller stored to LDS before the call).
__device__ __forceinline__ void ft4s_symbol_spectra(const F4BaseLds &L, const float2 *cx, const Ft4Tables &tb, const float2 *w32, float2 *s_w32,
                                                    float2 (*s_cs)[4], float (*s_mag)[4], float f1, int ibest, int tid)
{
    if (tid < 32) s_w32[tid] = w32[tid];
    f4_baseband(L, cx, tb, f1, tid);
    const F4Cd cd{L.cd};

    // ---- symbol spectra: thread e -> symbol k = e / 4, tone q = e % 4
    for (int e = tid; e < 4 * FT4S_NN; e += 256) {
        const int k = e >> 2, q = e & 3;
        const int m0 = ibest + F4C_NSS * k;
        float zr = 0.f, zi = 0.f;
#pragma unroll 8
        for (int t = 0; t < F4C_NSS; ++t) {
            const int m = m0 + t;
            const bool in = m >= 0 && m < F4C_NP;
            float2 c = cd.at(in ? m : 0);
            if (!in) c = make_float2(0.f, 0.f);
            const float2 s = s_w32[(q * t) & 31];
            zr = __builtin_fmaf(c.x, s.x, zr); zr = __builtin_fmaf(c.y, s.y, zr);
            zi = __builtin_fmaf(c.y, s.x, zi); zi = __builtin_fmaf(-c.x, s.y, zi);
        }
        const float2 z = make_float2(zr, zi);
        s_cs[k][q] = z;
        s_mag[k][q] = ft4s_mag(z);
    }
    __syncthreads();
}

// ---- ft4_report_kernel: the FT4 decode reports (cwslg_fetch_ft4_decode_reports) -----------------------------------------------------------------------
// (ft4r_tone: ft4_tone_device.hpp)

// One symbol: is the first maximum of the magnitudes at the encoded tone?  the power at the tone and at the tone two bins away
__device__ __forceinline__ bool ft4r_symbol(const float2 (*s_cs)[4], const float (*s_mag)[4], int n, int tone, float *sig, float *noi)
{
    const v4f m = *reinterpret_cast<const v4f *>(s_mag[n]);
    const float2 z0 = s_cs[n][0], z1 = s_cs[n][1], z2 = s_cs[n][2], z3 = s_cs[n][3];
    const float p0 = __builtin_fmaf(z0.x, z0.x, z0.y * z0.y), p1 = __builtin_fmaf(z1.x, z1.x, z1.y * z1.y);
    const float p2 = __builtin_fmaf(z2.x, z2.x, z2.y * z2.y), p3 = __builtin_fmaf(z3.x, z3.x, z3.y * z3.y);
    int km = 0;
    float vm = m.x;
    if (m.y > vm) { vm = m.y; km = 1; }
    if (m.z > vm) { vm = m.z; km = 2; }
    if (m.w > vm) { vm = m.w; km = 3; }
    const int u = (tone + 2) & 3;
    *sig = tone == 0 ? p0 : tone == 1 ? p1 : tone == 2 ? p2 : p3;
    *noi = u == 0 ? p0 : u == 1 ? p1 : u == 2 ? p2 : p3;
    return km == tone;
}

// One workgroup per emitted record p = blockIdx.x (grid sized by the caller's limit; the count min(out[0], max_out) is read on the device and the
// workgroups beyond it leave).  ft4_report_find: what the record's spectra are made from, before ft4s_symbol_spectra; false (workgroup-uniform):
// nothing to do.  s_u: 8 words of LDS scratch.
struct Ft4ReportJob { const float2 *cx; float f1; int ibest; unsigned k0, k1, k2; };
__device__ __forceinline__ bool ft4_report_find(const Ft4ReportArgs &ra, unsigned *s_u, Ft4ReportJob *job)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const CWSLG_GLOBAL unsigned *g_out = as_global(ra.out), *g_offsets = as_global(ra.offsets);
    const unsigned n_emit = min((unsigned)__builtin_amdgcn_readfirstlane((int)g_out[0]), (unsigned)max(ra.max_out, 0));
    const unsigned p = blockIdx.x;
    if (p >= n_emit) return false;                              // workgroup-uniform
    // the record's channel: the last c with offsets[c] <= p (offsets[0] = 0; channels without decodes make equal offsets)
    int lo_c = 0, hi_c = ra.n_chan;
    while (hi_c - lo_c > 1) {
        const int mid = (lo_c + hi_c) >> 1;
        const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane((int)g_offsets[mid]);
        if (o <= p) lo_c = mid; else hi_c = mid;
    }
    const CWSLG_GLOBAL Ft4ReportDesc *rd = as_global(ra.rdesc) + lo_c;
    const CWSLG_GLOBAL unsigned *orec = g_out + HARVEST_HEAD_WORDS + (size_t)p * HARVEST_REC_WORDS;
    const unsigned entry = orec[1] & 0xffffu, k0 = orec[2], k1 = orec[3], k2 = orec[4];

    // ---- the entry's slot: entries number the records in ascending slot order, so slot = 3 k + (entry - prefix(k)) for the candidate k with
    // prefix(k) <= entry < prefix(k) + nrec[k]; the prefix over nrec[] 256 candidates at a time, as decode_harvest_kernel's scan
    const CWSLG_GLOBAL int *g_nrec = as_global(rd->nrec);
    const int n = max(0, min(min(*as_global(rd->cnt), rd->cap), SYNC_MAXCAND_CAP));
    if (tid == 0) s_u[4] = 0xffffffffu;
    unsigned carry = 0u;
    for (int base = 0; base < n; base += 256) {
        const int k = base + tid;
        const unsigned v = k < n ? (unsigned)max(0, min(g_nrec[k], 3)) : 0u;
        unsigned inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_u[wv] = inc;
        __syncthreads();
        const unsigned w0 = s_u[0], w1 = s_u[1], w2 = s_u[2], w3 = s_u[3];
        const unsigned before = carry + (wv > 0 ? w0 : 0u) + (wv > 1 ? w1 : 0u) + (wv > 2 ? w2 : 0u) + (inc - v);
        if (entry >= before && entry < before + v) s_u[4] = 3u * (unsigned)k + (entry - before);
        __syncthreads();
        carry += w0 + w1 + w2 + w3;
    }
    __syncthreads();
    const unsigned slot = s_u[4];
    if (slot == 0xffffffffu) return false;                      // (no such entry: nothing is written; workgroup-uniform)
    const CWSLG_GLOBAL Ft4Rec *rec = as_global(rd->rec) + slot;
    job->cx = rd->cx; job->f1 = rec->f1_hz; job->ibest = rec->ibest;
    job->k0 = k0; job->k1 = k1; job->k2 = k2;
    return true;
}

// ft4_report_finish: behind ft4s_symbol_spectra, ONE wave's work -- the word of record p re-encoded, its 103 tones, the report.
__device__ __forceinline__ void ft4_report_finish(const Ft4ReportArgs &ra, const float2 (*s_cs)[4], const float (*s_mag)[4], unsigned k0, unsigned k1,
                                                  unsigned k2, int lane)
{
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const unsigned p = blockIdx.x;

    // ---- the codeword: lane l owns encoder rows l and l + 64 (rows 64..90 on lanes 0..26); XOR across the lanes (as decode_report_kernel) ----
    const int row_b = lane + 64 < REPORT_ENC_ROWS ? lane + 64 : lane;  // (a lane without a second row loads its first again and drops it)
    const CWSLG_GLOBAL v2u *ea = reinterpret_cast<const CWSLG_GLOBAL v2u *>(as_global(ra.enc) + (size_t)lane * REPORT_ENC_WORDS);
    const CWSLG_GLOBAL v2u *eb = reinterpret_cast<const CWSLG_GLOBAL v2u *>(as_global(ra.enc) + (size_t)row_b * REPORT_ENC_WORDS);
    const v2u a0 = ea[0], a1 = ea[1], a2 = ea[2], b0 = eb[0], b1 = eb[1], b2 = eb[2];
    // message bit k: byte k >> 3 of bits[12] (three little-endian words), MSB first
    const unsigned wa = lane < 32 ? k0 : k1;                                        // k = lane: bytes 0..7
    const unsigned bit_a = wa >> (8 * ((lane >> 3) & 3) + 7 - (lane & 7)) & 1u;
    const unsigned bit_b = lane + 64 < REPORT_ENC_ROWS ? k2 >> (8 * ((lane >> 3) & 3) + 7 - (lane & 7)) & 1u : 0u;     // k = lane + 64: bytes 8..11
    const unsigned ma = 0u - bit_a, mb = 0u - bit_b;
    unsigned c0 = (a0.x & ma) ^ (b0.x & mb), c1 = (a0.y & ma) ^ (b0.y & mb), c2 = (a1.x & ma) ^ (b1.x & mb);
    unsigned c3 = (a1.y & ma) ^ (b1.y & mb), c4 = (a2.x & ma) ^ (b2.x & mb), c5 = (a2.y & ma) ^ (b2.y & mb);
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        c0 ^= (unsigned)__shfl_xor((int)c0, h, 64); c1 ^= (unsigned)__shfl_xor((int)c1, h, 64); c2 ^= (unsigned)__shfl_xor((int)c2, h, 64);
        c3 ^= (unsigned)__shfl_xor((int)c3, h, 64); c4 ^= (unsigned)__shfl_xor((int)c4, h, 64); c5 ^= (unsigned)__shfl_xor((int)c5, h, 64);
    }

    // ---- lane l: symbol l, and symbol l + 64 where that is below 103 ----
    const bool two = lane + 64 < FT4S_NN;
    const int nb = two ? lane + 64 : lane;
    bool cos_a, cos_b;
    const int ta = ft4r_tone(c0, c1, c2, c3, c4, c5, lane, &cos_a), tb2 = ft4r_tone(c0, c1, c2, c3, c4, c5, nb, &cos_b);
    float sig_a, noi_a, sig_b, noi_b;
    const bool hit_a = ft4r_symbol(s_cs, s_mag, lane, ta, &sig_a, &noi_a), hit_b = ft4r_symbol(s_cs, s_mag, nb, tb2, &sig_b, &noi_b);
    const int nsync = __popcll(__ballot(cos_a && hit_a)) + __popcll(__ballot(two && cos_b && hit_b));
    const int nsymerr = __popcll(__ballot(!cos_a && !hit_a)) + __popcll(__ballot(two && !cos_b && !hit_b));
    const float xsig = ft8s_tree64(two ? sig_a + sig_b : sig_a), xnoise = ft8s_tree64(two ? noi_a + noi_b : noi_a);
    if (lane == 0) {
        const float r = xnoise > 0.0f ? xsig / xnoise - 1.0f : 0.0f;
        const float x = fminf(r > 0.1f ? r : 0.001f, 3.4028234663852886e38f);      // (an infinite ratio reports as the largest float's)
        const float db = (float)(10.0 * long_log10_fixed((double)x) - 20.8);
        v4u o;
        o.x = __float_as_uint(fmaxf(db, -21.0f)); o.y = __float_as_uint(xsig); o.z = __float_as_uint(xnoise);
        o.w = (unsigned)nsync | (unsigned)nsymerr << 16;
        *reinterpret_cast<CWSLG_GLOBAL v4u *>(as_global_rw(ra.rep) + (size_t)p * REPORT_WORDS) = o;
    }
}

// The decode reports of a fetch, grid (records).
__global__ __launch_bounds__(256) void ft4_report_kernel(Ft4Tables tb, const float2 *__restrict__ w32, Ft4ReportArgs ra)
{
    F4_BASE_LDS(L);
    __shared__ float2 s_cs[FT4S_NN][4];
    __shared__ __attribute__((aligned(16))) float s_mag[FT4S_NN][4];
    __shared__ float2 s_w32[32];
    __shared__ unsigned s_u[16];
    const int tid = threadIdx.x;
    Ft4ReportJob job;                                // what the spectra are made from: cx, f1_hz, ibest, and the word
    if (!ft4_report_find(ra, s_u, &job)) return;
    ft4s_symbol_spectra(L, job.cx, tb, w32, s_w32, s_cs, s_mag, job.f1, job.ibest, tid);
    if ((tid >> 6) == 0) ft4_report_finish(ra, s_cs, s_mag, job.k0, job.k1, job.k2, tid & 63);
}

// The boundary's soft bits, grid (3 max_cand, FT4 channels).
__global__ __launch_bounds__(256) void ft4_softbits_kernel(const Ft4Work *__restrict__ works, Ft4SoftRec *const *__restrict__ soft,
                                                           Ft4Tables tb, const float2 *__restrict__ w32, int max_cand)
{
    F4_BASE_LDS(L);
    __shared__ float2 s_cs[FT4S_NN][4];
    __shared__ __attribute__((aligned(16))) float s_mag[FT4S_NN][4];
    __shared__ __attribute__((aligned(16))) float s_bm[3][256];            // the three metric sets, padded with +0
    __shared__ float2 s_w32[32];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = blockIdx.x;
    const Ft4Work *w = works + blockIdx.y;
    const int cand = slot / 3, r = slot - 3 * cand;
    int ncand = *as_global(w->ncand);
    if (ncand > max_cand) ncand = max_cand;
    if (cand >= ncand) return;                      // workgroup-uniform, both
    if (r >= as_global(w->nrec)[cand]) return;
    const CWSLG_GLOBAL Ft4Rec *rec = as_global(w->rec) + slot;
    for (int e = tid; e < 3 * 256; e += 256) (&s_bm[0][0])[e] = 0.0f;
    ft4s_symbol_spectra(L, w->cx, tb, w32, s_w32, s_cs, s_mag, rec->f1_hz, rec->ibest, tid);

    // ---- nsync: lanes 0..15 of wave 0 take one Costas symbol each; first maximum over the tones (ties to the lowest tone)
    int nsync = 0;
    if (wv == 0) {
        bool hit = false;
        if (lane < 16) {
            const float *t = s_mag[33 * (lane >> 2) + (lane & 3)];
            int km = 0;
            float vm = t[0];
#pragma unroll
            for (int q = 1; q < 4; ++q) if (t[q] > vm) { vm = t[q]; km = q; }
            hit = km == (int)((FT4S_ICOS4 >> (2 * lane)) & 3u);
        }
        nsync = __popcll(__ballot(hit));
    }
    // ---- set 0: thread e -> metric 2 k + ib; s2[v] = |cs[k][graymap[v]]|
    if (tid < FT4S_NBM) {
        const v4f m = *reinterpret_cast<const v4f *>(s_mag[tid >> 1]);
        s_bm[0][tid] = (tid & 1) ? fmaxf(m.y, m.z) - fmaxf(m.x, m.w)       // index bit 0: v = 1, 3 against 0, 2
                                 : fmaxf(m.w, m.z) - fmaxf(m.x, m.y);      // index bit 1: v = 2, 3 against 0, 1
    }
    // ---- set 1: thread e -> metric e = 4 (pair) + ib of the pair's 16 two-symbol magnitudes
    if (tid < 204) {
        const int ks = 2 * (tid >> 2), sh = 3 - (tid & 3);
        float set = -1.0f, clr = -1.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float v = ft4s_mag(ft4s_add(s_cs[ks][ft4s_gray(i >> 2)], s_cs[ks + 1][ft4s_gray(i & 3)]));
            if ((i >> sh) & 1) set = fmaxf(set, v); else clr = fmaxf(clr, v);
        }
        s_bm[1][tid] = set - clr;
    }
    // ---- set 2: group = four symbols, 256 magnitudes, index i = 4 lane + d; metric ib pairs with index bit 7 - ib
    for (int grp = wv; grp < 25; grp += 4) {
        const int ks = 4 * grp;
        const float2 part = ft4s_add(ft4s_add(s_cs[ks][ft4s_gray(lane >> 4)], s_cs[ks + 1][ft4s_gray((lane >> 2) & 3)]),
                                     s_cs[ks + 2][ft4s_gray(lane & 3)]);
        float v[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) v[d] = ft4s_mag(ft4s_add(part, s_cs[ks + 3][ft4s_gray(d)]));
        float bm[8];
        // index bits 0, 1 (metrics 7, 6): set / clear maxima inside the lane, then over the whole wave
        float s7 = fmaxf(v[1], v[3]), c7 = fmaxf(v[0], v[2]), s6 = fmaxf(v[2], v[3]), c6 = fmaxf(v[0], v[1]);
#pragma unroll
        for (int h = 1; h < 64; h <<= 1) {
            s7 = fmaxf(s7, __shfl_xor(s7, h, 64)); c7 = fmaxf(c7, __shfl_xor(c7, h, 64));
            s6 = fmaxf(s6, __shfl_xor(s6, h, 64)); c6 = fmaxf(c6, __shfl_xor(c6, h, 64));
        }
        bm[7] = s7 - c7; bm[6] = s6 - c6;
        // index bit 2 + j = lane bit j (metric 5 - j): butterflies over the other five lane bits leave the set maximum on the lanes with
        // bit j and the clear maximum on those without; one exchange across bit j pairs them
        const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            float x = mx;
#pragma unroll
            for (int t = 0; t < 6; ++t) if (t != j) x = fmaxf(x, __shfl_xor(x, 1 << t, 64));
            const float y = __shfl_xor(x, 1 << j, 64);
            bm[5 - j] = ((lane >> j) & 1) ? x - y : y - x;
        }
        if (lane == 0) {
            *reinterpret_cast<v4f *>(&s_bm[2][8 * grp]) = v4f{bm[0], bm[1], bm[2], bm[3]};
            *reinterpret_cast<v4f *>(&s_bm[2][8 * grp + 4]) = v4f{bm[4], bm[5], bm[6], bm[7]};
        }
    }
    __syncthreads();
    // ---- the tails: the last symbol (pair) has no partner; copies of the un-normalised values
    if (tid < 2) { const float b = s_bm[0][204 + tid]; s_bm[1][204 + tid] = b; s_bm[2][204 + tid] = b; }
    else if (tid < 6) s_bm[2][198 + tid] = s_bm[1][198 + tid];
    __syncthreads();

    CWSLG_GLOBAL Ft4SoftRec *out = as_global_rw(soft[blockIdx.y]) + slot;
    // ---- nqual: hard decisions of set 0 at the four Costas blocks against the gray-decoded Costas tones
    if (wv == 0) {
        const bool agree = lane < 32 && (s_bm[0][66 * ((lane & 31) >> 3) + (lane & 7)] >= 0.0f) == (bool)((FT4S_QUAL >> (lane & 31)) & 1u);
        const int nqual = __popcll(__ballot(agree));
        if (lane == 0) { out->nsync = nsync; out->nqual = nqual; out->pad_ = 0; }
    }
    // ---- normalizebmet + llr: wave s takes set s
    if (wv < 3) {
        const float *b = s_bm[wv];
        const float b0 = b[lane], b1 = b[lane + 64], b2 = b[lane + 128], b3 = b[lane + 192];
        const float S1 = ft8s_tree64(((b0 + b1) + b2) + b3);
        const float S2 = ft8s_tree64(((b0 * b0 + b1 * b1) + b2 * b2) + b3 * b3);
        const float mean = S1 / 206.0f, m2 = S2 / 206.0f;
        const float var = m2 - mean * mean;
        const float sigma = sqrtf(var > 0.0f ? var : m2);
        const bool live = sigma != 0.0f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int o = lane + 64 * j;             // llr 0..57, 58..115, 116..173 <- entries 8..65, 74..131, 140..197
            if (o < FT4S_NBIT) out->llr[wv][o] = live ? (b[o + 8 * (1 + o / 58)] / sigma) * 2.83f : 0.0f;
        }
        if (lane == 0) out->sigma[wv] = sigma;
    }
}

// The boundary's launch: one workgroup per record slot of every FT4 channel.
inline void ft4_softbits_launch(hipStream_t s, const Ft4Work *d_works, Ft4SoftRec *const *d_soft, const Ft4Tables &tb, const float2 *d_w32, int max_cand, int n_chan)
{
    hipLaunchKernelGGL(ft4_softbits_kernel, dim3(3u * (unsigned)max_cand, (unsigned)n_chan), dim3(256), 0, s, d_works, d_soft, tb, d_w32, max_cand);
}

// The ONE further launch of cwslg_fetch_ft4_decode_reports, behind harvest_launch on the same stream and blocks: a workgroup per record that emit
// may have written -- the grid is sized by `lim`; the count, min(out[0], lim), is read on the device and the workgroups beyond it leave -- the
// reports to d_rep[lim][4].  Nothing to launch for lim == 0.  The library and tests/ft4_report_kernel_check.hip both launch through here.
inline void ft4_report_launch(hipStream_t s, const Ft4ReportDesc *d_rdesc, const unsigned *d_offsets, const unsigned *d_out, const uint32_t *d_enc,
                              unsigned *d_rep, const Ft4Tables &tb, const float2 *d_w32, int n_chan, int lim)
{
    if (lim <= 0) return;
    Ft4ReportArgs ra{};
    ra.n_chan = n_chan; ra.max_out = lim;
    ra.rdesc = d_rdesc; ra.offsets = d_offsets; ra.out = d_out; ra.enc = d_enc; ra.rep = d_rep;
    hipLaunchKernelGGL(ft4_report_kernel, dim3((unsigned)lim), dim3(256), 0, s, tb, d_w32, ra);
}

} // namespace cwslg
