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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ft4sync_kernels.hpp"
#include "ft8soft_kernels.hpp"

namespace cwslg {

constexpr int FT4S_NN = 103, FT4S_NBM = 206, FT4S_NBIT = 174;
struct Ft4SoftRec { float llr[3][FT4S_NBIT]; float sigma[3]; int32_t nsync, nqual, pad_; };       // = cwslg_ft4_soft
static_assert(sizeof(Ft4SoftRec) == 2112, "cwslg_ft4_soft is 2112 bytes");

// icos4 (0132 1023 2310 3201), two bits per entry [4 b + s]; the four hard-decision patterns of nqual, one bit per entry [8 block + j]
constexpr unsigned ft4s_pack2(const int (&v)[16]) { unsigned c = 0; for (int i = 0; i < 16; ++i) c |= (unsigned)v[i] << (2 * i); return c; }
constexpr unsigned ft4s_pack1(const int (&v)[32]) { unsigned c = 0; for (int i = 0; i < 32; ++i) c |= (unsigned)v[i] << i; return c; }
constexpr int FT4S_ICOS4_V[16] = {0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1};
constexpr int FT4S_QUAL_V[32] = {0, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1};
constexpr unsigned FT4S_ICOS4 = ft4s_pack2(FT4S_ICOS4_V), FT4S_QUAL = ft4s_pack1(FT4S_QUAL_V);

__device__ __forceinline__ float ft4s_mag(float2 z) { return sqrtf(__builtin_fmaf(z.x, z.x, z.y * z.y)); }
__device__ __forceinline__ float2 ft4s_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ int ft4s_gray(int v) { return v ^ (v >> 1); }                           // graymap 0,1,3,2

__global__ __launch_bounds__(256) void ft4_softbits_kernel(const Ft4Work *__restrict__ works, Ft4SoftRec *const *__restrict__ soft,
                                                           Ft4Tables tb, const float2 *__restrict__ w32, int max_cand)
{
    F4_BASE_LDS(L);
    __shared__ float2 s_cs[FT4S_NN][4];
    __shared__ __attribute__((aligned(16))) float s_mag[FT4S_NN][4];
    __shared__ __attribute__((aligned(16))) float s_bm[3][256];            // the three metric sets, padded with +0
    __shared__ float2 s_w32[32];
    const Ft4Work *w = works + blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = blockIdx.x, cand = slot / 3, r = slot - 3 * cand;
    int ncand = *as_global(w->ncand);
    if (ncand > max_cand) ncand = max_cand;
    if (cand >= ncand) return;                      // workgroup-uniform, both
    if (r >= as_global(w->nrec)[cand]) return;
    const CWSLG_GLOBAL Ft4Rec *rec = as_global(w->rec) + slot;
    const float f1 = rec->f1_hz;
    const int ibest = rec->ibest;
    if (tid < 32) s_w32[tid] = w32[tid];
    for (int e = tid; e < 3 * 256; e += 256) (&s_bm[0][0])[e] = 0.0f;
    f4_baseband(L, w, tb, f1, tid);                  // (its barriers also publish s_w32 and the padding)
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

} // namespace cwslg
