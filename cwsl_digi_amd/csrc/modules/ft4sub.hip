// ft4sub.hip -- the FT4 subtractor's two kernels, built into a code object of their own (lib/cwslgpu_ft4sub.hsaco) and launched by
// the library through hipModuleLaunchKernel (ft8sub_host.inc).  The contract is the header's (include/cwsl_gpu.h, "FT4 signal subtraction");
// tests/ft4_subtract_ref.py restates it in numpy, bit for bit: this file is built -ffp-contract=off, every float operation below is one un-fused
// float32 operation in the order the header gives, and the waveform's phase is uint32 arithmetic on the committed tables.
//   ft4_sub_fit_kernel    grid (min(n_total, max_out)): one 256-thread workgroup per emitted decode -> its device record (start, increment,
//                         per-symbol phase bases, tones, amplitude track) and its 28-byte cwslg_subtract_report
//   ft4_sub_apply_kernel  grid (71 time tiles, channels): residual = frame - the fitted waveforms of the channel's decodes, in emission order
// Both read the harvest's output block (head, 10-dword records, per-channel offsets) as ft4_report_kernel does.  The FT8 module's form
// (ft8sub.hip) with FT4's geometry: 18-sample blocks, so a thread keeps 36 waveform values where FT8 keeps 120, and 70 KB of LDS where FT8
// needs 122 KB.
// One step FT8's fit does not have (4a of the header): the first track's mean phase turn per block corrects the increment, and the block sums and
// the track are made once more -- the symbol metric of the two searches is too flat over a 48 ms symbol to settle the frequency to a grid step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../ft4sub_layout.hpp"
#include "../ft4_tone_device.hpp"
#define FT4SUB_TABLE __device__ const
#include "ft4sub_tables.inc"

using namespace cwslg;

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));

constexpr int SUB_WIN_F4 = (3 + F4SUB_NT * F4SUB_BLK + 2 * F4SUB_TAU_MAX + 3) / 4;          // 1180 aligned float4 of a tile's window
constexpr int SUB_WIN_WORDS = 4 * SUB_WIN_F4 + (4 * SUB_WIN_F4) / F4SUB_BLK + 1;          // one pad word per 18: lanes 19 words apart
constexpr int SUB_NTILES = (F4SUB_NBLK + F4SUB_NT - 1) / F4SUB_NT;                          // 13 tiles of 256 blocks (8 symbols)
constexpr int SUB_NP = (F4SUB_NTAU > F4SUB_NK ? F4SUB_NTAU : F4SUB_NK) * F4SUB_NSYM;        // time search: [55][103]; frequency search: [53][103]
// the last word a thread reads of its window: block 255, alignment slack 3, the latest offset, the block's last sample
static_assert(F4SUB_BLK * (F4SUB_NT - 1) + 3 + 2 * F4SUB_TAU_MAX + F4SUB_BLK - 1 < 4 * SUB_WIN_F4, "the tile's window covers every offset");

// phase (2^-32 turns) of sample v of a symbol whose first sample has phase `base`: the prefix of the per-sample increments
// inc + tp P[2][v'] + tc P[1][v'] + tn P[0][v'], v' < v (tp, tc, tn: tones of the preceding, this and the following symbol)
__device__ __forceinline__ unsigned sub_phase(unsigned base, unsigned inc, int v, unsigned tp, unsigned tc, unsigned tn)
{
    return base + (unsigned)v * inc + tp * FT4SUB_CP[2 * F4SUB_NSPS + v] + tc * FT4SUB_CP[F4SUB_NSPS + v] + tn * FT4SUB_CP[v];
}

// cos of 2 pi idx / 4096 from the quarter table: C[r], -C[1024 - r], -C[r], C[1024 - r] in the four quarters (r = idx mod 1024)
__device__ __forceinline__ float sub_cos(unsigned idx)
{
    const unsigned q = idx >> 10 & 3u, r = idx & 1023u;
    const float v = FT4SUB_COSQ[q & 1u ? 1024u - r : r];
    return q == 1u || q == 2u ? -v : v;
}

// cos, sin of a phase: the table index is its top 12 bits rounded to nearest; the sine is the cosine a quarter turn earlier
__device__ __forceinline__ v2f sub_cs(unsigned ph)
{
    const unsigned idx = (ph + 0x80000u) >> 20;
    return v2f{sub_cos(idx), sub_cos((idx - 1024u) & 4095u)};
}

__device__ __forceinline__ float sub_halve32(float a)
{
#pragma unroll
    for (int h = 16; h >= 1; h >>= 1) a = a + __shfl_down(a, h, 32);
    return a;
}

// samples of block b of a signal starting at `start` that lie inside the frame
__device__ __forceinline__ int sub_cnt(int start, int b)
{
    const int lo = start + F4SUB_BLK * b;
    return max(0, min(lo + F4SUB_BLK, F4SUB_N) - max(lo, 0));
}

// One tile (256 blocks = 8 symbols) of the signal against the frame at the time offsets it_lo .. it_hi - 1: the window is loaded ONCE with aligned
// 16-byte loads (+0 outside the frame), the thread's 18 waveform samples are made ONCE and kept in registers.  STORE: the block sums to s_blk;
// otherwise |symbol sum|^2 to s_P[it][symbol].
template <bool STORE>
__device__ __forceinline__ void sub_tile_pass(const float *__restrict__ frame, int n_valid, int i0, int c, unsigned inc, int it_lo, int it_hi, float *s_win, float *s_P,
                                              v2f *s_blk, const unsigned *s_tbase, const unsigned *s_tone)
{
    const int tid = threadIdx.x;
    const int w0 = i0 - F4SUB_TAU_MAX + c * (F4SUB_NT * F4SUB_BLK);
    const int a0 = w0 & ~3, r = w0 - a0;
    __syncthreads();                                        // (whoever read s_win before is done)
    for (int q4 = tid; q4 < SUB_WIN_F4; q4 += F4SUB_NT) {
        const int t = a0 + 4 * q4;
        const bool ok = t >= 0 && t + 3 < F4SUB_N;          // (t and the frame's length are multiples of 4: all four samples or none)
        const v4f x = ok ? *reinterpret_cast<const v4f *>(frame + t) : v4f{0.0f, 0.0f, 0.0f, 0.0f};
        const int q = 4 * q4;
        s_win[q + q / F4SUB_BLK] = t < n_valid ? x.x : 0.0f;
        s_win[q + 1 + (q + 1) / F4SUB_BLK] = t + 1 < n_valid ? x.y : 0.0f;
        s_win[q + 2 + (q + 2) / F4SUB_BLK] = t + 2 < n_valid ? x.z : 0.0f;
        s_win[q + 3 + (q + 3) / F4SUB_BLK] = t + 3 < n_valid ? x.w : 0.0f;
    }
    __syncthreads();
    const int b = F4SUB_NT * c + tid;
    const bool valid = b < F4SUB_NBLK;                      // (uniform over each group of 32 lanes: a symbol has 32 blocks)
    const int bb = valid ? b : 0;
    const int n = bb >> 5, vb = F4SUB_BLK * (bb & 31);
    const unsigned tp = s_tone[n > 0 ? n - 1 : 0], tc = s_tone[n], tn = s_tone[n < F4SUB_NSYM - 1 ? n + 1 : n];
    const unsigned base = s_tbase[n] + (unsigned)(n * F4SUB_NSPS) * inc;
    float wc[F4SUB_BLK], ws[F4SUB_BLK];
#pragma unroll
    for (int s = 0; s < F4SUB_BLK; ++s) {
        const v2f cs = sub_cs(sub_phase(base, inc, vb + s, tp, tc, tn));
        wc[s] = cs.x; ws[s] = cs.y;
    }
    const float *mine = s_win + (F4SUB_BLK + 1) * tid;
#pragma unroll 1
    for (int it = it_lo; it < it_hi; ++it) {
        // sample s of the block sits at window word m = m0 + s of this thread's run, padded word m + m / 18: at most one pad inside the block
        const int m0 = r + F4SUB_TAU_STEP * it, d0 = m0 / F4SUB_BLK, r0 = m0 - F4SUB_BLK * d0;
        const float *at = mine + m0 + d0;
        float re = 0.0f, im = 0.0f;
#pragma unroll
        for (int s = 0; s < F4SUB_BLK; ++s) {
            const float x = at[s + (r0 + s >= F4SUB_BLK ? 1 : 0)];
            re = re + x * wc[s];
            im = im - x * ws[s];
        }
        if (STORE) {
            if (valid) s_blk[b] = v2f{re, im};
        } else {
            const float sr = sub_halve32(re), si = sub_halve32(im);
            if (valid && (tid & 31) == 0) s_P[it * F4SUB_NSYM + n] = sr * sr + si * si;
        }
    }
}

// first maximum of s_M[0 .. count - 1] (thread 0), after every thread i < count has summed its row of s_P over the 103 symbols in ascending order
__device__ __forceinline__ int sub_pick(const float *s_P, float *s_M, int *s_arg, int count)
{
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid < count) {
        float m = 0.0f;
        for (int n = 0; n < F4SUB_NSYM; ++n) m = m + s_P[tid * F4SUB_NSYM + n];
        s_M[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
        float best = s_M[0];
        int arg = 0;
        for (int i = 1; i < count; ++i) {
            const float v = s_M[i];
            if (v > best) { best = v; arg = i; }
        }
        *s_arg = arg;
    }
    __syncthreads();
    return *s_arg;
}

// The frequency search at block rate: for k = -26..26 the block sums in s_blk, turned back by k DINC (18 b + 9), summed per symbol by a group of
// 32 lanes and squared into s_P[k][symbol]; -> the index 0..52 of the first maximum.
__device__ __forceinline__ int sub_freq_search(const v2f *s_blk, float *s_P, float *s_M, int *s_arg)
{
    const int tid = threadIdx.x;
    __syncthreads();
    for (int q0 = 0; q0 < F4SUB_NK * F4SUB_NSYM; q0 += F4SUB_NT / 32) {
        const int q = q0 + (tid >> 5);
        const bool valid = q < F4SUB_NK * F4SUB_NSYM;
        const int qq = valid ? q : 0;
        const int k = qq / F4SUB_NSYM - F4SUB_KF, n = qq % F4SUB_NSYM, b = F4SUB_BPS * n + (tid & 31);
        const v2f B = s_blk[b];
        const v2f cs = sub_cs((unsigned)(k * F4SUB_DINC) * (unsigned)(F4SUB_BLK * b + F4SUB_BLK / 2));
        const float sr = sub_halve32(B.x * cs.x + B.y * cs.y), si = sub_halve32(B.y * cs.x - B.x * cs.y);
        if (valid && (tid & 31) == 0) s_P[qq] = sr * sr + si * si;
    }
    return sub_pick(s_P, s_M, s_arg, F4SUB_NK);
}

// The amplitude track of the block sums in s_blk -> the record's track points, and the three figures, reduced into s_red[0..2][0] (valid behind the
// call for thread 0): Hann window over the blocks b - 48 .. b + 48 of the signal, ascending; normalised by the samples under it.
__device__ __forceinline__ void sub_track_figures(const v2f *s_blk, int start, unsigned *my, float (*s_red)[F4SUB_NT])
{
    const int tid = threadIdx.x;
    float e_rem = 0.0f, e_bef = 0.0f, e_aft = 0.0f;
    for (int b = tid; b < F4SUB_NBLK; b += F4SUB_NT) {
        float nre = 0.0f, nim = 0.0f, den = 0.0f;
        for (int j = 0; j <= 2 * F4SUB_HW; ++j) {
            const int bj = b - F4SUB_HW + j;
            const bool in = bj >= 0 && bj < F4SUB_NBLK;
            const v2f B = s_blk[in ? bj : 0];
            const float w = FT4SUB_WIN[j];
            nre = nre + w * (in ? B.x : 0.0f);
            nim = nim + w * (in ? B.y : 0.0f);
            den = den + w * (in ? (float)sub_cnt(start, bj) : 0.0f);
        }
        const bool ok = den > 0.0f;
        const float ar = ok ? nre / den : 0.0f, ai = ok ? nim / den : 0.0f;
        *reinterpret_cast<v2f *>(my + F4SUB_REC_TRACK + 2 * b) = v2f{ar, ai};
        // the figures, at block rate: A cos carries 2 |a|^2 per sample
        const v2f B = s_blk[b];
        const float cnt = (float)sub_cnt(start, b);
        const bool okc = cnt > 0.0f;
        const float dr = B.x - cnt * ar, di = B.y - cnt * ai;
        e_rem = e_rem + 2.0f * (ar * ar + ai * ai) * cnt;
        e_bef = e_bef + (okc ? 2.0f * (B.x * B.x + B.y * B.y) / cnt : 0.0f);
        e_aft = e_aft + (okc ? 2.0f * (dr * dr + di * di) / cnt : 0.0f);
    }
    __syncthreads();                                        // (whoever read s_red before is done)
    s_red[0][tid] = e_rem; s_red[1][tid] = e_bef; s_red[2][tid] = e_aft;
    for (int h = F4SUB_NT / 2; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            s_red[0][tid] = s_red[0][tid] + s_red[0][tid + h];
            s_red[1][tid] = s_red[1][tid] + s_red[1][tid + h];
            s_red[2][tid] = s_red[2][tid] + s_red[2][tid + h];
        }
    }
}

extern "C" __global__ __launch_bounds__(F4SUB_NT) void ft4_sub_fit_kernel(const SubDesc *__restrict__ desc, const unsigned *__restrict__ offsets,
                                                                         const unsigned *__restrict__ out, const uint32_t *__restrict__ enc,
                                                                         unsigned *__restrict__ recs, unsigned *__restrict__ rep, int n_chan, int max_out)
{
    __shared__ __attribute__((aligned(16))) float s_win[SUB_WIN_WORDS];
    __shared__ float s_P[SUB_NP];
    __shared__ __attribute__((aligned(8))) v2f s_blk[F4SUB_NBLK];
    __shared__ float s_red[3][F4SUB_NT];
    __shared__ float s_M[F4SUB_NTAU > F4SUB_NK ? F4SUB_NTAU : F4SUB_NK];
    __shared__ unsigned s_tbase[F4SUB_NSYM], s_tone[F4SUB_NSYM];
    __shared__ int s_arg;
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned n_emit = min(out[0], (unsigned)max(max_out, 0));
    const unsigned p = blockIdx.x;
    if (p >= n_emit) return;                                // workgroup-uniform
    // the record's channel: the last c with offsets[c] <= p
    int lo_c = 0, hi_c = n_chan;
    while (hi_c - lo_c > 1) {
        const int mid = (lo_c + hi_c) >> 1;
        if (offsets[mid] <= p) lo_c = mid; else hi_c = mid;
    }
    const float *frame = desc[lo_c].frame;
    const int n_valid = desc[lo_c].n_valid;
    const unsigned *rec = out + F4SUB_DEC_HEAD_WORDS + (size_t)p * F4SUB_DEC_WORDS;
    const unsigned k0 = rec[2], k1 = rec[3], k2 = rec[4];
    const float freq = __uint_as_float(rec[5]), dt = __uint_as_float(rec[6]);     // the record's f1_hz and dt_s

    // ---- the tones: wave 0 re-encodes the word as ft4_report_kernel does (lane l owns encoder rows l and l + 64; XOR across the lanes) ----
    if (tid < 64) {
        const int row_b = lane + 64 < F4SUB_ENC_ROWS ? lane + 64 : lane;
        const v2u *ea = reinterpret_cast<const v2u *>(enc + (size_t)lane * F4SUB_ENC_WORDS);
        const v2u *eb = reinterpret_cast<const v2u *>(enc + (size_t)row_b * F4SUB_ENC_WORDS);
        const v2u a0 = ea[0], a1 = ea[1], a2 = ea[2], b0 = eb[0], b1 = eb[1], b2 = eb[2];
        const unsigned wa = lane < 32 ? k0 : k1;
        const unsigned bit_a = wa >> (8 * ((lane >> 3) & 3) + 7 - (lane & 7)) & 1u;
        const unsigned bit_b = lane + 64 < F4SUB_ENC_ROWS ? k2 >> (8 * ((lane >> 3) & 3) + 7 - (lane & 7)) & 1u : 0u;
        const unsigned ma = 0u - bit_a, mb = 0u - bit_b;
        unsigned c0 = (a0.x & ma) ^ (b0.x & mb), c1 = (a0.y & ma) ^ (b0.y & mb), c2 = (a1.x & ma) ^ (b1.x & mb);
        unsigned c3 = (a1.y & ma) ^ (b1.y & mb), c4 = (a2.x & ma) ^ (b2.x & mb), c5 = (a2.y & ma) ^ (b2.y & mb);
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
            c0 ^= (unsigned)__shfl_xor((int)c0, h, 64); c1 ^= (unsigned)__shfl_xor((int)c1, h, 64); c2 ^= (unsigned)__shfl_xor((int)c2, h, 64);
            c3 ^= (unsigned)__shfl_xor((int)c3, h, 64); c4 ^= (unsigned)__shfl_xor((int)c4, h, 64); c5 ^= (unsigned)__shfl_xor((int)c5, h, 64);
        }
        bool costas;
        s_tone[lane] = (unsigned)ft4r_tone(c0, c1, c2, c3, c4, c5, lane, &costas);
        if (lane + 64 < F4SUB_NSYM) s_tone[lane + 64] = (unsigned)ft4r_tone(c0, c1, c2, c3, c4, c5, lane + 64, &costas);
    }
    __syncthreads();
    // what the tones of the symbols before add to the phase (the frequency's share, n 576 inc, is added where the increment is known)
    if (tid == 0) {
        unsigned acc = 0u;
        for (int n = 0; n < F4SUB_NSYM; ++n) {
            s_tbase[n] = acc;
            const unsigned tp = s_tone[n > 0 ? n - 1 : 0], tc = s_tone[n], tn = s_tone[n < F4SUB_NSYM - 1 ? n + 1 : n];
            acc += tp * FT4SUB_CPT[2] + tc * FT4SUB_CPT[1] + tn * FT4SUB_CPT[0];
        }
    }
    const unsigned inc0 = (unsigned)(long long)rint((double)freq * (4294967296.0 / 12000.0));
    float fs = rintf((dt + 0.5f) * 12000.0f);
    if (!(fs >= -400000.0f)) fs = -400000.0f;
    if (fs > 400000.0f) fs = 400000.0f;
    const int i0 = (int)fs - F4SUB_CAND_OFFSET;

    // ---- frequency search at block rate: the block sums at the record's time and frequency, turned back by k DINC (18 b + 9) ----
    constexpr int IT0 = F4SUB_TAU_MAX / F4SUB_TAU_STEP;
    for (int c = 0; c < SUB_NTILES; ++c) sub_tile_pass<true>(frame, n_valid, i0, c, inc0, IT0, IT0 + 1, s_win, s_P, s_blk, s_tbase, s_tone);
    const int ik = sub_freq_search(s_blk, s_P, s_M, &s_arg);
    const unsigned inc1 = inc0 + (unsigned)((ik - F4SUB_KF) * F4SUB_DINC);

    // ---- time search at the refined frequency, at sample rate ----
    for (int c = 0; c < SUB_NTILES; ++c) sub_tile_pass<false>(frame, n_valid, i0, c, inc1, 0, F4SUB_NTAU, s_win, s_P, s_blk, s_tbase, s_tone);
    const int it = sub_pick(s_P, s_M, &s_arg, F4SUB_NTAU);
    const int start = i0 - F4SUB_TAU_MAX + F4SUB_TAU_STEP * it;

    // ---- the frequency search once more, now that the symbols are aligned, and the block sums at the winner ----
    for (int c = 0; c < SUB_NTILES; ++c) sub_tile_pass<true>(frame, n_valid, i0, c, inc1, it, it + 1, s_win, s_P, s_blk, s_tbase, s_tone);
    const int ik2 = sub_freq_search(s_blk, s_P, s_M, &s_arg);
    const unsigned inc2 = inc1 + (unsigned)((ik2 - F4SUB_KF) * F4SUB_DINC);
    for (int c = 0; c < SUB_NTILES; ++c) sub_tile_pass<true>(frame, n_valid, i0, c, inc2, it, it + 1, s_win, s_P, s_blk, s_tbase, s_tone);
    __syncthreads();

    // ---- amplitude track, the track's phase slope -> the increment's last correction, the block sums and the track once more, the figures ----
    unsigned *my = recs + (size_t)p * F4SUB_REC_WORDS;
    sub_track_figures(s_blk, start, my, s_red);             // (the figures of this first track are not used)
    __syncthreads();                                        // (the track, written to the record by this workgroup, is read back below)
    {
        const v2f *track = reinterpret_cast<const v2f *>(my + F4SUB_REC_TRACK);
        float cr = 0.0f, ci = 0.0f;
        for (int b = tid; b < F4SUB_NBLK; b += F4SUB_NT) {
            const bool in = b < F4SUB_NBLK - 1;
            const v2f A0 = track[b], A1 = track[in ? b + 1 : b];
            cr = cr + (in ? A1.x * A0.x + A1.y * A0.y : 0.0f);
            ci = ci + (in ? A1.y * A0.x - A1.x * A0.y : 0.0f);
        }
        __syncthreads();                                    // (the first track's reduction in s_red is done with)
        s_red[0][tid] = ci; s_red[1][tid] = cr;
        for (int h = F4SUB_NT / 2; h >= 1; h >>= 1) {
            __syncthreads();
            if (tid < h) {
                s_red[0][tid] = s_red[0][tid] + s_red[0][tid + h];
                s_red[1][tid] = s_red[1][tid] + s_red[1][tid + h];
            }
        }
        if (tid == 0) {
            const float num = s_red[0][0], den = s_red[1][0];
            int dinc = 0;
            if (den > 0.0f) {
                double d = (double)(num / den) * F4SUB_SLOPE_K;
                if (!(d >= -2.0 * F4SUB_DINC)) d = -2.0 * F4SUB_DINC;
                if (d > 2.0 * F4SUB_DINC) d = 2.0 * F4SUB_DINC;
                dinc = (int)rint(d);
            }
            s_arg = dinc;
        }
        __syncthreads();
    }
    const unsigned inc = inc2 + (unsigned)s_arg;
    for (int c = 0; c < SUB_NTILES; ++c) sub_tile_pass<true>(frame, n_valid, i0, c, inc, it, it + 1, s_win, s_P, s_blk, s_tbase, s_tone);
    __syncthreads();
    sub_track_figures(s_blk, start, my, s_red);

    // ---- the record's head and the report ----
    if (tid < F4SUB_NSYM) my[F4SUB_REC_BASE + tid] = s_tbase[tid] + (unsigned)(tid * F4SUB_NSPS) * inc;
    if (tid < (F4SUB_NSYM + 3) / 4) {
        unsigned w = 0u;
        for (int e = 0; e < 4; ++e) if (4 * tid + e < F4SUB_NSYM) w |= s_tone[4 * tid + e] << (8 * e);
        my[F4SUB_REC_TONES + tid] = w;
    }
    if (tid == 0) {
        my[F4SUB_REC_START] = (unsigned)start;
        my[F4SUB_REC_INC] = inc;
        unsigned *o = rep + (size_t)p * F4SUB_REP_WORDS;
        o[0] = __float_as_uint((float)((double)inc * (12000.0 / 4294967296.0)));
        o[1] = __float_as_uint((float)(start - 6000) / 12000.0f);
        o[2] = __float_as_uint(s_red[0][0]);
        o[3] = __float_as_uint(s_red[1][0]);
        o[4] = __float_as_uint(s_red[2][0]);
        o[5] = (unsigned)max(0, min(start + F4SUB_NW, F4SUB_N) - max(start, 0));
        o[6] = ((unsigned)(ik - F4SUB_KF + ik2 - F4SUB_KF) & 0xffffu) | (unsigned)(it - F4SUB_TAU_MAX / F4SUB_TAU_STEP) << 16;
    }
}

// One workgroup per (time tile of 1024 samples, channel); a thread owns four consecutive samples.  The channel's emitted decodes are walked in
// order; each one's waveform is regenerated from the record's per-symbol phase base (no tile replays a signal from its start) and its track is
// interpolated linearly between block centres.  No atomics: a sample is read, reduced in registers and written by one thread.
extern "C" __global__ __launch_bounds__(F4SUB_NT) void ft4_sub_apply_kernel(const SubDesc *__restrict__ desc, const unsigned *__restrict__ offsets,
                                                                           const unsigned *__restrict__ out, const unsigned *__restrict__ recs,
                                                                           int n_chan, int max_out)
{
    const int ch = blockIdx.y, t0 = F4SUB_TILE * (int)blockIdx.x + 4 * (int)threadIdx.x;
    if (t0 >= F4SUB_N) return;                              // (the 71st tile's tail; t0 + 3 < 72576 otherwise)
    const unsigned n_total = out[0], n_emit = min(n_total, (unsigned)max(max_out, 0));
    const unsigned p_lo = min(offsets[ch], n_emit), p_hi = min(ch + 1 < n_chan ? offsets[ch + 1] : n_total, n_emit);
    const int n_valid = desc[ch].n_valid;
    v4f x = *reinterpret_cast<const v4f *>(desc[ch].frame + t0);
    if (t0 >= n_valid) x.x = 0.0f;
    if (t0 + 1 >= n_valid) x.y = 0.0f;
    if (t0 + 2 >= n_valid) x.z = 0.0f;
    if (t0 + 3 >= n_valid) x.w = 0.0f;
    for (unsigned p = p_lo; p < p_hi; ++p) {
        const unsigned *rec = recs + (size_t)p * F4SUB_REC_WORDS;
        const int start = (int)rec[F4SUB_REC_START];
        const unsigned inc = rec[F4SUB_REC_INC];
        const int u0 = t0 - start;
        if (u0 + 3 < 0 || u0 >= F4SUB_NW) continue;
        const v2f *track = reinterpret_cast<const v2f *>(rec + F4SUB_REC_TRACK);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int u = u0 + e;
            if (u < 0 || u >= F4SUB_NW) continue;
            const int n = u / F4SUB_NSPS, v = u - F4SUB_NSPS * n;
            const int np = n > 0 ? n - 1 : 0, nn = n < F4SUB_NSYM - 1 ? n + 1 : n;
            const unsigned tp = rec[F4SUB_REC_TONES + (np >> 2)] >> (8 * (np & 3)) & 0xffu;
            const unsigned tc = rec[F4SUB_REC_TONES + (n >> 2)] >> (8 * (n & 3)) & 0xffu;
            const unsigned tn = rec[F4SUB_REC_TONES + (nn >> 2)] >> (8 * (nn & 3)) & 0xffu;
            const v2f cs = sub_cs(sub_phase(rec[F4SUB_REC_BASE + n], inc, v, tp, tc, tn));
            // the track between block centres (sample 18 b + 8.5): in half samples, pp = 36 b at a centre
            const int pp = 2 * u - (F4SUB_BLK - 1);
            const int b0 = pp < 0 ? 0 : min(pp / (2 * F4SUB_BLK), F4SUB_NBLK - 2);
            const int m = pp - 2 * F4SUB_BLK * b0;
            const float g = (float)m * (1.0f / 36.0f);
            const v2f A0 = track[b0], A1 = track[b0 + 1];
            const float ar = m >= 2 * F4SUB_BLK ? A1.x : pp < 0 ? A0.x : A0.x + g * (A1.x - A0.x);
            const float ai = m >= 2 * F4SUB_BLK ? A1.y : pp < 0 ? A0.y : A0.y + g * (A1.y - A0.y);
            const float y = ar * cs.x - ai * cs.y;
            x[e] = x[e] - 2.0f * y;
        }
    }
    *reinterpret_cast<v4f *>(desc[ch].resid + t0) = x;
}
