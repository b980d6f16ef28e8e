// harvest_kernels.hpp -- cwslg_fetch_decodes: the decoded words of a whole FT8 / FT4 slot-clock group, chosen (BP before OSD, FT4: the smallest
// metric set) and de-duplicated per channel on the device, so that one copy brings "the decodes of this slot" to the host instead of one fetch
// per channel and stage.  The contract is the header's (include/cwsl_gpu.h, cwslg_decode); tests/decodes_ref.py restates it in numpy.
//
// This is a FETCH, not a stage: the kernel reads the records the chains have left on the device (d_cand / d_rec + d_nrec, the decode and OSD
// record arrays) and writes only its own blocks.  ONE symbol, decode_harvest_kernel, launched at most three times per call with a mode argument:
//   HARVEST_COUNT  grid (channels): decodes of the channel -> counts[ch]
//   HARVEST_SCAN   grid (1): exclusive prefix of counts -> offsets[], the total -> out[0]; 256 channels per pass with a running carry
//   HARVEST_EMIT   grid (channels): the same walk again, decode number p of the channel -> record offsets[ch] + p, if that is below max_out
// Count and emit, one 256-thread workgroup per channel: the SLOTS of the channel (FT8: list entry q = slot q; FT4: the slot layout [cand][3], of
// which slot 3 k + r exists iff r < nrec[k]) are walked 256 at a time; two ballots per pass give every existing slot its ENTRY (its index as
// cwslg_fetch_ft4_sync compacts the records -- the workgroup prefix over nrec) and every slot with a word its place in an LDS list that is
// thereby in ascending entry order: 12-byte key, rank (by_osd, nharderr, entry) in one word, (slot, set) in another.  Every listed word then
// looks for equal keys -- counting them (ndup) and giving way to a better rank -- and a third ballot pass numbers the survivors.  Integer work
// only; every global address goes through the global address space; no register array is indexed.
//
// cwslg_fetch_decode_reports adds a kernel of its own, launched ONCE behind the three above (FT8 only):
//   decode_report_kernel  grid (ceil(min(n_total, max_out) / 4)): one WAVE per emitted record, no workgroup barrier -> the 16-byte cwslg_decode_report
// of record p: the word is re-encoded (91 bits -> 174 -> 79 tones) with the systematic encoder of the loaded code and the channel's symbol-spectra
// plane is read at the candidate's grid position, with ft8_softbits_kernel's addressing.  The arithmetic is the header's (cwslg_decode_report),
// restated in tests/decode_reports_ref.py, bit for bit: this translation unit is built -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sync_kernels.hpp"
#include "ft8soft_kernels.hpp"
#include "ft8_tone_device.hpp"

namespace cwslg {

constexpr int HARVEST_COUNT = 0, HARVEST_SCAN = 1, HARVEST_EMIT = 2;
constexpr int HARVEST_NT = 256;
constexpr int HARVEST_MAXSLOTS = 3 * SYNC_MAXCAND_CAP;                  // FT4: three record slots per candidate
constexpr int HARVEST_REC_WORDS = 10;                                   // cwslg_decode is 40 bytes
constexpr int HARVEST_HEAD_WORDS = 4;                                   // out[0] = n_total; the records follow 16 bytes in
constexpr int REPORT_WORDS = 4;                                         // cwslg_decode_report is 16 bytes
constexpr int REPORT_ENC_ROWS = 91, REPORT_ENC_WORDS = 6;               // the encoder: OsdGen (ldpc_host.hpp), 91 rows of 6 dwords

// One channel that takes part, built by the host under the context mutex.
struct alignas(16) HarvestDesc {
    const int *cnt;          // the list's count
    const void *list;        // FT8: Cand[cap]; FT4: Ft4Rec[cap][3]
    const int *nrec;         // FT4: records per candidate, [cap]; FT8: null
    const void *msg;         // FT8: Ft8MsgRec[cap]; FT4: Ft4MsgRec[cap][3]
    const void *osd;         // FT8: OsdRec[cap]; FT4: Ft4OsdRec[cap][3]; null: the OSD records are not of this epoch
    int cap;                 // the list limit the arrays were sized for
    int ch_id;
};
static_assert(sizeof(HarvestDesc) == 48, "descriptor layout");

// What decode_report_kernel needs of the same channel, in an array of its own beside the HarvestDesc array (same index).
struct alignas(16) ReportDesc {
    const float *spectra;    // the channel's symbol-spectra plane, [372][nbins]
    const void *list;        // Cand[cap]
    int nbins;               // row pitch of the plane
    int pad_[3];
};
static_assert(sizeof(ReportDesc) == 32, "descriptor layout");
struct ReportRec { float snr_db, xsig, xnoise; int16_t nsync, nsymerr; };       // = cwslg_decode_report
static_assert(sizeof(ReportRec) == REPORT_WORDS * sizeof(unsigned), "cwslg_decode_report is 16 bytes");

// Ordered compaction over the workgroup: the number of flagged threads before this one (threads in ascending tid); *total = all of them.
// s_w: 4 words of LDS; two barriers.
__device__ __forceinline__ unsigned harvest_place(bool flag, unsigned *s_w, unsigned *total)
{
    const unsigned long long b = __ballot(flag);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned before = (unsigned)__popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wave] = (unsigned)__popcll(b);
    __syncthreads();
    const unsigned w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
    __syncthreads();
    *total = w0 + w1 + w2 + w3;
    return before + (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
}

// ---- decode_report_kernel ------------------------------------------------------------------------------------------------------------------------------
// (report_pick6, report_tone: ft8_tone_device.hpp)

// One symbol of the wave's power image: first maximum of the magnitudes at the encoded tone?  the power at the tone and at (tone + 4) mod 7
__device__ __forceinline__ bool report_symbol(const float *pw, int n, int tone, float *sig, float *noi)
{
    const v4f lo = *reinterpret_cast<const v4f *>(pw + 8 * n), hi = *reinterpret_cast<const v4f *>(pw + 8 * n + 4);
    const float s0 = sqrtf(lo.x), s1 = sqrtf(lo.y), s2 = sqrtf(lo.z), s3 = sqrtf(lo.w), s4 = sqrtf(hi.x), s5 = sqrtf(hi.y), s6 = sqrtf(hi.z), s7 = sqrtf(hi.w);
    int km = 0;
    float vm = s0;
    if (s1 > vm) { vm = s1; km = 1; }
    if (s2 > vm) { vm = s2; km = 2; }
    if (s3 > vm) { vm = s3; km = 3; }
    if (s4 > vm) { vm = s4; km = 4; }
    if (s5 > vm) { vm = s5; km = 5; }
    if (s6 > vm) { vm = s6; km = 6; }
    if (s7 > vm) { vm = s7; km = 7; }
    const int u = tone + 4;
    *sig = pw[8 * n + tone];
    *noi = pw[8 * n + (u >= 7 ? u - 7 : u)];
    return km == tone;
}

// One wave per emitted record.  s_pw: the wave's [80][8] image of powers (2560 bytes of LDS, private to the wave).
__device__ __forceinline__ void harvest_report_wave(const ReportDesc *rdesc, const unsigned *offsets, const unsigned *out, const uint32_t *enc,
                                                    unsigned *rep, int n_chan, int max_out, float *s_pw)
{
    typedef unsigned v2u __attribute__((ext_vector_type(2)));
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const CWSLG_GLOBAL unsigned *g_out = as_global(out), *g_offsets = as_global(offsets);
    const unsigned n_emit = min((unsigned)__builtin_amdgcn_readfirstlane((int)g_out[0]), (unsigned)max(max_out, 0));
    const unsigned p = blockIdx.x * (unsigned)FT8S_WAVES + (unsigned)wv;
    if (p >= n_emit) return;                                    // wave-uniform
    // the record's channel: the last c with offsets[c] <= p (offsets[0] = 0; channels without decodes make equal offsets)
    int lo_c = 0, hi_c = n_chan;
    while (hi_c - lo_c > 1) {
        const int mid = (lo_c + hi_c) >> 1;
        const unsigned o = (unsigned)__builtin_amdgcn_readfirstlane((int)g_offsets[mid]);
        if (o <= p) lo_c = mid; else hi_c = mid;
    }
    const CWSLG_GLOBAL ReportDesc *rd = as_global(rdesc) + lo_c;
    const CWSLG_GLOBAL unsigned *rec = g_out + HARVEST_HEAD_WORDS + (size_t)p * HARVEST_REC_WORDS;
    const unsigned entry = rec[1] & 0xffffu, k0 = rec[2], k1 = rec[3], k2 = rec[4];
    const CWSLG_GLOBAL int *cd = as_global(reinterpret_cast<const int *>(rd->list)) + (size_t)entry * 5u;     // Cand: freq_bin, time_step, ...
    const int i = cd[0], j = cd[1], nbins = rd->nbins;
    const CWSLG_GLOBAL float *spec = as_global(rd->spectra);

    // ---- the plane: ft8_softbits_kernel's 20 passes of 4 symbols x 16 bins, all loads in flight before anything else waits ----
    const int sub = lane >> 4, c = lane & 15;
    const int bin = i + c;
    const bool col_ok = c < 15 && bin >= 0 && bin <= FT8_NH1 && bin < nbins;
    float pv[20];
#pragma unroll
    for (int ps = 0; ps < 20; ++ps) {
        const int n = 4 * ps + sub;
        const int m = j + 12 + 4 * n;                          // 1-based symbol step
        const bool ok = col_ok && n < FT8S_NSYM && m >= 1 && m <= FT8_NHSYM;
        // (an element outside the plane fetches element 0 and drops it: no load under a condition)
        const float v = spec[ok ? (size_t)(m - 1) * (size_t)nbins + (size_t)bin : (size_t)0];
        pv[ps] = ok ? v : 0.0f;
    }

    // ---- the codeword: lane l owns encoder rows l and l + 64 (rows 64..90 on lanes 0..26); XOR across the lanes ----
    const int row_b = lane + 64 < REPORT_ENC_ROWS ? lane + 64 : lane;  // (a lane without a second row loads its first again and drops it)
    const CWSLG_GLOBAL v2u *ea = reinterpret_cast<const CWSLG_GLOBAL v2u *>(as_global(enc) + (size_t)lane * REPORT_ENC_WORDS);
    const CWSLG_GLOBAL v2u *eb = reinterpret_cast<const CWSLG_GLOBAL v2u *>(as_global(enc) + (size_t)row_b * REPORT_ENC_WORDS);
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

    // ---- the image of powers, private to this wave ----
    if (!(c & 1) && c < 15) {
#pragma unroll
        for (int ps = 0; ps < 20; ++ps) s_pw[8 * (4 * ps + sub) + (c >> 1)] = pv[ps];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- lane l: symbol l, and symbol l + 64 where that is below 79 ----
    const bool two = lane + 64 < FT8S_NSYM;
    const int nb = two ? lane + 64 : lane;
    bool cos_a, cos_b;
    const int ta = report_tone(c0, c1, c2, c3, c4, c5, lane, &cos_a), tb = report_tone(c0, c1, c2, c3, c4, c5, nb, &cos_b);
    float sig_a, noi_a, sig_b, noi_b;
    const bool hit_a = report_symbol(s_pw, lane, ta, &sig_a, &noi_a), hit_b = report_symbol(s_pw, nb, tb, &sig_b, &noi_b);
    const int nsync = __popcll(__ballot(cos_a && hit_a)) + __popcll(__ballot(two && cos_b && hit_b));
    const int nsymerr = __popcll(__ballot(!cos_a && !hit_a)) + __popcll(__ballot(two && !cos_b && !hit_b));
    const float xsig = ft8s_tree64(two ? sig_a + sig_b : sig_a), xnoise = ft8s_tree64(two ? noi_a + noi_b : noi_a);
    if (lane == 0) {
        const float r = xnoise > 0.0f ? xsig / xnoise - 1.0f : 0.0f;
        const float x = fminf(r > 0.1f ? r : 0.001f, 3.4028234663852886e38f);      // (an infinite ratio reports as the largest float's)
        const float db = (float)(10.0 * long_log10_fixed((double)x) - 27.0);
        v4u o;
        o.x = __float_as_uint(fmaxf(db, -24.0f)); o.y = __float_as_uint(xsig); o.z = __float_as_uint(xnoise);
        o.w = (unsigned)nsync | (unsigned)nsymerr << 16;
        *reinterpret_cast<CWSLG_GLOBAL v4u *>(as_global_rw(rep) + (size_t)p * REPORT_WORDS) = o;
    }
}

__global__ __launch_bounds__(64 * FT8S_WAVES) void decode_report_kernel(const ReportDesc *__restrict__ rdesc, const unsigned *__restrict__ offsets,
                                                                        const unsigned *__restrict__ out, const uint32_t *__restrict__ enc,
                                                                        unsigned *__restrict__ rep, int n_chan, int max_out)
{
    __shared__ __attribute__((aligned(16))) float s_pw[FT8S_WAVES][(FT8S_NSYM + 1) * 8];
    harvest_report_wave(rdesc, offsets, out, enc, rep, n_chan, max_out, s_pw[threadIdx.x >> 6]);
}

__global__ __launch_bounds__(HARVEST_NT) void decode_harvest_kernel(const HarvestDesc *__restrict__ desc, unsigned *__restrict__ counts,
                                                                    unsigned *__restrict__ offsets, unsigned *__restrict__ out, int n_chan, int max_out,
                                                                    int ft4, int mode)
{
    __shared__ __attribute__((aligned(16))) unsigned s_key[3][HARVEST_MAXSLOTS];      // the word: bits[12] as three little-endian words
    __shared__ unsigned s_rank[HARVEST_MAXSLOTS];        // by_osd << 28 | nharderr << 16 | entry: smaller is better, never equal
    __shared__ unsigned s_info[HARVEST_MAXSLOTS];        // slot | set << 12; after the de-duplication: | ndup << 16 | survivor << 15
    __shared__ unsigned s_w[4];
    const unsigned tid = threadIdx.x;
    CWSLG_GLOBAL unsigned *g_counts = as_global_rw(counts), *g_offsets = as_global_rw(offsets), *g_out = as_global_rw(out);

    if (mode == HARVEST_SCAN) {
        // exclusive prefix over the channel counts, 256 at a time: an inclusive scan inside each wave, the waves' totals through LDS, the carry
        // of the passes before in a wave-uniform register
        const unsigned lane = tid & 63u, wave = tid >> 6;
        unsigned carry = 0u;
        for (int base = 0; base < n_chan; base += HARVEST_NT) {
            const int i = base + (int)tid;
            const unsigned v = i < n_chan ? g_counts[i] : 0u;
            unsigned inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = (unsigned)__shfl_up((int)inc, d, 64);
                if ((int)lane >= d) inc += o;
            }
            if (lane == 63u) s_w[wave] = inc;
            __syncthreads();
            const unsigned w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
            __syncthreads();
            const unsigned before = (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
            if (i < n_chan) g_offsets[i] = carry + before + (inc - v);
            carry += w0 + w1 + w2 + w3;
        }
        if (tid == 0) g_out[0] = carry;
        return;
    }

    const int ch = (int)blockIdx.x;
    if (ch >= n_chan) return;
    const CWSLG_GLOBAL HarvestDesc *d = as_global(desc) + ch;
    const CWSLG_GLOBAL unsigned *g_list = as_global(reinterpret_cast<const unsigned *>(d->list));
    const CWSLG_GLOBAL unsigned *g_msg = as_global(reinterpret_cast<const unsigned *>(d->msg));
    const CWSLG_GLOBAL unsigned *g_osd = as_global(reinterpret_cast<const unsigned *>(d->osd));
    const CWSLG_GLOBAL int *g_nrec = as_global(d->nrec);
    const bool have_osd = d->osd != nullptr;
    const int n = max(0, min(min(*as_global(d->cnt), d->cap), SYNC_MAXCAND_CAP));
    const int n_slots = ft4 ? 3 * n : n;

    // ---- the walk: entry of every slot, word of every entry, the words listed in ascending entry order ----
    unsigned n_entries = 0u, m = 0u;
    for (int base = 0; base < n_slots; base += HARVEST_NT) {
        const int slot = base + (int)tid;
        bool exists = slot < n_slots;
        if (ft4 && exists) exists = slot % 3 < g_nrec[slot / 3];
        unsigned k0 = 0u, k1 = 0u, k2 = 0u, set = 0u, by_osd = 0u, nharderr = 0u;
        bool word = false;
        if (exists) {
            // the decode record(s): 5 words each -- bits, iters | nbad, nharderr | crc_ok << 16; FT4: three per slot
            const unsigned nset = ft4 ? 3u : 1u;
            const CWSLG_GLOBAL unsigned *mrec = g_msg + (size_t)slot * (5u * nset);
            const bool bp0 = (mrec[4] >> 16 & 0xffu) != 0u;
            const bool bp1 = ft4 && (mrec[9] >> 16 & 0xffu) != 0u;
            const bool bp2 = ft4 && (mrec[14] >> 16 & 0xffu) != 0u;
            if (bp0 || bp1 || bp2) {
                set = bp0 ? 0u : bp1 ? 1u : 2u;
                const CWSLG_GLOBAL unsigned *r = mrec + 5u * set;
                k0 = r[0]; k1 = r[1]; k2 = r[2];
                nharderr = r[4] & 0xffffu;
                word = true;
            } else if (have_osd) {
                // the OSD record(s): 6 words each -- bits, dmin, nharderr | nskip << 16, crc_ok | how << 8 | flip << 16
                const CWSLG_GLOBAL unsigned *orec = g_osd + (size_t)slot * (6u * nset);
                const bool o0 = (orec[5] & 0xffu) != 0u;
                const bool o1 = ft4 && (orec[11] & 0xffu) != 0u;
                const bool o2 = ft4 && (orec[17] & 0xffu) != 0u;
                if (o0 || o1 || o2) {
                    set = o0 ? 0u : o1 ? 1u : 2u;
                    const CWSLG_GLOBAL unsigned *r = orec + 6u * set;
                    k0 = r[0]; k1 = r[1]; k2 = r[2];
                    nharderr = r[4] & 0xffffu;
                    by_osd = 1u;
                    word = true;
                }
            }
            // the all-zero word (91 bits; byte 11 keeps bits 88..90 in its top three) has CRC 0 and would pass: it is no decode
            if ((k0 | k1 | (k2 & 0xe0ffffffu)) == 0u) word = false;
        }
        unsigned t_entries, t_words;
        const unsigned entry = n_entries + harvest_place(exists, s_w, &t_entries);
        const unsigned at = m + harvest_place(word, s_w, &t_words);
        if (word) {
            s_key[0][at] = k0; s_key[1][at] = k1; s_key[2][at] = k2;
            s_rank[at] = by_osd << 28 | (nharderr & 0xfffu) << 16 | entry;
            s_info[at] = (unsigned)slot | set << 12;
        }
        n_entries += t_entries;
        m += t_words;
    }
    __syncthreads();

    // ---- de-duplication: equal keys are one decode; the best rank stays and counts the others ----
    for (unsigned i = tid; i < m; i += HARVEST_NT) {
        const unsigned a0 = s_key[0][i], a1 = s_key[1][i], a2 = s_key[2][i], mine = s_rank[i];
        unsigned ndup = 0u;
        bool best = true;
        for (unsigned j = 0; j < m; ++j) {
            if (s_key[0][j] != a0) continue;
            if (s_key[1][j] != a1 || s_key[2][j] != a2) continue;
            ++ndup;
            if (s_rank[j] < mine) best = false;
        }
        s_info[i] = (s_info[i] & 0x3fffu) | (best ? 0x8000u : 0u) | min(ndup, 65535u) << 16;
    }
    __syncthreads();

    // ---- the survivors in ascending entry order ----
    const unsigned first = mode == HARVEST_EMIT ? g_offsets[ch] : 0u;
    unsigned n_out = 0u;
    for (unsigned base = 0; base < m; base += HARVEST_NT) {
        const unsigned i = base + tid;
        const unsigned info = i < m ? s_info[i] : 0u;
        const bool keep = (info & 0x8000u) != 0u;
        unsigned t_keep;
        const unsigned p = first + n_out + harvest_place(keep, s_w, &t_keep);
        n_out += t_keep;
        if (mode == HARVEST_EMIT && keep && p < (unsigned)max_out) {
            const unsigned rank = s_rank[i], slot = info & 0xfffu, set = info >> 12 & 3u, by_osd = rank >> 28;
            unsigned freq, dt, sync, dmin = 0u;
            if (ft4) {          // Ft4Rec: f0_hz, f1_hz, dt_s, sync, ...
                const CWSLG_GLOBAL unsigned *r = g_list + (size_t)slot * 8u;
                freq = r[1]; dt = r[2]; sync = r[3];
                if (by_osd) dmin = g_osd[(size_t)slot * 18u + 6u * set + 3u];
            } else {            // Cand: freq_bin, time_step, sync, freq_hz, dt_s
                const CWSLG_GLOBAL unsigned *r = g_list + (size_t)slot * 5u;
                sync = r[2]; freq = r[3]; dt = r[4];
                if (by_osd) dmin = g_osd[(size_t)slot * 6u + 3u];
            }
            CWSLG_GLOBAL unsigned *o = g_out + HARVEST_HEAD_WORDS + (size_t)p * HARVEST_REC_WORDS;
            o[0] = (unsigned)d->ch_id;
            o[1] = (rank & 0xffffu) | by_osd << 16 | set << 24;
            o[2] = s_key[0][i]; o[3] = s_key[1][i]; o[4] = s_key[2][i];
            o[5] = freq; o[6] = dt; o[7] = sync; o[8] = dmin;
            o[9] = (rank >> 16 & 0xfffu) | (info >> 16) << 16;
        }
    }
    if (mode == HARVEST_COUNT && tid == 0) g_counts[ch] = n_out;
}

// The launches of one call on stream `s`: count and emit with one workgroup per channel, the scan with one; `lim` records may be written, and
// with lim == 0 nothing may be, so emit is skipped and out[0] = n_total is all the caller gets.  The library (cwslg_fetch_decodes) and the
// stand-alone check of the kernel (tests/harvest_kernel_check.hip) both launch through here.  The caller asks hipGetLastError.
inline void harvest_launch(hipStream_t s, const HarvestDesc *d_desc, unsigned *d_counts, unsigned *d_offsets, unsigned *d_out, int n_chan, int lim, int ft4)
{
    for (int mode : {HARVEST_COUNT, HARVEST_SCAN, HARVEST_EMIT}) {
        if (mode == HARVEST_EMIT && lim == 0) break;
        hipLaunchKernelGGL(decode_harvest_kernel, dim3(mode == HARVEST_SCAN ? 1u : (unsigned)n_chan), dim3(HARVEST_NT), 0, s, d_desc, d_counts, d_offsets, d_out,
                           n_chan, lim, ft4 ? 1 : 0, mode);
    }
}

// The ONE further launch of cwslg_fetch_decode_reports, behind harvest_launch on the same stream and blocks: a wave per record that emit may have
// written (the count, min(out[0], lim), is read on the device; the waves beyond it leave), the reports to d_rep[lim][4].  Nothing to launch for
// lim == 0.  d_enc: the encoder's 91 x 6 dwords.  The library and tests/report_kernel_check.hip both launch through here.
inline void report_launch(hipStream_t s, const ReportDesc *d_rdesc, const unsigned *d_offsets, const unsigned *d_out, const uint32_t *d_enc, unsigned *d_rep,
                          int n_chan, int lim)
{
    if (lim <= 0) return;
    hipLaunchKernelGGL(decode_report_kernel, dim3((unsigned)((lim + FT8S_WAVES - 1) / FT8S_WAVES)), dim3(64 * FT8S_WAVES), 0, s, d_rdesc, d_offsets, d_out, d_enc,
                       d_rep, n_chan, lim);
}

} // namespace cwslg
