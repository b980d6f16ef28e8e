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
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sync_kernels.hpp"

namespace cwslg {

constexpr int HARVEST_COUNT = 0, HARVEST_SCAN = 1, HARVEST_EMIT = 2;
constexpr int HARVEST_NT = 256;
constexpr int HARVEST_MAXSLOTS = 3 * SYNC_MAXCAND_CAP;                  // FT4: three record slots per candidate
constexpr int HARVEST_REC_WORDS = 10;                                   // cwslg_decode is 40 bytes
constexpr int HARVEST_HEAD_WORDS = 4;                                   // out[0] = n_total; the records follow 16 bytes in

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

__global__ __launch_bounds__(HARVEST_NT) void decode_harvest_kernel(const HarvestDesc *__restrict__ desc, unsigned *__restrict__ counts,
                                                                    unsigned *__restrict__ offsets, unsigned *__restrict__ out, int n_chan, int max_out,
                                                                    int ft4, int mode)
{
    __shared__ unsigned s_key[3][HARVEST_MAXSLOTS];      // the word: bits[12] as three little-endian words
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

} // namespace cwslg
