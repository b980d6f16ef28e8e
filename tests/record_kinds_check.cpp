// Stand-alone check of csrc/record_kinds.hpp (built and run by tests/test_record_kinds.py): the one epoch rule and the kind table against the
// conditions of every fetch written out LONGHAND below, one `if` per fetch as the specification states them -- enumerated over every stamp and
// the frame's epoch in {0, E, E - 1} and every buffer present or absent.  Prints the number of states compared; exit status 1 and the first
// differing state on a mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "record_kinds.hpp"

using namespace cwslg;

namespace {

struct Chan {               // what the conditions read
    bool have_frame;
    uint64_t frame_t0, cand_t0, ft4c_t0, soft_t0, msg_t0, osd_t0, soft4_t0, msg4_t0, osd4_t0;
    bool d_block, d_ft4c, d_soft, d_msg, d_osd, d_ft4soft, d_ft4msg, d_ft4osd;
};

// ---- the specification: epoch returned, 0 = CWSLG_ERR_NO_FRAME ----------------------------------------------------------------------------------
uint64_t spec_fetch(int kind, const Chan &ch)
{
    switch (kind) {
    case REC_CAND:
        if (!ch.have_frame || !ch.d_block || !ch.cand_t0) return 0;
        return ch.cand_t0;
    case REC_FT4SYNC:
        if (!ch.have_frame || !ch.d_block || !ch.d_ft4c || !ch.ft4c_t0 || ch.ft4c_t0 != ch.cand_t0) return 0;
        return ch.ft4c_t0;
    case REC_SOFT8:
        if (!ch.have_frame || !ch.d_block || !ch.d_soft || !ch.soft_t0 || ch.soft_t0 != ch.frame_t0 || ch.soft_t0 != ch.cand_t0) return 0;
        return ch.soft_t0;
    case REC_MSG8:
        if (!ch.have_frame || !ch.d_block || !ch.d_msg || !ch.msg_t0 || ch.msg_t0 != ch.frame_t0 || ch.msg_t0 != ch.cand_t0 || ch.msg_t0 != ch.soft_t0) return 0;
        return ch.msg_t0;
    case REC_OSD8:
        if (!ch.have_frame || !ch.d_block || !ch.d_osd || !ch.osd_t0 || ch.osd_t0 != ch.frame_t0 || ch.osd_t0 != ch.cand_t0 || ch.osd_t0 != ch.soft_t0 ||
            ch.osd_t0 != ch.msg_t0)
            return 0;
        return ch.osd_t0;
    case REC_SOFT4:
        if (!ch.have_frame || !ch.d_block || !ch.d_ft4c || !ch.d_ft4soft || !ch.soft4_t0 || ch.soft4_t0 != ch.frame_t0 || ch.soft4_t0 != ch.cand_t0) return 0;
        return ch.soft4_t0;
    case REC_MSG4:
        if (!ch.have_frame || !ch.d_block || !ch.d_ft4c || !ch.d_ft4soft || !ch.d_ft4msg || !ch.msg4_t0 || ch.msg4_t0 != ch.frame_t0 ||
            ch.msg4_t0 != ch.cand_t0 || ch.msg4_t0 != ch.soft4_t0)
            return 0;
        return ch.msg4_t0;
    case REC_OSD4:
        if (!ch.have_frame || !ch.d_block || !ch.d_ft4c || !ch.d_ft4soft || !ch.d_ft4msg || !ch.d_ft4osd || !ch.osd4_t0 || ch.osd4_t0 != ch.frame_t0 ||
            ch.osd4_t0 != ch.cand_t0 || ch.osd4_t0 != ch.soft4_t0 || ch.osd4_t0 != ch.msg4_t0)
            return 0;
        return ch.osd4_t0;
    }
    return 0;
}

// cwslg_fetch_slot (which has returned CWSLG_ERR_NO_FRAME without a frame): the list, and the FT4 sync records with it, only if of the frame's epoch
uint64_t spec_slot(int kind, const Chan &ch)
{
    if (!ch.have_frame) return 0;
    if (ch.cand_t0 == ch.frame_t0 && ch.cand_t0 != 0) {
        if (ch.d_block) {
            if (kind == REC_CAND) return ch.frame_t0;
            if (kind == REC_FT4SYNC && ch.d_ft4c && ch.ft4c_t0 == ch.frame_t0) return ch.frame_t0;
        }
    }
    return 0;
}

// sync_launch: the stamps set at a boundary (bits), for a channel that has a sync stage
unsigned spec_queued(bool sync_ft8, bool sync_ft4, bool ft4_coherent, bool ft8_soft, bool ft8_decode, bool ft8_osd, bool ft4_soft, bool ft4_decode, bool ft4_osd)
{
    unsigned q = 0;
    if (!sync_ft8 && !sync_ft4) return q;
    q |= 1u << REC_CAND;
    if (sync_ft8 && ft8_soft) {
        q |= 1u << REC_SOFT8;
        if (ft8_decode) {
            q |= 1u << REC_MSG8;
            if (ft8_osd) q |= 1u << REC_OSD8;
        }
    }
    if (sync_ft4 && ft4_coherent) q |= 1u << REC_FT4SYNC;
    if (sync_ft4) {
        const bool soft = ft4_coherent && ft4_soft;
        if (soft) {
            q |= 1u << REC_SOFT4;
            if (ft4_decode) {
                q |= 1u << REC_MSG4;
                if (ft4_osd) q |= 1u << REC_OSD4;
            }
        }
    }
    return q;
}

struct Gate { RecChain chain; const char *text; };
const Gate kGates[REC_KINDS] = {
    {CHAIN_ANY, nullptr},
    {CHAIN_FT4, nullptr},
    {CHAIN_FT8, "soft bits exist for FT8 channels only (mode %s)"},
    {CHAIN_FT8, "decode records exist for FT8 channels only (mode %s)"},
    {CHAIN_FT8, "OSD records exist for FT8 channels only (mode %s)"},
    {CHAIN_FT4, "FT4 soft bits exist for FT4 channels only (mode %s)"},
    {CHAIN_FT4, "FT4 decode records exist for FT4 channels only (mode %s)"},
    {CHAIN_FT4, "FT4 OSD records exist for FT4 channels only (mode %s)"},
};

int report(const char *what, int kind, const Chan &ch, uint64_t got, uint64_t want)
{
    std::printf("MISMATCH %s kind %d: rule %llu, longhand %llu; have_frame %d frame %llu stamps cand %llu ft4c %llu soft %llu msg %llu osd %llu soft4 %llu msg4 %llu "
                "osd4 %llu; arrays block %d ft4c %d soft %d msg %d osd %d ft4soft %d ft4msg %d ft4osd %d\n",
                what, kind, (unsigned long long)got, (unsigned long long)want, ch.have_frame, (unsigned long long)ch.frame_t0, (unsigned long long)ch.cand_t0,
                (unsigned long long)ch.ft4c_t0, (unsigned long long)ch.soft_t0, (unsigned long long)ch.msg_t0, (unsigned long long)ch.osd_t0,
                (unsigned long long)ch.soft4_t0, (unsigned long long)ch.msg4_t0, (unsigned long long)ch.osd4_t0, ch.d_block, ch.d_ft4c, ch.d_soft, ch.d_msg, ch.d_osd,
                ch.d_ft4soft, ch.d_ft4msg, ch.d_ft4osd);
    return 1;
}

} // namespace

int main()
{
    const uint64_t E = 1700000015;
    const uint64_t vals[3] = {0, E, E - 1};
    // the gates: chain and wording per kind
    for (int k = 0; k < REC_KINDS; ++k) {
        const RecKindRow &r = kRecKinds[k];
        const bool same_text = (r.gate == nullptr) == (kGates[k].text == nullptr) && (!r.gate || std::strcmp(r.gate, kGates[k].text) == 0);
        if (r.chain != kGates[k].chain || !same_text) { std::printf("MISMATCH gate of kind %d\n", k); return 1; }
    }
    // the rule.  Per kind, exhaustively: the frame's epoch, the list's stamp and every stamp and array of the kind's own chain (a list and the FT4
    // sync records: of the FT4 chain); the other chain's stamps take one common value of the three and its arrays are all present or all absent.
    unsigned long long states = 0;
    for (int kind = 0; kind < REC_KINDS; ++kind) {
        const bool ft8_kind = kRecKinds[kind].chain == CHAIN_FT8;
        for (int hf = 0; hf < 2; ++hf)
        for (int fr = 0; fr < 3; ++fr)
        for (int st = 0; st < 243; ++st)                 // 3^5: cand, then four stamps of the chain (FT8: the fourth slot is the FT4 sync records')
        for (int pr = 0; pr < 32; ++pr)                  // 2^5 arrays likewise
        for (int os = 0; os < 3; ++os)
        for (int op = 0; op < 2; ++op) {
            int d[5], s = st;
            for (int j = 0; j < 5; ++j) { d[j] = s % 3; s /= 3; }
            Chan ch{};
            ch.have_frame = hf != 0;
            ch.frame_t0 = vals[fr];
            ch.cand_t0 = vals[d[0]];
            ch.d_block = pr & 1;
            ch.ft4c_t0 = vals[d[4]];
            ch.d_ft4c = (pr >> 4) & 1;
            const uint64_t a = vals[d[1]], b = vals[d[2]], c = vals[d[3]], o = vals[os];
            const bool pa = (pr >> 1) & 1, pb = (pr >> 2) & 1, pc = (pr >> 3) & 1, po = op != 0;
            if (ft8_kind) {
                ch.soft_t0 = a; ch.msg_t0 = b; ch.osd_t0 = c; ch.d_soft = pa; ch.d_msg = pb; ch.d_osd = pc;
                ch.soft4_t0 = ch.msg4_t0 = ch.osd4_t0 = o; ch.d_ft4soft = ch.d_ft4msg = ch.d_ft4osd = po;
            } else {
                ch.soft4_t0 = a; ch.msg4_t0 = b; ch.osd4_t0 = c; ch.d_ft4soft = pa; ch.d_ft4msg = pb; ch.d_ft4osd = pc;
                ch.soft_t0 = ch.msg_t0 = ch.osd_t0 = o; ch.d_soft = ch.d_msg = ch.d_osd = po;
            }
            uint64_t stamp[REC_KINDS];
            stamp[REC_CAND] = ch.cand_t0; stamp[REC_FT4SYNC] = ch.ft4c_t0; stamp[REC_SOFT8] = ch.soft_t0; stamp[REC_MSG8] = ch.msg_t0; stamp[REC_OSD8] = ch.osd_t0;
            stamp[REC_SOFT4] = ch.soft4_t0; stamp[REC_MSG4] = ch.msg4_t0; stamp[REC_OSD4] = ch.osd4_t0;
            const unsigned present = (ch.d_block ? 1u << REC_CAND : 0) | (ch.d_ft4c ? 1u << REC_FT4SYNC : 0) | (ch.d_soft ? 1u << REC_SOFT8 : 0) |
                                     (ch.d_msg ? 1u << REC_MSG8 : 0) | (ch.d_osd ? 1u << REC_OSD8 : 0) | (ch.d_ft4soft ? 1u << REC_SOFT4 : 0) |
                                     (ch.d_ft4msg ? 1u << REC_MSG4 : 0) | (ch.d_ft4osd ? 1u << REC_OSD4 : 0);
            const uint64_t got = records_epoch(kind, ch.have_frame, ch.frame_t0, stamp, present), want = spec_fetch(kind, ch);
            ++states;
            if (got != want) return report("fetch", kind, ch, got, want);
            if (kind == REC_CAND || kind == REC_FT4SYNC) {
                const uint64_t gs = records_epoch(kind, ch.have_frame, ch.frame_t0, stamp, present, true), ws = spec_slot(kind, ch);
                ++states;
                if (gs != ws) return report("slot", kind, ch, gs, ws);
            }
        }
    }
    // the stamps a boundary sets
    for (int m = 0; m < 1 << 9; ++m) {
        const bool f8 = m & 1, f4 = m & 2, coh = m & 4, s8 = m & 8, m8 = m & 16, o8 = m & 32, s4 = m & 64, m4 = m & 128, o4 = m & 256;
        if (f8 && f4) continue;                         // a channel has one mode
        bool on[REC_KINDS];
        on[REC_CAND] = true; on[REC_FT4SYNC] = coh; on[REC_SOFT8] = s8; on[REC_MSG8] = m8; on[REC_OSD8] = o8; on[REC_SOFT4] = s4; on[REC_MSG4] = m4; on[REC_OSD4] = o4;
        const unsigned got = records_queued(f8, f4, on), want = spec_queued(f8, f4, coh, s8, m8, o8, s4, m4, o4);
        ++states;
        if (got != want) { std::printf("MISMATCH queued: switches %03x: rule %02x, longhand %02x\n", m, got, want); return 1; }
    }
    std::printf("OK %llu states\n", states);
    return 0;
}
