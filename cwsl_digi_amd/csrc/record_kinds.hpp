// record_kinds.hpp -- the record kinds behind the FT8 / FT4 candidate lists and the ONE rule that says whether a channel's records of a kind may
// be handed out, and under which epoch.  Plain C++ on plain values (no HIP type, no library type): every fetch of sync_host.inc, cwslg_fetch_slot
// and sync_launch go through it, and tests/record_kinds_check.cpp enumerates it against the conditions written out longhand.
//
// A channel carries one stamp per kind: the start epoch of the frame the records of that kind now on the device were computed from (0: none).
// sync_launch stamps a kind with the frame's epoch iff it queues that stage at the boundary (records_queued); a stage that did not run keeps its
// OLD stamp, and the rule below then finds nothing to fetch -- never an older slot's records under the newer epoch.
#pragma once
#include <stdint.h>

namespace cwslg {

enum RecKind {
    REC_CAND,          // candidate list (FT8, FT4 and the 120 s modes)
    REC_FT4SYNC,       // FT4 sync records        (cwslg_enable_ft4_coherent)
    REC_SOFT8,         // FT8 soft-bit records    (cwslg_enable_ft8_softbits)
    REC_MSG8,          // FT8 decode records      (cwslg_enable_ft8_decode)
    REC_OSD8,          // FT8 OSD records         (cwslg_enable_ft8_osd)
    REC_SOFT4,         // FT4 soft-bit records    (cwslg_enable_ft4_softbits)
    REC_MSG4,          // FT4 decode records      (cwslg_enable_ft4_decode)
    REC_OSD4,          // FT4 OSD records         (cwslg_enable_ft4_osd)
    REC_KINDS
};
enum RecChain { CHAIN_ANY, CHAIN_FT8, CHAIN_FT4 };

constexpr unsigned rec_bit(int k) { return 1u << k; }

struct RecKindRow {
    RecChain chain;    // the channels that have records of this kind
    const char *gate;  // the fetch refuses every other channel with CWSLG_ERR_MODE and this text (%s: the channel's mode); null: no mode gate
    int prev;          // the stage it runs behind: queued at a boundary only if that one is (-1: runs at every boundary of the sync stage)
    unsigned need;     // arrays that must exist (bit k: the array of kind k; REC_CAND: the block that holds the list)
    unsigned same;     // stamps that must equal its own
    bool frame;        // its own stamp must also be the frame's epoch (a list is exempt: it survives a boundary that ran with the stage disabled)
};

// FT8 records need only their OWN array (the three are carved from one block); FT4 records need d_ft4c and every array up to their own.
// The FT4 chain's stamps are not compared with the sync records' (REC_FT4SYNC is in no `same` below).
constexpr RecKindRow kRecKinds[REC_KINDS] = {
    /* REC_CAND    */ {CHAIN_ANY, nullptr, -1, rec_bit(REC_CAND), 0, false},
    /* REC_FT4SYNC */ {CHAIN_FT4, nullptr, REC_CAND, rec_bit(REC_CAND) | rec_bit(REC_FT4SYNC), rec_bit(REC_CAND), false},
    /* REC_SOFT8   */ {CHAIN_FT8, "soft bits exist for FT8 channels only (mode %s)", REC_CAND, rec_bit(REC_CAND) | rec_bit(REC_SOFT8), rec_bit(REC_CAND), true},
    /* REC_MSG8    */ {CHAIN_FT8, "decode records exist for FT8 channels only (mode %s)", REC_SOFT8, rec_bit(REC_CAND) | rec_bit(REC_MSG8),
                       rec_bit(REC_CAND) | rec_bit(REC_SOFT8), true},
    /* REC_OSD8    */ {CHAIN_FT8, "OSD records exist for FT8 channels only (mode %s)", REC_MSG8, rec_bit(REC_CAND) | rec_bit(REC_OSD8),
                       rec_bit(REC_CAND) | rec_bit(REC_SOFT8) | rec_bit(REC_MSG8), true},
    /* REC_SOFT4   */ {CHAIN_FT4, "FT4 soft bits exist for FT4 channels only (mode %s)", REC_FT4SYNC,
                       rec_bit(REC_CAND) | rec_bit(REC_FT4SYNC) | rec_bit(REC_SOFT4), rec_bit(REC_CAND), true},
    /* REC_MSG4    */ {CHAIN_FT4, "FT4 decode records exist for FT4 channels only (mode %s)", REC_SOFT4,
                       rec_bit(REC_CAND) | rec_bit(REC_FT4SYNC) | rec_bit(REC_SOFT4) | rec_bit(REC_MSG4), rec_bit(REC_CAND) | rec_bit(REC_SOFT4), true},
    /* REC_OSD4    */ {CHAIN_FT4, "FT4 OSD records exist for FT4 channels only (mode %s)", REC_MSG4,
                       rec_bit(REC_CAND) | rec_bit(REC_FT4SYNC) | rec_bit(REC_SOFT4) | rec_bit(REC_MSG4) | rec_bit(REC_OSD4),
                       rec_bit(REC_CAND) | rec_bit(REC_SOFT4) | rec_bit(REC_MSG4), true},
};

// The epoch under which records of kind k may be handed out now, 0 if there is nothing to fetch.  stamp[]: the channel's stamps; present: bit j
// set if the array of kind j exists; with_frame: the records go out TOGETHER with the frame (cwslg_fetch_slot), so they must be of its epoch
// whatever the kind.
inline uint64_t records_epoch(int k, bool have_frame, uint64_t frame_t0, const uint64_t stamp[REC_KINDS], unsigned present, bool with_frame = false)
{
    const RecKindRow &r = kRecKinds[k];
    const uint64_t own = stamp[k];
    if (!have_frame || (present & r.need) != r.need || !own) return 0;
    if ((r.frame || with_frame) && own != frame_t0) return 0;
    for (int j = 0; j < REC_KINDS; ++j)
        if ((r.same & rec_bit(j)) && stamp[j] != own) return 0;
    return own;
}

// The kinds whose stage is queued at a boundary for a channel of the given chain (bits): on[k] is the stage's switch in the configuration in
// force (on[REC_CAND] is the sync stage itself), and a stage runs only behind the one it reads from.
inline unsigned records_queued(bool ft8, bool ft4, const bool on[REC_KINDS])
{
    unsigned q = 0;
    for (int k = 0; k < REC_KINDS; ++k) {       // (every row's prev has a smaller index)
        const RecKindRow &r = kRecKinds[k];
        const bool mine = r.chain == CHAIN_ANY ? (ft8 || ft4) : r.chain == CHAIN_FT8 ? ft8 : ft4;
        if (mine && on[k] && (r.prev < 0 || (q & rec_bit(r.prev)))) q |= rec_bit(k);
    }
    return q;
}

} // namespace cwslg
