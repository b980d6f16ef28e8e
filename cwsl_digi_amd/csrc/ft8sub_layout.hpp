// ft8sub_layout.hpp -- what the FT8 subtractor's host side (ft8sub_host.inc, in the library) and its kernels (modules/ft8sub.hip, a code object of
// their own: DESIGN.md 4.15) agree on: grids, record layouts, descriptors.  Plain constants and structs, no device code.
#pragma once
#include <stdint.h>

namespace cwslg {

constexpr int F8SUB_N = 180000;                    // samples of a frame
constexpr int F8SUB_NSPS = 1920, F8SUB_NSYM = 79, F8SUB_NW = F8SUB_NSPS * F8SUB_NSYM;
constexpr int F8SUB_BLK = 60, F8SUB_BPS = 32, F8SUB_NBLK = F8SUB_NSYM * F8SUB_BPS;      // 2528 blocks of 60 samples
constexpr int F8SUB_TAU_MAX = 240, F8SUB_TAU_STEP = 8, F8SUB_NTAU = 2 * F8SUB_TAU_MAX / F8SUB_TAU_STEP + 1;        // 61 time offsets
constexpr int F8SUB_DINC = 11185, F8SUB_KF = 52, F8SUB_NK = 2 * F8SUB_KF + 1;          // 105 frequency offsets of 0.03125 Hz
constexpr int F8SUB_CAND_STEP = 480;             // a candidate's dt_s lies one plane step (40 ms) after the signal's first sample
constexpr int F8SUB_HW = 48;                       // the track's window: blocks b - 48 .. b + 48
constexpr int F8SUB_NT = 256;                      // threads of either kernel's workgroup
constexpr int F8SUB_TILE = 4 * F8SUB_NT;           // apply: samples of a time tile
constexpr int F8SUB_NTILE = (F8SUB_N + F8SUB_TILE - 1) / F8SUB_TILE;

// the per-decode device record the fit leaves for the apply, in dwords: start, inc, base[79], tones (4 per dword), ..., track[2528][2] from 128
constexpr int F8SUB_REC_START = 0, F8SUB_REC_INC = 1, F8SUB_REC_BASE = 2, F8SUB_REC_TONES = 81, F8SUB_REC_TRACK = 128;
constexpr int F8SUB_REC_WORDS = F8SUB_REC_TRACK + 2 * F8SUB_NBLK;                    // 5184 dwords, 20736 bytes
constexpr int F8SUB_REP_WORDS = 7;                 // cwslg_subtract_report is 28 bytes
// what the kernels read of the harvest's output block and of the encoder (harvest_kernels.hpp: HARVEST_HEAD_WORDS, HARVEST_REC_WORDS, REPORT_ENC_*;
// the host side asserts that they agree)
constexpr int F8SUB_DEC_HEAD_WORDS = 4, F8SUB_DEC_WORDS = 10, F8SUB_ENC_ROWS = 91, F8SUB_ENC_WORDS = 6;

// One channel (flat call: one frame) that takes part.
struct alignas(16) SubDesc {
    const float *frame;      // [180000], 16-byte aligned, never written
    float *resid;            // [180000]
    int n_valid;             // samples from here on count as +0 (the zero tail of a short slot, which the device frame does not hold)
    int pad_[3];
};
static_assert(sizeof(SubDesc) == 32, "descriptor layout");

} // namespace cwslg
