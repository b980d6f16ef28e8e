// ft4sub_layout.hpp -- what the FT4 subtractor's host side (ft8sub_host.inc, in the library) and its kernels (modules/ft4sub.hip, a code object of
// their own: DESIGN.md 4.16) agree on: grids, record layouts.  The descriptor is the FT8 subtractor's SubDesc.  Plain constants, no device code.
#pragma once
#include <stdint.h>
#include "ft8sub_layout.hpp"

namespace cwslg {

constexpr int F4SUB_N = 72576;                     // samples of a frame: the decoder's F4C_NMAX
constexpr int F4SUB_NSPS = 576, F4SUB_NSYM = 103, F4SUB_NW = F4SUB_NSPS * F4SUB_NSYM;    // 59328 samples of a signal
constexpr int F4SUB_BLK = 18, F4SUB_BPS = 32, F4SUB_NBLK = F4SUB_NSYM * F4SUB_BPS;      // 3296 blocks of 18 samples
constexpr int F4SUB_TAU_MAX = 54, F4SUB_TAU_STEP = 2, F4SUB_NTAU = 2 * F4SUB_TAU_MAX / F4SUB_TAU_STEP + 1;        // 55 time offsets
constexpr int F4SUB_DINC = 27962, F4SUB_KF = 26, F4SUB_NK = 2 * F4SUB_KF + 1;          // 53 frequency offsets of 0.078125 Hz
constexpr double F4SUB_SLOPE_K = 4294967296.0 / (6.283185307179586 * F4SUB_BLK);      // the track's radians per block -> 2^-32 turns per sample
constexpr int F4SUB_CAND_OFFSET = 0;               // a record's dt_s, ibest / 666.67 - 0.5, names the signal's first sample itself
constexpr int F4SUB_HW = 48;                       // the track's window: blocks b - 48 .. b + 48
constexpr int F4SUB_NT = 256;                      // threads of either kernel's workgroup
constexpr int F4SUB_TILE = 4 * F4SUB_NT;           // apply: samples of a time tile
constexpr int F4SUB_NTILE = (F4SUB_N + F4SUB_TILE - 1) / F4SUB_TILE;     // 71
static_assert(F4SUB_N % 4 == 0 && F4SUB_NTILE == 71, "a thread's four samples lie inside the frame or outside it");

// the per-decode device record the fit leaves for the apply, in dwords: start, inc, base[103], tones (4 per dword, 26 dwords), ..., track[3296][2]
// from 132
constexpr int F4SUB_REC_START = 0, F4SUB_REC_INC = 1, F4SUB_REC_BASE = 2, F4SUB_REC_TONES = 105, F4SUB_REC_TRACK = 132;
constexpr int F4SUB_REC_WORDS = F4SUB_REC_TRACK + 2 * F4SUB_NBLK;                    // 6724 dwords, 26896 bytes
static_assert(F4SUB_REC_TONES + (F4SUB_NSYM + 3) / 4 <= F4SUB_REC_TRACK && F4SUB_REC_TRACK % 2 == 0 && F4SUB_REC_WORDS % 2 == 0, "record layout");
constexpr int F4SUB_REP_WORDS = F8SUB_REP_WORDS;   // cwslg_subtract_report is 28 bytes
// what the kernels read of the harvest's output block and of the encoder: the FT8 subtractor's constants (ft8sub_host.inc asserts them)
constexpr int F4SUB_DEC_HEAD_WORDS = F8SUB_DEC_HEAD_WORDS, F4SUB_DEC_WORDS = F8SUB_DEC_WORDS, F4SUB_ENC_ROWS = F8SUB_ENC_ROWS, F4SUB_ENC_WORDS = F8SUB_ENC_WORDS;

} // namespace cwslg
