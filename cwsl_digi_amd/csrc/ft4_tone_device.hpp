// ft4_tone_device.hpp -- the channel tone of one FT4 symbol from a codeword held in six registers (OsdGen bit layout), with the
// Costas blocks and the Gray map it needs.  Shared by ft4_report_kernel and the soft bits (ft4soft_kernels.hpp) and by the FT4 subtractor's module
// (modules/ft4sub.hip): one device text for the re-encoder's last step.  No rvec, as everywhere in the FT4 chain.
#pragma once
#include <hip/hip_runtime.h>
#include "ft8_tone_device.hpp"      // report_pick6

namespace cwslg {

// icos4 (0132 1023 2310 3201), two bits per entry [4 b + s]
constexpr unsigned ft4s_pack2(const int (&v)[16]) { unsigned c = 0; for (int i = 0; i < 16; ++i) c |= (unsigned)v[i] << (2 * i); return c; }
constexpr int FT4S_ICOS4_V[16] = {0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1};
constexpr unsigned FT4S_ICOS4 = ft4s_pack2(FT4S_ICOS4_V);

__device__ __forceinline__ int ft4s_gray(int v) { return v ^ (v >> 1); }                           // graymap 0,1,3,2

// the tone of symbol n (0..102) of the codeword c0..c5 (OsdGen bit layout); *costas: n is a Costas symbol
__device__ __forceinline__ int ft4r_tone(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned c4, unsigned c5, int n, bool *costas)
{
    const int blk = n < 33 ? 0 : n < 66 ? 1 : n < 99 ? 2 : 3, r = n - 33 * blk;
    *costas = r < 4;
    const int icos = (int)((FT4S_ICOS4 >> (2 * (4 * blk + (r < 4 ? r : 0)))) & 3u);
    const int d = n - 4 * (blk + 1);                                    // data symbol 0..86 (meaningless for a Costas symbol: clamped)
    const int t = 2 * (d < 0 ? 0 : d > 86 ? 86 : d);                    // even: cw[2d], cw[2d+1] lie in one word
    const unsigned x = report_pick6(c0, c1, c2, c3, c4, c5, t >> 5) >> (t & 31) & 3u;      // cw[2d] | cw[2d+1] << 1
    const int v = (int)((x & 1u) << 1 | x >> 1);
    return r < 4 ? icos : ft4s_gray(v);
}

} // namespace cwslg
