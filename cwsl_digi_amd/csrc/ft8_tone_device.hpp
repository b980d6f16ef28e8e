// ft8_tone_device.hpp -- the channel tone of one FT8 symbol from a codeword held in six registers (OsdGen bit layout).  Shared by
// decode_report_kernel (harvest_kernels.hpp) and the subtractor's module (modules/ft8sub.hip): one device text for the re-encoder's last step.
#pragma once
#include <hip/hip_runtime.h>

namespace cwslg {

__device__ __forceinline__ unsigned report_pick6(unsigned w0, unsigned w1, unsigned w2, unsigned w3, unsigned w4, unsigned w5, int i)
{
    return i == 0 ? w0 : i == 1 ? w1 : i == 2 ? w2 : i == 3 ? w3 : i == 4 ? w4 : w5;
}

// the tone of symbol n (0..78) of the codeword c0..c5 (OsdGen bit layout); *costas: n is a Costas symbol
__device__ __forceinline__ int report_tone(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned c4, unsigned c5, int n, bool *costas)
{
    const int blk = n < 36 ? 0 : n < 72 ? 1 : 2, r = n - 36 * blk;
    *costas = r < 7;
    const int icos7 = (0x2560413 >> (4 * (r < 7 ? r : 0))) & 7;        // 3,1,4,0,6,5,2
    const int d = n - (n < 36 ? 7 : 14);                                // data symbol 0..57 (meaningless for a Costas symbol: clamped)
    const int t = 3 * (d < 0 ? 0 : d > 57 ? 57 : d), wi = t >> 5;
    const unsigned lo = report_pick6(c0, c1, c2, c3, c4, c5, wi), hi = report_pick6(c1, c2, c3, c4, c5, 0u, wi);
    const unsigned x = (unsigned)((((unsigned long long)hi << 32) | lo) >> (t & 31)) & 7u;      // cw[3d] | cw[3d+1] << 1 | cw[3d+2] << 2
    const unsigned v = (x & 1u) << 2 | (x & 2u) | x >> 2;
    const int gray = (0x74652310 >> (4 * v)) & 7;                       // graymap 0,1,3,2,5,6,4,7
    return r < 7 ? icos7 : gray;
}

} // namespace cwslg
