// ft8soft_kernels.hpp -- FT8 soft bits on gfx950: per sync candidate the hard-decision Costas count and the 174 normalised bit
// metrics of upstream ft8b's nsym = 1 pass, taken from the symbol-spectra plane the search has just read.
//
// *** PARITY UNPINNED by the reference *** like the rest of the sync stage (sync_kernels.hpp).  The arithmetic is the one
// include/cwsl_gpu.h states for cwslg_ft8_soft and tests/ft8_softbits_ref.py restates in numpy, BIT FOR BIT: on the plane's own grid
// (one 40 ms step by one 3.125 Hz bin: no fine time / frequency search, the way ft8_lib decodes from its waterfall), symbol n at
// step j + 12 + 4 n, tone k at bin i + 2 k, s8 = sqrtf(power) correctly rounded, bmeta's three max-differences per data symbol
// through graymap, and normalizebmet with both 174-term sums as the fixed tree a wave evaluates: lane l holds b[l], b[l+64], b[l+128]
// (zero beyond 173), adds them left to right, then six halving steps across the lanes.  This translation unit is built
// -ffp-contract=off: every product, sum, quotient and root below is one float32 operation (hipcc's default keeps / and sqrtf
// correctly rounded).
//
// One wave per candidate, four candidates per workgroup, grid (ceil(max_cand / 4), FT8 channels): the count is read from d_ncand on the
// device -- no host round trip -- and the waves beyond it leave.  A candidate touches 79 rows x 15 consecutive floats of the plane: a pass
// of the wave fetches 4 symbols x 16 bins, i.e. per row ONE 60-byte segment (one or two 128-byte lines), 20 independent loads per lane
// in flight at once.  The magnitudes go through a wave-private 2.5 KB LDS image [80][8] so that lane t can pick up the eight tones of
// ITS bit's symbol; nothing is shared between waves, hence no workgroup barrier (waves leave independently).
// Traffic: 79 rows x 1-2 lines x 128 B = 10-20 KB of L2 / HBM lines per candidate in, 704 B out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cwslg {

constexpr int FT8S_NSYM = 79, FT8S_NBIT = 174, FT8S_WAVES = 4;
struct Ft8SoftRec { float llr[FT8S_NBIT]; float sigma; int32_t nsync; };       // = cwslg_ft8_soft
static_assert(sizeof(Ft8SoftRec) == 704, "cwslg_ft8_soft is 704 bytes");

// a[l] = a[l] + a[l+h] for l < h, h = 32 .. 1; the sum ends up on lane 0 and is handed to every lane
__device__ __forceinline__ float ft8s_tree64(float a)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h, 64);
    return __shfl(a, 0, 64);
}

__device__ __forceinline__ float ft8s_max4(float a, float b, float c, float d) { return fmaxf(fmaxf(a, b), fmaxf(c, d)); }

// bit metric t (0..173) from the wave's magnitude image: data symbol d = t / 3 (n = 7..35, 43..71), bit t % 3 of it, MSB first
__device__ __forceinline__ float ft8s_metric(const float *s8, int t)
{
    if (t >= FT8S_NBIT) return 0.0f;
    const int d = t / 3, bit = t - 3 * d;
    const int n = d + (d < 29 ? 7 : 14);
    const v4f lo = *reinterpret_cast<const v4f *>(s8 + 8 * n), hi = *reinterpret_cast<const v4f *>(s8 + 8 * n + 4);
    // s2[v] = s8[graymap[v]], graymap = 0,1,3,2,5,6,4,7
    const float s0 = lo.x, s1 = lo.y, s2 = lo.w, s3 = lo.z, s4 = hi.y, s5 = hi.z, s6 = hi.x, s7 = hi.w;
    if (bit == 0) return ft8s_max4(s4, s5, s6, s7) - ft8s_max4(s0, s1, s2, s3);
    if (bit == 1) return ft8s_max4(s2, s3, s6, s7) - ft8s_max4(s0, s1, s4, s5);
    return ft8s_max4(s1, s3, s5, s7) - ft8s_max4(s0, s2, s4, s6);
}

__global__ __launch_bounds__(64 * FT8S_WAVES) void ft8_softbits_kernel(const SyncWork *__restrict__ works, Ft8SoftRec *const *__restrict__ soft,
                                                                       int nbins, int maxcand)
{
    __shared__ __attribute__((aligned(16))) float s_mag[FT8S_WAVES][(FT8S_NSYM + 1) * 8];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = (int)blockIdx.x * FT8S_WAVES + wv;
    const SyncWork *w = works + blockIdx.y;
    const int ncand = min(*as_global(w->ncand), maxcand);
    if (q >= ncand) return;                                    // wave-uniform
    const CWSLG_GLOBAL SyncChannelBuffers::Cand *cd = as_global(w->cand) + q;
    const int i = cd->freq_bin, j = cd->time_step;
    const CWSLG_GLOBAL float *spec = as_global(w->spectra);
    float *s8 = s_mag[wv];

    // 20 passes of 4 symbols x 16 bins: lane = 16 (symbol within the pass) + bin offset; offset 15 is beyond tone 7 and is not fetched
    const int sub = lane >> 4, c = lane & 15;
    const int bin = i + c;
    const bool col_ok = c < 15 && bin >= 0 && bin <= FT8_NH1 && bin < nbins;
    float p[20];
#pragma unroll
    for (int ps = 0; ps < 20; ++ps) {
        const int n = 4 * ps + sub;
        const int m = j + 12 + 4 * n;                          // 1-based symbol step
        const bool ok = col_ok && n < FT8S_NSYM && m >= 1 && m <= FT8_NHSYM;
        // (an element outside the plane fetches element 0 and drops it: a load under a condition would be waited for on its own)
        const float v = spec[ok ? (size_t)(m - 1) * (size_t)nbins + (size_t)bin : (size_t)0];
        p[ps] = ok ? v : 0.0f;
    }
    if (!(c & 1) && c < 15) {
#pragma unroll
        for (int ps = 0; ps < 20; ++ps) s8[8 * (4 * ps + sub) + (c >> 1)] = sqrtf(p[ps]);
    }
    // the image is private to this wave, whose LDS operations complete in order: a compiler-level fence is all the hand-over needs
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // nsync: lanes 0..20 take one Costas symbol each; first maximum over the tones (ties to the lowest tone, Fortran maxloc)
    bool hit = false;
    if (lane < 21) {
        const int blk = lane / 7, r = lane - 7 * blk;
        const float *t = s8 + 8 * (36 * blk + r);
        int km = 0;
        float vm = t[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) if (t[k] > vm) { vm = t[k]; km = k; }
        const int icos7 = (0x2560413 >> (4 * r)) & 7;          // 3,1,4,0,6,5,2
        hit = km == icos7;
    }
    const int nsync = __popcll(__ballot(hit));

    // bmeta: lane l holds bits l, l + 64, l + 128
    const float b0 = ft8s_metric(s8, lane), b1 = ft8s_metric(s8, lane + 64), b2 = ft8s_metric(s8, lane + 128);
    // normalizebmet
    const float S1 = ft8s_tree64((b0 + b1) + b2);
    const float S2 = ft8s_tree64((b0 * b0 + b1 * b1) + b2 * b2);
    const float mean = S1 / 174.0f, m2 = S2 / 174.0f;
    const float var = m2 - mean * mean;
    const float sigma = sqrtf(var > 0.0f ? var : m2);
    CWSLG_GLOBAL Ft8SoftRec *out = as_global_rw(soft[blockIdx.y]) + q;
    const bool live = sigma != 0.0f;
    out->llr[lane] = live ? (b0 / sigma) * 2.83f : 0.0f;
    out->llr[lane + 64] = live ? (b1 / sigma) * 2.83f : 0.0f;
    if (lane + 128 < FT8S_NBIT) out->llr[lane + 128] = live ? (b2 / sigma) * 2.83f : 0.0f;
    if (lane == 0) { out->sigma = sigma; out->nsync = nsync; }
}

} // namespace cwslg
