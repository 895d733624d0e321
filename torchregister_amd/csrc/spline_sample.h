// The order 0 and order 3 samplers of the resampling kernels (include/trx.h: trx_transform_resample), shared by spline.hip (flow first, then the affine) and
// chain.hip (the affine first, then a flow): one body, so that the two chain orders agree bit for bit wherever their positions do.
#pragma once
#include "trx_common.h"

namespace trx {

// whole-sample mirror of any index into 0 .. n-1
__device__ __forceinline__ int spl_mirror(long long k, int n)
{
    if ((unsigned long long)k < (unsigned long long)n) return (int)k;
    if (n == 1) return 0;
    const long long top = 2LL * (n - 1);
    while (k < 0 || k >= n) k = k < 0 ? -k : top - k;
    return (int)k;
}

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // a 4-byte aligned quad: one global_load_dwordx4 at any voxel

// The tensor-product sum of one channel over the 4^ND taps: x innermost, then y, then z.  RUN: the x taps are idx[0][0] .. idx[0][0] + 3.
template <int ND, bool RUN>
__device__ __forceinline__ float spl_taps(const float *__restrict__ m, const int (&idx)[ND][4], const float (&w)[ND][4], int H, int W)
{
    float acc = 0.f;
#pragma unroll
    for (int kz = 0; kz < (ND == 3 ? 4 : 1); kz++) {
        float az = 0.f;
#pragma unroll
        for (int ky = 0; ky < 4; ky++) {
            const float *__restrict__ r = m + ((size_t)(ND == 3 ? idx[ND - 1][kz] : 0) * H + idx[1][ky]) * W;
            float c[4];
            if constexpr (RUN) {
                const f4u q = *(const f4u *)(r + idx[0][0]);
                c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w;
            } else {
#pragma unroll
                for (int kx = 0; kx < 4; kx++) c[kx] = r[idx[0][kx]];
            }
            float ax = w[0][0] * c[0];
#pragma unroll
            for (int kx = 1; kx < 4; kx++) ax = fmaf(w[0][kx], c[kx], ax);
            az = fmaf(w[1][ky], ax, az);
        }
        acc = ND == 3 ? fmaf(w[ND - 1][kz], az, acc) : az;
    }
    return acc;
}

// One output voxel of `channels` channels from its sample position ic (x, y(, z) order, voxels of the sampled lattice S = (W, H, D)): mov = the pair's
// first channel, chan_stride sampled voxels between channels, o = the voxel's slot in channel 0 of the output, nvox output voxels between channels.
// ORDER 0: mov[rint(ic)] per axis, half to even, 0 where a rounded index lies outside (the index is converted only once it is known to lie inside).
// ORDER 3: mov holds the coefficients; 0 where ic_a < -0.5 or ic_a > S_a - 0.5 on some axis, so floor(ic) is -1 .. S - 1 where it is converted.
// A NaN position compares false everywhere: 0 in both orders, and no address is formed from it.
template <int ND, int ORDER>
__device__ __forceinline__ void spl_sample_store(const float *__restrict__ mov, size_t chan_stride, int channels, const float (&ic)[ND], const int (&S)[3],
                                                 float *__restrict__ o, size_t nvox)
{
    if constexpr (ORDER == 0) {
        bool in = true;
        size_t src = 0;
#pragma unroll
        for (int a = ND - 1; a >= 0; a--) {
            const float r = rintf(ic[a]);
            in = in && (r >= 0.f) && (r < (float)S[a]);      // NaN compares false: zeros
            src = src * (size_t)S[a] + (size_t)(in ? (int)r : 0);
        }
        for (int ch = 0; ch < channels; ch++) __builtin_nontemporal_store(in ? mov[ch * chan_stride + src] : 0.f, o + ch * nvox);
    } else {
        bool in = true;
#pragma unroll
        for (int a = 0; a < ND; a++) in = in && (ic[a] >= -0.5f) && (ic[a] <= (float)S[a] - 0.5f);      // NaN: outside
        if (!in) {
            for (int ch = 0; ch < channels; ch++) __builtin_nontemporal_store(0.f, o + ch * nvox);
            return;
        }
        float w[ND][4];
        int idx[ND][4];
#pragma unroll
        for (int a = 0; a < ND; a++) {
            const float fl = floorf(ic[a]);
            const float r = ic[a] - fl, r2 = r * r, r3 = r2 * r, u = 1.f - r;
            const int i0 = (int)fl;                          // -1 .. S - 1 inside the field of view
            w[a][0] = u * u * u * (1.f / 6.f);
            w[a][1] = (3.f * r3 - 6.f * r2 + 4.f) * (1.f / 6.f);
            w[a][2] = (-3.f * r3 + 3.f * r2 + 3.f * r + 1.f) * (1.f / 6.f);
            w[a][3] = r3 * (1.f / 6.f);
#pragma unroll
            for (int k = 0; k < 4; k++) idx[a][k] = spl_mirror((long long)i0 - 1 + k, S[a]);
        }
        const bool run = idx[0][3] - idx[0][0] == 3;      // the four x taps are neighbours in memory (no mirror along x): one 16-byte load per row
        for (int ch = 0; ch < channels; ch++) {
            const float *__restrict__ m = mov + ch * chan_stride;
            const float acc = run ? spl_taps<ND, true>(m, idx, w, S[1], S[0]) : spl_taps<ND, false>(m, idx, w, S[1], S[0]);
            __builtin_nontemporal_store(acc, o + ch * nvox);
        }
    }
}

}  // namespace trx
