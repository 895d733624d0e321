// A dense flow sampled at a float position, S(f, p) (include/trx.h: trx_flow_compose's two samplers), shared by flowops.hip (composition, inversion) and
// chain.hip (points and target-space images through the whole transform): one statement of each, so that the users agree bit for bit.
//   Sb  border extension (padding 1): per axis pc = min(max(p, 0), S - 1), i0 = min(floor(pc), max(S - 2, 0)), t = pc - i0, corners i0 and
//       min(i0 + 1, S - 1).  Every index is clamped into its axis in float, before the conversion to int: no position forms an address outside f.
//   S0  zero padding (padding 0): svf_sample.h's corners; one outside the volume contributes zero and its (clamped) address is not read.
// The weight of a corner is (y-factor * x-factor) * z-factor, the corners are added z, y, x with x fastest, nd channels per corner.
#pragma once
#include "svf_sample.h"

namespace trx {

// Border extension on one axis: the two corner indices (both inside the axis, whatever p) and t.  A NaN position takes the first voxel; the kernels
// that must tell (the inversion, the point transform) test their values for finiteness themselves.
__device__ __forceinline__ void flo_axis(float p, int S, int (&c)[2], float &t)
{
    const float pc = fminf(fmaxf(p, 0.f), (float)(S - 1));
    c[0] = min((int)floorf(pc), max(S - 2, 0));
    t = pc - (float)c[0];
    c[1] = min(c[0] + 1, S - 1);
}

// acc = Sb(f, p) for the nd channels of f (p in the flow's channel order: 3-D z, y, x; 2-D y, x)
template <int ND>
__device__ __forceinline__ void flo_sample_border_at(const float *__restrict__ f, unsigned N, int D, int H, int W, const float (&p)[ND], float (&acc)[ND])
{
    const int S[3] = {D, H, W};
    int c[3][2];
    float t[3];
    c[0][0] = c[0][1] = 0;
    t[0] = 0.f;
#pragma unroll
    for (int a = 3 - ND; a < 3; a++) flo_axis(p[a - (3 - ND)], S[a], c[a], t[a]);
#pragma unroll
    for (int ch = 0; ch < ND; ch++) acc[ch] = 0.f;
#pragma unroll
    for (int kz = 0; kz < (ND == 3 ? 2 : 1); kz++)
#pragma unroll
        for (int ky = 0; ky < 2; ky++)
#pragma unroll
            for (int kx = 0; kx < 2; kx++) {
                float w = (ky ? t[1] : 1.f - t[1]) * (kx ? t[2] : 1.f - t[2]);
                if constexpr (ND == 3) w *= kz ? t[0] : 1.f - t[0];
                const size_t off = ((size_t)c[0][kz] * H + c[1][ky]) * W + c[2][kx];
#pragma unroll
                for (int ch = 0; ch < ND; ch++) acc[ch] = fmaf(w, f[(size_t)ch * N + off], acc[ch]);
            }
}

// acc = Sb(f, x + d): the position is ONE fp32 add of the voxel index and the displacement per axis
template <int ND>
__device__ __forceinline__ void flo_sample_border(const float *__restrict__ f, unsigned N, int D, int H, int W, const int (&x)[3], const float (&d)[ND],
                                                  float (&acc)[ND])
{
    float p[ND];
#pragma unroll
    for (int a = 3 - ND; a < 3; a++) p[a - (3 - ND)] = (float)x[a] + d[a - (3 - ND)];
    flo_sample_border_at<ND>(f, N, D, H, W, p, acc);
}

// acc = S0(f, .) over the corners of `ax` (svf_axes / svf_axes_at): svf_square_kernel's arithmetic, statement for statement
template <int ND>
__device__ __forceinline__ void flo_sample_zeros_axes(const float *__restrict__ f, unsigned N, int H, int W, const SvfAxis (&ax)[3], float (&acc)[ND])
{
#pragma unroll
    for (int c = 0; c < ND; c++) acc[c] = 0.f;
#pragma unroll
    for (int kz = 0; kz < (ND == 3 ? 2 : 1); kz++)
#pragma unroll
        for (int ky = 0; ky < 2; ky++)
#pragma unroll
            for (int kx = 0; kx < 2; kx++) {
                const bool ok = ax[0].ok[kz] & ax[1].ok[ky] & ax[2].ok[kx];
                float w = (ky ? ax[1].t : 1.f - ax[1].t) * (kx ? ax[2].t : 1.f - ax[2].t);
                if constexpr (ND == 3) w *= kz ? ax[0].t : 1.f - ax[0].t;
                const size_t off = ((size_t)ax[0].c[kz] * H + ax[1].c[ky]) * W + ax[2].c[kx];
#pragma unroll
                for (int c = 0; c < ND; c++) acc[c] = fmaf(w, ok ? f[(size_t)c * N + off] : 0.f, acc[c]);
            }
}

// acc = S(f, p) at a float position: PAD 1 Sb, PAD 0 S0
template <int ND, int PAD>
__device__ __forceinline__ void flo_sample_at(const float *__restrict__ f, unsigned N, int D, int H, int W, const float (&p)[ND], float (&acc)[ND])
{
    if constexpr (PAD == 0) {
        SvfAxis ax[3];
        svf_axes_at<ND>(p, D, H, W, ax);
        flo_sample_zeros_axes<ND>(f, N, H, W, ax, acc);
    } else {
        flo_sample_border_at<ND>(f, N, D, H, W, p, acc);
    }
}

}  // namespace trx
