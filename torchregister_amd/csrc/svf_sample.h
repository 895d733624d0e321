// The position / corner arithmetic of the dense-field sampler S(f, p) (include/trx.h: corners outside the volume contribute zero), shared by svf.hip
// (scaling and squaring, its adjoint) and flowops.hip (composition with zero padding): one statement, so that compose(u, u) gives the bits of one squaring.
#pragma once
#include "trx_common.h"

namespace trx {

// The two corners of one axis for the position p = index + displacement: indices (clamped into the axis for addressing), whether each
// lies inside, and t.  A position outside (-2, S + 1) - or NaN - has no corner inside; its index arithmetic is not done.
struct SvfAxis {
    int i0, c[2];
    bool ok[2];
    float t;
};

__device__ __forceinline__ SvfAxis svf_axis(float p, int S)
{
    SvfAxis a;
    const bool near = p > -2.f && p < (float)S + 1.f;
    const float pc = near ? p : -2.f, f = floorf(pc);
    a.i0 = (int)f;
    a.t = pc - f;
    a.ok[0] = (unsigned)a.i0 < (unsigned)S;
    a.ok[1] = (unsigned)(a.i0 + 1) < (unsigned)S;
    a.c[0] = min(max(a.i0, 0), S - 1);
    a.c[1] = min(max(a.i0 + 1, 0), S - 1);
    return a;
}

// voxel i of a [D][H][W] volume -> (z, y, x) (2-D: z = 0)
template <int ND> __device__ __forceinline__ void svf_coords(unsigned i, int H, int W, int (&x)[3])
{
    const unsigned r = i / (unsigned)W;
    x[2] = (int)(i - r * (unsigned)W);
    if constexpr (ND == 3) {
        x[0] = (int)(r / (unsigned)H);
        x[1] = (int)(r - (unsigned)x[0] * (unsigned)H);
    } else {
        x[0] = 0;
        x[1] = (int)r;
    }
}

// The axes of the sample at the float position p (channel order of `flow`: 3-D z, y, x; 2-D y, x), in slots 3 - ND .. 2
template <int ND> __device__ __forceinline__ void svf_axes_at(const float (&p)[ND], int D, int H, int W, SvfAxis (&ax)[3])
{
    const int S[3] = {D, H, W};
    if constexpr (ND == 2) {
        ax[0].i0 = 0; ax[0].c[0] = ax[0].c[1] = 0; ax[0].ok[0] = true; ax[0].ok[1] = false; ax[0].t = 0.f;
    }
#pragma unroll
    for (int a = 3 - ND; a < 3; a++) ax[a] = svf_axis(p[a - (3 - ND)], S[a]);
}

// ... at voxel x displaced by u: the position is ONE fp32 add per axis
template <int ND> __device__ __forceinline__ void svf_axes(const int (&x)[3], const float (&u)[ND], int D, int H, int W, SvfAxis (&ax)[3])
{
    float p[ND];
#pragma unroll
    for (int a = 3 - ND; a < 3; a++) p[a - (3 - ND)] = (float)x[a] + u[a - (3 - ND)];
    svf_axes_at<ND>(p, D, H, W, ax);
}

}  // namespace trx
