// Composition and fixed-point inversion of dense flows (include/trx.h: trx_flow_compose, trx_flow_invert; extension, the
// reference has neither).  CPU restatement: tests/flowops_ref.py.
//
// Definition: fields [B][nd][D][H][W] fp32 in voxels, channel a along spatial axis a; a warp is warped(x) = image(x + flow(x)); a position is ONE fp32
// add of the voxel index and the displacement.  S0(f, p) is svf.hip's sampler (svf_sample.h: corners outside the volume contribute zero); Sb(f, p) is
// border extension, per axis pc = min(max(p, 0), S - 1), i0 = min(floor(pc), max(S - 2, 0)), t = pc - i0, corners i0 and min(i0 + 1, S - 1): continuous
// in p with the Lipschitz constant of f, which the fixed-point iteration needs at the faces (S0 ramps to zero over one voxel there).  Both samplers
// live in flow_sample.h, which chain.hip shares.
//   compose   c(x) = second(x) + S(first, x + second(x)), S = Sb (padding 1) or S0 (padding 0).  With S0, compose(u, u) is svf_square_kernel's
//             arithmetic statement for statement: the bits of trx_svf_exp(2u, squarings = 1).
//   invert    v_0 = init or 0; v_{k+1}(y) = -Sb(u, y + v_k(y)); r = max_a |v_{k+1,a} - v_{k,a}|; the voxel stops after the first update with r <= tol
//             or after `iterations` updates; residual(y) = the r of its last update.  A non-finite v_k or sample ends the voxel with NaN in every
//             channel of v and in residual.
//
//   flow_compose_kernel<ND, PAD>   svf_square_kernel's launch shape: a thread per voxel, lanes along x, pairs on blockIdx.y.  It reads second(x) and
//                                  gathers 2^nd corners of nd channels of `first`; `second` is read at the voxel's own index only, so out may be second.
//   flow_invert_kernel<ND>         the same shape.  The whole iteration of a voxel stays in registers: v (nd floats), the voxel's index triple and r; every
//                                  update gathers 2^nd nd floats of u through L1 / L2 - all indices clamped, no load predicated - and a lane leaves the loop
//                                  when it has converged (a wave runs as long as its slowest lane).  One store of v and one of residual; no workspace,
//                                  no atomics, nothing shared between voxels: a voxel's result depends on u and its own init alone.
#include "flow_sample.h"

#include <cmath>

namespace trx {

// c(x) = second(x) + S(first, x + second(x)); pairs along blockIdx.y.  second and out may be the same buffer: no __restrict__ on them.
template <int ND, int PAD>
__global__ __launch_bounds__(TRX_BLOCK) void flow_compose_kernel(const float *__restrict__ first, const float *second, float *out, unsigned N, int D, int H, int W)
{
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float *u = first + (size_t)blockIdx.y * ND * N;
    const float *s = second + (size_t)blockIdx.y * ND * N;
    float *o = out + (size_t)blockIdx.y * ND * N;
    int x[3];
    svf_coords<ND>(i, H, W, x);
    float ux[ND], acc[ND];
#pragma unroll
    for (int c = 0; c < ND; c++) ux[c] = s[(size_t)c * N + i];
    if constexpr (PAD == 0) {      // svf_square_kernel's body with two fields
        SvfAxis ax[3];
        svf_axes<ND>(x, ux, D, H, W, ax);
        flo_sample_zeros_axes<ND>(u, N, H, W, ax, acc);
    } else {
        flo_sample_border<ND>(u, N, D, H, W, x, ux, acc);
    }
#pragma unroll
    for (int c = 0; c < ND; c++) o[(size_t)c * N + i] = ux[c] + acc[c];
}

// v(y) = the fixed point of v <- -Sb(u, y + v), all updates of a voxel in registers; init and inverse may be the same buffer (a voxel reads its own
// init before it writes): no __restrict__ on them.
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void flow_invert_kernel(const float *__restrict__ flow, const float *init, float *inverse, float *__restrict__ residual,
                                                                 unsigned N, int D, int H, int W, int iterations, float tol)
{
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float *u = flow + (size_t)blockIdx.y * ND * N;
    int x[3];
    svf_coords<ND>(i, H, W, x);
    float v[ND];
#pragma unroll
    for (int c = 0; c < ND; c++) v[c] = init ? init[((size_t)blockIdx.y * ND + c) * N + i] : 0.f;
    float r = 0.f;
    for (int k = 0; k < iterations; k++) {
        float s[ND];
        flo_sample_border<ND>(u, N, D, H, W, x, v, s);
        bool finite = true;
        float rk = 0.f;
#pragma unroll
        for (int c = 0; c < ND; c++) {
            const float vn = -s[c];
            finite = finite && std::isfinite(v[c]) && std::isfinite(vn);
            rk = fmaxf(rk, fabsf(vn - v[c]));
            v[c] = vn;
        }
        if (!finite) {
            r = __uint_as_float(0x7fc00000u);
#pragma unroll
            for (int c = 0; c < ND; c++) v[c] = r;
            break;
        }
        r = rk;
        if (r <= tol) break;
    }
    float *o = inverse + (size_t)blockIdx.y * ND * N;
#pragma unroll
    for (int c = 0; c < ND; c++) o[(size_t)c * N + i] = v[c];
    if (residual) residual[(size_t)blockIdx.y * N + i] = r;
}

// ndim, B, D, H, W -> status; the sizes trx_svf_exp accepts (B <= 65535 pairs on blockIdx.y, at most 2^31 voxels per volume)
static int flowops_geom(int ndim, int B, int D, int H, int W)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1) return TRX_ERR_ARG;
    if ((double)D * H * W > 2147483648.0) return TRX_ERR_ARG;
    return TRX_OK;
}

template <int ND, int PAD>
static int flow_compose_launch(const float *first, const float *second, float *out, int B, int D, int H, int W, hipStream_t s)
{
    const size_t N = (size_t)D * H * W;
    const dim3 grid((unsigned)((N + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)B);
    hipLaunchKernelGGL((flow_compose_kernel<ND, PAD>), grid, dim3(TRX_BLOCK), 0, s, first, second, out, (unsigned)N, D, H, W);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <int ND>
static int flow_invert_launch(const float *flow, const float *init, float *inverse, float *residual, int B, int D, int H, int W, int iterations, float tol,
                              hipStream_t s)
{
    const size_t N = (size_t)D * H * W;
    const dim3 grid((unsigned)((N + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)B);
    hipLaunchKernelGGL((flow_invert_kernel<ND>), grid, dim3(TRX_BLOCK), 0, s, flow, init, inverse, residual, (unsigned)N, D, H, W, iterations, tol);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" int trx_flow_compose(const float *first, const float *second, float *out, int ndim, int B, int D, int H, int W, int padding, void *stream)
{
    if (!first || !second || !out || out == first) return TRX_ERR_ARG;
    const int rc = flowops_geom(ndim, B, D, H, W);
    if (rc != TRX_OK) return rc;
    if (padding != 0 && padding != 1) return TRX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (ndim == 3) return padding ? flow_compose_launch<3, 1>(first, second, out, B, D, H, W, s) : flow_compose_launch<3, 0>(first, second, out, B, D, H, W, s);
    return padding ? flow_compose_launch<2, 1>(first, second, out, B, D, H, W, s) : flow_compose_launch<2, 0>(first, second, out, B, D, H, W, s);
}

extern "C" int trx_flow_invert(const float *flow, const float *init, float *inverse, float *residual, int ndim, int B, int D, int H, int W, int iterations,
                               float tol, void *stream)
{
    if (!flow || !inverse || inverse == flow) return TRX_ERR_ARG;
    const int rc = flowops_geom(ndim, B, D, H, W);
    if (rc != TRX_OK) return rc;
    if (iterations < 1 || iterations > 1000 || !std::isfinite(tol) || tol < 0.f) return TRX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    return ndim == 3 ? flow_invert_launch<3>(flow, init, inverse, residual, B, D, H, W, iterations, tol, s)
                     : flow_invert_launch<2>(flow, init, inverse, residual, B, D, H, W, iterations, tol, s);
}
