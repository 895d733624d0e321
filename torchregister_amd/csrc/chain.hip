// Points and target-space images through the whole transform, both ways (include/trx.h: trx_transform_points, trx_affine_then_flow_resample;
// DESIGN.md section 4.20; extension, the reference moves no point and has no inverse).  CPU restatement: tests/chain_ref.py.
//
// Definitions.  Lattices S = (D, H, W), 2-D: D = 1.  Points and flows: voxel-index units, component a along spatial axis a (z, y, x / y, x).  theta: an
// EFFECTIVE theta [B][TRX_PSTRIDE] between normalised cubes, rows and columns x, y, z.  norm_a(p)_c = (2 p_c + 1) / S_a,c - 1 (af_norm) and
// unnorm_b(m)_r = ((m_r + 1) S_b,r - 1) / 2 (unnorm<ND>): trx_affine_flow_warp's closed forms, through affine_coord.  S(f, p): flow_sample.h, Sb
// (padding 1) or S0 (padding 0).  From a start lattice S_a to an end lattice S_b:
//   chain 0, flow then affine (flow on S_a):   p' = p + S(flow, p), one fp32 add per axis;  out = unnorm_b(theta (norm_a(p'), 1));  theta NULL: out = p'
//   chain 1, affine then flow (flow on S_b):   q = unnorm_b(theta (norm_a(p), 1)), theta NULL: q = p;  out = q + S(flow, q), flow NULL: out = q
//
//   transform_points_kernel<ND, CHAIN, PAD>         a thread per point, pairs on blockIdx.y.  A point is read before it is written, so out may be points.
//                                                   A non-finite component gives NaN in every component of that point and the thread ends before any
//                                                   index arithmetic.  A finite point however far away is safe: both flow samplers clamp in float.
//   affine_then_flow_resample_kernel<ND, ORDER, PAD> flow_compose_kernel's launch shape: a thread per OUTPUT voxel y of S_a, lanes along x, pairs on
//                                                   blockIdx.y.  Chain 1's position of y, then one sample of src (on S_b) for every channel: order 0 and
//                                                   3 are spl_sample_store (spline_sample.h, trx_transform_resample's body), order 1 is sample3 /
//                                                   sample2 (trx_common.h, trx_flow_warp's sampler) at the position clamped into [-2, S + 1] per axis -
//                                                   every finite position keeps its value (beyond -1 and S all corners lie outside), a NaN becomes -2: 0
//                                                   as in the other orders, and no unbounded float is converted to an index.  theta is read once per
//                                                   thread from uniform addresses (scalar loads); the flow and image gathers go through L1 / L2; out is a
//                                                   stream written once (non-temporal).  No LDS, no workspace, no atomics, no host sync.
#include <cmath>
#include <cstdint>

#include "flow_sample.h"
#include "spline_sample.h"

namespace trx {

// three ints as a kernel argument: D, H, W
struct ChainSize {
    int D, H, W;
};

// (x, y, z)-ordered coordinate under theta of the tensor-ordered position p on lattice a, un-normalised on lattice b
template <int ND>
__device__ __forceinline__ void chain_affine(const float (&te)[ND * (ND + 1)], const float (&p)[ND], ChainSize a, ChainSize b, float (&ic)[ND])
{
    const float xn = af_norm(p[ND - 1], a.W);
    const float yn = af_norm(p[ND - 2], a.H);
    float zn = 0.f;
    if constexpr (ND == 3) zn = af_norm(p[0], a.D);
    affine_coord<ND>(te, xn, yn, zn, b.D, b.H, b.W, ic);
}

// theta's row of a pair, ND (ND + 1) uniform floats
template <int ND>
__device__ __forceinline__ void chain_theta(const float *__restrict__ theta, int b, float (&te)[ND * (ND + 1)])
{
#pragma unroll
    for (int k = 0; k < ND * (ND + 1); k++) te[k] = theta ? theta[(size_t)b * TRX_PSTRIDE + k] : 0.f;
}

// points / out [B][P][ND]; they may be the same buffer: no __restrict__ on them.  sa: the start lattice, sb: the end lattice.
template <int ND, int CHAIN, int PAD>
__global__ __launch_bounds__(TRX_BLOCK) void transform_points_kernel(const float *points, float *out, unsigned P, const float *__restrict__ theta,
                                                                     const float *__restrict__ flow, ChainSize sa, ChainSize sb)
{
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= P) return;
    const int b = blockIdx.y;
    const size_t at = ((size_t)b * P + i) * ND;
    float te[ND * (ND + 1)];
    chain_theta<ND>(theta, b, te);
    float p[ND];
    bool finite = true;
#pragma unroll
    for (int c = 0; c < ND; c++) {
        p[c] = points[at + c];
        finite = finite && std::isfinite(p[c]);
    }
    if (!finite) {
#pragma unroll
        for (int c = 0; c < ND; c++) out[at + c] = __uint_as_float(0x7fc00000u);
        return;
    }
    const ChainSize sf = CHAIN == 0 ? sa : sb;      // the lattice the flow lives on
    const unsigned N = (unsigned)sf.D * (unsigned)sf.H * (unsigned)sf.W;
    const float *__restrict__ u = flow ? flow + (size_t)b * ND * N : nullptr;
    float s[ND], ic[ND];
    if constexpr (CHAIN == 0) {
        if (u) {
            flo_sample_at<ND, PAD>(u, N, sf.D, sf.H, sf.W, p, s);
#pragma unroll
            for (int c = 0; c < ND; c++) p[c] = p[c] + s[c];
        }
        if (theta) {
            chain_affine<ND>(te, p, sa, sb, ic);
#pragma unroll
            for (int c = 0; c < ND; c++) p[c] = ic[ND - 1 - c];
        }
    } else {
        if (theta) {
            chain_affine<ND>(te, p, sa, sb, ic);
#pragma unroll
            for (int c = 0; c < ND; c++) p[c] = ic[ND - 1 - c];
        }
        if (u) {
            flo_sample_at<ND, PAD>(u, N, sf.D, sf.H, sf.W, p, s);
#pragma unroll
            for (int c = 0; c < ND; c++) p[c] = p[c] + s[c];
        }
    }
#pragma unroll
    for (int c = 0; c < ND; c++) out[at + c] = p[c];
}

// out [B][channels][*so] = src [B][channels][*ss] (src_stride elements between pairs) sampled at chain 1's position of every voxel of so; the flow
// lives on ss.  theta NULL: so == ss and q = the voxel's own index.
template <int ND, int ORDER, int PAD>
__global__ __launch_bounds__(TRX_BLOCK) void affine_then_flow_resample_kernel(const float *__restrict__ src, size_t src_stride, ChainSize ss,
                                                                              const float *__restrict__ theta, const float *__restrict__ flow, int channels,
                                                                              ChainSize so, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const unsigned nout = (unsigned)so.D * (unsigned)so.H * (unsigned)so.W, nsrc = (unsigned)ss.D * (unsigned)ss.H * (unsigned)ss.W;
    float te[ND * (ND + 1)];
    chain_theta<ND>(theta, b, te);
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= nout) return;
    int x[3];
    svf_coords<ND>(i, so.H, so.W, x);
    float q[ND], ic[ND];      // q: tensor order (the flow's); ic: x, y(, z) (the samplers')
#pragma unroll
    for (int c = 0; c < ND; c++) q[c] = (float)x[3 - ND + c];
    if (theta) {
        chain_affine<ND>(te, q, so, ss, ic);
    } else {
#pragma unroll
        for (int c = 0; c < ND; c++) ic[c] = q[ND - 1 - c];
    }
    if (flow) {
        float s[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) q[c] = ic[ND - 1 - c];
        flo_sample_at<ND, PAD>(flow + (size_t)b * ND * nsrc, nsrc, ss.D, ss.H, ss.W, q, s);
#pragma unroll
        for (int c = 0; c < ND; c++) ic[c] = q[ND - 1 - c] + s[ND - 1 - c];
    }
    const float *__restrict__ m = src + (size_t)b * src_stride;
    float *__restrict__ o = out + (size_t)b * channels * nout + i;
    const int S[3] = {ss.W, ss.H, ss.D};      // x, y, z: the order of the coordinate
    if constexpr (ORDER == 1) {
#pragma unroll
        for (int a = 0; a < ND; a++) ic[a] = fminf(fmaxf(ic[a], -2.f), (float)S[a] + 1.f);      // a NaN becomes -2: every corner outside
        for (int ch = 0; ch < channels; ch++) {
            float v;
            if constexpr (ND == 3) v = sample3(m + (size_t)ch * nsrc, ss.D, ss.H, ss.W, ic[0], ic[1], ic[2]).v;
            else v = sample2(m + (size_t)ch * nsrc, ss.H, ss.W, ic[0], ic[1]).v;
            __builtin_nontemporal_store(v, o + (size_t)ch * nout);
        }
    } else {
        spl_sample_store<ND, ORDER>(m, nsrc, channels, ic, S, o, nout);
    }
}

// [host] a lattice of the entry points: status of its sizes
static int chain_size(int ndim, const int *s)
{
    if (!s) return TRX_ERR_ARG;
    if (ndim == 2 && s[0] != 1) return TRX_ERR_NDIM;
    if (s[0] < 1 || s[1] < 1 || s[2] < 1) return TRX_ERR_ARG;
    if ((double)s[0] * s[1] * s[2] >= 2147483648.0) return TRX_ERR_ARG;
    return TRX_OK;
}

// [host] whether [a, a + na) and [b, b + nb) share a byte
static bool chain_overlap(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

template <int ND, int CHAIN>
static void points_launch(int padding, dim3 grid, hipStream_t s, const float *points, float *out, unsigned P, const float *theta, const float *flow, ChainSize sa,
                          ChainSize sb)
{
    if (padding) hipLaunchKernelGGL((transform_points_kernel<ND, CHAIN, 1>), grid, dim3(TRX_BLOCK), 0, s, points, out, P, theta, flow, sa, sb);
    else hipLaunchKernelGGL((transform_points_kernel<ND, CHAIN, 0>), grid, dim3(TRX_BLOCK), 0, s, points, out, P, theta, flow, sa, sb);
}

template <int ND, int ORDER>
static void resample_launch(int padding, dim3 grid, hipStream_t s, const float *src, size_t src_stride, ChainSize ss, const float *theta, const float *flow,
                            int channels, ChainSize so, float *out)
{
    if (padding)
        hipLaunchKernelGGL((affine_then_flow_resample_kernel<ND, ORDER, 1>), grid, dim3(TRX_BLOCK), 0, s, src, src_stride, ss, theta, flow, channels, so, out);
    else
        hipLaunchKernelGGL((affine_then_flow_resample_kernel<ND, ORDER, 0>), grid, dim3(TRX_BLOCK), 0, s, src, src_stride, ss, theta, flow, channels, so, out);
}

}  // namespace trx

using namespace trx;

extern "C" int trx_transform_points(const float *points, float *out, int ndim, int B, int P, const float *theta, const float *flow, const int *from_size,
                                    const int *to_size, int chain, int padding, void *stream)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (!points || !out || (!theta && !flow)) return TRX_ERR_ARG;
    if (chain != 0 && chain != 1) return TRX_ERR_ARG;
    int rc = chain_size(ndim, from_size);
    if (rc != TRX_OK) return rc;
    const bool reads_to = theta || chain == 1;      // chain 0 without theta ends on the start lattice: to_size is not read
    if (reads_to) {
        rc = chain_size(ndim, to_size);
        if (rc != TRX_OK) return rc;
        if (!theta && (from_size[0] != to_size[0] || from_size[1] != to_size[1] || from_size[2] != to_size[2])) return TRX_ERR_ARG;
    }
    if (B < 1 || B > 65535 || P < 1) return TRX_ERR_ARG;
    if (padding != 0 && padding != 1) return TRX_ERR_ARG;
    const ChainSize sa = {from_size[0], from_size[1], from_size[2]};
    const ChainSize sb = reads_to ? ChainSize{to_size[0], to_size[1], to_size[2]} : sa;
    const size_t bytes = (size_t)B * (size_t)P * (size_t)ndim * sizeof(float);
    if (out != points && chain_overlap(out, bytes, points, bytes)) return TRX_ERR_ARG;
    if (flow) {
        const ChainSize sf = chain == 0 ? sa : sb;
        if (chain_overlap(out, bytes, flow, (size_t)B * ndim * sf.D * sf.H * sf.W * sizeof(float))) return TRX_ERR_ARG;
    }
    const dim3 grid(((unsigned)P + TRX_BLOCK - 1) / TRX_BLOCK, (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (ndim == 3) {
        if (chain == 0) points_launch<3, 0>(padding, grid, s, points, out, (unsigned)P, theta, flow, sa, sb);
        else points_launch<3, 1>(padding, grid, s, points, out, (unsigned)P, theta, flow, sa, sb);
    } else {
        if (chain == 0) points_launch<2, 0>(padding, grid, s, points, out, (unsigned)P, theta, flow, sa, sb);
        else points_launch<2, 1>(padding, grid, s, points, out, (unsigned)P, theta, flow, sa, sb);
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_affine_then_flow_resample(const float *src, size_t src_stride, const int *src_size, const float *theta, const float *flow, int ndim, int B,
                                             int channels, const int *out_size, int order, int padding, float *out, void *stream)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (!src || !out || (!theta && !flow)) return TRX_ERR_ARG;
    int rc = chain_size(ndim, src_size);
    if (rc == TRX_OK) rc = chain_size(ndim, out_size);
    if (rc != TRX_OK) return rc;
    if (!theta && (src_size[0] != out_size[0] || src_size[1] != out_size[1] || src_size[2] != out_size[2])) return TRX_ERR_ARG;
    if (B < 1 || B > 65535 || channels < 1) return TRX_ERR_ARG;
    if (order != 0 && order != 1 && order != 3) return TRX_ERR_ARG;
    if (padding != 0 && padding != 1) return TRX_ERR_ARG;
    const ChainSize ss = {src_size[0], src_size[1], src_size[2]}, so = {out_size[0], out_size[1], out_size[2]};
    const size_t nsrc = (size_t)ss.D * ss.H * ss.W, nout = (size_t)so.D * so.H * so.W;
    if (src_stride < (size_t)channels * nsrc) return TRX_ERR_ARG;
    const size_t out_bytes = (size_t)B * channels * nout * sizeof(float);
    if (chain_overlap(out, out_bytes, src, ((size_t)(B - 1) * src_stride + (size_t)channels * nsrc) * sizeof(float))) return TRX_ERR_ARG;
    if (flow && chain_overlap(out, out_bytes, flow, (size_t)B * ndim * nsrc * sizeof(float))) return TRX_ERR_ARG;
    const dim3 grid((unsigned)((nout + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    if (ndim == 3) {
        if (order == 0) resample_launch<3, 0>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
        else if (order == 1) resample_launch<3, 1>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
        else resample_launch<3, 3>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
    } else {
        if (order == 0) resample_launch<2, 0>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
        else if (order == 1) resample_launch<2, 1>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
        else resample_launch<2, 3>(padding, grid, s, src, src_stride, ss, theta, flow, channels, so, out);
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
