// Jacobian determinant of a dense flow and the folding penalty on it (include/trx.h: trx_flow_jacobian, trx_flow_folding; DESIGN.md section 4.18;
// extension, the reference has neither).  CPU restatement: tests/jacobian_ref.py.
//
// Definition: flow [B][nd][D][H][W] in voxels, channel a along spatial axis a.  D_b u is the central difference along axis b, one-sided on the first
// and the last voxel of the axis, 0 on an axis of one voxel - written once, in jac_at, as sc (u(min(i + 1, S - 1)) - u(max(i - 1, 0))) with sc = 1/2
// where both neighbours exist and 1 elsewhere: every index is clamped, no load is predicated.  J[a][b] = delta_ab + D_b u_a, det = det J,
// P_b = (1 / N) sum_x max(0, eps - det(x))^2.
//
//   jac_map_kernel<ND, false>   trx_flow_jacobian: a block takes kFoldChunk consecutive voxels of one pair, lanes along x (VoxelWalk), 2 nd^2 loads per
//                               voxel of which the y and z neighbours are cache hits of the rows around; one store.
//   jac_map_kernel<ND, true>    the same with the hinge: h = eps - det where det < eps, h^2 added in fp64 in ascending voxels per thread, a fixed shuffle
//                               tree per wave and the four waves in order -> one fp64 partial per block.
//   fold_reduce_kernel          one wave per pair sums its partials in a fixed order -> penalty[b].
//   fold_backward_kernel        gather: voxel y reads det at its 2 nd stencil neighbours (the clamped index names the voxel itself on a face, where the
//                               one-sided difference has a term of its own) and only where det < eps forms that neighbour's J and the column of its
//                               cofactor matrix; dflow[a](y) (+)= -(2 weight / N) sum_b sum_{n in {lower, upper}} c_b(n, y) h(n) cof J(n)[a][b], with
//                               c_b the coefficient of u(y) in (D_b u)(n).  A voxel without an active neighbour costs 2 nd cached loads and nd stores
//                               (nd loads more when it accumulates); a block whose reach holds no active voxel at all - every partial sum it touches
//                               is exactly 0 - costs those few doubles and, accumulating, nothing else.
// No atomics, every sum in a fixed order: the same bits on every call, and a pair's result does not depend on the batch around it.
#include "jacobian.h"

#include <cmath>

namespace trx {

// J at the voxel with linear index c and per-axis indices i (channel / axis order: z, y, x; 2-D: y, x)
template <int ND>
__device__ __forceinline__ void jac_at(const float *__restrict__ f, unsigned nvox, unsigned c, const int (&i)[ND], const int (&S)[ND], const unsigned (&st)[ND],
                                       float (&J)[ND][ND])
{
#pragma unroll
    for (int b = 0; b < ND; b++) {
        const int ip = min(i[b] + 1, S[b] - 1), im = max(i[b] - 1, 0);
        const float sc = ip - im == 2 ? 0.5f : 1.0f;
        const unsigned op = c + (unsigned)(ip - i[b]) * st[b], om = c - (unsigned)(i[b] - im) * st[b];
#pragma unroll
        for (int a = 0; a < ND; a++) J[a][b] = fmaf(sc, f[(size_t)a * nvox + op] - f[(size_t)a * nvox + om], a == b ? 1.0f : 0.0f);
    }
}

// d det / d J[a][b]
template <int ND>
__device__ __forceinline__ float jac_cof(const float (&J)[ND][ND], int a, int b)
{
    if constexpr (ND == 3) {
        const int a1 = (a + 1) % 3, a2 = (a + 2) % 3, b1 = (b + 1) % 3, b2 = (b + 2) % 3;
        return J[a1][b1] * J[a2][b2] - J[a1][b2] * J[a2][b1];
    } else {
        return a == b ? J[1 - a][1 - b] : -J[1 - a][1 - b];
    }
}

template <int ND>
__device__ __forceinline__ float jac_det(const float (&J)[ND][ND])
{
    if constexpr (ND == 3) return fmaf(J[0][0], jac_cof<3>(J, 0, 0), fmaf(J[0][1], jac_cof<3>(J, 0, 1), J[0][2] * jac_cof<3>(J, 0, 2)));
    else return J[0][0] * J[1][1] - J[0][1] * J[1][0];
}

template <int ND>
__device__ __forceinline__ void jac_sizes(int D, int H, int W, int (&S)[ND], unsigned (&st)[ND])
{
    if constexpr (ND == 3) {
        S[0] = D; S[1] = H; S[2] = W;
        st[0] = (unsigned)H * (unsigned)W; st[1] = (unsigned)W; st[2] = 1u;
    } else {
        S[0] = H; S[1] = W;
        st[0] = (unsigned)W; st[1] = 1u;
    }
}

template <int ND>
__device__ __forceinline__ void jac_index(const VoxelWalk &vw, int (&i)[ND])
{
    if constexpr (ND == 3) { i[0] = vw.z; i[1] = vw.y; i[2] = vw.x; }
    else { i[0] = vw.y; i[1] = vw.x; }      // D == 1: the walk's z stays 0
}

template <int ND, bool FOLD>
__global__ __launch_bounds__(TRX_BLOCK) void jac_map_kernel(const float *__restrict__ flow, float *__restrict__ det, unsigned nvox, int D, int H, int W,
                                                              float threshold, double *__restrict__ partials)
{
    __shared__ double wsum[TRX_WAVES];
    const int tid = threadIdx.x;
    const float *__restrict__ f = flow + (size_t)blockIdx.y * ND * nvox;
    float *__restrict__ out = det + (size_t)blockIdx.y * nvox;
    int S[ND];
    unsigned st[ND];
    jac_sizes<ND>(D, H, W, S, st);
    const unsigned first = blockIdx.x * (unsigned)kFoldChunk, last = min(nvox, first + (unsigned)kFoldChunk);
    double s = 0.0;
    for (VoxelWalk vw(first + tid, TRX_BLOCK, H, W); vw.i < last; vw.next(H, W)) {
        int i[ND];
        jac_index<ND>(vw, i);
        float J[ND][ND];
        jac_at<ND>(f, nvox, vw.i, i, S, st, J);
        const float d = jac_det<ND>(J);
        out[vw.i] = d;
        if constexpr (FOLD) {   // a select, not a branch: the loads of the next voxel are not held behind it (a NaN determinant stays a NaN)
            const double h = d >= threshold ? 0.0 : (double)(threshold - d);
            s = fma(h, h, s);
        }
    }
    if constexpr (FOLD) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if ((tid & 63) == 0) wsum[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < TRX_WAVES; w++) t += wsum[w];
            partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

__global__ __launch_bounds__(64) void fold_reduce_kernel(const double *__restrict__ partials, int nchunk, unsigned nvox, float *__restrict__ penalty)
{
    const float p = fold_penalty_from_partials(partials + (size_t)blockIdx.x * nchunk, nchunk, nvox);
    if (threadIdx.x == 0) penalty[blockIdx.x] = p;
}

template <int ND, bool ACC>
__global__ __launch_bounds__(TRX_BLOCK) void fold_backward_kernel(const float *__restrict__ flow, const float *__restrict__ det,
                                                                    const double *__restrict__ partials, float *__restrict__ dflow, unsigned nvox, int D, int H,
                                                                    int W, float threshold, float scale)
{
    const float *__restrict__ f = flow + (size_t)blockIdx.y * ND * nvox;
    const float *__restrict__ dt = det + (size_t)blockIdx.y * nvox;
    float *__restrict__ g = dflow + (size_t)blockIdx.y * ND * nvox;
    int S[ND];
    unsigned st[ND];
    jac_sizes<ND>(D, H, W, S, st);
    const unsigned first = blockIdx.x * (unsigned)kFoldChunk, last = min(nvox, first + (unsigned)kFoldChunk);
    {   // The stencil neighbours of the block's voxels [first, last) lie in the block's own chunk and in the 2 nd windows [first -+ st[b], last - 1 -+ st[b]]
        // (an index that leaves the pair is clamped by the stencil to the voxel itself, hence to the own chunk; clamping the window's end to the pair
        // instead can only add a chunk).  A window is no longer than a chunk, so it lies in the chunks of its two ends: 4 nd + 1 partial sums.  Where
        // all of them are exactly 0 no voxel in reach is active (h > 0 has h^2 > 0 in fp64; a NaN partial is not 0) and the gradient is exactly 0 here:
        // accumulating, the block has nothing to read or write.  Most of a real run's blocks leave here.
        const double *__restrict__ pp = partials + (size_t)blockIdx.y * gridDim.x;
        int any = 0;
        if (threadIdx.x < 4 * ND) {
            const int b = threadIdx.x >> 2;
            const unsigned sb = b == 0 ? st[0] : b == 1 ? st[1] : st[ND - 1];
            const unsigned v = (threadIdx.x & 1) ? last - 1u : first;
            const unsigned t = (threadIdx.x & 2) ? min(nvox - 1u, v + sb) : (v >= sb ? v - sb : 0u);
            any = !(pp[t / (unsigned)kFoldChunk] == 0.0);
        } else if (threadIdx.x == 4 * ND) {
            any = !(pp[blockIdx.x] == 0.0);
        }
        if (!__syncthreads_or(any)) {
            if constexpr (!ACC) {
                const float zero = scale * 0.f;      // what the voxel loop below stores for an inactive voxel, sign included
                for (unsigned v = first + threadIdx.x; v < last; v += TRX_BLOCK)
#pragma unroll
                    for (int a = 0; a < ND; a++) g[(size_t)a * nvox + v] = zero;
            }
            return;
        }
    }
    for (VoxelWalk vw(first + threadIdx.x, TRX_BLOCK, H, W); vw.i < last; vw.next(H, W)) {
        int i[ND];
        jac_index<ND>(vw, i);
        // the voxels n whose D_b reads u(y), and the coefficient of u(y) there: per axis the lower neighbour (+sc(n)) and the upper one (-sc(n)); on a
        // face the clamped index is y itself, whose one-sided difference holds u(y) with -1 (first voxel) / +1 (last voxel); an axis of one voxel: nothing
        unsigned n[2 * ND];
        int jn[2 * ND];
        float cf[2 * ND], dn[2 * ND], old[ND];
#pragma unroll
        for (int b = 0; b < ND; b++) {
            const int j = i[b], Sb = S[b];
            const float edge = Sb > 1 ? 1.0f : 0.0f;
            jn[2 * b] = max(j - 1, 0);
            jn[2 * b + 1] = min(j + 1, Sb - 1);
            cf[2 * b] = j >= 1 ? (jn[2 * b] >= 1 && jn[2 * b] <= Sb - 2 ? 0.5f : 1.0f) : -edge;
            cf[2 * b + 1] = j <= Sb - 2 ? (jn[2 * b + 1] >= 1 && jn[2 * b + 1] <= Sb - 2 ? -0.5f : -1.0f) : edge;
            n[2 * b] = vw.i - (unsigned)(j - jn[2 * b]) * st[b];
            n[2 * b + 1] = vw.i + (unsigned)(jn[2 * b + 1] - j) * st[b];
        }
        // every load the inactive path needs is issued here, before the first branch: 2 nd determinants (cached) and, accumulating, the nd old values
#pragma unroll
        for (int e = 0; e < 2 * ND; e++) dn[e] = dt[n[e]];
        if constexpr (ACC) {
#pragma unroll
            for (int a = 0; a < ND; a++) old[a] = g[(size_t)a * nvox + vw.i];
        }
        float acc[ND];
#pragma unroll
        for (int a = 0; a < ND; a++) acc[a] = 0.f;
#pragma unroll
        for (int e = 0; e < 2 * ND; e++) {
            const int b = e / 2;
            if (!(dn[e] >= threshold) && cf[e] != 0.f) {
                int in[ND];
#pragma unroll
                for (int a = 0; a < ND; a++) in[a] = a == b ? jn[e] : i[a];
                float J[ND][ND];
                jac_at<ND>(f, nvox, n[e], in, S, st, J);
                const float q = cf[e] * (threshold - dn[e]);
#pragma unroll
                for (int a = 0; a < ND; a++) acc[a] = fmaf(q, jac_cof<ND>(J, a, b), acc[a]);
            }
        }
#pragma unroll
        for (int a = 0; a < ND; a++) {
            const size_t o = (size_t)a * nvox + vw.i;
            if constexpr (ACC) g[o] = fmaf(scale, acc[a], old[a]);
            else g[o] = scale * acc[a];
        }
    }
}

int fold_geom(int ndim, int B, int D, int H, int W, FoldGeom *g)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || (double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    g->ndim = ndim; g->B = B; g->D = D; g->H = H; g->W = W;
    g->nvox = (unsigned)D * (unsigned)H * (unsigned)W;
    g->nchunk = (g->nvox + kFoldChunk - 1) / kFoldChunk;
    g->part_offset = ((size_t)B * g->nvox * sizeof(float) + 255) & ~(size_t)255;
    g->ws_bytes = g->part_offset + (((size_t)B * g->nchunk * sizeof(double) + 255) & ~(size_t)255);
    return TRX_OK;
}

template <bool FOLD>
static int jac_map_launch(const FoldGeom &g, const float *flow, float *det, float threshold, double *partials, hipStream_t s)
{
    const dim3 grid(g.nchunk, (unsigned)g.B), block(TRX_BLOCK);
    if (g.ndim == 3) hipLaunchKernelGGL((jac_map_kernel<3, FOLD>), grid, block, 0, s, flow, det, g.nvox, g.D, g.H, g.W, threshold, partials);
    else hipLaunchKernelGGL((jac_map_kernel<2, FOLD>), grid, block, 0, s, flow, det, g.nvox, g.D, g.H, g.W, threshold, partials);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

int fold_forward_impl(const FoldGeom &g, const float *flow, float threshold, void *workspace, hipStream_t s)
{
    return jac_map_launch<true>(g, flow, (float *)workspace, threshold, (double *)((char *)workspace + g.part_offset), s);
}

int fold_backward_impl(const FoldGeom &g, const float *flow, float threshold, float weight, float *dflow, int accumulate, const void *workspace, hipStream_t s)
{
    const dim3 grid(g.nchunk, (unsigned)g.B), block(TRX_BLOCK);
    const float scale = (float)(-2.0 * (double)weight / (double)g.nvox);
    const float *det = (const float *)workspace;
    const double *part = (const double *)((const char *)workspace + g.part_offset);
    if (g.ndim == 3 && accumulate) hipLaunchKernelGGL((fold_backward_kernel<3, true>), grid, block, 0, s, flow, det, part, dflow, g.nvox, g.D, g.H, g.W, threshold, scale);
    else if (g.ndim == 3) hipLaunchKernelGGL((fold_backward_kernel<3, false>), grid, block, 0, s, flow, det, part, dflow, g.nvox, g.D, g.H, g.W, threshold, scale);
    else if (accumulate) hipLaunchKernelGGL((fold_backward_kernel<2, true>), grid, block, 0, s, flow, det, part, dflow, g.nvox, g.D, g.H, g.W, threshold, scale);
    else hipLaunchKernelGGL((fold_backward_kernel<2, false>), grid, block, 0, s, flow, det, part, dflow, g.nvox, g.D, g.H, g.W, threshold, scale);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" int trx_flow_jacobian(const float *flow, int ndim, int B, int D, int H, int W, float *det, void *stream)
{
    if (!flow || !det) return TRX_ERR_ARG;
    FoldGeom g;
    const int rc = fold_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    return jac_map_launch<false>(g, flow, det, 0.f, nullptr, (hipStream_t)stream);
}

extern "C" size_t trx_flow_folding_workspace_bytes(int ndim, int B, int D, int H, int W)
{
    FoldGeom g;
    if (fold_geom(ndim, B, D, H, W, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

extern "C" int trx_flow_folding(const float *flow, int ndim, int B, int D, int H, int W, float threshold, float weight, float *penalty, float *dflow,
                                int accumulate, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!flow || !penalty || !workspace) return TRX_ERR_ARG;
    FoldGeom g;
    int rc = fold_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    if (!std::isfinite(threshold) || !std::isfinite(weight) || weight < 0.f) return TRX_ERR_ARG;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = fold_forward_impl(g, flow, threshold, workspace, s)) != TRX_OK) return rc;
    hipLaunchKernelGGL(fold_reduce_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double *)((char *)workspace + g.part_offset), (int)g.nchunk, g.nvox, penalty);
    TRX_CHECK_LAUNCH();
    if (dflow) return fold_backward_impl(g, flow, threshold, weight, dflow, accumulate, workspace, s);
    return TRX_OK;
}
