// Normalised gradient field criterion of (target, warped) (include/trx.h: trx_ngf_loss_grad; extension, the reference has none).
// CPU restatement: tests/ngf_ref.py.
//
// Definition: D_a I is the central difference along axis a over the voxel size h_a, one-sided on the first and the last voxel of the axis, 0 on an axis of
// one voxel - jac_at's convention (csrc/jacobian.hip): sc (I(min(i + 1, S - 1)) - I(max(i - 1, 0))) / h with sc = 1/2 where both neighbours exist and 1
// elsewhere; every index is clamped, no load is predicated.  gT = D target, gW = D warped, s = <gW, gT>, a = |gW|^2 + eps_w^2, b = |gT|^2 + eps_t^2,
// r = s^2 / (a b) (0 where a b == 0), loss = alpha (1 - mean over the mask of r).
//
//   ngf_forward_kernel<ND, MASK, GRAD>  a block takes kNgfChunk consecutive voxels of one pair, lanes along x (VoxelWalk): 2 nd loads of each image per voxel,
//                                       of which the y and z neighbours are cache hits of the rows around.  r is added in fp64 in ascending voxels per
//                                       thread, a fixed shuffle tree per wave and the four waves in order -> one fp64 partial and one mask count per block.
//                                       GRAD: q = dr / dgW = 2 s gT / (a b) - 2 s^2 gW / (a^2 b) (0 outside the mask and where a b == 0) -> workspace [B][nd][N].
//   ngf_reduce_kernel                   one wave per pair sums its partials and counts in a fixed order -> loss[b] and the scale -alpha / N_m (workspace).
//   ngf_backward_kernel<ND>             gather: voxel y reads q_a at its two neighbours along axis a (the clamped index names the voxel itself on a face,
//                                       where the one-sided difference has a term of its own) with the coefficient of I(y) in (D_a I)(neighbour):
//                                       grad_warped(y) = scale_b sum_a sum_{n in {lower, upper}} c_a(n, y) q_a(n).  2 nd cached loads, one store.
// No atomics, every sum in a fixed order: the same bits on every call, a pair's result does not depend on the batch around it, and an all-ones mask gives
// the bits of no mask (the same r, the same N_m).
#include "ngf.h"

#include <cmath>

namespace trx {

struct NgfAxes {
    float hinv[3];   // 1 / h per axis, in the tensor's axis order (2-D: y, x)
};

template <int ND>
__device__ __forceinline__ void ngf_sizes(int D, int H, int W, int (&S)[ND], unsigned (&st)[ND])
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
__device__ __forceinline__ void ngf_index(const VoxelWalk &vw, int (&i)[ND])
{
    if constexpr (ND == 3) { i[0] = vw.z; i[1] = vw.y; i[2] = vw.x; }
    else { i[0] = vw.y; i[1] = vw.x; }      // D == 1: the walk's z stays 0
}

template <int ND, bool MASK, bool GRAD>
__global__ __launch_bounds__(TRX_BLOCK) void ngf_forward_kernel(const float *__restrict__ target, const float *__restrict__ warped,
                                                                  const unsigned char *__restrict__ mask, const float *__restrict__ eps,
                                                                  float *__restrict__ q, double *__restrict__ partials, unsigned *__restrict__ counts,
                                                                  unsigned nvox, int D, int H, int W, NgfAxes ax)
{
    __shared__ double wsum[TRX_WAVES];
    __shared__ unsigned wcnt[TRX_WAVES];
    const int tid = threadIdx.x;
    const float *__restrict__ T = target + (size_t)blockIdx.y * nvox;
    const float *__restrict__ Wp = warped + (size_t)blockIdx.y * nvox;
    const unsigned char *__restrict__ M = MASK ? mask + (size_t)blockIdx.y * nvox : nullptr;
    float *__restrict__ qo = GRAD ? q + (size_t)blockIdx.y * ND * nvox : nullptr;
    const float et = eps[2 * blockIdx.y], ew = eps[2 * blockIdx.y + 1];
    const float et2 = et * et, ew2 = ew * ew;
    int S[ND];
    unsigned st[ND];
    ngf_sizes<ND>(D, H, W, S, st);
    const unsigned first = blockIdx.x * (unsigned)kNgfChunk, last = min(nvox, first + (unsigned)kNgfChunk);
    double sum = 0.0;
    unsigned cnt = 0;
    for (VoxelWalk vw(first + tid, TRX_BLOCK, H, W); vw.i < last; vw.next(H, W)) {
        int i[ND];
        ngf_index<ND>(vw, i);
        float gT[ND], gW[ND];
#pragma unroll
        for (int b = 0; b < ND; b++) {
            const int ip = min(i[b] + 1, S[b] - 1), im = max(i[b] - 1, 0);
            const float c = (ip - im == 2 ? 0.5f : 1.0f) * ax.hinv[b];
            const unsigned op = vw.i + (unsigned)(ip - i[b]) * st[b], om = vw.i - (unsigned)(i[b] - im) * st[b];
            gT[b] = c * (T[op] - T[om]);
            gW[b] = c * (Wp[op] - Wp[om]);
        }
        float s = 0.f, a = ew2, bb = et2;
#pragma unroll
        for (int b = 0; b < ND; b++) {
            s = fmaf(gW[b], gT[b], s);
            a = fmaf(gW[b], gW[b], a);
            bb = fmaf(gT[b], gT[b], bb);
        }
        const float ab = a * bb;
        bool in = ab != 0.f;      // selects, not branches: a b == 0 has r = 0 and q = 0, never 0 / 0
        if constexpr (MASK) {
            const bool m = M[vw.i] != 0;
            cnt += m ? 1u : 0u;
            in = in && m;
        }
        const float r = in ? s * s / ab : 0.f;
        sum += (double)r;
        if constexpr (GRAD) {
            const float c1 = 2.0f * s / ab, c2 = s / a;
#pragma unroll
            for (int b = 0; b < ND; b++) qo[(size_t)b * nvox + vw.i] = in ? c1 * (gT[b] - c2 * gW[b]) : 0.f;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        if constexpr (MASK) cnt += __shfl_down(cnt, off, 64);
    }
    if ((tid & 63) == 0) {
        wsum[tid >> 6] = sum;
        wcnt[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < TRX_WAVES; w++) { t += wsum[w]; n += wcnt[w]; }
        const size_t o = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[o] = t;
        if constexpr (MASK) counts[o] = n;
    }
}

// One wave per pair.  Lane l adds rows l, l + 64, ... in ascending order, then a fixed shuffle tree; the rows are loaded 16 at a time before they are
// added, as fold_penalty_from_partials does (a row past the end counts as +0, which changes no bit).  counts == nullptr: N_m = N.
__global__ __launch_bounds__(64) void ngf_reduce_kernel(const double *__restrict__ partials, const unsigned *__restrict__ counts, int nchunk, unsigned nvox,
                                                        float alpha, float *__restrict__ loss, float *__restrict__ scale)
{
    constexpr int kAhead = 16;
    const double *__restrict__ p = partials + (size_t)blockIdx.x * nchunk;
    const unsigned *__restrict__ c = counts ? counts + (size_t)blockIdx.x * nchunk : nullptr;
    double s = 0.0;
    unsigned n = 0;
    for (int r = threadIdx.x & 63; r < nchunk; r += 64 * kAhead) {
        double v[kAhead];
        unsigned m[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const int row = min(r + 64 * k, nchunk - 1);      // the index is clamped, the value selected: no load is predicated
            const double x = p[row];
            const unsigned y = c ? c[row] : 0u;
            v[k] = r + 64 * k < nchunk ? x : 0.0;
            m[k] = r + 64 * k < nchunk ? y : 0u;
        }
#pragma unroll
        for (int k = 0; k < kAhead; k++) { s += v[k]; n += m[k]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_down(s, off, 64);
        n += __shfl_down(n, off, 64);
    }
    if (threadIdx.x == 0) {
        const unsigned nm = c ? n : nvox;
        loss[blockIdx.x] = nm ? (float)((double)alpha * (1.0 - s / (double)nm)) : 0.f;
        scale[blockIdx.x] = nm ? (float)(-(double)alpha / (double)nm) : 0.f;
    }
}

template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void ngf_backward_kernel(const float *__restrict__ q, const float *__restrict__ scale, float *__restrict__ grad,
                                                                   unsigned nvox, int D, int H, int W, NgfAxes ax)
{
    const float *__restrict__ qi = q + (size_t)blockIdx.y * ND * nvox;
    float *__restrict__ g = grad + (size_t)blockIdx.y * nvox;
    const float sc = scale[blockIdx.y];
    int S[ND];
    unsigned st[ND];
    ngf_sizes<ND>(D, H, W, S, st);
    const unsigned first = blockIdx.x * (unsigned)kNgfChunk, last = min(nvox, first + (unsigned)kNgfChunk);
    for (VoxelWalk vw(first + threadIdx.x, TRX_BLOCK, H, W); vw.i < last; vw.next(H, W)) {
        int i[ND];
        ngf_index<ND>(vw, i);
        // the voxels n whose D_b reads I(y), and the coefficient of I(y) there: per axis the lower neighbour (+sc(n)) and the upper one (-sc(n)); on a
        // face the clamped index is y itself, whose one-sided difference holds I(y) with -1 (first voxel) / +1 (last voxel); an axis of one voxel: nothing
        float cf[2 * ND], qn[2 * ND];
#pragma unroll
        for (int b = 0; b < ND; b++) {
            const int j = i[b], Sb = S[b];
            const float edge = Sb > 1 ? 1.0f : 0.0f;
            const int jl = max(j - 1, 0), ju = min(j + 1, Sb - 1);
            cf[2 * b] = (j >= 1 ? (jl >= 1 && jl <= Sb - 2 ? 0.5f : 1.0f) : -edge) * ax.hinv[b];
            cf[2 * b + 1] = (j <= Sb - 2 ? (ju >= 1 && ju <= Sb - 2 ? -0.5f : -1.0f) : edge) * ax.hinv[b];
            qn[2 * b] = qi[(size_t)b * nvox + (vw.i - (unsigned)(j - jl) * st[b])];
            qn[2 * b + 1] = qi[(size_t)b * nvox + (vw.i + (unsigned)(ju - j) * st[b])];
        }
        float acc = 0.f;
#pragma unroll
        for (int e = 0; e < 2 * ND; e++) acc = fmaf(cf[e], qn[e], acc);
        g[vw.i] = sc * acc;
    }
}

int ngf_geom(int ndim, int B, int D, int H, int W, NgfGeom *g)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || (double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    g->ndim = ndim; g->B = B; g->D = D; g->H = H; g->W = W;
    g->nvox = (unsigned)D * (unsigned)H * (unsigned)W;
    g->nchunk = (g->nvox + kNgfChunk - 1) / kNgfChunk;
    const size_t a256 = 255;
    g->part_offset = ((size_t)B * ndim * g->nvox * sizeof(float) + a256) & ~a256;
    g->count_offset = g->part_offset + (((size_t)B * g->nchunk * sizeof(double) + a256) & ~a256);
    g->scale_offset = g->count_offset + (((size_t)B * g->nchunk * sizeof(unsigned) + a256) & ~a256);
    g->ws_bytes = g->scale_offset + (((size_t)B * sizeof(float) + a256) & ~a256);
    g->hinv[0] = g->hinv[1] = g->hinv[2] = 1.0f;
    return TRX_OK;
}

int ngf_cfg_check(const trx_ngf_cfg *cfg, NgfGeom *g)
{
    if (!cfg || !cfg->eps || !std::isfinite(cfg->alpha)) return TRX_ERR_ARG;
    for (int a = 0; a < g->ndim && cfg->voxel; a++) {
        const float h = cfg->voxel[a];
        if (!std::isfinite(h) || !(h > 0.f)) return TRX_ERR_ARG;
        g->hinv[a] = (float)(1.0 / (double)h);
        if (!std::isfinite(g->hinv[a])) return TRX_ERR_ARG;
    }
    return TRX_OK;
}

template <int ND>
static int ngf_launch(const NgfGeom &g, const float *target, const float *warped, const trx_ngf_cfg *cfg, float *loss, float *grad_warped, void *workspace,
                      hipStream_t s)
{
    char *ws = (char *)workspace;
    float *q = (float *)ws, *scale = (float *)(ws + g.scale_offset);
    double *part = (double *)(ws + g.part_offset);
    unsigned *counts = (unsigned *)(ws + g.count_offset);
    NgfAxes ax;
    for (int a = 0; a < 3; a++) ax.hinv[a] = g.hinv[a];
    const dim3 grid(g.nchunk, (unsigned)g.B), block(TRX_BLOCK);
    const unsigned char *mask = cfg->mask;
    if (mask && grad_warped)
        hipLaunchKernelGGL((ngf_forward_kernel<ND, true, true>), grid, block, 0, s, target, warped, mask, cfg->eps, q, part, counts, g.nvox, g.D, g.H, g.W, ax);
    else if (mask)
        hipLaunchKernelGGL((ngf_forward_kernel<ND, true, false>), grid, block, 0, s, target, warped, mask, cfg->eps, q, part, counts, g.nvox, g.D, g.H, g.W, ax);
    else if (grad_warped)
        hipLaunchKernelGGL((ngf_forward_kernel<ND, false, true>), grid, block, 0, s, target, warped, mask, cfg->eps, q, part, counts, g.nvox, g.D, g.H, g.W, ax);
    else
        hipLaunchKernelGGL((ngf_forward_kernel<ND, false, false>), grid, block, 0, s, target, warped, mask, cfg->eps, q, part, counts, g.nvox, g.D, g.H, g.W, ax);
    TRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(ngf_reduce_kernel, dim3((unsigned)g.B), dim3(64), 0, s, (const double *)part, mask ? (const unsigned *)counts : (const unsigned *)nullptr,
                       (int)g.nchunk, g.nvox, cfg->alpha, loss, scale);
    TRX_CHECK_LAUNCH();
    if (grad_warped) {
        hipLaunchKernelGGL(ngf_backward_kernel<ND>, grid, block, 0, s, (const float *)q, (const float *)scale, grad_warped, g.nvox, g.D, g.H, g.W, ax);
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}

int ngf_loss_grad_impl(const NgfGeom &g, const float *target, const float *warped, const trx_ngf_cfg *cfg, float *loss, float *grad_warped, void *workspace,
                       hipStream_t s)
{
    return g.ndim == 3 ? ngf_launch<3>(g, target, warped, cfg, loss, grad_warped, workspace, s)
                       : ngf_launch<2>(g, target, warped, cfg, loss, grad_warped, workspace, s);
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_ngf_workspace_bytes(int ndim, int B, int D, int H, int W)
{
    NgfGeom g;
    if (ngf_geom(ndim, B, D, H, W, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

extern "C" int trx_ngf_loss_grad(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_ngf_cfg *cfg, float *loss,
                                 float *grad_warped, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!target || !warped || !cfg || !loss || !workspace) return TRX_ERR_ARG;
    NgfGeom g;
    int rc = ngf_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    if ((rc = ngf_cfg_check(cfg, &g)) != TRX_OK) return rc;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    return ngf_loss_grad_impl(g, target, warped, cfg, loss, grad_warped, workspace, (hipStream_t)stream);
}
