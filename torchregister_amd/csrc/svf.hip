// Stationary velocity field (Arsigny et al. 2006; extension, the reference has no such model): the exponential of a velocity field by
// scaling and squaring (trx_svf_exp) and its exact adjoint (trx_svf_exp_backward).  The loop over them, trx_bspline_svf_run, lives in
// bspline.hip beside the loop it shares.  CPU restatement: tests/svf_ref.py.
//
// Definition (include/trx.h): S(f, p) = the bi / trilinear sample of the field f at the voxel position p, corners outside the volume
// contributing zero (trx_flow_warp's sampler).  With K squarings and sign s:
//   u_0 = s 2^-K v;   u_{k+1}(x) = u_k(x) + S(u_k, x + u_k(x));   flow = u_K.
// A position is ONE fp32 add of the voxel index and the displacement, i0 = floor(p), t = p - i0, and corner kappa has the weight
// prod_a (kappa_a ? t_a : 1 - t_a).  Adjoint of one squaring, g = dL/du_{k+1}:
//   dL/du_c(y) = g_c(y) + sum_x sum_kappa [i0(x) + kappa = y] w_kappa(t(x)) g_c(x) + sum_kappa ok_kappa (dw_kappa/dt_c)(t(y)) sum_a g_a(y) u_a(i0(y) + kappa).
//
// Forward: one launch for u_0 and one per squaring, a thread per voxel: it reads u(x) and gathers 2^nd corners of nd channels
// (24 B/voxel moved in 3-D while the gather hits cache; displacements of level k are at most 2^(k-K) max|v|).  The levels u_0 .. u_{K-1}
// stay in the workspace for the backward.
//
// Backward, per level from K - 1 down to 0, two launches:
//   splat   the second term, a scatter-add, in FIXED POINT in the manner of mi_dev.h: with m = max |g| of the pair (an order-free
//           atomicMax on the bit pattern of fabsf, left by the previous level's finishing pass) and m < 2^E, a contribution w g is rounded
//           once to a multiple of q = 2^(E - 31) - an integer of magnitude <= 2^31 - and added with 64-bit integer atomics.  A voxel
//           receives at most one corner per source voxel, <= 2^31 of them, so a sum stays below 2^62.  Integer adds commute: any
//           schedule gives the same bits, and nothing a pair adds depends on another pair.  A block takes a tile of source voxels and
//           accumulates into an LDS copy of the tile and a halo of 2 voxels (every corner of a source with |u| < 2 lands there), then
//           adds the touched cells to the pair's accumulator in global memory, one add per cell; corners beyond the halo go to global
//           memory directly.  m = 0: no splat.
//   finish  counts -> fp32 (and the accumulator back to zero), + g(y) + the third term (the forward's gather with the weights'
//           derivatives), written as dL/du_k - at level 0 times s 2^-K, as dvel - and max |dL/du_k| for the next splat.
// A pair whose m is not finite gets NaN everywhere.  No float atomics.
#include "svf_sample.h"

#include <algorithm>

namespace trx {

constexpr int kSvfMaxSquarings = 12;
constexpr int kSvfHalo = 2;

// Source tile of the splat and its accumulator in LDS (tile + halo on every axis); 2-D has no z axis.
template <int ND> struct SvfTile {
    static constexpr int TZ = ND == 3 ? 8 : 1, TY = ND == 3 ? 8 : 16, TX = ND == 3 ? 8 : 32;
    static constexpr int AZ = ND == 3 ? TZ + 2 * kSvfHalo : 1, AY = TY + 2 * kSvfHalo, AX = TX + 2 * kSvfHalo;
    static constexpr int VOX = TZ * TY * TX, CELLS = AZ * AY * AX;
};

struct SvfLayout {
    size_t N, nflow;                                   // voxels per volume, floats per field [B][nd][N]
    size_t o_levels, o_g, o_acc, o_max, level_bytes, ws_bytes;
};

// ndim, B, D, H, W, squarings -> status and (for accepted arguments) the workspace layout:
//   levels u_0 .. u_{K-1} (K fields) | two gradient fields | int64 accumulator [B][nd][N] | maxima [K][B]; each part 256-byte aligned
static int svf_layout(int ndim, int B, int D, int H, int W, int K, SvfLayout *l)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1) return TRX_ERR_ARG;
    if (K < 0 || K > kSvfMaxSquarings) return TRX_ERR_ARG;
    if ((double)D * H * W > 2147483648.0) return TRX_ERR_ARG;
    l->N = (size_t)D * H * W;
    l->nflow = (size_t)B * ndim * l->N;
    l->level_bytes = (l->nflow * sizeof(float) + 255) & ~(size_t)255;
    l->o_levels = 0;
    l->o_g = l->o_levels + (size_t)K * l->level_bytes;
    l->o_acc = l->o_g + (K > 0 ? 2 * l->level_bytes : 0);
    l->o_max = l->o_acc + (K > 0 ? (l->nflow * sizeof(unsigned long long) + 255) & ~(size_t)255 : 0);
    l->ws_bytes = l->o_max + (((size_t)(kSvfMaxSquarings + 1) * B * sizeof(unsigned) + 255) & ~(size_t)255);
    return TRX_OK;
}

// out = a * in (a = +-2^-K: exact)
__global__ __launch_bounds__(TRX_BLOCK) void svf_scale_kernel(const float *__restrict__ in, float *__restrict__ out, size_t n, float a)
{
    for (size_t i = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * TRX_BLOCK) out[i] = a * in[i];
}

// u_{k+1}(x) = u_k(x) + S(u_k, x + u_k(x)); pairs along blockIdx.y
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void svf_square_kernel(const float *__restrict__ src, float *__restrict__ dst, unsigned N, int D, int H, int W)
{
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= N) return;
    const float *u = src + (size_t)blockIdx.y * ND * N;
    float *o = dst + (size_t)blockIdx.y * ND * N;
    int x[3];
    svf_coords<ND>(i, H, W, x);
    float ux[ND], acc[ND];
#pragma unroll
    for (int c = 0; c < ND; c++) { ux[c] = u[(size_t)c * N + i]; acc[c] = 0.f; }
    SvfAxis ax[3];
    svf_axes<ND>(x, ux, D, H, W, ax);
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
                for (int c = 0; c < ND; c++) acc[c] = fmaf(w, ok ? u[(size_t)c * N + off] : 0.f, acc[c]);
            }
#pragma unroll
    for (int c = 0; c < ND; c++) o[(size_t)c * N + i] = ux[c] + acc[c];
}

// maxbits[pair] = max over the pair's n floats of the bit pattern of |g| (a NaN is larger than every finite value and than infinity)
__device__ __forceinline__ void svf_block_max(unsigned mine, unsigned *__restrict__ dst)
{
    __shared__ unsigned s_max[TRX_WAVES];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine = max(mine, (unsigned)__shfl_down((int)mine, off, 64));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned m = s_max[0];
#pragma unroll
        for (int w = 1; w < TRX_WAVES; w++) m = max(m, s_max[w]);
        if (m) atomicMax(dst, m);
    }
}

__global__ __launch_bounds__(TRX_BLOCK) void svf_max_kernel(const float *__restrict__ g, size_t n, unsigned *__restrict__ maxbits)
{
    const float *p = g + (size_t)blockIdx.y * n;
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * TRX_BLOCK) m = max(m, __float_as_uint(fabsf(p[i])));
    svf_block_max(m, maxbits + blockIdx.y);
}

// m (bit pattern, finite, non-zero) -> E with m < 2^E, and 2^n as a double for the |n| <= 160 that occur
__device__ __forceinline__ int svf_exponent(unsigned mbits) { return (int)(mbits >> 23) - 126; }
__device__ __forceinline__ double svf_pow2(int n) { return __longlong_as_double((long long)(1023 + n) << 52); }

// The splat of one level: acc[pair][c][y] += round(w_kappa(t(x)) g_c(x) / q) over the in-bounds corners y = i0(x) + kappa of every source x
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void svf_splat_kernel(const float *__restrict__ gin, const float *__restrict__ uin, unsigned long long *__restrict__ accum,
                                                                const unsigned *__restrict__ maxbits, unsigned N, int D, int H, int W, int nty, int ntx)
{
    using T = SvfTile<ND>;
    __shared__ unsigned long long s_acc[ND][T::CELLS];
    const unsigned mb = maxbits[blockIdx.y];
    if (mb == 0 || mb >= 0x7f800000u) return;          // nothing to add; not finite: the finishing pass writes NaN
    const double inv_q = svf_pow2(31 - svf_exponent(mb));
    const float *g = gin + (size_t)blockIdx.y * ND * N, *u = uin + (size_t)blockIdx.y * ND * N;
    unsigned long long *acc = accum + (size_t)blockIdx.y * ND * N;
    for (int e = threadIdx.x; e < ND * T::CELLS; e += TRX_BLOCK) (&s_acc[0][0])[e] = 0ull;
    __syncthreads();
    const unsigned t = blockIdx.x;
    const int o[3] = {(int)(t / (unsigned)ntx / (unsigned)nty) * T::TZ, (int)(t / (unsigned)ntx % (unsigned)nty) * T::TY, (int)(t % (unsigned)ntx) * T::TX};
    for (int e = threadIdx.x; e < T::VOX; e += TRX_BLOCK) {
        const int x[3] = {o[0] + e / (T::TX * T::TY), o[1] + e / T::TX % T::TY, o[2] + e % T::TX};
        if (x[0] >= D || x[1] >= H || x[2] >= W) continue;
        const size_t i = ((size_t)x[0] * H + x[1]) * W + x[2];
        float gx[ND], ux[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) { gx[c] = g[(size_t)c * N + i]; ux[c] = u[(size_t)c * N + i]; }
        SvfAxis ax[3];
        svf_axes<ND>(x, ux, D, H, W, ax);
#pragma unroll
        for (int kz = 0; kz < (ND == 3 ? 2 : 1); kz++)
#pragma unroll
            for (int ky = 0; ky < 2; ky++)
#pragma unroll
                for (int kx = 0; kx < 2; kx++) {
                    if (!(ax[0].ok[kz] & ax[1].ok[ky] & ax[2].ok[kx])) continue;
                    float w = (ky ? ax[1].t : 1.f - ax[1].t) * (kx ? ax[2].t : 1.f - ax[2].t);
                    if constexpr (ND == 3) w *= kz ? ax[0].t : 1.f - ax[0].t;
                    const int y[3] = {ax[0].i0 + kz, ax[1].i0 + ky, ax[2].i0 + kx};      // inside the volume
                    const int rz = ND == 3 ? y[0] - o[0] + kSvfHalo : 0, ry = y[1] - o[1] + kSvfHalo, rx = y[2] - o[2] + kSvfHalo;
                    const bool local = (unsigned)rz < (unsigned)T::AZ && (unsigned)ry < (unsigned)T::AY && (unsigned)rx < (unsigned)T::AX;
                    const int cell = (rz * T::AY + ry) * T::AX + rx;
                    const size_t off = ((size_t)y[0] * H + y[1]) * W + y[2];
#pragma unroll
                    for (int c = 0; c < ND; c++) {
                        const long long cnt = __double2ll_rn((double)(w * gx[c]) * inv_q);
                        if (cnt == 0) continue;
                        if (local) atomicAdd(&s_acc[c][cell], (unsigned long long)cnt);
                        else atomicAdd(acc + (size_t)c * N + off, (unsigned long long)cnt);
                    }
                }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < T::CELLS; e += TRX_BLOCK) {
        const int y[3] = {ND == 3 ? o[0] + e / (T::AX * T::AY) - kSvfHalo : 0, o[1] + e / T::AX % T::AY - kSvfHalo, o[2] + e % T::AX - kSvfHalo};
        if ((unsigned)y[0] >= (unsigned)D || (unsigned)y[1] >= (unsigned)H || (unsigned)y[2] >= (unsigned)W) continue;
        const size_t off = ((size_t)y[0] * H + y[1]) * W + y[2];
#pragma unroll
        for (int c = 0; c < ND; c++) {
            const unsigned long long v = s_acc[c][e];
            if (v) atomicAdd(acc + (size_t)c * N + off, v);
        }
    }
}

// dL/du_k = scale (g + splat + the derivative of the sample with respect to its position), the accumulator back to zero, max |dL/du_k|
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void svf_finish_kernel(const float *__restrict__ gin, const float *__restrict__ uin, unsigned long long *__restrict__ accum,
                                                                 const unsigned *__restrict__ maxbits, unsigned *__restrict__ maxbits_out, float *__restrict__ out,
                                                                 float scale, unsigned N, int D, int H, int W)
{
    const unsigned i = blockIdx.x * TRX_BLOCK + threadIdx.x;
    const unsigned mb = maxbits[blockIdx.y];
    unsigned mine = 0;
    if (i < N) {
        const float *g = gin + (size_t)blockIdx.y * ND * N, *u = uin + (size_t)blockIdx.y * ND * N;
        unsigned long long *acc = accum + (size_t)blockIdx.y * ND * N;
        float *o = out + (size_t)blockIdx.y * ND * N;
        float gx[ND], ux[ND], r[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) { gx[c] = g[(size_t)c * N + i]; ux[c] = u[(size_t)c * N + i]; r[c] = gx[c]; }
        if (mb != 0 && mb < 0x7f800000u) {
            const double q = svf_pow2(svf_exponent(mb) - 31);
#pragma unroll
            for (int c = 0; c < ND; c++) {
                const long long cnt = (long long)acc[(size_t)c * N + i];
                if (cnt != 0) {
                    acc[(size_t)c * N + i] = 0ull;
                    r[c] += (float)((double)cnt * q);
                }
            }
        }
        int x[3];
        svf_coords<ND>(i, H, W, x);
        SvfAxis ax[3];
        svf_axes<ND>(x, ux, D, H, W, ax);
        float d[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) d[c] = 0.f;
#pragma unroll
        for (int kz = 0; kz < (ND == 3 ? 2 : 1); kz++)
#pragma unroll
            for (int ky = 0; ky < 2; ky++)
#pragma unroll
                for (int kx = 0; kx < 2; kx++) {
                    const bool ok = ax[0].ok[kz] & ax[1].ok[ky] & ax[2].ok[kx];
                    const size_t off = ((size_t)ax[0].c[kz] * H + ax[1].c[ky]) * W + ax[2].c[kx];
                    float s = 0.f;                                   // sum_a g_a(y) u_a(corner)
#pragma unroll
                    for (int c = 0; c < ND; c++) s = fmaf(gx[c], ok ? u[(size_t)c * N + off] : 0.f, s);
                    const float wz = ND == 3 ? (kz ? ax[0].t : 1.f - ax[0].t) : 1.f, wy = ky ? ax[1].t : 1.f - ax[1].t, wx = kx ? ax[2].t : 1.f - ax[2].t;
                    const float sz = kz ? s : -s, sy = ky ? s : -s, sx = kx ? s : -s;
                    if constexpr (ND == 3) {
                        d[0] = fmaf(wy * wx, sz, d[0]);
                        d[1] = fmaf(wz * wx, sy, d[1]);
                        d[2] = fmaf(wz * wy, sx, d[2]);
                    } else {
                        d[0] = fmaf(wx, sy, d[0]);
                        d[1] = fmaf(wy, sx, d[1]);
                    }
                }
#pragma unroll
        for (int c = 0; c < ND; c++) {
            float v = scale * (r[c] + d[c]);
            if (mb >= 0x7f800000u) v = __uint_as_float(0x7fc00000u);
            o[(size_t)c * N + i] = v;
            mine = max(mine, __float_as_uint(fabsf(v)));
        }
    }
    if (maxbits_out) svf_block_max(mine, maxbits_out + blockIdx.y);
}

static dim3 svf_stream_grid(size_t n) { return dim3((unsigned)std::max<size_t>(1, std::min<size_t>((n + TRX_BLOCK - 1) / TRX_BLOCK, 4096))); }

template <int ND>
static int svf_exp_launch(const SvfLayout &l, const float *vel, float *flow, int B, int D, int H, int W, int K, int inverse, char *ws, hipStream_t s)
{
    const float a = (inverse ? -1.f : 1.f) / (float)(1 << K);
    float *first = K > 0 ? (float *)(ws + l.o_levels) : flow;
    hipLaunchKernelGGL(svf_scale_kernel, svf_stream_grid(l.nflow), dim3(TRX_BLOCK), 0, s, vel, first, l.nflow, a);
    TRX_CHECK_LAUNCH();
    const dim3 grid((unsigned)((l.N + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)B);
    for (int k = 0; k < K; k++) {
        const float *src = (const float *)(ws + l.o_levels + (size_t)k * l.level_bytes);
        float *dst = k + 1 < K ? (float *)(ws + l.o_levels + (size_t)(k + 1) * l.level_bytes) : flow;
        hipLaunchKernelGGL((svf_square_kernel<ND>), grid, dim3(TRX_BLOCK), 0, s, src, dst, (unsigned)l.N, D, H, W);
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}

template <int ND>
static int svf_backward_launch(const SvfLayout &l, const float *dflow, float *dvel, int B, int D, int H, int W, int K, int inverse, char *ws, hipStream_t s)
{
    using T = SvfTile<ND>;
    const float a = (inverse ? -1.f : 1.f) / (float)(1 << K);
    if (K == 0) {
        hipLaunchKernelGGL(svf_scale_kernel, svf_stream_grid(l.nflow), dim3(TRX_BLOCK), 0, s, dflow, dvel, l.nflow, a);
        TRX_CHECK_LAUNCH();
        return TRX_OK;
    }
    unsigned long long *acc = (unsigned long long *)(ws + l.o_acc);
    unsigned *maxbits = (unsigned *)(ws + l.o_max);            // [level][B]: max |dL/du_{level + 1}|
    if (hipMemsetAsync(acc, 0, l.ws_bytes - l.o_acc, s) != hipSuccess) return TRX_ERR_HIP;      // the accumulator and the maxima behind it
    const size_t per_pair = (size_t)ND * l.N;
    hipLaunchKernelGGL(svf_max_kernel, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((per_pair + TRX_BLOCK - 1) / TRX_BLOCK, 1024)), (unsigned)B),
                       dim3(TRX_BLOCK), 0, s, dflow, per_pair, maxbits + (size_t)(K - 1) * B);
    TRX_CHECK_LAUNCH();
    const int ntz = (D + T::TZ - 1) / T::TZ, nty = (H + T::TY - 1) / T::TY, ntx = (W + T::TX - 1) / T::TX;
    const dim3 sgrid((unsigned)((size_t)ntz * nty * ntx), (unsigned)B), fgrid((unsigned)((l.N + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)B);
    const float *gin = dflow;
    for (int k = K - 1; k >= 0; k--) {
        const float *u = (const float *)(ws + l.o_levels + (size_t)k * l.level_bytes);
        float *gout = k == 0 ? dvel : (float *)(ws + l.o_g + (size_t)(k & 1) * l.level_bytes);
        const unsigned *mk = maxbits + (size_t)k * B;
        hipLaunchKernelGGL((svf_splat_kernel<ND>), sgrid, dim3(TRX_BLOCK), 0, s, gin, u, acc, mk, (unsigned)l.N, D, H, W, nty, ntx);
        TRX_CHECK_LAUNCH();
        hipLaunchKernelGGL((svf_finish_kernel<ND>), fgrid, dim3(TRX_BLOCK), 0, s, gin, u, acc, mk, k > 0 ? maxbits + (size_t)(k - 1) * B : (unsigned *)nullptr, gout,
                           k == 0 ? a : 1.f, (unsigned)l.N, D, H, W);
        TRX_CHECK_LAUNCH();
        gin = gout;
    }
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_svf_workspace_bytes(int ndim, int B, int D, int H, int W, int squarings)
{
    SvfLayout l;
    if (svf_layout(ndim, B, D, H, W, squarings, &l) != TRX_OK) return 0;
    return l.ws_bytes;
}

extern "C" int trx_svf_exp(const float *vel, float *flow, int ndim, int B, int D, int H, int W, int squarings, int inverse, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    if (!vel || !flow || !workspace) return TRX_ERR_ARG;
    SvfLayout l;
    const int rc = svf_layout(ndim, B, D, H, W, squarings, &l);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < l.ws_bytes) return TRX_ERR_WORKSPACE;
    return ndim == 3 ? svf_exp_launch<3>(l, vel, flow, B, D, H, W, squarings, inverse, (char *)workspace, (hipStream_t)stream)
                     : svf_exp_launch<2>(l, vel, flow, B, D, H, W, squarings, inverse, (char *)workspace, (hipStream_t)stream);
}

extern "C" int trx_svf_exp_backward(const float *vel, const float *dflow, float *dvel, int ndim, int B, int D, int H, int W, int squarings, int inverse,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    if (!vel || !dflow || !dvel || !workspace) return TRX_ERR_ARG;
    SvfLayout l;
    const int rc = svf_layout(ndim, B, D, H, W, squarings, &l);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < l.ws_bytes) return TRX_ERR_WORKSPACE;
    return ndim == 3 ? svf_backward_launch<3>(l, dflow, dvel, B, D, H, W, squarings, inverse, (char *)workspace, (hipStream_t)stream)
                     : svf_backward_launch<2>(l, dflow, dvel, B, D, H, W, squarings, inverse, (char *)workspace, (hipStream_t)stream);
}
