// Parzen joint-histogram mutual information (Mattes et al. 2003; extension, the reference's NMILoss is a Gaussian KDE on a re-sampled lattice and
// cannot run in 3-D): loss and d loss / d warped of a (target, warped) pair - trx_mi_loss_grad.  Definition: include/trx.h; CPU restatement:
// tests/mi_ref.py.  The target falls into one of K bins (box window), the warped image spreads the cubic B-spline weights of its coordinate over
// four of K bins; P [K][K] is the mean of those weights, the loss is built from the entropies of P and of its marginals.
//
// Three kernels behind one memset of the pair tables:
//   mi_hist_kernel   reads t and w once (8 B/voxel).  A block takes kMiChunk voxels and keeps K x K tables of 64-bit cells in LDS - one per wave
//                    while four fit into 64 KB (K <= 45), fewer above (K = 64: two, waves 0 / 2 and 1 / 3 share) - and adds the voxel's four
//                    weights in FIXED POINT with integer LDS adds: TRX_MI_ONE = 2^31 units per voxel, three weights converted from fp32 (exact for
//                    weights >= 2^-8, to the nearest unit below), the largest one - a middle weight, >= 0.479 - as the remainder, so that a voxel adds
//                    exactly TRX_MI_ONE.  At the end of the chunk the block sums its tables and adds the non-empty cells to the pair's 64-bit table
//                    in global memory with integer atomics (a pair has < 2^31 voxels: no cell passes 2^62).  Integer addition is associative: the
//                    same bits on every call, whatever the order the blocks arrive in, and a pair's table does not depend on the batch around it.
//                    No float atomics.  (32-bit cells would need 2^20 units per voxel to hold a wave's 4096 voxels; an outer weight r^3 / 6 below
//                    2^-21 - r < 0.014 - then adds nothing, cells fed by such weights alone read P = 0 and their G = 0 where it should be
//                    ~ log N: an error of 1e-4 max|G| in the gradient of those voxels.  With 2^31 units the cut is r < 1.1e-3 and 6e-7 max|G|,
//                    the size of fp32 rounding in r itself.)
//   mi_table_kernel  one block per pair: P = counts / (N TRX_MI_ONE), marginals, entropies (fp64, every sum in a fixed order), loss[b], and the
//                    table G = d loss / d P scaled by s_w / N, rounded to fp32, into the workspace.
//   mi_grad_kernel   reads t and w again, writes grad (12 B/voxel): a block copies the pair's G to LDS (16 KB at K = 64), a voxel recomputes
//                    (a, c, r) and gathers four entries.
// Region of interest (cfg->mask, one byte per voxel of the target lattice, non-zero = the voxel counts): each of the three kernels has a second
// instance, chosen by the host from cfg->mask != NULL; the unmasked instances are the code they were.  The masked passes read 9 and 9 B/voxel: the
// histogram adds only voxels inside the mask, the gradient writes 0 outside it, and the table kernel takes N_m from the counts it is given.
// Fixed point: each converted weight is off by at most 2^-32 (and exact above 2^-8), the remainder absorbs the fp32 rounding of the four weights
// (their sum is 1 to 2e-7) plus at most 3 * 2^-32, so beyond fp32 rounding of the weights themselves
//   |P[a][k] - exact| <= 1.5 * 2^-31 * n[a][k] / N   (n: voxels that touch the cell)   and   sum over cells <= 3 * 2^-31.
#include "mi_dev.h"   // scales and bins of a voxel, the LDS accumulate / flush, the gather from G: shared with affine_mi.hip

#include <cmath>

namespace trx {

template <bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void mi_hist_kernel(const float *__restrict__ target, const float *__restrict__ warped, unsigned N, int K, int T,
                                                              const float *__restrict__ range, unsigned long long *__restrict__ counts,
                                                              const unsigned char *__restrict__ mask)
{
    extern __shared__ unsigned long long mi_lds[];           // [T][K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    mi_lds_clear(mi_lds, T * KK);
    const MiScale m = mi_scale(range, b, K);
    const float *t = target + (size_t)b * N, *w = warped + (size_t)b * N;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;
    unsigned long long *mine = mi_lds + ((tid >> 6) % T) * KK;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
#pragma unroll 4
    for (unsigned i = first + tid; i < last; i += TRX_BLOCK) {
        const bool on = mi_counts<MASKED>(mk, i);      // the three streams are loaded side by side; a voxel outside the mask adds nothing
        const MiVoxel v = mi_voxel(__builtin_nontemporal_load(t + i), __builtin_nontemporal_load(w + i), m, K);
        if (on) mi_accumulate(mine, v, K);
    }
    __syncthreads();
    mi_flush(mi_lds, T, KK, counts + (size_t)b * KK);
}

// sum of the block's 256 values in a fixed tree; every thread gets the total
__device__ __forceinline__ double mi_block_sum(double v, double *red)
{
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = TRX_BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double mi_plogp(double p) { return p > 0.0 ? p * log(p) : 0.0; }

// MASKED: N (the host's voxel count) is replaced by N_m = (sum of the pair's counts) / TRX_MI_ONE - every voxel inside the mask added exactly
// TRX_MI_ONE, so the integer sum of the K^2 cells gives N_m exactly and in any order, without a counter of its own and without a host sync.  From
// there on the arithmetic is the unmasked instance's, operation for operation: an all-ones mask gives its bits.  N_m = 0: loss 0, G 0.
template <bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void mi_table_kernel(const unsigned long long *__restrict__ counts, unsigned N, int K, float alpha, int normalized,
                                                               const float *__restrict__ range, float *__restrict__ loss, float *__restrict__ G)
{
    __shared__ double s_p[64 * 64];
    __shared__ double s_pt[64], s_pw[64], s_red[TRX_BLOCK];
    const int b = blockIdx.x, tid = threadIdx.x, KK = K * K;
    if constexpr (MASKED) {
        __shared__ unsigned long long s_units;
        if (tid == 0) s_units = 0ull;
        __syncthreads();
        unsigned long long mine = 0ull;
        for (int i = tid; i < KK; i += TRX_BLOCK) mine += counts[(size_t)b * KK + i];
        if (mine) atomicAdd(&s_units, mine);
        __syncthreads();
        N = (unsigned)(s_units / TRX_MI_ONE);
        if (N == 0u) {                                   // an empty mask: nothing to normalise by (the whole block takes this branch)
            if (tid == 0 && loss) loss[b] = 0.f;
            if (G)
                for (int i = tid; i < KK; i += TRX_BLOCK) G[(size_t)b * KK + i] = 0.f;
            return;
        }
    }
    const double inv = 1.0 / ((double)N * (double)TRX_MI_ONE);
    for (int i = tid; i < KK; i += TRX_BLOCK) s_p[i] = (double)counts[(size_t)b * KK + i] * inv;
    __syncthreads();
    if (tid < K) {
        double s = 0.0;
        for (int k = 0; k < K; k++) s += s_p[tid * K + k];
        s_pt[tid] = s;
    } else if (tid >= 64 && tid < 64 + K) {
        const int k = tid - 64;
        double s = 0.0;
        for (int a = 0; a < K; a++) s += s_p[a * K + k];
        s_pw[k] = s;
    }
    __syncthreads();
    double e = 0.0;
    for (int i = tid; i < KK; i += TRX_BLOCK) e -= mi_plogp(s_p[i]);
    const double h_tw = mi_block_sum(e, s_red);
    const double h_t = mi_block_sum(tid < K ? -mi_plogp(s_pt[tid]) : 0.0, s_red);
    const double h_w = mi_block_sum(tid < K ? -mi_plogp(s_pw[tid]) : 0.0, s_red);
    const bool dead = normalized && !(h_tw > 0.0);
    if (tid == 0 && loss) loss[b] = (float)(normalized ? (dead ? 0.0 : (double)alpha * (2.0 - (h_t + h_w) / h_tw)) : (double)alpha * (h_tw - h_w));
    if (!G) return;
    const MiScale m = mi_scale(range, b, K);
    const double scale = (double)alpha * (double)m.s_w / (double)N;
    for (int i = tid; i < KK; i += TRX_BLOCK) {
        const double p = s_p[i];
        double g = 0.0;
        if (p > 0.0 && !dead) {
            const int a = i / K, k = i - a * K;
            const double d_tw = -log(p) - 1.0, d_w = -log(s_pw[k]) - 1.0;
            if (normalized) g = -((-log(s_pt[a]) - 1.0 + d_w) / h_tw - (h_t + h_w) * d_tw / (h_tw * h_tw));
            else g = d_tw - d_w;
        }
        G[(size_t)b * KK + i] = (float)(scale * g);
    }
}

template <bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void mi_grad_kernel(const float *__restrict__ target, const float *__restrict__ warped, unsigned N, int K,
                                                              const float *__restrict__ range, const float *__restrict__ G, float *__restrict__ grad,
                                                              const unsigned char *__restrict__ mask)
{
    extern __shared__ float mi_g[];                // [K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    for (int i = tid; i < KK; i += TRX_BLOCK) mi_g[i] = G[(size_t)b * KK + i];
    __syncthreads();
    const MiScale m = mi_scale(range, b, K);
    const float *t = target + (size_t)b * N, *w = warped + (size_t)b * N;
    float *out = grad + (size_t)b * N;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
#pragma unroll 4
    for (unsigned i = first + tid; i < last; i += TRX_BLOCK) {
        const bool on = mi_counts<MASKED>(mk, i);
        const float g = mi_voxel_grad(mi_g, mi_voxel(__builtin_nontemporal_load(t + i), __builtin_nontemporal_load(w + i), m, K), K);
        out[i] = on ? g : 0.f;                           // the array is fully written: exactly 0 outside the mask
    }
}

struct MiGeom {
    unsigned N, nchunk;
    size_t g_offset, ws_bytes;
};

static int mi_geom(int ndim, int B, int D, int H, int W, int bins, MiGeom *g)
{
    if ((ndim != 2 && ndim != 3) || (ndim == 2 && D != 1)) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || (double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    if (bins < 8 || bins > 64) return TRX_ERR_ARG;
    g->N = (unsigned)D * (unsigned)H * (unsigned)W;
    g->nchunk = (g->N + kMiChunk - 1) / kMiChunk;
    g->g_offset = ((size_t)B * bins * bins * sizeof(unsigned long long) + 255) & ~(size_t)255;
    g->ws_bytes = g->g_offset + (((size_t)B * bins * bins * sizeof(float) + 255) & ~(size_t)255);
    return TRX_OK;
}

int launch_mi_table(const unsigned long long *counts, unsigned N, int B, const trx_mi_cfg *cfg, bool from_counts, float *loss, float *G, hipStream_t s)
{
    if (cfg->mask || from_counts)
        hipLaunchKernelGGL(mi_table_kernel<true>, dim3((unsigned)B), dim3(TRX_BLOCK), 0, s, counts, N, cfg->bins, cfg->alpha, cfg->normalized ? 1 : 0, cfg->range, loss, G);
    else
        hipLaunchKernelGGL(mi_table_kernel<false>, dim3((unsigned)B), dim3(TRX_BLOCK), 0, s, counts, N, cfg->bins, cfg->alpha, cfg->normalized ? 1 : 0, cfg->range, loss, G);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_mi_workspace_bytes(int ndim, int B, int D, int H, int W, int bins)
{
    MiGeom g;
    if (mi_geom(ndim, B, D, H, W, bins, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

// Checks every entry point shares (before any HIP call), then the memset of the pair's counts and the histogram pass
static int mi_histogram_impl(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_mi_cfg *cfg, void *workspace,
                             size_t workspace_bytes, hipStream_t s, MiGeom *g)
{
    if (!target || !warped || !cfg || !cfg->range || !workspace) return TRX_ERR_ARG;
    const int rc = mi_geom(ndim, B, D, H, W, cfg->bins, g);
    if (rc != TRX_OK) return rc;
    if (!std::isfinite(cfg->alpha)) return TRX_ERR_ARG;
    if (workspace_bytes < g->ws_bytes) return TRX_ERR_WORKSPACE;
    const int K = cfg->bins, T = mi_tables(K);
    unsigned long long *counts = (unsigned long long *)workspace;
    if (hipMemsetAsync(counts, 0, (size_t)B * K * K * sizeof(unsigned long long), s) != hipSuccess) return TRX_ERR_HIP;
    const dim3 grid(g->nchunk, (unsigned)B), block(TRX_BLOCK);
    const size_t lds = (size_t)T * K * K * sizeof(unsigned long long);
    if (cfg->mask)
        hipLaunchKernelGGL(mi_hist_kernel<true>, grid, block, lds, s, target, warped, g->N, K, T, cfg->range, counts, cfg->mask);
    else
        hipLaunchKernelGGL(mi_hist_kernel<false>, grid, block, lds, s, target, warped, g->N, K, T, cfg->range, counts, (const unsigned char *)nullptr);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_mi_loss_grad(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_mi_cfg *cfg, float *loss,
                                float *grad_warped, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!loss) return TRX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    MiGeom g;
    const int rc = mi_histogram_impl(target, warped, ndim, B, D, H, W, cfg, workspace, workspace_bytes, s, &g);
    if (rc != TRX_OK) return rc;
    const int K = cfg->bins;
    float *G = (float *)((char *)workspace + g.g_offset);
    const int rc_table = launch_mi_table((const unsigned long long *)workspace, g.N, B, cfg, false, loss, grad_warped ? G : (float *)nullptr, s);
    if (rc_table != TRX_OK) return rc_table;
    if (!grad_warped) return TRX_OK;
    const dim3 grid(g.nchunk, (unsigned)B), block(TRX_BLOCK);
    if (cfg->mask)
        hipLaunchKernelGGL(mi_grad_kernel<true>, grid, block, (size_t)K * K * sizeof(float), s, target, warped, g.N, K, cfg->range, (const float *)G, grad_warped, cfg->mask);
    else
        hipLaunchKernelGGL(mi_grad_kernel<false>, grid, block, (size_t)K * K * sizeof(float), s, target, warped, g.N, K, cfg->range, (const float *)G, grad_warped,
                           (const unsigned char *)nullptr);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// The histogram pass alone: counts[B][K][K] (64-bit, TRX_MI_ONE units per voxel) at the start of the workspace, nothing else.
extern "C" int trx_mi_histogram(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_mi_cfg *cfg, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    MiGeom g;
    return mi_histogram_impl(target, warped, ndim, B, D, H, W, cfg, workspace, workspace_bytes, (hipStream_t)stream, &g);
}
