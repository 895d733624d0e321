// Rigid / affine registration under the Parzen joint-histogram mutual information (csrc/mi.hip, include/trx.h: trx_mi_loss_grad) without a warped
// volume: trx_affine_mi_loss_grad and the device-side loop trx_affine_mi_run.  DESIGN.md section 4.10.
//
// Per evaluation, for all B pairs (each with its own theta and its own range), behind one memset of the pair tables:
//   ami_hist_kernel   pass 1.  A block takes kMiChunk consecutive output voxels of one pair (waves along x), forms the sampling coordinate from theta with the
//                     arithmetic of the row-walking affine kernels (affine_accum_kernel: base-coordinate tables or the closed form, unnorm<ND>), samples
//                     moving (sample3 / sample2: zero padding), reads target and adds the voxel to the block's LDS tables exactly as mi_hist_kernel does
//                     (mi_dev.h: fixed point, 64-bit integer adds, LDS then global).  8 B/voxel read (moving through the caches), nothing written.
//   mi_table_kernel   unchanged (mi.hip, through launch_mi_table): loss[b] and G = d loss / d P scaled by s_w / N.
//   ami_grad_kernel   pass 2.  The same voxels, the same sampling arithmetic (so the same bins), gw = [inside] sum_j G[a][c - 1 + j] beta'_j(r) from the
//                     pair's G in LDS, times the sampler's spatial derivative, times d coordinate / d theta = (xn, yn, zn, 1): nd (nd + 1) sums per
//                     thread (fp32, ascending voxels), the block's sum in fp64 in a fixed order -> one partial row per block.  8 B/voxel read, 48 B per block written.
//   launch_bwd_finalize (one evaluation) / ami_update_kernel (the loop)   one block per pair: the partial rows in fp64 in reduce_partials' fixed order, scaled by S / 2 per row of theta - what
//                     trx_affine_warp_backward returns for grad_out = gw - then (the loop) the epilogue of the affine step (fin_load / fin_update).
// A pair gets ceil(N / kMiChunk) blocks and partial rows: a function of (D, H, W) alone.  Integer histogram sums are associative, every float sum
// has a fixed order: a pair's loss and gradient are the same bits on every call and whatever batch surrounds it.  No float atomics.
// The loop's update kernel also zeroes the pair's counts for the next iteration, so an iteration is four launches: pass 1, table, pass 2, update.
// Region of interest (cfg->mask): both passes have a second instance that reads the voxel's mask byte first (9 B/voxel inside the
// mask, 1 outside) and skips a voxel outside it before any coordinate is formed - nothing is sampled, nothing enters the LDS tables or the thread's
// sums.  A block whose chunk lies wholly outside the mask still clears and flushes (adding nothing) and still writes its partial row (zeros): the
// reduction reads a fixed number of rows.  The table kernel takes N_m from the counts; the update kernel zeroes all K x K cells, masked or not.
#include "affine_finalize.h"   // reduce_partials, fin_load / fin_update (the epilogue of the affine step), launch_bwd_finalize (affine_host.h)
#include "mi_dev.h"

#include <cmath>

namespace trx {

struct AmiGeom {
    unsigned N, nchunk;
    int nt;                                         // nd (nd + 1): floats per partial row
    size_t o_g, o_part, o_loss, ws_bytes;           // counts at 0 | G | partial rows | loss [B] (the loop's)
};

static size_t ami_align(size_t n) { return (n + 255) & ~(size_t)255; }

// the batch geometry without its pointers (the workspace query is host arithmetic on sizes) and the layout of the workspace
static int ami_geom(const trx_volumes *v, int bins, AmiGeom *g)
{
    if (!v) return TRX_ERR_ARG;
    if ((v->ndim != 2 && v->ndim != 3) || (v->ndim == 2 && v->D != 1)) return TRX_ERR_NDIM;
    if (v->B < 1 || v->B > 65535 || v->D < 1 || v->H < 1 || v->W < 1 || (double)v->D * v->H * v->W >= 2147483648.0) return TRX_ERR_ARG;
    if (bins < 8 || bins > 64) return TRX_ERR_ARG;
    const size_t B = (size_t)v->B, KK = (size_t)bins * bins;
    g->N = (unsigned)v->D * (unsigned)v->H * (unsigned)v->W;
    g->nchunk = (g->N + kMiChunk - 1) / kMiChunk;
    g->nt = v->ndim * (v->ndim + 1);
    g->o_g = ami_align(B * KK * sizeof(unsigned long long));
    g->o_part = g->o_g + ami_align(B * KK * sizeof(float));
    g->o_loss = g->o_part + ami_align(B * g->nchunk * g->nt * sizeof(float));
    g->ws_bytes = g->o_loss + ami_align(B * sizeof(float));
    return TRX_OK;
}

// The sample of output voxel (x, y, z) of pair theta `th`: value and derivative with respect to the un-normalised source coordinate
template <int ND>
struct AmiSample {
    float v, d[ND];
};
template <int ND>
__device__ __forceinline__ AmiSample<ND> ami_sample(const trx_volumes &vol, const float *__restrict__ th, const float *__restrict__ mov, int x, int y, int z, float xn,
                                                    float yn, float zn)
{
    const int D = vol.D, H = vol.H, W = vol.W;
    AmiSample<ND> r;
    if constexpr (ND == 3) {
        const float ix = unnorm<3>(fmaf(th[1], yn, fmaf(th[0], xn, fmaf(th[2], zn, th[3]))), (float)W);
        const float iy = unnorm<3>(fmaf(th[5], yn, fmaf(th[4], xn, fmaf(th[6], zn, th[7]))), (float)H);
        const float iz = unnorm<3>(fmaf(th[9], yn, fmaf(th[8], xn, fmaf(th[10], zn, th[11]))), (float)D);
        const Samp3 s = sample3(mov, D, H, W, ix, iy, iz);
        r.v = s.v; r.d[0] = s.dx; r.d[1] = s.dy; r.d[2] = s.dz;
    } else {
        const float ix = unnorm<2>(fmaf(th[1], yn, fmaf(th[0], xn, th[2])), (float)W);
        const float iy = unnorm<2>(fmaf(th[4], yn, fmaf(th[3], xn, th[5])), (float)H);
        const Samp2 s = sample2(mov, H, W, ix, iy);
        r.v = s.v; r.d[0] = s.dx; r.d[1] = s.dy;
    }
    return r;
}

// pass 1: warp and histogram
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_hist_kernel(trx_volumes vol, const float *__restrict__ theta, unsigned N, int K, int T, const float *__restrict__ range,
                                                               unsigned long long *__restrict__ counts, const unsigned char *__restrict__ mask)
{
    extern __shared__ unsigned long long ami_lds[];           // [T][K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    mi_lds_clear(ami_lds, T * KK);
    const MiScale m = mi_scale(range, b, K);
    const float *__restrict__ th = theta + (size_t)b * TRX_PSTRIDE;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ tgt = vol.target + (size_t)b * vol.target_stride;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;      // dense, whatever target_stride says
    unsigned long long *mine = ami_lds + ((tid >> 6) % T) * KK;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
    for (VoxelWalk vw(first + tid, TRX_BLOCK, vol.H, vol.W); vw.i < last; vw.next(vol.H, vol.W)) {
        if (!mi_counts<MASKED>(mk, vw.i)) continue;      // before any coordinate: a voxel outside the mask costs its mask byte and nothing else
        const float xn = base_coord(vol.xn, vw.x, vol.W), yn = base_coord(vol.yn, vw.y, vol.H), zn = ND == 3 ? base_coord(vol.zn, vw.z, vol.D) : 0.f;
        const AmiSample<ND> s = ami_sample<ND>(vol, th, mov, vw.x, vw.y, vw.z, xn, yn, zn);
        mi_accumulate(mine, mi_voxel(__builtin_nontemporal_load(tgt + vw.i), s.v, m, K), K);
    }
    __syncthreads();
    mi_flush(ami_lds, T, KK, counts + (size_t)b * KK);
}

// The block's 256 x NV per-thread sums -> out[NV]: fp64 from here on (a voxel's terms cancel to a gradient orders of magnitude below them, and the
// fused pass may not be noisier than the warped-volume chain it replaces), a fixed shuffle tree per wave, the four waves in order, one rounding to
// fp32 per row entry.  Every thread of the block calls it.
template <int NV>
__device__ __forceinline__ void ami_block_sum_store(const float (&vals)[NV], float *__restrict__ out)
{
    __shared__ double wsum[TRX_WAVES][NV];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; k++) {
        double v = (double)vals[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) wsum[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < TRX_WAVES; w++) t += wsum[w][threadIdx.x];
        out[threadIdx.x] = (float)t;
    }
}

// pass 2: gradient rows
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_grad_kernel(trx_volumes vol, const float *__restrict__ theta, unsigned N, int K, const float *__restrict__ range,
                                                               const float *__restrict__ G, float *__restrict__ partials, const unsigned char *__restrict__ mask)
{
    constexpr int NT = ND * (ND + 1);
    extern __shared__ float ami_g[];                // [K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    for (int i = tid; i < KK; i += TRX_BLOCK) ami_g[i] = G[(size_t)b * KK + i];
    __syncthreads();
    const MiScale m = mi_scale(range, b, K);
    const float *__restrict__ th = theta + (size_t)b * TRX_PSTRIDE;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ tgt = vol.target + (size_t)b * vol.target_stride;
    float vals[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) vals[k] = 0.f;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
    for (VoxelWalk vw(first + tid, TRX_BLOCK, vol.H, vol.W); vw.i < last; vw.next(vol.H, vol.W)) {
        if (!mi_counts<MASKED>(mk, vw.i)) continue;      // grad_warped is 0 there: nothing is sampled, the row below is still written (zeros if the chunk is empty)
        const float xn = base_coord(vol.xn, vw.x, vol.W), yn = base_coord(vol.yn, vw.y, vol.H), zn = ND == 3 ? base_coord(vol.zn, vw.z, vol.D) : 0.f;
        const AmiSample<ND> s = ami_sample<ND>(vol, th, mov, vw.x, vw.y, vw.z, xn, yn, zn);
        const float gw = mi_voxel_grad(ami_g, mi_voxel(__builtin_nontemporal_load(tgt + vw.i), s.v, m, K), K);
#pragma unroll
        for (int c = 0; c < ND; c++) {      // row c of theta: d coordinate_c / d theta[c][.] = (xn, yn, zn, 1)
            const float q = gw * s.d[c];
            float *row = vals + c * (ND + 1);
            row[0] = fmaf(xn, q, row[0]);
            row[1] = fmaf(yn, q, row[1]);
            if constexpr (ND == 3) row[2] = fmaf(zn, q, row[2]);
            row[ND] += q;
        }
    }
    ami_block_sum_store<NT>(vals, partials + ((size_t)b * gridDim.x + blockIdx.x) * NT);
}

// The loop's epilogue, one block per pair: the pair's partial rows -> dL/dtheta, the loss of the table kernel, then the affine step's epilogue
// (records, pose chain rule, optimiser, theta of the next forward); the pair's counts are zeroed for the next iteration's pass 1.
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_update_kernel(const float *__restrict__ partials, int nblk, const float *__restrict__ loss, int D, int H, int W,
                                                                     trx_opt_cfg oc, trx_affine_state st, unsigned long long *__restrict__ counts, int KK)
{
    constexpr int NT = ND * (ND + 1);
    constexpr int NPOSE = (ND == 3) ? 6 : 3;
    __shared__ double S[64];
    __shared__ double sh_dth[NT];
    __shared__ float sh_pose[NPOSE];
    const int b = blockIdx.x, i = threadIdx.x;
    const bool rigid = st.mode == TRX_PARAM_RIGID;
    float *param = st.param + (size_t)b * TRX_PSTRIDE, *theta = st.theta + (size_t)b * TRX_PSTRIDE;
    float *am = st.adam_m ? st.adam_m + (size_t)b * TRX_PSTRIDE : nullptr, *av = st.adam_v ? st.adam_v + (size_t)b * TRX_PSTRIDE : nullptr;
    FinRegs<ND> r;
    float lossf = 0.f;
    if (i < 64) {
        r = fin_load<ND>(param, theta, am, av, st.step + b, st.best_loss + b, oc.kind == TRX_OPT_ADAM, rigid, i);
        lossf = loss[b];
    }
    reduce_partials<NT>(partials + (size_t)b * nblk * NT, nblk, S);
    for (int k = i; k < KK; k += TRX_FIN_THREADS) counts[(size_t)b * KK + k] = 0ull;
    if (i >= 64) return;
    const double scale[3] = {0.5 * W, 0.5 * H, 0.5 * D};
    const int ic = min(i, NT - 1);
    double bc1, rsbc2;
    fin_bias(oc, r.t, bc1, rsbc2);
    fin_update<ND>((double)lossf, scale[ic / (ND + 1)] * S[ic], bc1, rsbc2, r, b, i, oc, st, param, theta, am, av, st.step + b, true, nullptr, sh_dth, sh_pose);
}

// pass 1 -> table -> (need_grad) pass 2 of one evaluation at `theta`; the counts must be zero
static int ami_evaluate(const trx_volumes *vol, const trx_mi_cfg *cfg, const AmiGeom &g, const float *theta, float *loss, bool need_grad, void *workspace, hipStream_t s)
{
    const int K = cfg->bins, T = mi_tables(K);
    unsigned long long *counts = (unsigned long long *)workspace;
    float *G = (float *)((char *)workspace + g.o_g), *partials = (float *)((char *)workspace + g.o_part);
    const dim3 grid(g.nchunk, (unsigned)vol->B), block(TRX_BLOCK);
    const unsigned char *mask = cfg->mask;               // read here on every evaluation, so on every iteration of the loop
    const size_t lds = (size_t)T * K * K * sizeof(unsigned long long);
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (mask) hipLaunchKernelGGL((ami_hist_kernel<ND, true>), grid, block, lds, s, *vol, theta, g.N, K, T, cfg->range, counts, mask);
        else hipLaunchKernelGGL((ami_hist_kernel<ND, false>), grid, block, lds, s, *vol, theta, g.N, K, T, cfg->range, counts, mask);
    });
    TRX_CHECK_LAUNCH();
    const int rc = launch_mi_table(counts, g.N, vol->B, cfg, loss, need_grad ? G : (float *)nullptr, s);
    if (rc != TRX_OK || !need_grad) return rc;
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (mask) hipLaunchKernelGGL((ami_grad_kernel<ND, true>), grid, block, (size_t)K * K * sizeof(float), s, *vol, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
        else hipLaunchKernelGGL((ami_grad_kernel<ND, false>), grid, block, (size_t)K * K * sizeof(float), s, *vol, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// what both entry points refuse, before any HIP call
static int ami_check(const trx_volumes *vol, const trx_mi_cfg *cfg, const void *workspace, size_t workspace_bytes, AmiGeom *g)
{
    if (!vol || !cfg || !cfg->range || !workspace || !vol->moving || !vol->target) return TRX_ERR_ARG;
    const int rc = ami_geom(vol, cfg->bins, g);
    if (rc != TRX_OK) return rc;
    if (!std::isfinite(cfg->alpha)) return TRX_ERR_ARG;
    if (workspace_bytes < g->ws_bytes) return TRX_ERR_WORKSPACE;
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_affine_mi_workspace_bytes(const trx_volumes *vol, int bins)
{
    AmiGeom g;
    if (ami_geom(vol, bins, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

extern "C" int trx_affine_mi_loss_grad(const trx_volumes *vol, const trx_mi_cfg *cfg, const float *theta, float *loss, float *dtheta, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if (!theta || !loss) return TRX_ERR_ARG;
    AmiGeom g;
    int rc = ami_check(vol, cfg, workspace, workspace_bytes, &g);
    if (rc != TRX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, (size_t)vol->B * cfg->bins * cfg->bins * sizeof(unsigned long long), s) != hipSuccess) return TRX_ERR_HIP;
    rc = ami_evaluate(vol, cfg, g, theta, loss, dtheta != nullptr, workspace, s);
    if (rc != TRX_OK || !dtheta) return rc;
    return launch_bwd_finalize(vol, (const float *)((char *)workspace + g.o_part), (int)g.nchunk, dtheta, s);
}

extern "C" int trx_affine_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_affine_state *st, int iters, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (iters < 0 || !st || !opt) return TRX_ERR_ARG;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    AmiGeom g;
    const int rc = ami_check(vol, cfg, workspace, workspace_bytes, &g);
    if (rc != TRX_OK) return rc;
    if (!st->param || !st->theta || !st->best_theta || !st->best_loss || !st->best_idx || !st->step) return TRX_ERR_ARG;
    if (opt->kind != TRX_OPT_SGD && opt->kind != TRX_OPT_ADAM) return TRX_ERR_ARG;
    if (opt->kind == TRX_OPT_ADAM && (!st->adam_m || !st->adam_v)) return TRX_ERR_ARG;
    if (st->mode != TRX_PARAM_AFFINE && st->mode != TRX_PARAM_RIGID) return TRX_ERR_ARG;
    if (iters == 0) return TRX_OK;
    hipStream_t s = (hipStream_t)stream;
    const int KK = cfg->bins * cfg->bins;
    unsigned long long *counts = (unsigned long long *)workspace;
    float *loss = (float *)((char *)workspace + g.o_loss);
    const float *partials = (const float *)((char *)workspace + g.o_part);
    if (hipMemsetAsync(counts, 0, (size_t)vol->B * KK * sizeof(unsigned long long), s) != hipSuccess) return TRX_ERR_HIP;
    for (int k = 0; k < iters; k++) {
        const int r = ami_evaluate(vol, cfg, g, st->theta, loss, true, workspace, s);
        if (r != TRX_OK) return r;
        with_ndim(vol->ndim, [&](auto nd) {
            hipLaunchKernelGGL((ami_update_kernel<decltype(nd)::value>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, (const float *)loss, vol->D,
                               vol->H, vol->W, *opt, *st, counts, KK);
        });
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}
