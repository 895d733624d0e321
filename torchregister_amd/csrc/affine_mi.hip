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
// Two lattices (trx_moving_grid, DESIGN.md section 4.13: trx_affine_mi_loss_grad_grids, trx_affine_mi_run_grids, trx_affine_warp_grids): the voxels walked,
// the mask and the base coordinates are the target lattice's, the sample is taken at theta (.) scale in a moving volume of its own size, and the
// reduction multiplies the sums by the scales.  Each pass and the update have ONE body (ami_hist_body / ami_grad_body / ami_update_body<.., XL>): XL picks
// theta_eff and the moving sizes (ami_pose) where the one-lattice instance reads theta in place and vol's sizes.  The __global__ kernels (*_kernel one lattice,
// *_grids_kernel two: their names and arguments are the launch interface) only forward to the body.  The sampling coordinate is affine_coord (trx_common.h),
// shared with the cross-lattice warp here, the composed warp (affine_flow.hip) and the lattice warp (affine_lattice.hip).
// Overlap only (trx_moving_grid.overlap / .mask; two lattices): a third instance of each pass (OV, *_overlap_kernel) forms the
// coordinate, tests it against [0, S - 1] on every axis and then against the moving-mask byte at rint(i), and skips the voxel in front of the sampler and of
// the target load - the masked instances' `continue`, one step later.  N_valid comes from the counts as N_m does (launch_mi_table's from_counts); the
// other instances, and the kernels that take the moving lattice without the rule (MovingLattice: the struct's first 60 bytes), keep their code.
// World geometry (trx_moving_grid.world; two lattices): a fourth instance of each pass (WD, *_world_kernel, with or without OV) whose
// prologue forms theta_eff = (L Theta R)[:ND] in fp64 from the pair's record (ami_theta_eff_world, trx_common.h) where the others form theta (.) scale - the
// voxel loop is the same statement -, an update / finalise instance that applies the matrix chain rule (ami_world_chain) behind the unchanged reduction, and
// trx_affine_world_theta, which runs the prologue's device function on its own.  The other instances keep their code (profiles/affine_mi_world_codegen.txt).
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

// The sample of the output voxel at normalised position (xn, yn, zn) under theta `th`, in a moving volume of D x H x W: value and derivative with respect
// to the un-normalised source coordinate
template <int ND>
struct AmiSample {
    float v, d[ND];
};
template <int ND>
__device__ __forceinline__ AmiSample<ND> ami_sample_at(const float *__restrict__ mov, int D, int H, int W, const float (&ic)[ND])
{
    AmiSample<ND> r;
    if constexpr (ND == 3) {
        const Samp3 s = sample3(mov, D, H, W, ic[0], ic[1], ic[2]);
        r.v = s.v; r.d[0] = s.dx; r.d[1] = s.dy; r.d[2] = s.dz;
    } else {
        const Samp2 s = sample2(mov, H, W, ic[0], ic[1]);
        r.v = s.v; r.d[0] = s.dx; r.d[1] = s.dy;
    }
    return r;
}
template <int ND>
__device__ __forceinline__ AmiSample<ND> ami_sample(const float *__restrict__ th, const float *__restrict__ mov, int D, int H, int W, float xn, float yn, float zn)
{
    float ic[ND];
    affine_coord<ND>(th, xn, yn, zn, D, H, W, ic);
    return ami_sample_at<ND>(mov, D, H, W, ic);
}
// The same under the overlap rule (OV; trx_moving_grid.overlap): the coordinate is formed by the same statement, tested
// (overlap_valid: the bounds, then the moving-mask byte), and only a valid one is sampled.  Returns false for a voxel that does not count.
template <int ND, bool OV>
__device__ __forceinline__ bool ami_sample_valid(const float *__restrict__ th, const float *__restrict__ mov, int D, int H, int W, float xn, float yn, float zn,
                                                 const unsigned char *__restrict__ mmask, AmiSample<ND> &s)
{
    if constexpr (OV) {
        float ic[ND];
        affine_coord<ND>(th, xn, yn, zn, D, H, W, ic);
        if (!overlap_valid<ND>(ic, D, H, W, mmask)) return false;
        s = ami_sample_at<ND>(mov, D, H, W, ic);
    } else {
        s = ami_sample<ND>(th, mov, D, H, W, xn, yn, zn);
    }
    return true;
}

// What a block samples pair b with: theta's row in place and vol's sizes, or (XL, two lattices: trx_moving_grid) theta_eff = theta (.) scale,
// formed once per block into `te` (ami_theta_eff, trx_common.h), and the moving lattice's sizes.  Returns the row the voxel loop reads.
// WD (world geometry: trx_moving_grid.world): theta_eff = (L Theta R)[:ND] from the pair's record `w` instead (ami_theta_eff_world).
template <int ND, bool XL, bool WD = false>
__device__ __forceinline__ const float *ami_pose(const trx_volumes &vol, const MovingLattice *mg, const float *__restrict__ th, float (&te)[ND * (ND + 1)], int &D, int &H,
                                                 int &W, const double *__restrict__ w = nullptr)
{
    if constexpr (XL) {
        if constexpr (WD) ami_theta_eff_world<ND>(th, w, te);
        else ami_theta_eff<ND>(th, *mg, te);
        D = mg->D; H = mg->H; W = mg->W;
        return te;
    } else {
        D = vol.D; H = vol.H; W = vol.W;
        return th;
    }
}

// pass 1: warp and histogram.  mg: the moving lattice (XL) or unused
// OV (two lattices only): the overlap rule - mmask: the moving masks [B][moving lattice] or nullptr
// WD (two lattices only): world geometry - world: the records [B][TRX_WORLD_STRIDE]; only the prologue differs
template <int ND, bool MASKED, bool XL, bool OV = false, bool WD = false>
__device__ __forceinline__ void ami_hist_body(const trx_volumes &vol, const MovingLattice *mg, const float *__restrict__ theta, unsigned N, int K, int T,
                                              const float *__restrict__ range, unsigned long long *__restrict__ counts, const unsigned char *__restrict__ mask,
                                              const unsigned char *__restrict__ mmask = nullptr, const double *__restrict__ world = nullptr)
{
    extern __shared__ unsigned long long ami_lds[];           // [T][K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    mi_lds_clear(ami_lds, T * KK);
    const MiScale m = mi_scale(range, b, K);
    float te[ND * (ND + 1)];
    int Dm, Hm, Wm;
    const float *__restrict__ th = ami_pose<ND, XL, WD>(vol, mg, theta + (size_t)b * TRX_PSTRIDE, te, Dm, Hm, Wm, WD ? world + (size_t)b * TRX_WORLD_STRIDE : nullptr);
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ tgt = vol.target + (size_t)b * vol.target_stride;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;      // dense, whatever target_stride says
    const unsigned char *mm = (OV && mmask) ? mmask + (size_t)b * Dm * Hm * Wm : nullptr;
    unsigned long long *mine = ami_lds + ((tid >> 6) % T) * KK;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
    for (VoxelWalk vw(first + tid, TRX_BLOCK, vol.H, vol.W); vw.i < last; vw.next(vol.H, vol.W)) {
        if (!mi_counts<MASKED>(mk, vw.i)) continue;      // before any coordinate: a voxel outside the mask costs its mask byte and nothing else
        const float xn = base_coord(vol.xn, vw.x, vol.W), yn = base_coord(vol.yn, vw.y, vol.H), zn = ND == 3 ? base_coord(vol.zn, vw.z, vol.D) : 0.f;
        AmiSample<ND> s;
        if (!ami_sample_valid<ND, OV>(th, mov, Dm, Hm, Wm, xn, yn, zn, mm, s)) continue;      // (OV) rejected behind its coordinate: nothing gathered, the target not read
        mi_accumulate(mine, mi_voxel(__builtin_nontemporal_load(tgt + vw.i), s.v, m, K), K);
    }
    __syncthreads();
    mi_flush(ami_lds, T, KK, counts + (size_t)b * KK);
}
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_hist_kernel(trx_volumes vol, const float *__restrict__ theta, unsigned N, int K, int T, const float *__restrict__ range,
                                                               unsigned long long *__restrict__ counts, const unsigned char *__restrict__ mask)
{
    ami_hist_body<ND, MASKED, false>(vol, nullptr, theta, N, K, T, range, counts, mask);
}
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_hist_grids_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, unsigned N, int K, int T,
                                                                     const float *__restrict__ range, unsigned long long *__restrict__ counts,
                                                                     const unsigned char *__restrict__ mask)
{
    ami_hist_body<ND, MASKED, true>(vol, &mg, theta, N, K, T, range, counts, mask);
}
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_hist_overlap_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, unsigned N, int K, int T,
                                                                       const float *__restrict__ range, unsigned long long *__restrict__ counts,
                                                                       const unsigned char *__restrict__ mask, const unsigned char *__restrict__ mmask)
{
    ami_hist_body<ND, MASKED, true, true>(vol, &mg, theta, N, K, T, range, counts, mask, mmask);
}
// world geometry: with (OV) or without the overlap rule; mg's scale is not read
template <int ND, bool MASKED, bool OV>
__global__ __launch_bounds__(TRX_BLOCK) void ami_hist_world_kernel(trx_volumes vol, MovingLattice mg, const double *__restrict__ world, const float *__restrict__ theta,
                                                                     unsigned N, int K, int T, const float *__restrict__ range, unsigned long long *__restrict__ counts,
                                                                     const unsigned char *__restrict__ mask, const unsigned char *__restrict__ mmask)
{
    ami_hist_body<ND, MASKED, true, OV, true>(vol, &mg, theta, N, K, T, range, counts, mask, mmask, world);
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

// pass 2: gradient rows.  XL: the rows are sums of gw * (sampler derivative in moving voxels) * (xn, yn, zn, 1) - dL/dtheta_eff up to the S / 2 of the MOVING
// sizes; the reduction behind the pass applies that and the scales.
template <int ND, bool MASKED, bool XL, bool OV = false, bool WD = false>
__device__ __forceinline__ void ami_grad_body(const trx_volumes &vol, const MovingLattice *mg, const float *__restrict__ theta, unsigned N, int K,
                                              const float *__restrict__ range, const float *__restrict__ G, float *__restrict__ partials,
                                              const unsigned char *__restrict__ mask, const unsigned char *__restrict__ mmask = nullptr,
                                              const double *__restrict__ world = nullptr)
{
    constexpr int NT = ND * (ND + 1);
    extern __shared__ float ami_g[];                // [K][K]
    const int b = blockIdx.y, tid = threadIdx.x, KK = K * K;
    for (int i = tid; i < KK; i += TRX_BLOCK) ami_g[i] = G[(size_t)b * KK + i];
    __syncthreads();
    const MiScale m = mi_scale(range, b, K);
    float te[NT];
    int Dm, Hm, Wm;
    const float *__restrict__ th = ami_pose<ND, XL, WD>(vol, mg, theta + (size_t)b * TRX_PSTRIDE, te, Dm, Hm, Wm, WD ? world + (size_t)b * TRX_WORLD_STRIDE : nullptr);
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ tgt = vol.target + (size_t)b * vol.target_stride;
    float vals[NT];
#pragma unroll
    for (int k = 0; k < NT; k++) vals[k] = 0.f;
    const unsigned char *mk = MASKED ? mask + (size_t)b * N : nullptr;
    const unsigned char *mm = (OV && mmask) ? mmask + (size_t)b * Dm * Hm * Wm : nullptr;
    const unsigned first = blockIdx.x * (unsigned)kMiChunk, last = min(N, first + (unsigned)kMiChunk);
    for (VoxelWalk vw(first + tid, TRX_BLOCK, vol.H, vol.W); vw.i < last; vw.next(vol.H, vol.W)) {
        if (!mi_counts<MASKED>(mk, vw.i)) continue;      // grad_warped is 0 there: nothing is sampled, the row below is still written (zeros if the chunk is empty)
        const float xn = base_coord(vol.xn, vw.x, vol.W), yn = base_coord(vol.yn, vw.y, vol.H), zn = ND == 3 ? base_coord(vol.zn, vw.z, vol.D) : 0.f;
        AmiSample<ND> s;
        if (!ami_sample_valid<ND, OV>(th, mov, Dm, Hm, Wm, xn, yn, zn, mm, s)) continue;      // (OV) validity is constant under the gradient: the voxel adds nothing
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
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_grad_kernel(trx_volumes vol, const float *__restrict__ theta, unsigned N, int K, const float *__restrict__ range,
                                                               const float *__restrict__ G, float *__restrict__ partials, const unsigned char *__restrict__ mask)
{
    ami_grad_body<ND, MASKED, false>(vol, nullptr, theta, N, K, range, G, partials, mask);
}
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_grad_grids_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, unsigned N, int K,
                                                                     const float *__restrict__ range, const float *__restrict__ G, float *__restrict__ partials,
                                                                     const unsigned char *__restrict__ mask)
{
    ami_grad_body<ND, MASKED, true>(vol, &mg, theta, N, K, range, G, partials, mask);
}
template <int ND, bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void ami_grad_overlap_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, unsigned N, int K,
                                                                       const float *__restrict__ range, const float *__restrict__ G, float *__restrict__ partials,
                                                                       const unsigned char *__restrict__ mask, const unsigned char *__restrict__ mmask)
{
    ami_grad_body<ND, MASKED, true, true>(vol, &mg, theta, N, K, range, G, partials, mask, mmask);
}
template <int ND, bool MASKED, bool OV>
__global__ __launch_bounds__(TRX_BLOCK) void ami_grad_world_kernel(trx_volumes vol, MovingLattice mg, const double *__restrict__ world, const float *__restrict__ theta,
                                                                     unsigned N, int K, const float *__restrict__ range, const float *__restrict__ G,
                                                                     float *__restrict__ partials, const unsigned char *__restrict__ mask,
                                                                     const unsigned char *__restrict__ mmask)
{
    ami_grad_body<ND, MASKED, true, OV, true>(vol, &mg, theta, N, K, range, G, partials, mask, mmask, world);
}

// The loop's epilogue, one block per pair: the pair's partial rows -> dL/dtheta, the loss of the table kernel, then the affine step's epilogue
// (records, pose chain rule, optimiser, theta of the next forward); the pair's counts are zeroed for the next iteration's pass 1.
// D, H, W: the sizes the sampler un-normalised with (the S / 2 per row of theta) - the moving lattice's in a cross-lattice run (XL), where the state's theta
// is the unscaled one and lane i's dL/dtheta_i = dL/dtheta_eff_i * gscale[i], formed in fp64 in front of the epilogue (gscale == 1: the same bits).
// world (XL, nullable; trx_moving_grid.world): the records - lane i's dL/dtheta_i is the matrix chain rule ami_world_chain instead, gscale is not read.
template <int ND, bool XL>
__device__ __forceinline__ void ami_update_body(const float *__restrict__ partials, int nblk, const float *__restrict__ loss, int D, int H, int W, const trx_opt_cfg &oc,
                                                const trx_affine_state &st, unsigned long long *__restrict__ counts, int KK, const float *gscale,
                                                const double *__restrict__ world = nullptr)
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
    double row_scale = scale[ic / (ND + 1)];
    if constexpr (XL) {
        float gs = 1.f;
#pragma unroll
        for (int k = 0; k < NT; k++) gs = (k == ic) ? gscale[k] : gs;      // (selects: a lane-indexed read of a kernel argument would go through scratch)
        row_scale *= (double)gs;
    }
    double dth = row_scale * S[ic];
    if constexpr (XL) {
        if (world) dth = ami_world_chain<ND>(S, scale, world + (size_t)b * TRX_WORLD_STRIDE, ic);      // block-uniform
    }
    fin_update<ND>((double)lossf, dth, bc1, rsbc2, r, b, i, oc, st, param, theta, am, av, st.step + b, true, nullptr, sh_dth, sh_pose);
}
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_update_kernel(const float *__restrict__ partials, int nblk, const float *__restrict__ loss, int D, int H, int W,
                                                                     trx_opt_cfg oc, trx_affine_state st, unsigned long long *__restrict__ counts, int KK)
{
    ami_update_body<ND, false>(partials, nblk, loss, D, H, W, oc, st, counts, KK, nullptr);
}
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_update_grids_kernel(const float *__restrict__ partials, int nblk, const float *__restrict__ loss, MovingLattice mg,
                                                                           trx_opt_cfg oc, trx_affine_state st, unsigned long long *__restrict__ counts, int KK)
{
    ami_update_body<ND, true>(partials, nblk, loss, mg.D, mg.H, mg.W, oc, st, counts, KK, mg.scale);
}
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_update_world_kernel(const float *__restrict__ partials, int nblk, const float *__restrict__ loss, MovingLattice mg,
                                                                           const double *__restrict__ world, trx_opt_cfg oc, trx_affine_state st,
                                                                           unsigned long long *__restrict__ counts, int KK)
{
    ami_update_body<ND, true>(partials, nblk, loss, mg.D, mg.H, mg.W, oc, st, counts, KK, mg.scale, world);
}

// Behind one cross-lattice evaluation: launch_bwd_finalize's reduction (reduce_partials' fixed order) with the moving sizes in S / 2 and the scales on top,
// dtheta[k] = (S_row / 2 * scale[k]) * sum - one rounding to fp32, as there.
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_grids_finalize_kernel(const float *__restrict__ partials, int nblk, MovingLattice mg, float *__restrict__ dtheta)
{
    constexpr int NT = ND * (ND + 1);
    __shared__ double S[64];
    const int b = blockIdx.x, i = threadIdx.x;
    reduce_partials<NT>(partials + (size_t)b * nblk * NT, nblk, S);
    if (i >= NT) return;
    const double scale[3] = {0.5 * mg.W, 0.5 * mg.H, 0.5 * mg.D};
    float gs = 1.f;
#pragma unroll
    for (int k = 0; k < NT; k++) gs = (k == i) ? mg.scale[k] : gs;
    dtheta[(size_t)b * TRX_PSTRIDE + i] = (float)(scale[i / (ND + 1)] * (double)gs * S[i]);
}

// ... and under world geometry: the matrix chain rule (ami_world_chain) on the same reduction
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void ami_world_finalize_kernel(const float *__restrict__ partials, int nblk, MovingLattice mg, const double *__restrict__ world,
                                                                             float *__restrict__ dtheta)
{
    constexpr int NT = ND * (ND + 1);
    __shared__ double S[64];
    const int b = blockIdx.x, i = threadIdx.x;
    reduce_partials<NT>(partials + (size_t)b * nblk * NT, nblk, S);
    if (i >= NT) return;
    const double scale[3] = {0.5 * mg.W, 0.5 * mg.H, 0.5 * mg.D};
    dtheta[(size_t)b * TRX_PSTRIDE + i] = (float)ami_world_chain<ND>(S, scale, world + (size_t)b * TRX_WORLD_STRIDE, i);
}

// trx_affine_world_theta: one thread per pair runs the passes' own statement
template <int ND>
__global__ void ami_world_theta_kernel(const double *__restrict__ world, const float *__restrict__ theta, int B, float *__restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float raw[ND * (ND + 1)];
    ami_world_theta<ND>(theta + (size_t)b * TRX_PSTRIDE, world + (size_t)b * TRX_WORLD_STRIDE, raw);
#pragma unroll
    for (int k = 0; k < TRX_PSTRIDE; k++) out[(size_t)b * TRX_PSTRIDE + k] = k < ND * (ND + 1) ? raw[k] : 0.f;
}

// The cross-lattice forward warp (trx_affine_warp_grids): affine_warp_kernel's walk over the TARGET lattice (vol's sizes and tables), every channel sampled in
// a moving volume of mg's sizes at theta_eff (formed once per block, as in the two passes).  chan_stride: moving voxels between channels.
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void affine_warp_grids_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, int channels,
                                                                      size_t chan_stride, float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int Dm = mg.D, Hm = mg.H, Wm = mg.W;
    const size_t nvox = (size_t)vol.D * vol.H * vol.W;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    float *__restrict__ o = out + (size_t)b * channels * nvox;
    float th[ND * (ND + 1)];
    ami_theta_eff<ND>(theta + (size_t)b * TRX_PSTRIDE, mg, th);
    for (VoxelWalk vw(blockIdx.x * TRX_BLOCK + threadIdx.x, gridDim.x * TRX_BLOCK, vol.H, vol.W); vw.i < nvox; vw.next(vol.H, vol.W)) {
        const float xn = base_coord(vol.xn, vw.x, vol.W), yn = base_coord(vol.yn, vw.y, vol.H), zn = ND == 3 ? base_coord(vol.zn, vw.z, vol.D) : 0.f;
        float ic[ND];
        affine_coord<ND>(th, xn, yn, zn, Dm, Hm, Wm, ic);
        for (int ch = 0; ch < channels; ch++) {
            if constexpr (ND == 3) o[ch * nvox + vw.i] = sample3(mov + ch * chan_stride, Dm, Hm, Wm, ic[0], ic[1], ic[2]).v;
            else o[ch * nvox + vw.i] = sample2(mov + ch * chan_stride, Hm, Wm, ic[0], ic[1]).v;
        }
    }
}

// pass 1 -> table -> (need_grad) pass 2 of one evaluation at `theta`; the counts must be zero.  mg != nullptr: the cross-lattice instances
static int ami_evaluate(const trx_volumes *vol, const trx_moving_grid *mg, const trx_mi_cfg *cfg, const AmiGeom &g, const float *theta, float *loss, bool need_grad,
                        void *workspace, hipStream_t s)
{
    const int K = cfg->bins, T = mi_tables(K);
    unsigned long long *counts = (unsigned long long *)workspace;
    float *G = (float *)((char *)workspace + g.o_g), *partials = (float *)((char *)workspace + g.o_part);
    const dim3 grid(g.nchunk, (unsigned)vol->B), block(TRX_BLOCK);
    const unsigned char *mask = cfg->mask;               // read here on every evaluation, so on every iteration of the loop
    const bool ov = mg && mg->overlap;                   // the overlap rule: N_valid comes from the counts, as N_m does under a mask
    const double *wd = mg ? mg->world : nullptr;         // world geometry: the *_world_kernel instances
    const size_t lds = (size_t)T * K * K * sizeof(unsigned long long);
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (wd) {
            const unsigned char *mm = ov ? mg->mask : nullptr;
            if (ov && mask) hipLaunchKernelGGL((ami_hist_world_kernel<ND, true, true>), grid, block, lds, s, *vol, *mg, wd, theta, g.N, K, T, cfg->range, counts, mask, mm);
            else if (ov) hipLaunchKernelGGL((ami_hist_world_kernel<ND, false, true>), grid, block, lds, s, *vol, *mg, wd, theta, g.N, K, T, cfg->range, counts, mask, mm);
            else if (mask) hipLaunchKernelGGL((ami_hist_world_kernel<ND, true, false>), grid, block, lds, s, *vol, *mg, wd, theta, g.N, K, T, cfg->range, counts, mask, mm);
            else hipLaunchKernelGGL((ami_hist_world_kernel<ND, false, false>), grid, block, lds, s, *vol, *mg, wd, theta, g.N, K, T, cfg->range, counts, mask, mm);
        } else if (ov) {
            if (mask) hipLaunchKernelGGL((ami_hist_overlap_kernel<ND, true>), grid, block, lds, s, *vol, *mg, theta, g.N, K, T, cfg->range, counts, mask, mg->mask);
            else hipLaunchKernelGGL((ami_hist_overlap_kernel<ND, false>), grid, block, lds, s, *vol, *mg, theta, g.N, K, T, cfg->range, counts, mask, mg->mask);
        } else if (mg) {
            if (mask) hipLaunchKernelGGL((ami_hist_grids_kernel<ND, true>), grid, block, lds, s, *vol, *mg, theta, g.N, K, T, cfg->range, counts, mask);
            else hipLaunchKernelGGL((ami_hist_grids_kernel<ND, false>), grid, block, lds, s, *vol, *mg, theta, g.N, K, T, cfg->range, counts, mask);
        } else if (mask) hipLaunchKernelGGL((ami_hist_kernel<ND, true>), grid, block, lds, s, *vol, theta, g.N, K, T, cfg->range, counts, mask);
        else hipLaunchKernelGGL((ami_hist_kernel<ND, false>), grid, block, lds, s, *vol, theta, g.N, K, T, cfg->range, counts, mask);
    });
    TRX_CHECK_LAUNCH();
    const int rc = launch_mi_table(counts, g.N, vol->B, cfg, ov, loss, need_grad ? G : (float *)nullptr, s);
    if (rc != TRX_OK || !need_grad) return rc;
    const size_t glds = (size_t)K * K * sizeof(float);
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (wd) {
            const unsigned char *mm = ov ? mg->mask : nullptr;
            if (ov && mask) hipLaunchKernelGGL((ami_grad_world_kernel<ND, true, true>), grid, block, glds, s, *vol, *mg, wd, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mm);
            else if (ov) hipLaunchKernelGGL((ami_grad_world_kernel<ND, false, true>), grid, block, glds, s, *vol, *mg, wd, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mm);
            else if (mask) hipLaunchKernelGGL((ami_grad_world_kernel<ND, true, false>), grid, block, glds, s, *vol, *mg, wd, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mm);
            else hipLaunchKernelGGL((ami_grad_world_kernel<ND, false, false>), grid, block, glds, s, *vol, *mg, wd, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mm);
        } else if (ov) {
            if (mask) hipLaunchKernelGGL((ami_grad_overlap_kernel<ND, true>), grid, block, glds, s, *vol, *mg, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mg->mask);
            else hipLaunchKernelGGL((ami_grad_overlap_kernel<ND, false>), grid, block, glds, s, *vol, *mg, theta, g.N, K, cfg->range, (const float *)G, partials, mask, mg->mask);
        } else if (mg) {
            if (mask) hipLaunchKernelGGL((ami_grad_grids_kernel<ND, true>), grid, block, glds, s, *vol, *mg, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
            else hipLaunchKernelGGL((ami_grad_grids_kernel<ND, false>), grid, block, glds, s, *vol, *mg, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
        } else if (mask) hipLaunchKernelGGL((ami_grad_kernel<ND, true>), grid, block, glds, s, *vol, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
        else hipLaunchKernelGGL((ami_grad_kernel<ND, false>), grid, block, glds, s, *vol, theta, g.N, K, cfg->range, (const float *)G, partials, mask);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// (what the cross-lattice entry points refuse on top of the others: ami_grid_check, affine_host.h)
// what the entry points refuse, before any HIP call (grids: a cross-lattice entry point, mg its moving lattice); the workspace size comes last
static int ami_check(const trx_volumes *vol, const trx_moving_grid *mg, bool grids, const trx_mi_cfg *cfg, const void *workspace, size_t workspace_bytes, AmiGeom *g)
{
    if (!vol || !cfg || !cfg->range || !workspace || !vol->moving || !vol->target || (grids && !mg)) return TRX_ERR_ARG;
    int rc = ami_geom(vol, cfg->bins, g);
    if (rc == TRX_OK && grids) rc = ami_grid_check(vol->ndim, mg, true);
    if (rc != TRX_OK) return rc;
    if (!std::isfinite(cfg->alpha)) return TRX_ERR_ARG;
    if (grids && mg->mask && !mg->overlap) return TRX_ERR_ARG;      // a moving mask is part of the overlap rule
    if (workspace_bytes < g->ws_bytes) return TRX_ERR_WORKSPACE;
    return TRX_OK;
}

// the entry points proper; mg == nullptr: one lattice, the launches of before
static int ami_loss_grad(const trx_volumes *vol, const trx_moving_grid *mg, const trx_mi_cfg *cfg, const float *theta, float *loss, float *dtheta, void *workspace,
                         size_t workspace_bytes, bool grids, void *stream)
{
    if (!theta || !loss) return TRX_ERR_ARG;
    AmiGeom g;
    int rc = ami_check(vol, mg, grids, cfg, workspace, workspace_bytes, &g);
    if (rc != TRX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, (size_t)vol->B * cfg->bins * cfg->bins * sizeof(unsigned long long), s) != hipSuccess) return TRX_ERR_HIP;
    rc = ami_evaluate(vol, mg, cfg, g, theta, loss, dtheta != nullptr, workspace, s);
    if (rc != TRX_OK || !dtheta) return rc;
    const float *partials = (const float *)((char *)workspace + g.o_part);
    if (!mg) return launch_bwd_finalize(vol, partials, (int)g.nchunk, dtheta, s);
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (mg->world) hipLaunchKernelGGL((ami_world_finalize_kernel<ND>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, *mg, mg->world, dtheta);
        else hipLaunchKernelGGL((ami_grids_finalize_kernel<ND>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, *mg, dtheta);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

static int ami_run(const trx_volumes *vol, const trx_moving_grid *mg, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_affine_state *st, int iters,
                   void *workspace, size_t workspace_bytes, bool grids, void *stream)
{
    if (iters < 0 || !st || !opt) return TRX_ERR_ARG;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    AmiGeom g;
    int rc = ami_check(vol, mg, grids, cfg, workspace, workspace_bytes, &g);
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
        const int r = ami_evaluate(vol, mg, cfg, g, st->theta, loss, true, workspace, s);
        if (r != TRX_OK) return r;
        with_ndim(vol->ndim, [&](auto nd) {
            constexpr int ND = decltype(nd)::value;
            if (mg && mg->world) hipLaunchKernelGGL((ami_update_world_kernel<ND>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, (const float *)loss, *mg, mg->world, *opt, *st, counts, KK);
            else if (mg) hipLaunchKernelGGL((ami_update_grids_kernel<ND>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, (const float *)loss, *mg, *opt, *st, counts, KK);
            else hipLaunchKernelGGL((ami_update_kernel<ND>), dim3((unsigned)vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, (int)g.nchunk, (const float *)loss, vol->D, vol->H, vol->W, *opt, *st, counts, KK);
        });
        TRX_CHECK_LAUNCH();
    }
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
    return ami_loss_grad(vol, nullptr, cfg, theta, loss, dtheta, workspace, workspace_bytes, false, stream);
}

extern "C" int trx_affine_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_affine_state *st, int iters, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return ami_run(vol, nullptr, cfg, opt, st, iters, workspace, workspace_bytes, false, stream);
}

extern "C" int trx_affine_mi_loss_grad_grids(const trx_volumes *vol, const trx_moving_grid *mg, const trx_mi_cfg *cfg, const float *theta, float *loss, float *dtheta,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    return ami_loss_grad(vol, mg, cfg, theta, loss, dtheta, workspace, workspace_bytes, true, stream);
}

extern "C" int trx_affine_mi_run_grids(const trx_volumes *vol, const trx_moving_grid *mg, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_affine_state *st,
                                       int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    return ami_run(vol, mg, cfg, opt, st, iters, workspace, workspace_bytes, true, stream);
}

extern "C" int trx_affine_warp_grids(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, int channels, float *out, void *stream)
{
    if (!mg) return TRX_ERR_ARG;
    int rc = check_vol(vol, false);
    if (rc == TRX_OK) rc = ami_grid_check(vol->ndim, mg);
    if (rc != TRX_OK) return rc;
    if (!theta || !out || channels < 1) return TRX_ERR_ARG;
    const int nt = vol->ndim * (vol->ndim + 1);
    bool same = mg->D == vol->D && mg->H == vol->H && mg->W == vol->W;
    for (int k = 0; k < nt; k++) same = same && mg->scale[k] == 1.0f;
    if (same) return trx_affine_warp(vol, theta, channels, out, stream);      // one lattice: the warp of before (its tiled kernels in 3-D), the same bits
    hipStream_t s = (hipStream_t)stream;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W, nmov = (size_t)mg->D * mg->H * mg->W;
    size_t nb = (nvox + TRX_BLOCK - 1) / TRX_BLOCK;
    if (nb > 8192) nb = 8192;
    const dim3 grid((unsigned)nb, (unsigned)vol->B), block(TRX_BLOCK);
    with_ndim(vol->ndim, [&](auto nd) {
        hipLaunchKernelGGL((affine_warp_grids_kernel<decltype(nd)::value>), grid, block, 0, s, *vol, *mg, theta, channels, nmov, out);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_affine_world_theta(const trx_moving_grid *mg, int ndim, int B, const float *theta, float *theta_eff, void *stream)
{
    if (!mg || !mg->world || !theta || !theta_eff || B < 1 || B > 65535) return TRX_ERR_ARG;
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    with_ndim(ndim, [&](auto nd) {
        hipLaunchKernelGGL((ami_world_theta_kernel<decltype(nd)::value>), dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, mg->world, theta, B, theta_eff);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
