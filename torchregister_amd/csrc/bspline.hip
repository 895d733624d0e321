// Cubic B-spline free-form deformation (Rueckert et al. 1999; extension, the reference has no such model): the operator between a control
// lattice and a dense flow (trx_bspline_expand), its exact adjoint (trx_bspline_reduce) and a device-side optimisation loop over them
// (trx_bspline_run).  CPU restatement: tests/bspline_ref.py.
//
// Definition (include/trx.h): an axis of S voxels with spacing d has G = (S - 1) / d + 4 control points, point i at voxel (i - 1) d; at
// voxel x, i0 = x / d, t = (x % d) / d and the four weights B0..B3(t) of the uniform cubic B-spline act on points i0 .. i0 + 3 (always
// inside the lattice).  There are only min(d, S) distinct weight quadruples per axis: every block forms them in fp64, rounds them to
// fp32 once and keeps them in LDS.
//
// Both operators are separable and run as one 1-D pass per axis:
//   expand  z, y, x: the lattice grows one axis at a time, so only the x pass touches a full-size array (it writes the flow, and reads
//           `base` when there is one); its reads of the [D][H][Gx] intermediate are cache hits (each value serves d voxels of a row);
//   reduce  x, y, z: the x pass reads dflow exactly once - a tile of rows goes through LDS, where each voxel is used by its four control
//           points - and the y and z passes run on arrays W / dx times smaller.
// Every sum runs in a fixed order (expand: l = 0..3 per voxel; reduce: each of a control point's four cells in ascending voxel order,
// then the four partial sums from the farthest cell to the nearest) with no atomics: the same bits on every call, and a volume's result
// does not depend on the volumes around it.  Intermediates live in the caller's workspace.
//
// Cache hints: `base` and `dflow` are read once per call and carry the non-temporal hint; the flow written by expand is
// read again at once by the loss-and-gradient passes behind it, so its stores carry none.
#include "trx_common.h"

#include <algorithm>

namespace trx {

#define TRX_BSPLINE_MAX_SPACING 1024   // the weight table of an axis (16 B per entry) and a 4-point span of the reduce tile stay in LDS
static const int kBsTileFloats = 4096; // voxels of dflow a block of the reduce x pass holds in LDS

template <typename T> __device__ __forceinline__ T bs_ld_stream(const T *p) { return __builtin_nontemporal_load(p); }

// B0..B3 at t = r / d, formed in fp64, stored in fp32
__device__ __forceinline__ float4 bspline_weights(int r, int d)
{
    const double t = (double)r / (double)d, t2 = t * t, t3 = t2 * t, u = 1.0 - t;
    float4 w;
    w.x = (float)(u * u * u / 6.0);
    w.y = (float)((3.0 * t3 - 6.0 * t2 + 4.0) / 6.0);
    w.z = (float)((-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0);
    w.w = (float)(t3 / 6.0);
    return w;
}

__device__ __forceinline__ void bspline_fill_table(float4 *tab, int nt, int d)
{
    for (int i = threadIdx.x; i < nt; i += TRX_BLOCK) tab[i] = bspline_weights(i, d);
    __syncthreads();
}

// One axis of a volume [outer][S or G][inner], any inner (the z and y passes; grid-stride over the outputs, volumes along blockIdx.y).
//   REDUCE false: in [outer][G][inner] -> out [outer][S][inner], out(j) = sum_l B_l(j % d) in(j / d + l)
//   REDUCE true:  in [outer][S][inner] -> out [outer][G][inner], out(k) = sum_l sum_r B_l(r) in((k - l) d + r): per cell l in ascending r,
//                 then ((l3 + l2) + l1) + l0
template <bool REDUCE>
__global__ __launch_bounds__(TRX_BLOCK) void bspline_axis_kernel(const float *__restrict__ in, float *__restrict__ out, int nvol, unsigned outer,
                                                                   int S, int G, unsigned inner, int d)
{
    extern __shared__ float4 bs_tab[];
    const int nt = min(d, S);
    bspline_fill_table(bs_tab, nt, d);
    const unsigned n_in = outer * (unsigned)(REDUCE ? S : G) * inner, n_out = outer * (unsigned)(REDUCE ? G : S) * inner;
    for (int v = blockIdx.y; v < nvol; v += gridDim.y) {
        const float *src = in + (size_t)v * n_in;
        float *dst = out + (size_t)v * n_out;
        for (unsigned e = blockIdx.x * TRX_BLOCK + threadIdx.x; e < n_out; e += gridDim.x * TRX_BLOCK) {
            const unsigned k = e % inner, r = e / inner;
            if constexpr (!REDUCE) {
                const unsigned j = r % (unsigned)S, p = r / (unsigned)S;
                const unsigned q = j / (unsigned)d, rr = j - q * (unsigned)d;
                const float4 w = bs_tab[rr];
                const float *col = src + ((size_t)p * (unsigned)G + q) * inner + k;
                float acc = w.x * col[0];
                acc = fmaf(w.y, col[inner], acc);
                acc = fmaf(w.z, col[2 * (size_t)inner], acc);
                acc = fmaf(w.w, col[3 * (size_t)inner], acc);
                dst[e] = acc;
            } else {
                const unsigned c = r % (unsigned)G, p = r / (unsigned)G;
                const float *col = src + (size_t)p * (unsigned)S * inner + k;
                // the four cells (c - l) d .. (c - l) d + d - 1 behind control point c, each summed on its own (four independent chains)
                int cnt[4];
                const float *cell[4];
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    const long j0 = ((long)c - l) * d;
                    const bool valid = j0 >= 0 && j0 < S;
                    cnt[l] = valid ? (int)min((long)d, (long)S - j0) : 0;
                    cell[l] = col + (valid ? (size_t)j0 * inner : 0);
                }
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                for (int rr = 0; rr < nt; rr++) {
                    const float4 w = bs_tab[rr];
                    const size_t o = (size_t)rr * inner;
                    if (rr < cnt[0]) a0 = fmaf(w.x, cell[0][o], a0);
                    if (rr < cnt[1]) a1 = fmaf(w.y, cell[1][o], a1);
                    if (rr < cnt[2]) a2 = fmaf(w.z, cell[2][o], a2);
                    if (rr < cnt[3]) a3 = fmaf(w.w, cell[3][o], a3);
                }
                dst[e] = ((a3 + a2) + a1) + a0;
            }
        }
    }
}

// The x pass of expand (inner = 1): out [rows][W] = base + sum_l B_l(x % d) in [rows][G](x / d + l).  A thread keeps its x - hence its
// x / d and its four weights - and walks rows; a block is 2^tw_log2 voxels wide (the smallest power of two that covers min(W, 256)) and
// TRX_BLOCK >> tw_log2 rows high.
__global__ __launch_bounds__(TRX_BLOCK) void bspline_expand_x_kernel(const float *__restrict__ in, const float *__restrict__ base, float *__restrict__ out,
                                                                       int nvol, unsigned rows, int W, int G, int d, int tw_log2)
{
    extern __shared__ float4 bs_tab[];
    bspline_fill_table(bs_tab, min(d, W), d);
    const int TW = 1 << tw_log2, rpb = TRX_BLOCK >> tw_log2;
    const int xl = threadIdx.x & (TW - 1), rsub = threadIdx.x >> tw_log2;
    for (int v = blockIdx.y; v < nvol; v += gridDim.y) {
        const float *src = in + (size_t)v * rows * (unsigned)G;
        const float *bs = base ? base + (size_t)v * rows * (unsigned)W : nullptr;
        float *dst = out + (size_t)v * rows * (unsigned)W;
        for (int xc = 0; xc < W; xc += TW) {
            const int x = xc + xl;
            if (x >= W) continue;
            const int q = x / d, rr = x - q * d;
            const float4 w = bs_tab[rr];
            for (unsigned row = blockIdx.x * rpb + rsub; row < rows; row += gridDim.x * rpb) {
                const float *p = src + (size_t)row * (unsigned)G + q;
                float acc = w.x * p[0];
                acc = fmaf(w.y, p[1], acc);
                acc = fmaf(w.z, p[2], acc);
                acc = fmaf(w.w, p[3], acc);
                const size_t o = (size_t)row * (unsigned)W + x;
                dst[o] = bs ? bs_ld_stream(bs + o) + acc : acc;
            }
        }
    }
}

// The x pass of reduce (inner = 1): out [rows][G](k) = sum_l sum_r B_l(r) in [rows][W]((k - l) d + r), in bspline_axis_kernel<true>'s
// order.  A block takes a tile of R rows by Kc control points: the voxels behind them, [max(0, (k0 - 3) d), min(W, (k0 + Kc) d)), are
// loaded into LDS once (coalesced), then each (row, k) of the tile sums its up to 4 d voxels from LDS (one 16-byte read of the weight
// table per four voxels).  Rows of at most kBsTileFloats voxels are one segment (Kc = G, no voxel is loaded twice); longer rows are cut
// into segments that re-read 3 d voxels each.  Lanes of the summing phase read LDS at a stride of d floats: for even d every d-th
// voxel is followed by one float of padding (stride d + 1:
// reduce 148 us against 180 us unpadded at 1 x 256^3, d = 8, profiles/r08a_bspline.txt).
struct ReduceXPlan {
    int R, Kc, nseg, n, pad, rowlen;   // rowlen: floats per tile row in LDS
    unsigned magic;                    // floor(c / d) = umulhi(c, magic) for the c < 2^32 / d of a tile row
    size_t lds_bytes;
};

static ReduceXPlan reduce_x_plan(unsigned rows, int W, int G, int d)
{
    ReduceXPlan p{};
    if (W <= kBsTileFloats) {
        p.Kc = G; p.nseg = 1; p.n = W;
        p.R = (int)std::min<unsigned>(rows, (unsigned)std::max(1, kBsTileFloats / W));
    } else {
        p.Kc = std::max(1, kBsTileFloats / d - 3); p.nseg = (G + p.Kc - 1) / p.Kc; p.n = (p.Kc + 3) * d;
        p.R = 1;
    }
    p.pad = (d % 2 == 0) ? 1 : 0;
    p.rowlen = p.n + (p.pad ? p.n / d + 1 : 0);
    p.magic = d > 1 ? (unsigned)((((unsigned long long)1 << 32) + (unsigned)d - 1) / (unsigned)d) : 0u;
    p.lds_bytes = (size_t)std::min(d, W) * sizeof(float4) + (size_t)p.R * p.rowlen * sizeof(float);
    return p;
}

__global__ __launch_bounds__(TRX_BLOCK) void bspline_reduce_x_kernel(const float *__restrict__ in, float *__restrict__ out, int nvol, unsigned rows,
                                                                       int W, int G, int d, ReduceXPlan pl, int tw_log2)
{
    extern __shared__ float4 bs_tab[];
    const int nt = min(d, W);
    bspline_fill_table(bs_tab, nt, d);
    float *tile = (float *)(bs_tab + nt);
    const int TW = 1 << tw_log2, rpb = TRX_BLOCK >> tw_log2;
    const int xl = threadIdx.x & (TW - 1), rsub = threadIdx.x >> tw_log2;
    const unsigned nrt = (rows + pl.R - 1) / pl.R, ntile = nrt * (unsigned)pl.nseg;
    for (int v = blockIdx.y; v < nvol; v += gridDim.y) {
        const float *src = in + (size_t)v * rows * (unsigned)W;
        float *dst = out + (size_t)v * rows * (unsigned)G;
        for (unsigned t = blockIdx.x; t < ntile; t += gridDim.x) {
            const unsigned rt = t / (unsigned)pl.nseg, seg = t - rt * (unsigned)pl.nseg;
            const unsigned row0 = rt * (unsigned)pl.R;
            const int nr = (int)min((unsigned)pl.R, rows - row0);
            const int k0 = (int)seg * pl.Kc, nk = min(pl.Kc, G - k0);
            const int c0 = max(0, k0 - 3);                                   // first lattice cell (i0) of the tile
            const int x0 = c0 * d, n = (int)min((long)W, (long)(k0 + nk) * d) - x0;   // 1 <= n <= pl.n
            for (int r = rsub; r < nr; r += rpb) {
                const float *line = src + (size_t)(row0 + r) * (unsigned)W + x0;
                float *trow = tile + r * pl.rowlen;
                for (int c = xl; c < n; c += TW) trow[c + (pl.pad ? (int)__umulhi((unsigned)c, pl.magic) : 0)] = bs_ld_stream(line + c);
            }
            __syncthreads();
            for (int o = threadIdx.x; o < nr * nk; o += TRX_BLOCK) {
                const int r = o / nk, k = k0 + (o - r * nk);
                const float *trow = tile + r * pl.rowlen;
                int cnt[4];
                const float *cell[4];
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    const int cp = k - l;
                    const long xs = (long)cp * d;
                    const bool valid = cp >= 0 && xs < W;
                    cnt[l] = valid ? (int)min((long)d, (long)W - xs) : 0;
                    cell[l] = trow + (valid ? (cp - c0) * (d + pl.pad) : 0);
                }
                float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
                for (int rr = 0; rr < nt; rr++) {
                    const float4 w = bs_tab[rr];
                    if (rr < cnt[0]) a0 = fmaf(w.x, cell[0][rr], a0);
                    if (rr < cnt[1]) a1 = fmaf(w.y, cell[1][rr], a1);
                    if (rr < cnt[2]) a2 = fmaf(w.z, cell[2][rr], a2);
                    if (rr < cnt[3]) a3 = fmaf(w.w, cell[3][rr], a3);
                }
                dst[(size_t)(row0 + r) * (unsigned)G + k] = ((a3 + a2) + a1) + a0;
            }
            __syncthreads();
        }
    }
}

// Per pair, written by bspline_decide_kernel, read by bspline_update_kernel (block-uniform)
struct BsCoef {
    float step_size, inv_sqrt_bc2;
    int mode;   // kBsNormal: update; kBsHit: update, and keep the flow of this forward in flow_last; kBsSkip: the pair has stopped
};
constexpr int kBsNormal = 0, kBsHit = 1, kBsSkip = 2;

// One thread per pair: the loss curve, the step counter, the early stop (trx_flow_state's semantics: the iteration that meets stop_crit
// still applies its update, later ones are no-ops) and the Adam scalars of this iteration.
__global__ void bspline_decide_kernel(const float *__restrict__ terms, int B, trx_opt_cfg oc, float *__restrict__ losses, int losses_capacity,
                                      int *__restrict__ step, float stop_crit, int *__restrict__ stopped, BsCoef *__restrict__ coef)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    BsCoef c;
    if (stopped && stopped[b] != 0) {
        c.step_size = 0.f; c.inv_sqrt_bc2 = 1.f; c.mode = kBsSkip;
        coef[b] = c;
        return;
    }
    const int t = step[b];
    const float total = terms[b * 4];
    if (oc.kind == TRX_OPT_ADAM) {
        const double bc1 = 1.0 - ipow((double)oc.beta1, t + 1), bc2 = 1.0 - ipow((double)oc.beta2, t + 1);
        c.step_size = (float)((double)oc.lr / bc1);
        c.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    } else {
        c.step_size = oc.lr;
        c.inv_sqrt_bc2 = 1.f;
    }
    c.mode = kBsNormal;
    if (stopped && total <= stop_crit) {
        c.mode = kBsHit;
        stopped[b] = 1;
    }
    coef[b] = c;
    if (losses && t < losses_capacity) losses[(size_t)b * losses_capacity + t] = total;
    step[b] = t + 1;
}

// SGD / Adam on the control points of pair blockIdx.y (the arithmetic of flow_update_kernel, csrc/flow.hip), and - when the caller keeps
// flow_last - the copy of this forward's flow for a pair that stops here or on the last iteration of a call.
__global__ __launch_bounds__(TRX_BLOCK) void bspline_update_kernel(float *__restrict__ ctrl, const float *__restrict__ dctrl, float *__restrict__ adam_m,
                                                                     float *__restrict__ adam_v, size_t nctrl, const BsCoef *__restrict__ coef,
                                                                     trx_opt_cfg oc, const float *__restrict__ flow, float *__restrict__ flow_last,
                                                                     size_t nflow, int save_last)
{
    const int b = blockIdx.y;
    const BsCoef c = coef[b];
    if (c.mode == kBsSkip) return;
    const size_t stride = (size_t)gridDim.x * TRX_BLOCK, first = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x;
    float *p = ctrl + (size_t)b * nctrl;
    const float *g = dctrl + (size_t)b * nctrl;
    if (oc.kind == TRX_OPT_ADAM) {
        float *am = adam_m + (size_t)b * nctrl, *av = adam_v + (size_t)b * nctrl;
        for (size_t i = first; i < nctrl; i += stride) {
            const float gi = g[i], m0 = am[i], v0 = av[i];
            const float mi = m0 + (gi - m0) * (1.0f - oc.beta1);
            const float vi = oc.beta2 * v0 + (1.0f - oc.beta2) * gi * gi;
            am[i] = mi; av[i] = vi;
            const float denom = sqrtf(vi) * c.inv_sqrt_bc2 + oc.eps;
            p[i] = p[i] - c.step_size * (mi / denom);
        }
    } else {
        for (size_t i = first; i < nctrl; i += stride) p[i] = p[i] - c.step_size * g[i];
    }
    if (flow_last && (save_last || c.mode == kBsHit)) {
        const float *src = flow + (size_t)b * nflow;
        float *dst = flow_last + (size_t)b * nflow;
        for (size_t i = first; i < nflow; i += stride) dst[i] = src[i];
    }
}

struct BsGeom {
    int ndim, B, S[3], d[3], G[3];   // axes z, y, x (2-D: S[0] = G[0] = d[0] = 1, no z pass)
    size_t t1, t2;                   // floats per volume (pair and channel) of [D][Gy][Gx] and [D][H][Gx]
    size_t t2_offset;                // floats from the workspace's start to the [D][H][Gx] intermediates
    size_t lattice_bytes;            // both intermediates of all volumes
    size_t terms_offset, coef_offset, dctrl_offset, flow_offset, flow_bytes, ws_bytes;   // the loop's part: terms[B][4], BsCoef[B], dL/dctrl, trx_flow_loss_grad's workspace
};

static int bspline_geom(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, BsGeom *g)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1) return TRX_ERR_ARG;
    if ((double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    if (ndim == 2) sz = 1;
    if (sz < 1 || sy < 1 || sx < 1 || sz > TRX_BSPLINE_MAX_SPACING || sy > TRX_BSPLINE_MAX_SPACING || sx > TRX_BSPLINE_MAX_SPACING) return TRX_ERR_ARG;
    g->ndim = ndim; g->B = B;
    g->S[0] = D; g->S[1] = H; g->S[2] = W;
    g->d[0] = sz; g->d[1] = sy; g->d[2] = sx;
    for (int a = 0; a < 3; a++) g->G[a] = (g->S[a] - 1) / g->d[a] + 4;
    if (ndim == 2) g->G[0] = 1;
    const double gx = g->G[2], gy = g->G[1], gz = g->G[0];
    if ((double)D * H * gx >= 2147483648.0 || (double)D * gy * gx >= 2147483648.0 || gz * gy * gx >= 2147483648.0) return TRX_ERR_ARG;   // 32-bit indices
    const size_t nvol = (size_t)B * ndim;
    g->t1 = ndim == 3 ? (size_t)D * g->G[1] * g->G[2] : 0;
    g->t2 = (size_t)D * H * g->G[2];
    g->t2_offset = (nvol * g->t1 + 63) / 64 * 64;
    g->lattice_bytes = ((g->t2_offset + nvol * g->t2) * sizeof(float) + 255) & ~(size_t)255;
    g->flow_bytes = flow_workspace_size(ndim, B, D, H, W);   // the checks above are trx_flow_workspace_bytes' own
    g->terms_offset = g->lattice_bytes;
    g->coef_offset = g->terms_offset + (((size_t)B * 4 * sizeof(float) + 255) & ~(size_t)255);
    g->dctrl_offset = g->coef_offset + (((size_t)B * sizeof(BsCoef) + 255) & ~(size_t)255);
    g->flow_offset = g->dctrl_offset + ((nvol * g->G[0] * g->G[1] * g->G[2] * sizeof(float) + 255) & ~(size_t)255);
    g->ws_bytes = g->flow_offset + g->flow_bytes;
    return TRX_OK;
}

static dim3 bs_grid(size_t work_blocks, int nvol)
{
    const unsigned gy = (unsigned)std::min(nvol, 65535);
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>(work_blocks, std::max<size_t>(1, 8192 / gy)));
    return dim3(gx, gy);
}

static int bs_tw_log2(int W)
{
    int l2 = 0;
    while ((1 << l2) < std::min(W, TRX_BLOCK)) l2++;
    return l2;
}

template <bool REDUCE>
static int launch_bs_axis(const float *in, float *out, int nvol, const int shape[3], int axis, int S, int G, int d, hipStream_t s)
{
    unsigned outer = 1, inner = 1;
    for (int a = 0; a < axis; a++) outer *= (unsigned)shape[a];
    for (int a = axis + 1; a < 3; a++) inner *= (unsigned)shape[a];
    const size_t n_out = (size_t)outer * (REDUCE ? G : S) * inner;
    const size_t lds = (size_t)std::min(d, S) * sizeof(float4);
    hipLaunchKernelGGL((bspline_axis_kernel<REDUCE>), bs_grid((n_out + TRX_BLOCK - 1) / TRX_BLOCK, nvol), dim3(TRX_BLOCK), lds, s, in, out, nvol, outer, S, G,
                       inner, d);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

static int bspline_expand_impl(const BsGeom &g, const float *ctrl, const float *base, float *flow, void *workspace, hipStream_t s)
{
    const int nvol = g.B * g.ndim;
    float *t1 = (float *)workspace, *t2 = t1 + g.t2_offset;
    const float *src = ctrl;
    int shape[3] = {g.G[0], g.G[1], g.G[2]};
    int rc;
    if (g.ndim == 3) {
        if ((rc = launch_bs_axis<false>(src, t1, nvol, shape, 0, g.S[0], g.G[0], g.d[0], s)) != TRX_OK) return rc;
        shape[0] = g.S[0];
        src = t1;
    }
    if ((rc = launch_bs_axis<false>(src, t2, nvol, shape, 1, g.S[1], g.G[1], g.d[1], s)) != TRX_OK) return rc;
    const unsigned rows = (unsigned)g.S[0] * (unsigned)g.S[1];
    const int W = g.S[2], tw = bs_tw_log2(W), rpb = TRX_BLOCK >> tw;
    hipLaunchKernelGGL(bspline_expand_x_kernel, bs_grid(((size_t)rows + rpb - 1) / rpb, nvol), dim3(TRX_BLOCK), (size_t)std::min(g.d[2], W) * sizeof(float4), s,
                       (const float *)t2, base, flow, nvol, rows, W, g.G[2], g.d[2], tw);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

static int bspline_reduce_impl(const BsGeom &g, const float *dflow, float *dctrl, void *workspace, hipStream_t s)
{
    const int nvol = g.B * g.ndim;
    float *t1 = (float *)workspace, *t2 = t1 + g.t2_offset;
    const unsigned rows = (unsigned)g.S[0] * (unsigned)g.S[1];
    const int W = g.S[2], tw = bs_tw_log2(W);
    const ReduceXPlan pl = reduce_x_plan(rows, W, g.G[2], g.d[2]);
    const size_t ntile = (size_t)((rows + pl.R - 1) / pl.R) * pl.nseg;
    hipLaunchKernelGGL(bspline_reduce_x_kernel, bs_grid(ntile, nvol), dim3(TRX_BLOCK), pl.lds_bytes, s, dflow, t2, nvol, rows, W, g.G[2], g.d[2], pl, tw);
    TRX_CHECK_LAUNCH();
    int shape[3] = {g.S[0], g.S[1], g.G[2]};
    int rc;
    if ((rc = launch_bs_axis<true>(t2, g.ndim == 3 ? t1 : dctrl, nvol, shape, 1, g.S[1], g.G[1], g.d[1], s)) != TRX_OK) return rc;
    if (g.ndim == 3) {
        shape[1] = g.G[1];
        if ((rc = launch_bs_axis<true>(t1, dctrl, nvol, shape, 0, g.S[0], g.G[0], g.d[0], s)) != TRX_OK) return rc;
    }
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" int trx_bspline_grid(int ndim, int D, int H, int W, int sz, int sy, int sx, int *grid)
{
    if (!grid) return TRX_ERR_ARG;
    BsGeom g;
    const int rc = bspline_geom(ndim, 1, D, H, W, sz, sy, sx, &g);
    if (rc != TRX_OK) return rc;
    grid[0] = g.G[0]; grid[1] = g.G[1]; grid[2] = g.G[2];
    return TRX_OK;
}

extern "C" size_t trx_bspline_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx)
{
    BsGeom g;
    if (bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

extern "C" int trx_bspline_expand(const float *ctrl, const float *base, float *flow, int ndim, int B, int D, int H, int W, int sz, int sy, int sx,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ctrl || !flow || !workspace) return TRX_ERR_ARG;
    BsGeom g;
    const int rc = bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    return bspline_expand_impl(g, ctrl, base, flow, workspace, (hipStream_t)stream);
}

extern "C" int trx_bspline_reduce(const float *dflow, float *dctrl, int ndim, int B, int D, int H, int W, int sz, int sy, int sx, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    if (!dflow || !dctrl || !workspace) return TRX_ERR_ARG;
    BsGeom g;
    const int rc = bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    return bspline_reduce_impl(g, dflow, dctrl, workspace, (hipStream_t)stream);
}

extern "C" int trx_bspline_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                               int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!vol || !vol->moving || !vol->target || !loss || !opt || !st || !spacing || !workspace) return TRX_ERR_ARG;
    if (!st->ctrl || !st->flow || !st->dflow || !st->step) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_geom(vol->ndim, vol->B, vol->D, vol->H, vol->W, spacing[0], spacing[1], spacing[2], &g);
    if (rc != TRX_OK) return rc;
    if (opt->kind != TRX_OPT_SGD && opt->kind != TRX_OPT_ADAM) return TRX_ERR_ARG;
    if (opt->kind == TRX_OPT_ADAM && (!st->adam_m || !st->adam_v)) return TRX_ERR_ARG;
    if (iters < 0 || (st->losses && st->losses_capacity < 0)) return TRX_ERR_ARG;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *terms = (float *)(ws + g.terms_offset);
    BsCoef *coef = (BsCoef *)(ws + g.coef_offset);
    float *dctrl = (float *)(ws + g.dctrl_offset);
    const size_t nctrl = (size_t)g.ndim * g.G[0] * g.G[1] * g.G[2], nflow = (size_t)g.ndim * vol->D * vol->H * vol->W;
    const size_t work = std::max(nctrl, st->flow_last ? nflow : (size_t)0);
    const dim3 ugrid((unsigned)std::max<size_t>(1, std::min<size_t>((work + TRX_BLOCK - 1) / TRX_BLOCK, std::max(1, 2048 / vol->B))), (unsigned)vol->B);
    for (int i = 0; i < iters; i++) {
        if ((rc = bspline_expand_impl(g, st->ctrl, st->base, st->flow, workspace, s)) != TRX_OK) return rc;
        if ((rc = trx_flow_loss_grad(vol, loss, st->flow, terms, st->dflow, ws + g.flow_offset, g.flow_bytes, stream)) != TRX_OK) return rc;
        if ((rc = bspline_reduce_impl(g, st->dflow, dctrl, workspace, s)) != TRX_OK) return rc;
        hipLaunchKernelGGL(bspline_decide_kernel, dim3((vol->B + 63) / 64), dim3(64), 0, s, (const float *)terms, vol->B, *opt, st->losses, st->losses_capacity,
                           st->step, st->stop_crit, st->stopped, coef);
        TRX_CHECK_LAUNCH();
        hipLaunchKernelGGL(bspline_update_kernel, ugrid, dim3(TRX_BLOCK), 0, s, st->ctrl, (const float *)dctrl, st->adam_m, st->adam_v, nctrl,
                           (const BsCoef *)coef, *opt, (const float *)st->flow, st->flow_last, nflow, i + 1 == iters ? 1 : 0);
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}

extern "C" int trx_bspline_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    return trx_bspline_run(vol, loss, opt, st, spacing, 1, workspace, workspace_bytes, stream);
}
