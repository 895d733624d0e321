// Cubic B-spline free-form deformation (Rueckert et al. 1999; extension, the reference has no such model): the operator between a control
// lattice and a dense flow (trx_bspline_expand), its exact adjoint (trx_bspline_reduce) and a device-side optimisation loop over them
// (trx_bspline_run), and the bending energy of the lattice with its gradient (trx_bspline_bending; in the loop: trx_bspline_state.bending_weight).
// The same loop with other data terms: mutual information (trx_bspline_mi_run, csrc/mi.hip) and the diffeomorphic form, in which the expanded
// lattice is a stationary velocity field (trx_bspline_svf_run, csrc/svf.hip).  The displacement loops with a folding penalty on the Jacobian determinant
// of the total flow: trx_bspline_run_fold, trx_bspline_mi_run_fold (the penalty's kernels: csrc/jacobian.hip).  The normalised gradient field as the data
// term, every route behind one entry point: trx_bspline_ngf_run (csrc/ngf.hip).
// CPU restatements: tests/bspline_ref.py, tests/bspline_bending_ref.py, tests/jacobian_ref.py.
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
#include "affine_host.h"   // ami_grid_check (trx_bspline_mi_run_grids); includes trx_common.h
#include "jacobian.h"      // the folding penalty of the *_fold entry points (csrc/jacobian.hip)
#include "ngf.h"           // the data term of trx_bspline_ngf_run (csrc/ngf.hip)

#include <algorithm>
#include <cmath>

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

// One pair: the loss curve, the step counter, the early stop (trx_flow_state's semantics: the iteration that meets stop_crit still applies
// its update, later ones are no-ops) and the Adam scalars of this iteration.  `penalty` = lambda E_b joins the data term before the
// early stop and the record (BEND only).  The data term of pair b is terms[b * tstride] (trx_flow_loss_grad: 4, trx_mi_loss_grad: 1).
template <bool BEND>
__device__ __forceinline__ void bspline_decide_pair(int b, float penalty, const float *__restrict__ terms, int tstride, const trx_opt_cfg &oc, float *__restrict__ losses,
                                                    int losses_capacity, int *__restrict__ step, float stop_crit, int *__restrict__ stopped,
                                                    BsCoef *__restrict__ coef)
{
    BsCoef c;
    if (stopped && stopped[b] != 0) {
        c.step_size = 0.f; c.inv_sqrt_bc2 = 1.f; c.mode = kBsSkip;
        coef[b] = c;
        return;
    }
    const int t = step[b];
    float total = terms[b * tstride];
    if constexpr (BEND) total += penalty;
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

// One thread per pair (bending_weight = 0)
__global__ void bspline_decide_kernel(const float *__restrict__ terms, int tstride, int B, trx_opt_cfg oc, float *__restrict__ losses, int losses_capacity,
                                      int *__restrict__ step, float stop_crit, int *__restrict__ stopped, BsCoef *__restrict__ coef)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    bspline_decide_pair<false>(b, 0.f, terms, tstride, oc, losses, losses_capacity, step, stop_crit, stopped, coef);
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

// ---- Bending energy (include/trx.h: trx_bspline_bending; CPU restatement: tests/bspline_bending_ref.py) ----------------------------------
// Gram form: with R_a^(k) = M_a^(k)^T M_a^(k) ([G][G], non-zero only for |i - j| <= 3),
//   g = dE/dctrl_c = (2 / N) sum_{kz + ky + kx = 2} mult_k (R_z^(kz) (x) R_y^(ky) (x) R_x^(kx)) ctrl_c,   E = 1/2 sum_c <ctrl_c, g>.
// bspline_gram_kernel writes the bands R[a][k][G_a][7] once per call; bspline_bending_kernel applies them to lattice tiles in LDS.

// weight l of the k-th derivative (with respect to the voxel coordinate) of the cubic B-spline at t, fp64
__device__ __forceinline__ double bspline_dweight(int k, int l, double t, double d)
{
    const double u = 1.0 - t, t2 = t * t;
    double w;
    if (k == 0) {
        const double t3 = t2 * t;
        w = l == 0 ? u * u * u / 6.0 : l == 1 ? (3.0 * t3 - 6.0 * t2 + 4.0) / 6.0 : l == 2 ? (-3.0 * t3 + 3.0 * t2 + 3.0 * t + 1.0) / 6.0 : t3 / 6.0;
        return w;
    }
    if (k == 1) {
        w = l == 0 ? -u * u / 2.0 : l == 1 ? (3.0 * t2 - 4.0 * t) / 2.0 : l == 2 ? (-3.0 * t2 + 2.0 * t + 1.0) / 2.0 : t2 / 2.0;
        return w / d;
    }
    w = l == 0 ? u : l == 1 ? 3.0 * t - 2.0 : l == 2 ? 1.0 - 3.0 * t : t;
    return w / (d * d);
}

struct BendAxes {
    int S[3], d[3], G[3];
};

// R[a][k][i][m] = sum_x M_a^(k)[x][i] M_a^(k)[x][i + m - 3] (0 where i + m - 3 is outside the lattice): one thread per entry, the at most
// 4 d voxels that both control points see in ascending x, the fp32 weights multiplied and summed in fp64, stored as fp32.
__global__ __launch_bounds__(TRX_BLOCK) void bspline_gram_kernel(float *__restrict__ R, BendAxes ax)
{
    const int n0 = 21 * ax.G[0], n1 = 21 * ax.G[1], n = n0 + n1 + 21 * ax.G[2];
    for (int e = blockIdx.x * TRX_BLOCK + threadIdx.x; e < n; e += gridDim.x * TRX_BLOCK) {
        const int a = e < n0 ? 0 : e < n0 + n1 ? 1 : 2;
        const int r = e - (a == 0 ? 0 : a == 1 ? n0 : n0 + n1);
        const int S = ax.S[a], d = ax.d[a], G = ax.G[a];
        const int k = r / (7 * G), i = r / 7 % G, j = i + r % 7 - 3;
        double s = 0.0;
        if (j >= 0 && j < G) {
            for (int c = max(max(i, j) - 3, 0); c <= min(i, j); c++) {      // the cells (i0) whose four points hold both i and j
                const long x0 = (long)c * d;
                if (x0 >= S) break;
                const int nx = (int)min((long)d, (long)S - x0);
                for (int rr = 0; rr < nx; rr++) {
                    const double t = (double)rr / (double)d;
                    s += (double)(float)bspline_dweight(k, i - c, t, (double)d) * (double)(float)bspline_dweight(k, j - c, t, (double)d);
                }
            }
        }
        R[e] = (float)s;
    }
}

// Output tile of the bending kernel and its input tile (a halo of 3 points on every axis that has a band); 2-D has no z axis.
template <int ND> struct BendTile {
    static constexpr int TZ = ND == 3 ? 8 : 1, TY = ND == 3 ? 8 : 16, TX = ND == 3 ? 8 : 32, HZ = ND == 3 ? 3 : 0;
    static constexpr int IZ = TZ + 2 * HZ, IY = TY + 6, IX = TX + 6;
    static constexpr int NA = ND == 3 ? 3 : 1;     // arrays behind the y pass: one per kz
    static constexpr int TMAX = TX;                // the longest tile edge
    static constexpr int PL = TY * TX;             // outputs per z plane
};

// One lattice tile of one volume (pair and channel) per step of a block:
//   load   the tile with its halo (zeros outside the lattice) and the bands' rows of the tile into LDS;
//   x pass X_k = R_x^(k) tile, k = 0, 1, 2                                       [IZ][IY][TX] each;
//   y pass the six products R_y^(ky) X_kx with kx + ky <= 2, summed by the kz = 2 - kx - ky they meet in the z pass, with their
//          multiplicities: A_0 = Y_20 + Y_02 + 2 Y_11, A_1 = 2 (Y_10 + Y_01), A_2 = Y_00   [IZ][TY][TX] each (2-D: A_0 is the result);
//   z pass g = (2 / N) sum_kz R_z^(kz) A_kz, dctrl (+)= weight g, and 1/2 sum c g over the tile -> partials[volume][tile].
// A thread keeps its x (x pass) or its (y, x) (y pass) and with it its 21 band coefficients in registers.  No atomics; the tile's energy is
// summed in fp64 by a fixed tree.
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void bspline_bending_kernel(const float *__restrict__ ctrl, const float *__restrict__ R, float *__restrict__ dctrl,
                                                                      float *__restrict__ partials, int nvol, int Gz, int Gy, int Gx, int nty, int ntx,
                                                                      unsigned ntile, float scale, float weight, int accumulate)
{
    using T = BendTile<ND>;
    __shared__ float s_in[T::IZ * T::IY * T::IX];
    __shared__ float s_x[3][T::IZ * T::IY * T::TX];
    __shared__ float s_a[T::NA][T::IZ * T::PL];
    __shared__ float s_r[3][3][T::TMAX][7];        // [axis][k][row of the tile][tap]
    __shared__ double s_red[TRX_WAVES];
    const int tid = threadIdx.x;
    const float *Rax[3] = {R, R + 21 * Gz, R + 21 * (Gz + Gy)};
    const int G[3] = {Gz, Gy, Gx}, TT[3] = {T::TZ, T::TY, T::TX};
    const size_t nlat = (size_t)Gz * Gy * Gx;
    for (int v = blockIdx.y; v < nvol; v += gridDim.y) {
        const float *src = ctrl + (size_t)v * nlat;
        float *dst = dctrl ? dctrl + (size_t)v * nlat : nullptr;
        for (unsigned t = blockIdx.x; t < ntile; t += gridDim.x) {
            const int tx = (int)(t % (unsigned)ntx), ty = (int)(t / (unsigned)ntx % (unsigned)nty), tz = (int)(t / (unsigned)ntx / (unsigned)nty);
            const int o[3] = {tz * T::TZ, ty * T::TY, tx * T::TX};
            for (int e = tid; e < 3 * 3 * T::TMAX * 7; e += TRX_BLOCK) {
                const int tap = e % 7, row = e / 7 % T::TMAX, k = e / (7 * T::TMAX) % 3, a = e / (21 * T::TMAX);
                const int i = o[a] + row;
                const bool live = (ND == 3 || a > 0) && row < TT[a] && i < G[a];
                s_r[a][k][row][tap] = live ? Rax[a][((size_t)k * G[a] + i) * 7 + tap] : 0.f;
            }
            for (int e = tid; e < T::IZ * T::IY * T::IX; e += TRX_BLOCK) {
                const int gx = o[2] + e % T::IX - 3, gy = o[1] + e / T::IX % T::IY - 3, gz = o[0] + e / (T::IX * T::IY) - T::HZ;
                const bool inside = gx >= 0 && gx < Gx && gy >= 0 && gy < Gy && gz >= 0 && gz < Gz;
                s_in[e] = inside ? src[((size_t)gz * Gy + gy) * Gx + gx] : 0.f;
            }
            __syncthreads();
            {   // x pass
                const int xo = tid % T::TX;
                float r[3][7];
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int m = 0; m < 7; m++) r[k][m] = s_r[2][k][xo][m];
                for (int row = tid / T::TX; row < T::IZ * T::IY; row += TRX_BLOCK / T::TX) {
                    const float *p = s_in + row * T::IX + xo;
                    float c[7];
#pragma unroll
                    for (int m = 0; m < 7; m++) c[m] = p[m];
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        float acc = r[k][0] * c[0];
#pragma unroll
                        for (int m = 1; m < 7; m++) acc = fmaf(r[k][m], c[m], acc);
                        s_x[k][row * T::TX + xo] = acc;
                    }
                }
            }
            __syncthreads();
            for (int q = tid % T::PL; q < T::PL; q += TRX_BLOCK) {   // y pass
                const int xo = q % T::TX, yo = q / T::TX;
                float r[3][7];
#pragma unroll
                for (int k = 0; k < 3; k++)
#pragma unroll
                    for (int m = 0; m < 7; m++) r[k][m] = s_r[1][k][yo][m];
                for (int iz = T::PL < TRX_BLOCK ? tid / T::PL : 0; iz < T::IZ; iz += T::PL < TRX_BLOCK ? TRX_BLOCK / T::PL : 1) {
                    const int base = (iz * T::IY + yo) * T::TX + xo;
                    float y00 = 0.f, y10 = 0.f, y20 = 0.f, y01 = 0.f, y11 = 0.f, y02 = 0.f;
#pragma unroll
                    for (int m = 0; m < 7; m++) {
                        const float x0 = s_x[0][base + m * T::TX], x1 = s_x[1][base + m * T::TX], x2 = s_x[2][base + m * T::TX];
                        y00 = fmaf(r[0][m], x0, y00); y10 = fmaf(r[0][m], x1, y10); y20 = fmaf(r[0][m], x2, y20);
                        y01 = fmaf(r[1][m], x0, y01); y11 = fmaf(r[1][m], x1, y11);
                        y02 = fmaf(r[2][m], x0, y02);
                    }
                    s_a[0][iz * T::PL + q] = (y20 + y02) + 2.f * y11;
                    if constexpr (ND == 3) {
                        s_a[1][iz * T::PL + q] = 2.f * (y10 + y01);
                        s_a[2][iz * T::PL + q] = y00;
                    }
                }
            }
            __syncthreads();
            double part = 0.0;
            for (int e = tid; e < T::TZ * T::PL; e += TRX_BLOCK) {   // z pass, the gradient and the tile's energy
                const int q = e % T::PL, zo = e / T::PL, xo = q % T::TX, yo = q / T::TX;
                float g;
                if constexpr (ND == 3) {
                    g = 0.f;
#pragma unroll
                    for (int k = 0; k < 3; k++)
#pragma unroll
                        for (int m = 0; m < 7; m++) g = fmaf(s_r[0][k][zo][m], s_a[k][(zo + m) * T::PL + q], g);
                } else {
                    g = s_a[0][q];
                }
                g *= scale;
                const int gz = o[0] + zo, gy = o[1] + yo, gx = o[2] + xo;
                if (gz < Gz && gy < Gy && gx < Gx) {
                    part += (double)(s_in[((zo + T::HZ) * T::IY + yo + 3) * T::IX + xo + 3] * g);
                    if (dst) {
                        const size_t i = ((size_t)gz * Gy + gy) * Gx + gx;
                        dst[i] = accumulate ? fmaf(weight, g, dst[i]) : weight * g;
                    }
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
            if ((tid & 63) == 0) s_red[tid >> 6] = part;
            __syncthreads();
            if (tid == 0) partials[(size_t)v * ntile + t] = (float)(0.5 * (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]));
            __syncthreads();
        }
    }
}

// Sum of n partials by the 64 threads of a block, in ascending order: thread l sums the l-th of 64 contiguous runs, then the 64 run sums are
// added in ascending l; fp64 throughout.  Every thread gets the total.
__device__ __forceinline__ double bspline_sum_partials(const float *__restrict__ p, int n)
{
    __shared__ double s_run[64];
    const int run = (n + 63) / 64, lo = min(n, (int)threadIdx.x * run), hi = min(n, lo + run);
    double s = 0.0;
    for (int i = lo; i < hi; i++) s += (double)p[i];
    s_run[threadIdx.x] = s;
    __syncthreads();
    double total = 0.0;
    for (int l = 0; l < 64; l++) total += s_run[l];
    return total;
}

// energy[b] = sum of the pair's partials (its ndim volumes, tiles in ascending order); one block of 64 threads per pair
__global__ __launch_bounds__(64) void bspline_energy_kernel(const float *__restrict__ partials, int per_pair, float *__restrict__ energy)
{
    const double e = bspline_sum_partials(partials + (size_t)blockIdx.x * per_pair, per_pair);
    if (threadIdx.x == 0) energy[blockIdx.x] = (float)e;
}

// bspline_decide_kernel with the penalty: one block of 64 threads per pair sums the pair's partials, thread 0 decides on
// terms[b][0] + lambda E_b
__global__ __launch_bounds__(64) void bspline_decide_bending_kernel(const float *__restrict__ terms, int tstride, const float *__restrict__ partials, int per_pair,
                                                                      float lambda, trx_opt_cfg oc, float *__restrict__ losses, int losses_capacity,
                                                                      int *__restrict__ step, float stop_crit, int *__restrict__ stopped,
                                                                      BsCoef *__restrict__ coef)
{
    const int b = blockIdx.x;
    const double e = bspline_sum_partials(partials + (size_t)b * per_pair, per_pair);
    if (threadIdx.x == 0) bspline_decide_pair<true>(b, lambda * (float)e, terms, tstride, oc, losses, losses_capacity, step, stop_crit, stopped, coef);
}

// bspline_decide_bending_kernel with the folding penalty (the *_fold entry points, weight > 0): one wave per pair sums the bending partials (where
// lambda > 0) and the folding partials, lane 0 decides on terms[b][0] + (lambda E_b + weight P_b)
__global__ __launch_bounds__(64) void bspline_decide_fold_kernel(const float *__restrict__ terms, int tstride, const float *__restrict__ partials, int per_pair,
                                                                   float lambda, const double *__restrict__ fold_partials, int nchunk, unsigned nvox,
                                                                   float fold_weight, trx_opt_cfg oc, float *__restrict__ losses, int losses_capacity,
                                                                   int *__restrict__ step, float stop_crit, int *__restrict__ stopped,
                                                                   BsCoef *__restrict__ coef)
{
    const int b = blockIdx.x;
    const double e = partials ? bspline_sum_partials(partials + (size_t)b * per_pair, per_pair) : 0.0;
    const float p = fold_penalty_from_partials(fold_partials + (size_t)b * nchunk, nchunk, nvox);
    if (threadIdx.x == 0)
        bspline_decide_pair<true>(b, fmaf(fold_weight, p, lambda * (float)e), terms, tstride, oc, losses, losses_capacity, step, stop_crit, stopped, coef);
}

// The folding penalty of a *_fold run: its geometry, its settings and its workspace (behind the unpenalised entry point's)
struct FoldRun {
    FoldGeom g;
    float weight, threshold;
    void *ws;
};

struct BsGeom {
    int ndim, B, S[3], d[3], G[3];   // axes z, y, x (2-D: S[0] = G[0] = d[0] = 1, no z pass)
    size_t t1, t2;                   // floats per volume (pair and channel) of [D][Gy][Gx] and [D][H][Gx]
    size_t t2_offset;                // floats from the workspace's start to the [D][H][Gx] intermediates
    size_t lattice_bytes;            // both intermediates of all volumes
    size_t terms_offset, coef_offset, dctrl_offset, flow_offset, flow_bytes, ws_bytes;   // the loop's part: terms[B][4], BsCoef[B], dL/dctrl, trx_flow_loss_grad's workspace
    int bend_nt[3];                  // tiles of the bending kernel per axis
    size_t bend_ntile;               // per volume
    size_t gram_offset, part_offset; // the bending energy's part: the bands R[a][k][G_a][7], partials[B ndim][bend_ntile]
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
    const int tile[3] = {ndim == 3 ? BendTile<3>::TZ : BendTile<2>::TZ, ndim == 3 ? BendTile<3>::TY : BendTile<2>::TY, ndim == 3 ? BendTile<3>::TX : BendTile<2>::TX};
    for (int a = 0; a < 3; a++) g->bend_nt[a] = (g->G[a] + tile[a] - 1) / tile[a];
    g->bend_ntile = (size_t)g->bend_nt[0] * g->bend_nt[1] * g->bend_nt[2];
    g->gram_offset = (g->flow_offset + g->flow_bytes + 255) & ~(size_t)255;
    g->part_offset = g->gram_offset + (((size_t)21 * ((size_t)g->G[0] + g->G[1] + g->G[2]) * sizeof(float) + 255) & ~(size_t)255);
    g->ws_bytes = g->part_offset + ((nvol * g->bend_ntile * sizeof(float) + 255) & ~(size_t)255);
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

static int bspline_gram_impl(const BsGeom &g, void *workspace, hipStream_t s)
{
    BendAxes ax;
    for (int a = 0; a < 3; a++) { ax.S[a] = g.S[a]; ax.d[a] = g.d[a]; ax.G[a] = g.G[a]; }
    const int n = 21 * (g.G[0] + g.G[1] + g.G[2]);
    hipLaunchKernelGGL(bspline_gram_kernel, dim3((unsigned)std::min(1024, (n + TRX_BLOCK - 1) / TRX_BLOCK)), dim3(TRX_BLOCK), 0, s,
                       (float *)((char *)workspace + g.gram_offset), ax);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// dctrl (nullable) = (accumulate ? dctrl : 0) + weight dE/dctrl, and the tiles' energies into the workspace; the bands must be there
static int bspline_bending_impl(const BsGeom &g, const float *ctrl, float *dctrl, float weight, int accumulate, void *workspace, hipStream_t s)
{
    const int nvol = g.B * g.ndim;
    const float *R = (const float *)((char *)workspace + g.gram_offset);
    float *partials = (float *)((char *)workspace + g.part_offset);
    const float scale = (float)(2.0 / ((double)g.S[0] * g.S[1] * g.S[2]));
    const dim3 grid = bs_grid(g.bend_ntile, nvol);
    if (g.ndim == 3)
        hipLaunchKernelGGL(bspline_bending_kernel<3>, grid, dim3(TRX_BLOCK), 0, s, ctrl, R, dctrl, partials, nvol, g.G[0], g.G[1], g.G[2], g.bend_nt[1],
                           g.bend_nt[2], (unsigned)g.bend_ntile, scale, weight, accumulate);
    else
        hipLaunchKernelGGL(bspline_bending_kernel<2>, grid, dim3(TRX_BLOCK), 0, s, ctrl, R, dctrl, partials, nvol, g.G[0], g.G[1], g.G[2], g.bend_nt[1],
                           g.bend_nt[2], (unsigned)g.bend_ntile, scale, weight, accumulate);
    TRX_CHECK_LAUNCH();
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

extern "C" int trx_bspline_bending(const float *ctrl, float *energy, float *dctrl, float weight, int accumulate, int ndim, int B, int D, int H, int W,
                                   int sz, int sy, int sx, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!ctrl || !energy || !workspace) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = bspline_gram_impl(g, workspace, s)) != TRX_OK) return rc;
    if ((rc = bspline_bending_impl(g, ctrl, dctrl, weight, accumulate, workspace, s)) != TRX_OK) return rc;
    hipLaunchKernelGGL(bspline_energy_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float *)((char *)workspace + g.part_offset),
                       (int)(g.ndim * g.bend_ntile), energy);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// The checks trx_bspline_run and trx_bspline_mi_run share (everything but the data term's own arguments and the workspace size)
static int bspline_run_checks(const trx_volumes *vol, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing, int iters, void *workspace,
                              BsGeom *g)
{
    if (!vol || !vol->moving || !vol->target || !opt || !st || !spacing || !workspace) return TRX_ERR_ARG;
    if (!st->ctrl || !st->flow || !st->dflow || !st->step) return TRX_ERR_ARG;
    const int rc = bspline_geom(vol->ndim, vol->B, vol->D, vol->H, vol->W, spacing[0], spacing[1], spacing[2], g);
    if (rc != TRX_OK) return rc;
    if (opt->kind != TRX_OPT_SGD && opt->kind != TRX_OPT_ADAM) return TRX_ERR_ARG;
    if (opt->kind == TRX_OPT_ADAM && (!st->adam_m || !st->adam_v)) return TRX_ERR_ARG;
    if (iters < 0 || (st->losses && st->losses_capacity < 0)) return TRX_ERR_ARG;
    if (!(st->bending_weight >= 0.f) || !std::isfinite(st->bending_weight)) return TRX_ERR_ARG;
    return TRX_OK;
}

// The loop both data terms share.  data_term(): the launches that turn st->flow into the pairs' data terms (terms[b * tstride]) and st->dflow.
template <typename DataTerm>
static int bspline_loop(const BsGeom &g, const trx_volumes *vol, const trx_opt_cfg *opt, const trx_bspline_state *st, int iters, const float *terms,
                        int tstride, void *workspace, hipStream_t s, DataTerm data_term, const FoldRun *fold = nullptr)
{
    int rc;
    char *ws = (char *)workspace;
    BsCoef *coef = (BsCoef *)(ws + g.coef_offset);
    float *dctrl = (float *)(ws + g.dctrl_offset);
    const float lambda = st->bending_weight;
    const size_t nctrl = (size_t)g.ndim * g.G[0] * g.G[1] * g.G[2], nflow = (size_t)g.ndim * vol->D * vol->H * vol->W;
    const size_t work = std::max(nctrl, st->flow_last ? nflow : (size_t)0);
    const dim3 ugrid((unsigned)std::max<size_t>(1, std::min<size_t>((work + TRX_BLOCK - 1) / TRX_BLOCK, std::max(1, 2048 / vol->B))), (unsigned)vol->B);
    const bool bend = lambda > 0.f;
    if (bend && iters > 0 && (rc = bspline_gram_impl(g, workspace, s)) != TRX_OK) return rc;   // once per call: the bands depend on the geometry alone
    for (int i = 0; i < iters; i++) {
        if ((rc = bspline_expand_impl(g, st->ctrl, st->base, st->flow, workspace, s)) != TRX_OK) return rc;
        if ((rc = data_term()) != TRX_OK) return rc;
        if (fold) {   // on the TOTAL flow base + expand(ctrl): dflow += weight dP/dflow; base receives nothing, as ever
            if ((rc = fold_forward_impl(fold->g, st->flow, fold->threshold, fold->ws, s)) != TRX_OK) return rc;
            if ((rc = fold_backward_impl(fold->g, st->flow, fold->threshold, fold->weight, st->dflow, 1, fold->ws, s)) != TRX_OK) return rc;
        }
        if ((rc = bspline_reduce_impl(g, st->dflow, dctrl, workspace, s)) != TRX_OK) return rc;
        if (fold) {
            if (bend && (rc = bspline_bending_impl(g, st->ctrl, dctrl, lambda, 1, workspace, s)) != TRX_OK) return rc;
            hipLaunchKernelGGL(bspline_decide_fold_kernel, dim3((unsigned)vol->B), dim3(64), 0, s, terms, tstride,
                               bend ? (const float *)(ws + g.part_offset) : (const float *)nullptr, (int)(g.ndim * g.bend_ntile), lambda,
                               (const double *)((const char *)fold->ws + fold->g.part_offset), (int)fold->g.nchunk, fold->g.nvox, fold->weight, *opt, st->losses,
                               st->losses_capacity, st->step, st->stop_crit, st->stopped, coef);
        } else if (bend) {
            if ((rc = bspline_bending_impl(g, st->ctrl, dctrl, lambda, 1, workspace, s)) != TRX_OK) return rc;
            hipLaunchKernelGGL(bspline_decide_bending_kernel, dim3((unsigned)vol->B), dim3(64), 0, s, terms, tstride, (const float *)(ws + g.part_offset),
                               (int)(g.ndim * g.bend_ntile), lambda, *opt, st->losses, st->losses_capacity, st->step, st->stop_crit, st->stopped, coef);
        } else {
            hipLaunchKernelGGL(bspline_decide_kernel, dim3((vol->B + 63) / 64), dim3(64), 0, s, terms, tstride, vol->B, *opt, st->losses,
                               st->losses_capacity, st->step, st->stop_crit, st->stopped, coef);
        }
        TRX_CHECK_LAUNCH();
        hipLaunchKernelGGL(bspline_update_kernel, ugrid, dim3(TRX_BLOCK), 0, s, st->ctrl, (const float *)dctrl, st->adam_m, st->adam_v, nctrl,
                           (const BsCoef *)coef, *opt, (const float *)st->flow, st->flow_last, nflow, i + 1 == iters ? 1 : 0);
        TRX_CHECK_LAUNCH();
    }
    return TRX_OK;
}

extern "C" int trx_bspline_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                               int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!loss) return TRX_ERR_ARG;
    BsGeom g;
    const int rc = bspline_run_checks(vol, opt, st, spacing, iters, workspace, &g);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    char *ws = (char *)workspace;
    float *terms = (float *)(ws + g.terms_offset);
    return bspline_loop(g, vol, opt, st, iters, terms, 4, workspace, (hipStream_t)stream, [&]() {
        return trx_flow_loss_grad(vol, loss, st->flow, terms, st->dflow, ws + g.flow_offset, g.flow_bytes, stream);
    });
}

// The *_fold entry points: the penalty's settings (refused before any HIP call) and its workspace, which starts at the next 256-byte boundary behind
// the unpenalised entry point's `base_bytes`.  weight == 0: no FoldRun, the loop is the unpenalised one launch for launch; the workspace size is still
// the *_fold query's, so a caller sizes it once whatever the weight.
static int fold_cfg_check(const trx_fold_cfg *fold)
{
    if (!fold || !std::isfinite(fold->weight) || !std::isfinite(fold->threshold) || fold->weight < 0.f) return TRX_ERR_ARG;
    return TRX_OK;
}

static size_t fold_ws_offset(size_t base_bytes) { return (base_bytes + 255) & ~(size_t)255; }

static int fold_run_setup(const BsGeom &g, const trx_fold_cfg *fold, void *workspace, size_t base_bytes, size_t workspace_bytes, FoldRun *fr)
{
    const int rc = fold_geom(g.ndim, g.B, g.S[0], g.S[1], g.S[2], &fr->g);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < fold_ws_offset(base_bytes) + fr->g.ws_bytes) return TRX_ERR_WORKSPACE;
    fr->weight = fold->weight; fr->threshold = fold->threshold;
    fr->ws = (char *)workspace + fold_ws_offset(base_bytes);
    return TRX_OK;
}

extern "C" size_t trx_bspline_fold_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx)
{
    const size_t base = trx_bspline_workspace_bytes(ndim, B, D, H, W, sz, sy, sx), fold = trx_flow_folding_workspace_bytes(ndim, B, D, H, W);
    return base && fold ? fold_ws_offset(base) + fold : 0;
}

extern "C" int trx_bspline_run_fold(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                                    const trx_fold_cfg *fold, int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!loss) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_run_checks(vol, opt, st, spacing, iters, workspace, &g);
    if (rc == TRX_OK) rc = fold_cfg_check(fold);
    if (rc != TRX_OK) return rc;
    FoldRun fr;
    if ((rc = fold_run_setup(g, fold, workspace, g.ws_bytes, workspace_bytes, &fr)) != TRX_OK) return rc;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    char *ws = (char *)workspace;
    float *terms = (float *)(ws + g.terms_offset);
    return bspline_loop(g, vol, opt, st, iters, terms, 4, workspace, (hipStream_t)stream, [&]() {
        return trx_flow_loss_grad(vol, loss, st->flow, terms, st->dflow, ws + g.flow_offset, g.flow_bytes, stream);
    }, fr.weight > 0.f ? &fr : nullptr);
}

// Free-form deformation + mutual information (csrc/mi.hip): behind the loop's workspace lie the warped volumes, dL/dwarped and trx_mi_loss_grad's
// workspace; the pairs' losses take the place of terms[B][4] (stride 1).
struct BsMiLayout {
    size_t o_warped, o_go, o_mi, mi_bytes, ws_bytes;
};

static int bspline_mi_layout(const BsGeom &g, int bins, BsMiLayout *l)
{
    l->mi_bytes = trx_mi_workspace_bytes(g.ndim, g.B, g.S[0], g.S[1], g.S[2], bins);
    if (l->mi_bytes == 0) return TRX_ERR_ARG;
    const size_t vols = (((size_t)g.B * g.S[0] * g.S[1] * g.S[2] * sizeof(float)) + 255) & ~(size_t)255;
    l->o_warped = (g.ws_bytes + 255) & ~(size_t)255;
    l->o_go = l->o_warped + vols;
    l->o_mi = l->o_go + vols;
    l->ws_bytes = l->o_mi + l->mi_bytes;
    return TRX_OK;
}

extern "C" size_t trx_bspline_mi_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins)
{
    BsGeom g;
    BsMiLayout l;
    if (bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g) != TRX_OK || bspline_mi_layout(g, bins, &l) != TRX_OK) return 0;
    return l.ws_bytes;
}

// Under the overlap rule (trx_moving_grid.overlap) the B N validity bytes of an iteration lie behind that workspace
static size_t bspline_mi_valid_bytes(const BsGeom &g) { return (((size_t)g.B * g.S[0] * g.S[1] * g.S[2]) + 255) & ~(size_t)255; }

extern "C" size_t trx_bspline_mi_grids_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins, const trx_moving_grid *mg)
{
    BsGeom g;
    BsMiLayout l;
    if (bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g) != TRX_OK || bspline_mi_layout(g, bins, &l) != TRX_OK) return 0;
    return l.ws_bytes + ((mg && mg->overlap) ? bspline_mi_valid_bytes(g) : 0);
}

// Both mutual-information loops.  mg == nullptr: one lattice, the warp is trx_flow_warp.  Otherwise the deformation is composed with the initial affine
// `theta`, the moving image on a lattice of its own (csrc/affine_flow.hip): the same checks, workspace and launches with the composed
// warp and its backward where trx_flow_warp / trx_flow_warp_backward stand.  theta is read on the device on every iteration and never written.
static int bspline_mi_run_impl(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const trx_mi_cfg *cfg, const trx_opt_cfg *opt,
                               const trx_bspline_state *st, const int *spacing, int iters, void *workspace, size_t workspace_bytes, void *stream,
                               const trx_fold_cfg *fold = nullptr, bool with_fold = false)
{
    if (!cfg || !cfg->range) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_run_checks(vol, opt, st, spacing, iters, workspace, &g);
    if (rc == TRX_OK && mg) rc = ami_grid_check(vol->ndim, mg);
    if (rc != TRX_OK) return rc;
    BsMiLayout l;
    if ((rc = bspline_mi_layout(g, cfg->bins, &l)) != TRX_OK) return rc;
    if (!std::isfinite(cfg->alpha)) return TRX_ERR_ARG;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W;
    if (vol->B > 1 && vol->target_stride != nvox) return TRX_ERR_ARG;   // the histogram kernels take a dense [B][D][H][W] target
    if (mg && mg->mask && !mg->overlap) return TRX_ERR_ARG;      // a moving mask is part of the overlap rule
    const bool ov = mg && mg->overlap;
    if (workspace_bytes < l.ws_bytes + (ov ? bspline_mi_valid_bytes(g) : 0)) return TRX_ERR_WORKSPACE;
    FoldRun fr;
    const FoldRun *frp = nullptr;
    if (with_fold) {   // trx_bspline_mi_run_fold: the penalty's workspace lies behind everything above
        if ((rc = fold_cfg_check(fold)) != TRX_OK) return rc;
        if ((rc = fold_run_setup(g, fold, workspace, l.ws_bytes + (ov ? bspline_mi_valid_bytes(g) : 0), workspace_bytes, &fr)) != TRX_OK) return rc;
        if (fr.weight > 0.f) frp = &fr;
    }
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    char *ws = (char *)workspace;
    float *mloss = (float *)(ws + g.terms_offset), *warped = (float *)(ws + l.o_warped), *go = (float *)(ws + l.o_go);
    if (ov) {      // warp -> validity at the warp's coordinates -> the masked criterion on the validity bytes -> warp backward (grad_warped is 0 at an invalid voxel)
        unsigned char *valid = (unsigned char *)(ws + l.ws_bytes);
        trx_mi_cfg vcfg = *cfg;
        vcfg.mask = valid;
        return bspline_loop(g, vol, opt, st, iters, mloss, 1, workspace, (hipStream_t)stream, [&]() {
            int r = trx_affine_flow_warp(vol, mg, theta, st->flow, 1, warped, stream);
            if (r != TRX_OK) return r;
            if ((r = trx_affine_flow_valid(vol, mg, theta, st->flow, cfg->mask, valid, stream)) != TRX_OK) return r;
            r = trx_mi_loss_grad(vol->target, warped, vol->ndim, vol->B, vol->D, vol->H, vol->W, &vcfg, mloss, go, ws + l.o_mi, l.mi_bytes, stream);
            if (r != TRX_OK) return r;
            return trx_affine_flow_warp_backward(vol, mg, theta, st->flow, 1, go, st->dflow, stream);
        }, frp);
    }
    return bspline_loop(g, vol, opt, st, iters, mloss, 1, workspace, (hipStream_t)stream, [&]() {
        int r = mg ? trx_affine_flow_warp(vol, mg, theta, st->flow, 1, warped, stream) : trx_flow_warp(vol, st->flow, 1, warped, stream);
        if (r != TRX_OK) return r;
        r = trx_mi_loss_grad(vol->target, warped, vol->ndim, vol->B, vol->D, vol->H, vol->W, cfg, mloss, go, ws + l.o_mi, l.mi_bytes, stream);
        if (r != TRX_OK) return r;
        return mg ? trx_affine_flow_warp_backward(vol, mg, theta, st->flow, 1, go, st->dflow, stream) : trx_flow_warp_backward(vol, st->flow, 1, go, st->dflow, stream);
    }, frp);
}

extern "C" int trx_bspline_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                                  int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    return bspline_mi_run_impl(vol, nullptr, nullptr, cfg, opt, st, spacing, iters, workspace, workspace_bytes, stream);
}

extern "C" int trx_bspline_mi_run_grids(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const trx_mi_cfg *cfg, const trx_opt_cfg *opt,
                                        const trx_bspline_state *st, const int *spacing, int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!mg || !theta) return TRX_ERR_ARG;      // (with the impl's first refusal: one return code, as before)
    return bspline_mi_run_impl(vol, mg, theta, cfg, opt, st, spacing, iters, workspace, workspace_bytes, stream);
}

extern "C" size_t trx_bspline_mi_fold_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins, const trx_moving_grid *mg)
{
    const size_t base = trx_bspline_mi_grids_workspace_bytes(ndim, B, D, H, W, sz, sy, sx, bins, mg), fold = trx_flow_folding_workspace_bytes(ndim, B, D, H, W);
    return base && fold ? fold_ws_offset(base) + fold : 0;
}

// trx_bspline_mi_run (mg and theta NULL) and trx_bspline_mi_run_grids (both given), the overlap rule included, with the folding penalty
extern "C" int trx_bspline_mi_run_fold(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const trx_mi_cfg *cfg, const trx_opt_cfg *opt,
                                       const trx_bspline_state *st, const int *spacing, const trx_fold_cfg *fold, int iters, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    if ((mg == nullptr) != (theta == nullptr)) return TRX_ERR_ARG;
    return bspline_mi_run_impl(vol, mg, theta, cfg, opt, st, spacing, iters, workspace, workspace_bytes, stream, fold, true);
}

// Free-form deformation + normalised gradient field (csrc/ngf.hip): the mutual-information loop's layout with trx_ngf_loss_grad's workspace where
// trx_mi_loss_grad's stands, and the folding penalty's workspace behind it whatever the weight - one query for every route.
struct BsNgfLayout {
    size_t o_warped, o_go, o_ngf, o_fold, ws_bytes;
};

static int bspline_ngf_layout(const BsGeom &g, BsNgfLayout *l)
{
    const size_t ngf = trx_ngf_workspace_bytes(g.ndim, g.B, g.S[0], g.S[1], g.S[2]), fold = trx_flow_folding_workspace_bytes(g.ndim, g.B, g.S[0], g.S[1], g.S[2]);
    if (ngf == 0 || fold == 0) return TRX_ERR_ARG;
    const size_t vols = (((size_t)g.B * g.S[0] * g.S[1] * g.S[2] * sizeof(float)) + 255) & ~(size_t)255;
    l->o_warped = (g.ws_bytes + 255) & ~(size_t)255;
    l->o_go = l->o_warped + vols;
    l->o_ngf = l->o_go + vols;
    l->o_fold = fold_ws_offset(l->o_ngf + ngf);
    l->ws_bytes = l->o_fold + fold;
    return TRX_OK;
}

extern "C" size_t trx_bspline_ngf_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, const trx_moving_grid *mg)
{
    BsGeom g;
    BsNgfLayout l;
    if (bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g) != TRX_OK || bspline_ngf_layout(g, &l) != TRX_OK) return 0;
    if (mg && (ami_grid_check(ndim, mg) != TRX_OK || mg->overlap || mg->mask)) return 0;
    return l.ws_bytes;
}

extern "C" int trx_bspline_ngf_run(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const trx_ngf_cfg *cfg, const trx_opt_cfg *opt,
                                   const trx_bspline_state *st, const int *spacing, const trx_fold_cfg *fold, int iters, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    if (!cfg || (mg == nullptr) != (theta == nullptr)) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_run_checks(vol, opt, st, spacing, iters, workspace, &g);
    if (rc == TRX_OK && mg) rc = ami_grid_check(vol->ndim, mg);
    if (rc != TRX_OK) return rc;
    if (mg && (mg->overlap || mg->mask)) return TRX_ERR_ARG;      // the overlap rule is not built for this criterion
    NgfGeom ng;
    if ((rc = ngf_geom(g.ndim, g.B, g.S[0], g.S[1], g.S[2], &ng)) != TRX_OK) return rc;
    if ((rc = ngf_cfg_check(cfg, &ng)) != TRX_OK) return rc;
    if (fold && (rc = fold_cfg_check(fold)) != TRX_OK) return rc;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W;
    if (vol->B > 1 && vol->target_stride != nvox) return TRX_ERR_ARG;   // the criterion takes a dense [B][D][H][W] target
    BsNgfLayout l;
    if ((rc = bspline_ngf_layout(g, &l)) != TRX_OK) return rc;
    if (workspace_bytes < l.ws_bytes) return TRX_ERR_WORKSPACE;
    FoldRun fr;
    const FoldRun *frp = nullptr;
    if (fold && fold->weight > 0.f) {
        if ((rc = fold_geom(g.ndim, g.B, g.S[0], g.S[1], g.S[2], &fr.g)) != TRX_OK) return rc;
        fr.weight = fold->weight; fr.threshold = fold->threshold;
        fr.ws = (char *)workspace + l.o_fold;
        frp = &fr;
    }
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    char *ws = (char *)workspace;
    float *nloss = (float *)(ws + g.terms_offset), *warped = (float *)(ws + l.o_warped), *go = (float *)(ws + l.o_go);
    hipStream_t s = (hipStream_t)stream;
    return bspline_loop(g, vol, opt, st, iters, nloss, 1, workspace, s, [&]() {
        int r = mg ? trx_affine_flow_warp(vol, mg, theta, st->flow, 1, warped, stream) : trx_flow_warp(vol, st->flow, 1, warped, stream);
        if (r != TRX_OK) return r;
        if ((r = ngf_loss_grad_impl(ng, vol->target, warped, cfg, nloss, go, ws + l.o_ngf, s)) != TRX_OK) return r;
        return mg ? trx_affine_flow_warp_backward(vol, mg, theta, st->flow, 1, go, st->dflow, stream) : trx_flow_warp_backward(vol, st->flow, 1, go, st->dflow, stream);
    }, frp);
}

// Diffeomorphic free-form deformation (csrc/svf.hip): the expanded lattice is a stationary velocity field.  Behind the loop's workspace lie
// phi = exp(v), dL/dphi and trx_svf_exp's workspace (the kept levels, which its backward reads).
struct BsSvfLayout {
    size_t o_phi, o_dphi, o_svf, svf_bytes, ws_bytes;
};

static int bspline_svf_layout(const BsGeom &g, int squarings, BsSvfLayout *l)
{
    l->svf_bytes = trx_svf_workspace_bytes(g.ndim, g.B, g.S[0], g.S[1], g.S[2], squarings);
    if (l->svf_bytes == 0) return TRX_ERR_ARG;
    const size_t field = (((size_t)g.B * g.ndim * g.S[0] * g.S[1] * g.S[2] * sizeof(float)) + 255) & ~(size_t)255;
    l->o_phi = (g.ws_bytes + 255) & ~(size_t)255;
    l->o_dphi = l->o_phi + field;
    l->o_svf = l->o_dphi + field;
    l->ws_bytes = l->o_svf + l->svf_bytes;
    return TRX_OK;
}

extern "C" size_t trx_bspline_svf_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int squarings)
{
    BsGeom g;
    BsSvfLayout l;
    if (bspline_geom(ndim, B, D, H, W, sz, sy, sx, &g) != TRX_OK || bspline_svf_layout(g, squarings, &l) != TRX_OK) return 0;
    return l.ws_bytes;
}

extern "C" int trx_bspline_svf_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                                   int squarings, int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!loss) return TRX_ERR_ARG;
    BsGeom g;
    int rc = bspline_run_checks(vol, opt, st, spacing, iters, workspace, &g);
    if (rc != TRX_OK) return rc;
    BsSvfLayout l;
    if ((rc = bspline_svf_layout(g, squarings, &l)) != TRX_OK) return rc;
    if (workspace_bytes < l.ws_bytes) return TRX_ERR_WORKSPACE;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    char *ws = (char *)workspace;
    float *terms = (float *)(ws + g.terms_offset), *phi = (float *)(ws + l.o_phi), *dphi = (float *)(ws + l.o_dphi);
    if (squarings == 0)   // exp is the identity: trx_bspline_run's data term, launch for launch
        return bspline_loop(g, vol, opt, st, iters, terms, 4, workspace, (hipStream_t)stream, [&]() {
            return trx_flow_loss_grad(vol, loss, st->flow, terms, st->dflow, ws + g.flow_offset, g.flow_bytes, stream);
        });
    return bspline_loop(g, vol, opt, st, iters, terms, 4, workspace, (hipStream_t)stream, [&]() {
        int r = trx_svf_exp(st->flow, phi, g.ndim, g.B, g.S[0], g.S[1], g.S[2], squarings, 0, ws + l.o_svf, l.svf_bytes, stream);
        if (r != TRX_OK) return r;
        r = trx_flow_loss_grad(vol, loss, phi, terms, dphi, ws + g.flow_offset, g.flow_bytes, stream);
        if (r != TRX_OK) return r;
        return trx_svf_exp_backward(st->flow, dphi, st->dflow, g.ndim, g.B, g.S[0], g.S[1], g.S[2], squarings, 0, ws + l.o_svf, l.svf_bytes, stream);
    });
}

extern "C" int trx_bspline_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    return trx_bspline_run(vol, loss, opt, st, spacing, 1, workspace, workspace_bytes, stream);
}
