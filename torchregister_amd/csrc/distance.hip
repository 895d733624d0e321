// Euclidean distance transform, mask surface and label overlap counts (include/trx.h: trx_distance_transform, trx_mask_surface, trx_label_overlap;
// DESIGN.md section 4.22; extension, the reference has none of them).  CPU restatement: tests/distance_ref.py.
//
// The squared distance is separable: d2(z, y, x) = min_z' [ w_z (z - z')^2 + min_y' [ w_y (y - y')^2 + min_x' w_x (x - x')^2 ] ] over features (z', y', x'),
// one pass per axis, each a min-plus g(i) = min_j f(j) + w (i - j)^2 along its lines.  Without voxel sizes (ISO) w = 1 and every value is an unsigned
// integer below 2^30 (sizes <= 16384), "no feature" is kNone = 2^31 - 1: kNone + w k^2 < 2^32 does not wrap and stays above every real value, so no
// pass special-cases it.  With voxel sizes the values are fp32, "no feature" is +inf.
//
//   edt_row_kernel<ISO>          the contiguous axis.  One wave per row, 64 voxels per step.  The step's ballot gives every lane the nearest feature at
//                                or left of it (highest set bit at or below the lane) and at or right of it (lowest set bit at or above); the last feature
//                                of earlier steps is carried; where the step's word has no bit above a lane the first feature of a later step is found by
//                                looking ahead and kept until the walk passes it (a word is loaded at most twice).  No LDS, no barrier.  Tie: the left one.
//   edt_line_kernel<ISO, ...>    a strided axis: the volume as [outer][n][inner], the pass along n.  A wave owns one output index i and 64 consecutive
//                                lines (lanes along `inner`, the contiguous direction), so every access at a fixed j is one 256-byte run.  Exact outward
//                                search: j = i -+ k for growing k, four k per round with their loads issued together, until w k^2 >= the best of every
//                                lane (the ballot) or both ends are passed.  A candidate replaces the best only when strictly smaller, the lower index first:
//                                the argmin is a fixed function of the input.  Which entries of a line hold a value at all is the same for all lines of
//                                a plane (pass y: the rows with a feature, one byte each from pass x) or of the pair (pass z: the planes with one, one
//                                byte each from pass y): the search starts at that range [first, last] and never leaves it, so empty space around the
//                                features costs nothing.  Cost per output: the steps from the range's near end until w k^2 >= the best, at most
//                                last - first + 1; O(n^2) per line at worst (features at both ends of the axis and none the search can stop at).
//   nearest                      pass x keeps its argmin x' and pass y (3-D) its argmin y' as int16 in the workspace; the last pass gathers
//                                y' = ny(z', y, x), x' = nx(z', y', x).  Nothing of this is stored or read when `nearest` is NULL.
//   mask_surface_kernel          one voxel per thread: foreground with a face neighbour that is background or outside.
//   label_overlap_kernel         a block takes kOverlapChunk voxels of a pair; 3 L 32-bit counters in LDS; a thread keeps the run of equal label pairs it
//                                sees in a register and adds it to LDS when the pair changes; non-zero counters are flushed with 64-bit integer adds.
// The transform has no atomics and no floating-point sum: the same bits on every call, a pair's bits do not depend on the batch around it.
#include "trx_common.h"

#include <cmath>
#include <type_traits>

namespace trx {

constexpr unsigned kNone = 0x7fffffffu;      // ISO: no feature on the lines seen so far
constexpr int kMaxSize = 16384;              // 3 * 16383^2 < 2^30
constexpr int kLineRows = TRX_WAVES;         // output indices per block of edt_line_kernel
constexpr int kRound = 4;                    // k per round of the outward search
constexpr unsigned kOverlapChunk = 16384;    // voxels per block of label_overlap_kernel

template <bool ISO>
using edt_t = std::conditional_t<ISO, unsigned, float>;

// w k^2
template <bool ISO>
__device__ __forceinline__ edt_t<ISO> edt_cost(int k, float w)
{
    if constexpr (ISO) return (unsigned)(k * k);
    else return w * (float)(k * k);
}

template <bool ISO>
__device__ __forceinline__ edt_t<ISO> edt_none()
{
    if constexpr (ISO) return kNone;
    else return INFINITY;
}

template <bool ISO>
__global__ __launch_bounds__(TRX_BLOCK) void edt_row_kernel(const unsigned char *__restrict__ mask, edt_t<ISO> *__restrict__ out, short *__restrict__ nx,
                                                             unsigned char *__restrict__ row_any, unsigned rows, int W, float w)
{
    const int lane = threadIdx.x & 63;
    const unsigned row = blockIdx.x * (unsigned)TRX_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;      // wave-uniform
    const size_t base = ((size_t)blockIdx.y * rows + row) * (size_t)W;
    const unsigned char *__restrict__ m = mask + base;
    constexpr int kNoRight = 0x7fffffff;
    int left = -1;        // the last feature before the step
    int next = -1;        // the first feature at or behind the end of the step, kNoRight if there is none; stale while it lies before that end
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const unsigned long long word = __ballot(x < W && m[min(x, W - 1)] != 0);
        if (!(word >> 63) && next < x0 + 64) {      // some lane has no feature right of it in this word
            next = kNoRight;
            for (int t0 = x0 + 64; t0 < W; t0 += 64) {
                const int t = t0 + lane;
                const unsigned long long ahead = __ballot(t < W && m[min(t, W - 1)] != 0);
                if (ahead) {
                    next = t0 + __builtin_ctzll(ahead);
                    break;
                }
            }
        }
        const unsigned long long at_or_left = word & (~0ull >> (63 - lane)), at_or_right = word >> lane;
        const int l = at_or_left ? x0 + 63 - __builtin_clzll(at_or_left) : left;
        const int r = at_or_right ? x + __builtin_ctzll(at_or_right) : next;
        const int dl = l >= 0 ? x - l : kNoRight, dr = r != kNoRight ? r - x : kNoRight;
        const int n = dl <= dr ? l : r;      // both missing: l = -1
        if (x < W) {
            const int d = x - n;
            out[base + x] = n < 0 ? edt_none<ISO>() : d == 0 ? edt_t<ISO>(0) : edt_cost<ISO>(d, w);
            if (nx) nx[base + x] = (short)n;
        }
        if (word) left = x0 + 63 - __builtin_clzll(word);
    }
    if (lane == 0) row_any[(size_t)blockIdx.y * rows + row] = left >= 0;
}

// The pass along n of [outer][n][inner] (per pair).  FINAL: `out` is dist2 (fp32, +inf for "no feature").  arg_out (nullable): this pass's argmin as
// int16.  nearest (nullable, FINAL only): the composed index, ND channels; ny is read only for ND == 3.  any [pairs][any_stride]: byte o n + j says whether
// the entries j of the lines of `o` hold a value at all - it is the same for every line of an `o` (pass y: the row (z, j) has a feature; pass z: the
// plane j has one), so the wave knows the range [first, last] outside of which every candidate is "no feature" and starts its search at the range:
// exact, and what keeps a far feature from costing its distance in steps.  plane_any (nullable, pass y of 3-D): whether the plane `o` has a row at all.
template <bool ISO, bool FINAL, int ND>
__global__ __launch_bounds__(TRX_BLOCK) void edt_line_kernel(const edt_t<ISO> *__restrict__ in, void *__restrict__ out_, int n, unsigned inner, unsigned nvox,
                                                              float w, const unsigned char *__restrict__ any, unsigned any_stride,
                                                              unsigned char *__restrict__ plane_any, short *__restrict__ arg_out,
                                                              const short *__restrict__ nx, const short *__restrict__ ny, int *__restrict__ nearest, int H, int W)
{
    using T = edt_t<ISO>;
    const int lane = threadIdx.x & 63;
    const unsigned npc = (inner + 63u) / 64u, nic = ((unsigned)n + kLineRows - 1u) / kLineRows;
    const unsigned pc = blockIdx.x % npc, t = blockIdx.x / npc;
    const unsigned o = t / nic;
    const int i = (int)((t - o * nic) * kLineRows + (threadIdx.x >> 6));
    if (i >= n) return;      // wave-uniform
    const unsigned p = pc * 64u + lane;
    const bool valid = p < inner;
    const unsigned pl = valid ? p : inner - 1u;      // a lane behind the end repeats the last line and stores nothing
    const size_t pair = (size_t)blockIdx.y * nvox;
    const unsigned line = o * (unsigned)n * inner + pl;
    const T *__restrict__ f = in + pair + line;
    int first = n, last = -1;
    {
        const unsigned char *__restrict__ a = any + (size_t)blockIdx.y * any_stride + (size_t)o * (unsigned)n;
        for (int j0 = 0; j0 < n; j0 += 64 * kRound) {      // kRound bytes per lane in flight, then their ballots in ascending order
            bool set[kRound];
#pragma unroll
            for (int u = 0; u < kRound; u++) {
                const int j = j0 + 64 * u + lane;
                set[u] = j < n && a[min(j, n - 1)] != 0;
            }
#pragma unroll
            for (int u = 0; u < kRound; u++) {
                const unsigned long long word = __ballot(set[u]);
                if (word) {
                    if (last < 0) first = j0 + 64 * u + __builtin_ctzll(word);
                    last = j0 + 64 * u + 63 - __builtin_clzll(word);
                }
            }
        }
        if (plane_any && i == 0 && pc == 0 && lane == 0) plane_any[(size_t)blockIdx.y * (any_stride / (unsigned)n) + o] = first <= last;
    }
    T best = f[(size_t)i * inner];
    int bj = i;
    for (int k0 = max(1, max(first - i, i - last)); i - k0 >= first || i + k0 <= last; k0 += kRound) {
        if (__all(!(edt_cost<ISO>(k0, w) < best))) break;
        T lo[kRound], hi[kRound];
#pragma unroll
        for (int u = 0; u < kRound; u++) {      // clamped indices: every load is in the line, the ones out of range are not compared
            lo[u] = f[(size_t)max(i - k0 - u, 0) * inner];
            hi[u] = f[(size_t)min(i + k0 + u, n - 1) * inner];
        }
#pragma unroll
        for (int u = 0; u < kRound; u++) {
            const int k = k0 + u;
            const T wk = edt_cost<ISO>(k, w);
            const T cl = lo[u] + wk, ch = hi[u] + wk;
            if (i - k >= first && cl < best) { best = cl; bj = i - k; }
            if (i + k <= last && ch < best) { best = ch; bj = i + k; }
        }
    }
    if (!valid) return;
    const unsigned v = line + (unsigned)i * inner;      // the voxel inside the pair
    if constexpr (!FINAL) {
        ((T *)out_)[pair + v] = best;
        if (arg_out) arg_out[pair + v] = (short)bj;
    } else {
        bool none;
        float d;
        if constexpr (ISO) { none = best >= kNone; d = none ? INFINITY : (float)best; }
        else { none = best == INFINITY; d = best; }
        ((float *)out_)[pair + v] = d;
        if (nearest) {
            int idx[ND];
            if constexpr (ND == 3) {      // the pass along z: outer = 1, p = y W + x
                const int x = (int)(p % (unsigned)W);
                idx[0] = bj;
                idx[1] = none ? -1 : ny[pair + (size_t)bj * inner + p];
                idx[2] = none ? -1 : nx[pair + ((size_t)bj * H + idx[1]) * W + x];
            } else {                      // the pass along y of a plane: p = x
                idx[0] = bj;
                idx[1] = none ? -1 : nx[pair + (size_t)bj * W + p];
            }
            if (none) idx[0] = -1;
#pragma unroll
            for (int a = 0; a < ND; a++) nearest[((size_t)blockIdx.y * ND + a) * nvox + v] = idx[a];
        }
    }
}

__global__ __launch_bounds__(TRX_BLOCK) void mask_surface_kernel(const unsigned char *__restrict__ mask, unsigned char *__restrict__ surface, unsigned nvox, int D,
                                                                  int H, int W)
{
    const unsigned v = blockIdx.x * (unsigned)TRX_BLOCK + threadIdx.x;
    if (v >= nvox) return;
    const unsigned char *__restrict__ m = mask + (size_t)blockIdx.y * nvox;
    unsigned char s = 0;
    if (m[v]) {
        const unsigned r = v / (unsigned)W, HW = (unsigned)H * (unsigned)W;
        const int x = (int)(v - r * (unsigned)W), z = (int)(r / (unsigned)H), y = (int)(r - (unsigned)z * (unsigned)H);
        // an axis of one voxel has both neighbours outside: every foreground voxel of a plane is a surface voxel of a 3-D call with D == 1;
        // the 2-D call (D == 1 by contract) has no z neighbours, and the host passes D = 0 for it
        bool open = x == 0 || x == W - 1 || y == 0 || y == H - 1 || (D > 0 && (z == 0 || z == D - 1));
        if (!open) {
            open = !m[v - 1] || !m[v + 1] || !m[v - (unsigned)W] || !m[v + (unsigned)W];
            if (D > 0) open = open || !m[v - HW] || !m[v + HW];
        }
        s = open ? 1 : 0;
    }
    surface[(size_t)blockIdx.y * nvox + v] = s;
}

template <typename LabelT>
__global__ __launch_bounds__(TRX_BLOCK) void label_overlap_kernel(const LabelT *__restrict__ a, const LabelT *__restrict__ b, unsigned nvox, unsigned L,
                                                                   unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned table[];      // [L][3]
    for (unsigned k = threadIdx.x; k < 3u * L; k += TRX_BLOCK) table[k] = 0u;
    __syncthreads();
    const LabelT *__restrict__ pa = a + (size_t)blockIdx.y * nvox, *__restrict__ pb = b + (size_t)blockIdx.y * nvox;
    const unsigned first = blockIdx.x * kOverlapChunk, last = min(nvox, first + kOverlapChunk);
    unsigned ra = L, rb = L, run = 0;      // the run of equal pairs in flight; a label outside [0, L) is folded to L and counts nowhere
    for (unsigned v = first + threadIdx.x; v < last; v += TRX_BLOCK) {
        const unsigned la = min((unsigned)pa[v], L), lb = min((unsigned)pb[v], L);      // a negative int32 is a large unsigned
        if (la != ra || lb != rb) {
            if (run) {
                if (ra < L) atomicAdd(&table[3u * ra], run);
                if (rb < L) atomicAdd(&table[3u * rb + 1u], run);
                if (ra < L && ra == rb) atomicAdd(&table[3u * ra + 2u], run);
            }
            ra = la; rb = lb; run = 0;
        }
        run++;
    }
    if (run) {
        if (ra < L) atomicAdd(&table[3u * ra], run);
        if (rb < L) atomicAdd(&table[3u * rb + 1u], run);
        if (ra < L && ra == rb) atomicAdd(&table[3u * ra + 2u], run);
    }
    __syncthreads();
    unsigned long long *__restrict__ c = counts + (size_t)blockIdx.y * 3u * L;
    for (unsigned k = threadIdx.x; k < 3u * L; k += TRX_BLOCK)
        if (table[k]) atomicAdd(&c[k], (unsigned long long)table[k]);
}

struct DistGeom {
    int ndim, B, D, H, W;
    unsigned nvox;
    size_t nx_offset, ny_offset, row_any_offset, plane_any_offset, ws_bytes;
};

static size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

// [host] TRX_OK or the refusal shared by the entry points of this file
static int dist_geom(int ndim, int B, int D, int H, int W, DistGeom *g)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (B < 1 || B > 65535 || D < 1 || H < 1 || W < 1 || D > kMaxSize || H > kMaxSize || W > kMaxSize || (double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    g->ndim = ndim; g->B = B; g->D = D; g->H = H; g->W = W;
    g->nvox = (unsigned)D * (unsigned)H * (unsigned)W;
    const size_t total = (size_t)B * g->nvox;
    g->nx_offset = round256(total * 4);
    g->ny_offset = g->nx_offset + round256(total * 2);
    g->row_any_offset = g->ny_offset + (ndim == 3 ? round256(total * 2) : 0);
    g->plane_any_offset = g->row_any_offset + round256((size_t)B * D * H);
    g->ws_bytes = g->plane_any_offset + round256((size_t)B * D);
    return TRX_OK;
}

template <bool ISO>
static int distance_launch(const DistGeom &g, const unsigned char *mask, const float *w, float *dist2, int *nearest, void *workspace, hipStream_t s)
{
    using T = edt_t<ISO>;
    T *buf = (T *)workspace;
    short *nx = nearest ? (short *)((char *)workspace + g.nx_offset) : nullptr;
    short *ny = nearest && g.ndim == 3 ? (short *)((char *)workspace + g.ny_offset) : nullptr;
    unsigned char *row_any = (unsigned char *)workspace + g.row_any_offset, *plane_any = (unsigned char *)workspace + g.plane_any_offset;
    const unsigned rows = (unsigned)g.D * (unsigned)g.H, B = (unsigned)g.B;
    const dim3 block(TRX_BLOCK);
    const unsigned xc = ((unsigned)g.W + 63u) / 64u;
    // 3-D: x -> dist2 (as scratch), y -> workspace, z -> dist2;  2-D: x -> workspace, y -> dist2
    T *row_out = g.ndim == 3 ? (T *)dist2 : buf;
    hipLaunchKernelGGL(edt_row_kernel<ISO>, dim3((rows + TRX_WAVES - 1) / TRX_WAVES, B), block, 0, s, mask, row_out, nx, row_any, rows, g.W, w[g.ndim - 1]);
    TRX_CHECK_LAUNCH();
    const dim3 ygrid(xc * (((unsigned)g.H + kLineRows - 1u) / kLineRows) * (unsigned)g.D, B);
    if (g.ndim == 2) {
        hipLaunchKernelGGL((edt_line_kernel<ISO, true, 2>), ygrid, block, 0, s, (const T *)buf, (void *)dist2, g.H, (unsigned)g.W, g.nvox, w[0],
                           (const unsigned char *)row_any, rows, (unsigned char *)nullptr, (short *)nullptr, (const short *)nx, (const short *)nullptr, nearest, g.H, g.W);
        TRX_CHECK_LAUNCH();
        return TRX_OK;
    }
    hipLaunchKernelGGL((edt_line_kernel<ISO, false, 3>), ygrid, block, 0, s, (const T *)dist2, (void *)buf, g.H, (unsigned)g.W, g.nvox, w[1],
                       (const unsigned char *)row_any, rows, plane_any, ny, (const short *)nullptr,
                       (const short *)nullptr, (int *)nullptr, g.H, g.W);
    TRX_CHECK_LAUNCH();
    const unsigned HW = (unsigned)g.H * (unsigned)g.W;
    const dim3 zgrid(((HW + 63u) / 64u) * (((unsigned)g.D + kLineRows - 1u) / kLineRows), B);
    hipLaunchKernelGGL((edt_line_kernel<ISO, true, 3>), zgrid, block, 0, s, (const T *)buf, (void *)dist2, g.D, HW, g.nvox, w[0],
                       (const unsigned char *)plane_any, (unsigned)g.D, (unsigned char *)nullptr, (short *)nullptr, (const short *)nx,
                       (const short *)ny, nearest, g.H, g.W);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_distance_workspace_bytes(int ndim, int B, int D, int H, int W)
{
    DistGeom g;
    if (dist_geom(ndim, B, D, H, W, &g) != TRX_OK) return 0;
    return g.ws_bytes;
}

extern "C" int trx_distance_transform(const unsigned char *mask, int ndim, int B, int D, int H, int W, const float *voxel, float *dist2, int *nearest,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    if (!mask || !dist2 || !workspace) return TRX_ERR_ARG;
    DistGeom g;
    const int rc = dist_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    float w[3] = {1.f, 1.f, 1.f};
    if (voxel) {
        for (int a = 0; a < ndim; a++) {
            if (!std::isfinite(voxel[a]) || !(voxel[a] > 0.f)) return TRX_ERR_ARG;
            w[a] = voxel[a] * voxel[a];
        }
    }
    if (workspace_bytes < g.ws_bytes) return TRX_ERR_WORKSPACE;
    if (voxel) return distance_launch<false>(g, mask, w, dist2, nearest, workspace, (hipStream_t)stream);
    return distance_launch<true>(g, mask, w, dist2, nearest, workspace, (hipStream_t)stream);
}

extern "C" int trx_mask_surface(const unsigned char *mask, int ndim, int B, int D, int H, int W, unsigned char *surface, void *stream)
{
    if (!mask || !surface) return TRX_ERR_ARG;
    DistGeom g;
    const int rc = dist_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    hipLaunchKernelGGL(mask_surface_kernel, dim3((g.nvox + TRX_BLOCK - 1) / TRX_BLOCK, (unsigned)B), dim3(TRX_BLOCK), 0, (hipStream_t)stream, mask, surface, g.nvox,
                       ndim == 3 ? D : 0, H, W);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_label_overlap(const void *a, const void *b, int label_bytes, int ndim, int B, int D, int H, int W, int L, unsigned long long *counts,
                                 void *stream)
{
    if (!a || !b || !counts) return TRX_ERR_ARG;
    DistGeom g;
    const int rc = dist_geom(ndim, B, D, H, W, &g);
    if (rc != TRX_OK) return rc;
    if (L < 1 || L > 4096 || (label_bytes != 1 && label_bytes != 4)) return TRX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)B * L * 3 * sizeof(unsigned long long), s) != hipSuccess) return TRX_ERR_HIP;
    const dim3 grid((g.nvox + kOverlapChunk - 1) / kOverlapChunk, (unsigned)B), block(TRX_BLOCK);
    const size_t lds = (size_t)3 * L * sizeof(unsigned);
    if (label_bytes == 1)
        hipLaunchKernelGGL(label_overlap_kernel<unsigned char>, grid, block, lds, s, (const unsigned char *)a, (const unsigned char *)b, g.nvox, (unsigned)L, counts);
    else
        hipLaunchKernelGGL(label_overlap_kernel<unsigned>, grid, block, lds, s, (const unsigned *)a, (const unsigned *)b, g.nvox, (unsigned)L, counts);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
