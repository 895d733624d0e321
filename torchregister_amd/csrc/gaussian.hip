// Gaussian smoothing and resampling between grid sizes (trx_gaussian_resample, include/trx.h).  Separable: one 1-D pass per
// axis whose sigma gives a radius R > 0 or whose size changes.  Along an axis of S voxels
//
//     s(i)   = sum_{t = 0 .. 2R} g_t x(i - R + t)       g: the normalised Gaussian, formed in fp64 on the host, handed over as fp32 in the kernel
//                                                        arguments (uniform: the compiler reads them through scalar loads); indices clamped to
//                                                        [0, S - 1] (border) or the tap left out (zeros)
//     out(j) = (1 - l) s(i0) + l s(i1)                   at F.interpolate's position, u / i0 / i1 / l formed as resample_axis_kernel (csrc/pyramid.hip)
//                                                        forms them, u in fp64; an axis that keeps its size: out(j) = s(j)
//
// Taps are summed in fp32 in the order t = 0 .. 2R, s(i0) before s(i1): no atomics, the same bits on every call, and an output depends on its own row
// or column only - not on the batch, the tile or the segment it was computed in.
//
// Both kernels run one wave per block, so every index that is not the lane's is uniform (scalar registers, scalar branches).
//   x pass:       a block stages a run of the row plus its halo in LDS - the run starts on a 256-byte boundary of the buffer, every load instruction
//                 is one whole 256-byte run - and each lane forms its outputs from LDS (consecutive lanes, consecutive words: conflict-free where the
//                 axis keeps its size; a shrink by f strides the reads by f).
//   y / z passes: a wave owns 64 adjacent x-columns and walks a segment of the axis.  The live input rows - 2R + 2 of them plus the rows of one
//                 batch of loads - sit in an LDS ring, 256 bytes per row; a lane only ever touches its own column of the ring, so there is no
//                 barrier.  Rows arrive in batches of GAUSS_BATCH independent 256-byte loads; a row is fetched once per segment, and a segment's
//                 first 2R rows are the only ones its neighbour fetches too.
// Passes run strongest shrink first and intermediates go through the workspace a chunk of volumes at a time: resample_plan's rule (resample_plan.h).
#include <cmath>

#include "resample_plan.h"
#include "trx_common.h"

namespace trx {

#define GAUSS_WAVE 64
#define GAUSS_BATCH 8            // rows per batch of loads in the y / z passes
#define GAUSS_ROW_FLOATS 2048    // LDS floats of an x-pass block (8 KiB)
#define GAUSS_ROW_OUT 256        // outputs of an x-pass tile, where the staged run allows it
#define GAUSS_MAX_BLOCKS (1u << 20)

struct GaussTaps {
    int R;
    float g[2 * TRX_GAUSSIAN_MAX_RADIUS + 1];
};

struct GaussAxis {
    int S, So;       // sizes along the axis
    double scale;    // F.interpolate's ratio
    int align, keep; // keep: S == So (u = j, l = 0)
    int zeros;       // padding 0
};

// F.interpolate's source position of output j, as resample_axis_kernel forms it
__device__ __forceinline__ void gauss_position(const GaussAxis &ax, int j, int &i0, int &i1, float &l)
{
    if (ax.keep) {
        i0 = i1 = j;
        l = 0.f;
        return;
    }
    const double u = ax.align ? (double)j * ax.scale : fmax(((double)j + 0.5) * ax.scale - 0.5, 0.0);
    i0 = min((int)u, ax.S - 1);
    i1 = i0 + (i0 < ax.S - 1 ? 1 : 0);
    l = (i1 == i0) ? 0.f : (float)(u - (double)i0);
}

// ---- pass along x: rows [nrows][S] -> [nrows][So]; a tile = `tile` outputs of one row
__global__ __launch_bounds__(GAUSS_WAVE) void gauss_row_kernel(const float *__restrict__ in, float *__restrict__ out, unsigned long long nrows,
                                                                GaussAxis ax, int tile, int ntile, GaussTaps tp)
{
    __shared__ float run[GAUSS_ROW_FLOATS];
    const int lane = threadIdx.x, R = tp.R, S = ax.S, So = ax.So;
    const unsigned long long nwork = nrows * (unsigned long long)ntile;
    for (unsigned long long w = blockIdx.x; w < nwork; w += gridDim.x) {
        const unsigned long long row = w / (unsigned)ntile;
        const int j0 = (int)(w - row * (unsigned)ntile) * tile, j1 = min(j0 + tile, So);
        const float *__restrict__ src = in + row * (unsigned long long)S;
        int a0, a1, b0, b1;
        float lt;
        gauss_position(ax, j0, a0, a1, lt);
        gauss_position(ax, j1 - 1, b0, b1, lt);
        int lo = a0 - R;
        const int hi = b1 + R;                                                           // inclusive
        lo -= (int)(((long long)(row * (unsigned long long)S) + (long long)lo) & 63);    // back to a 256-byte boundary of the buffer
        const int count = min(hi - lo + 1, GAUSS_ROW_FLOATS);                            // (the host sizes `tile` so that the min never bites)
        for (int e = lane; e < count; e += GAUSS_WAVE) {
            const int q = lo + e;
            const bool inside = q >= 0 && q < S;
            float v = 0.f;
            if (inside || !ax.zeros) v = src[min(max(q, 0), S - 1)];
            run[e] = v;
        }
        __syncthreads();
        for (int j = j0 + lane; j < j1; j += GAUSS_WAVE) {
            int i0, i1;
            float l;
            gauss_position(ax, j, i0, i1, l);
            const float *p = run + (i0 - R - lo);
            float acc = 0.f;
#pragma unroll 8
            for (int t = 0; t <= 2 * R; t++) acc = fmaf(tp.g[t], p[t], acc);
            if (!ax.keep) {
                const float *p1 = p + (i1 - i0);
                float acc1 = 0.f;
#pragma unroll 8
                for (int t = 0; t <= 2 * R; t++) acc1 = fmaf(tp.g[t], p1[t], acc1);
                acc = (1.f - l) * acc + l * acc1;
            }
            out[row * (unsigned long long)So + (unsigned)j] = acc;
        }
        __syncthreads();
    }
}

// s(c) of the lane's column from the ring: rows [b, b + NR) live, row b in slot sb
__device__ __forceinline__ float gauss_col_sum(const float *ring, const GaussTaps &tp, int c, int S, int zeros, int b, int sb, int NR)
{
    const int R = tp.R;
    float acc = 0.f;
    for (int t = 0; t <= 2 * R; t++) {
        const int q = c - R + t;
        if (zeros && (q < 0 || q >= S)) continue;
        int s = sb + (min(max(q, 0), S - 1) - b);
        if (s >= NR) s -= NR;
        acc = fmaf(tp.g[t], ring[s * GAUSS_WAVE], acc);
    }
    return acc;
}

// ---- passes along y and z: [outer][S][inner] -> [outer][So][inner]; a work item = 64 columns of one outer index over `seg` outputs
__global__ __launch_bounds__(GAUSS_WAVE) void gauss_col_kernel(const float *__restrict__ in, float *__restrict__ out, unsigned long long outer,
                                                                unsigned inner, GaussAxis ax, int seg, int nseg, int NR, GaussTaps tp)
{
    extern __shared__ __align__(16) float ring_all[];
    const int lane = threadIdx.x, R = tp.R, S = ax.S, So = ax.So;
    float *ring = ring_all + lane;
    const unsigned ngroup = (inner + GAUSS_WAVE - 1) / GAUSS_WAVE;
    const unsigned long long nwork = outer * ngroup * (unsigned)nseg;
    for (unsigned long long w = blockIdx.x; w < nwork; w += gridDim.x) {
        const unsigned long long og = w / (unsigned)nseg;
        const int ja = (int)(w - og * (unsigned)nseg) * seg, jb = min(ja + seg, So);
        const unsigned long long o = og / ngroup;
        const unsigned k = (unsigned)(og - o * ngroup) * GAUSS_WAVE + lane;
        const bool live = k < inner;
        const float *__restrict__ src = in + o * (unsigned long long)S * inner + (live ? k : 0);
        float *__restrict__ dst = out + o * (unsigned long long)So * inner + (live ? k : 0);
        int e0, e1;
        float lt;
        gauss_position(ax, jb - 1, e0, e1, lt);
        const int seg_last = min(e1 + R, S - 1);      // the last row this segment reads
        int b = -1, sb = 0;                           // oldest live row and its slot
        int next = 0, snext = 0;                      // next row to load and its slot
        for (int j = ja; j < jb; j++) {
            int i0, i1;
            float l;
            gauss_position(ax, j, i0, i1, l);
            const int nb = max(i0 - R, 0);
            if (b < 0 || nb >= next) {                // the segment's first output, or a shrink that skips rows: start the ring afresh
                b = next = nb;
                sb = snext = 0;
            } else {
                sb += nb - b;                         // nb - b < next - b <= NR
                if (sb >= NR) sb -= NR;
                b = nb;
            }
            const int need = min(i1 + R, S - 1);
            while (next <= need) {
                float v[GAUSS_BATCH];
#pragma unroll
                for (int p = 0; p < GAUSS_BATCH; p++) v[p] = (live && next + p <= seg_last) ? src[(unsigned long long)(next + p) * inner] : 0.f;
#pragma unroll
                for (int p = 0; p < GAUSS_BATCH; p++) {
                    if (next + p <= seg_last) {
                        int s = snext + p;
                        if (s >= NR) s -= NR;
                        ring[s * GAUSS_WAVE] = v[p];
                    }
                }
                const int n = min(GAUSS_BATCH, seg_last - next + 1);
                next += n;
                snext += n;
                if (snext >= NR) snext -= NR;
            }
            float acc = gauss_col_sum(ring, tp, i0, S, ax.zeros, b, sb, NR);
            if (!ax.keep) acc = (1.f - l) * acc + l * gauss_col_sum(ring, tp, i1, S, ax.zeros, b, sb, NR);
            if (live) dst[(unsigned long long)j * inner] = acc;
        }
    }
}

// [host] radius of a sigma (voxels) and the normalised taps; false: the radius is above the cap
static bool gauss_taps(float sigma, float truncate, GaussTaps &tp)
{
    const double r = (double)truncate * (double)sigma + 0.5;
    if (r >= (double)TRX_GAUSSIAN_MAX_RADIUS + 1.0) return false;
    const int R = (int)r;
    tp.R = R;
    double g[2 * TRX_GAUSSIAN_MAX_RADIUS + 1], sum = 0.0;
    for (int t = 0; t <= 2 * R; t++) {
        const double d = R > 0 ? (double)(t - R) / (double)sigma : 0.0;
        g[t] = std::exp(-0.5 * d * d);
        sum += g[t];
    }
    for (int t = 0; t <= 2 * R; t++) tp.g[t] = (float)(g[t] / sum);
    return true;
}

static int gauss_launch(const float *in, float *out, int nvol, const int shape[3], int axis, int So, int align, int zeros, const GaussTaps &tp,
                        hipStream_t s)
{
    unsigned long long outer = (unsigned long long)nvol;
    unsigned inner = 1;
    for (int a = 0; a < axis; a++) outer *= (unsigned)shape[a];
    for (int a = axis + 1; a < 3; a++) inner *= (unsigned)shape[a];
    GaussAxis ax{};
    ax.S = shape[axis];
    ax.So = So;
    ax.align = align;
    ax.keep = ax.S == So;
    ax.zeros = zeros;
    ax.scale = align ? (So > 1 ? (double)(ax.S - 1) / (double)(So - 1) : 0.0) : (double)ax.S / (double)So;
    const int R = tp.R;
    if (axis == 2) {
        // outputs per tile: the staged run - ceil((tile - 1) scale) + 2 inputs, the halo 2R, up to 63 floats of alignment - fits the LDS
        const double room = (double)(GAUSS_ROW_FLOATS - 2 * R - 2 - 63 - 4);
        const double ratio = ax.keep ? 1.0 : ax.scale;
        int tile = GAUSS_ROW_OUT;
        if (ratio * (tile - 1) > room) tile = 1 + (int)(room / ratio);
        tile = std::max(1, std::min(tile, So));
        const int ntile = (So + tile - 1) / tile;
        const unsigned long long nwork = outer * (unsigned long long)ntile;
        const unsigned grid = (unsigned)std::min<unsigned long long>(nwork, GAUSS_MAX_BLOCKS);
        hipLaunchKernelGGL(gauss_row_kernel, dim3(grid), dim3(GAUSS_WAVE), 0, s, in, out, outer, ax, tile, ntile, tp);
        TRX_CHECK_LAUNCH();
        return TRX_OK;
    }
    const int NR = 2 * R + 2 + GAUSS_BATCH;
    const size_t lds = (size_t)NR * GAUSS_WAVE * sizeof(float);
    if (lds > 48 * 1024 && hipFuncSetAttribute((const void *)gauss_col_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TRX_ERR_HIP;
    // segments along the axis until the launch has about 4096 waves; a segment re-reads 2R rows of its neighbour, so it is not made shorter than that
    const unsigned long long columns = outer * ((inner + GAUSS_WAVE - 1) / GAUSS_WAVE);
    const int min_seg = std::max(8, 2 * R);
    int nseg = (int)std::min<unsigned long long>((4096 + columns - 1) / columns, (unsigned long long)((So + min_seg - 1) / min_seg));
    nseg = std::max(1, nseg);
    const int seg = (So + nseg - 1) / nseg;
    nseg = (So + seg - 1) / seg;
    const unsigned long long nwork = columns * (unsigned long long)nseg;
    const unsigned grid = (unsigned)std::min<unsigned long long>(nwork, GAUSS_MAX_BLOCKS);
    hipLaunchKernelGGL(gauss_col_kernel, dim3(grid), dim3(GAUSS_WAVE), lds, s, in, out, outer, inner, ax, seg, nseg, NR, tp);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// the largest workspace any choice of filtered axes needs: the query does not see the sigmas
static size_t gauss_workspace(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo)
{
    size_t bytes = 0;
    for (int m = 0; m < 8; m++) {
        if (ndim == 2 && (m & 1)) continue;      // no sigma along z
        const bool also[3] = {(m & 1) != 0, (m & 2) != 0, (m & 4) != 0};
        bytes = std::max(bytes, resample_plan(N, D, H, W, Do, Ho, Wo, also).ws_bytes);
    }
    return bytes;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_gaussian_workspace_bytes(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo)
{
    if (resample_check(ndim, N, D, H, W, Do, Ho, Wo) != TRX_OK) return 0;
    return gauss_workspace(ndim, N, D, H, W, Do, Ho, Wo);
}

extern "C" int trx_gaussian_resample(const float *in, float *out, int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo, const float *sigma,
                                     float truncate, int align_corners, int padding, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!in || !out || !workspace || !sigma) return TRX_ERR_ARG;
    const int rc = resample_check(ndim, N, D, H, W, Do, Ho, Wo);
    if (rc != TRX_OK) return rc;
    if ((align_corners != 0 && align_corners != 1) || (padding != 0 && padding != 1)) return TRX_ERR_ARG;
    if (!std::isfinite(truncate) || truncate <= 0.f) return TRX_ERR_ARG;
    GaussTaps taps[3];
    bool also[3] = {false, false, false};
    for (int a = 0; a < 3; a++) {
        const float sg = a < 3 - ndim ? 0.f : sigma[a - (3 - ndim)];
        if (!std::isfinite(sg) || sg < 0.f) return TRX_ERR_ARG;
        if (!gauss_taps(sg, truncate, taps[a])) return TRX_ERR_ARG;
        also[a] = taps[a].R > 0;
    }
    if (workspace_bytes < gauss_workspace(ndim, N, D, H, W, Do, Ho, Wo)) return TRX_ERR_WORKSPACE;
    const ResamplePlan pl = resample_plan(N, D, H, W, Do, Ho, Wo, also);
    hipStream_t s = (hipStream_t)stream;
    const size_t in_vol = (size_t)D * H * W, out_vol = (size_t)Do * Ho * Wo;
    if (pl.npass == 0) {
        if (in != out && hipMemcpyAsync(out, in, (size_t)N * in_vol * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess) return TRX_ERR_HIP;
        return TRX_OK;
    }
    float *t1 = (float *)workspace, *t2 = t1 + pl.t2_offset;
    const int So[3] = {Do, Ho, Wo};
    for (int n0 = 0; n0 < N; n0 += pl.chunk) {
        const int nv = std::min(pl.chunk, N - n0);
        int shape[3] = {D, H, W};
        const float *src = in + (size_t)n0 * in_vol;
        for (int i = 0; i < pl.npass; i++) {
            float *dst = i == pl.npass - 1 ? out + (size_t)n0 * out_vol : (i == 0 ? t1 : t2);
            const int a = pl.axis[i];
            const int r = gauss_launch(src, dst, nv, shape, a, So[a], align_corners, padding == 0, taps[a], s);
            if (r != TRX_OK) return r;
            shape[a] = So[a];
            src = dst;
        }
    }
    return TRX_OK;
}
