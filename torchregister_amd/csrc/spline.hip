// Nearest-neighbour and cubic B-spline resampling through the final transform: trx_spline_coefficients and
// trx_transform_resample.  Both are gathers: no atomics, no allocation, no host sync, the same bits on every call, and a volume's result does not
// depend on the batch around it.
//
// Coefficients.  c = the interpolating cubic B-spline's coefficients of s with whole-sample mirror boundaries (index i outside 0 .. n-1 reflects about 0
// and n-1, period 2 (n-1)).  The recursive filter's impulse response is h[j] = sqrt(3) z^|j|, z = sqrt(3) - 2; the kernels apply it directly,
//   c[k] = sum_{|j| <= 16} h[j] s[mirror(k - j)],
// truncated where |z|^17 = 1.9e-10 (4.5e-9 of the range over a whole volume), every output independent of every other.  One pass per axis longer than
// one voxel, each a full-size read and write (the workspace holds the intermediate).  The y and z passes walk with x across the wave - a wave's loads and
// stores are consecutive in memory - and a thread owns 8 consecutive outputs of its line, so that it loads 40 voxels for them instead of 8 x 33 (one thread
// per output was bound by the load count: 1 x 256^3 took 260 us for the three passes, 143 us with the runs).  The x pass stages 64 outputs and the 16-voxel
// halo on either side of four rows through LDS (1.5 KiB a block), mirrored while loading, so that global memory sees whole lines once.  The mirror is a
// loop of reflections on a 64-bit index: it survives n = 2, where a halo crosses the volume sixteen times.  Sums run from the outermost pair of taps
// inwards, the same order in every path.
//
// Resample.  One thread per TARGET voxel, x fastest.  Its position comes from one of the two existing chains: theta == NULL: p = x + flow(x), one fp32
// add per axis (trx_flow_warp), in the target lattice; else af_coord (trx_common.h), trx_affine_flow_warp's closed form with theta_eff = theta (.) scale and
// the MOVING sizes, a missing flow being zero.  Order 0 is flow_warp_nearest_kernel's rule (rint, zero where the rounded index lies outside).  Order 3
// reads the COEFFICIENTS: per axis i0 = floor(p), r = p - i0, taps i0 - 1 .. i0 + 2 mirrored, the Parzen window's weights of mi_dev.h; 0 when
// p_a < -0.5 or p_a > S_a - 0.5 on some axis (a NaN position too).  Coordinates, the 3 x 4 weights and the 3 x 4 mirrored indices are formed once per
// voxel and shared by the channels; 64 taps per channel in 3-D, 16 in 2-D, through the caches - where the four x taps are neighbours in memory (no mirror
// along x) a row is one 16-byte load at 4-byte alignment, 16 loads instead of 64 (1 x 256^3 at 0.2 rad: 1135 -> 721 us); flow and out are streams touched
// once and carry the non-temporal hint.  No LDS.
// CPU restatement: tests/spline_ref.py.
#include <cstdint>

#include "affine_host.h"
#include "spline_sample.h"

namespace trx {

constexpr int kSplReach = 16;                 // taps on either side of the centre
constexpr int kSplTile = 64, kSplRows = 4;    // the x pass: outputs per row and rows per block (a wave per row)
constexpr int kSplRun = 8;                    // the y and z passes: consecutive outputs of a thread

// h[j] = sqrt(3) z^j, j = 0 .. 16, formed on the host in fp64: a kernel argument, so the unrolled sums read it from SGPRs
struct SplTaps {
    float h[kSplReach + 1];
};

// The x pass.  src / dst: N volumes of `rows` lines of W voxels, vol_stride elements apart.  W == 1: a copy (an axis of one voxel is left alone).
__global__ __launch_bounds__(kSplTile * kSplRows) void spl_x_kernel(const float *__restrict__ src, float *__restrict__ dst, int rows, int W, size_t vol_stride,
                                                                    SplTaps t)
{
    __shared__ float tile[kSplRows][kSplTile + 2 * kSplReach];
    const int lane = threadIdx.x & (kSplTile - 1), w = threadIdx.x / kSplTile;
    const unsigned tiles = ((unsigned)W + kSplTile - 1) / kSplTile;
    const unsigned rb = blockIdx.x / tiles;
    const int x0 = (int)(blockIdx.x - rb * tiles) * kSplTile;
    const long long row = (long long)rb * kSplRows + w;
    const bool live = row < rows;
    const size_t line = (size_t)blockIdx.y * vol_stride + (size_t)(live ? row : 0) * (size_t)W;
    if (live)
        for (int k = lane; k < kSplTile + 2 * kSplReach; k += kSplTile) tile[w][k] = src[line + spl_mirror((long long)x0 - kSplReach + k, W)];
    __syncthreads();
    const long long x = (long long)x0 + lane;
    if (live && x < W) {
        const float *__restrict__ c = &tile[w][lane + kSplReach];
        float acc = c[0];
        if (W > 1) {
            acc = 0.f;
#pragma unroll
            for (int j = kSplReach; j >= 1; j--) acc = fmaf(t.h[j], c[-j] + c[j], acc);
            acc = fmaf(t.h[0], c[0], acc);
        }
        dst[line + x] = acc;
    }
}

// The y and z passes: an axis of n > 1 voxels whose neighbours lie `stride` elements apart (y: W, z: H W).  A thread owns kSplRun consecutive outputs of
// one line: it loads the kSplRun + 32 voxels they reach once (5 loads per output instead of 33), mirrored where the run comes within 16 voxels of an end.
// Threads are numbered (outer, run, inner), inner = the `stride` voxels that lie between neighbours: a wave's loads and stores are consecutive in memory.
// threads = lines x runs per line, per volume.
__global__ __launch_bounds__(TRX_BLOCK) void spl_axis_kernel(const float *__restrict__ src, float *__restrict__ dst, unsigned threads, int n, unsigned stride,
                                                             size_t vol_stride, SplTaps t)
{
    const size_t tix = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (tix >= threads) return;
    const unsigned runs = ((unsigned)n + kSplRun - 1) / kSplRun;
    const unsigned q = (unsigned)tix / stride, inner = (unsigned)tix - q * stride, outer = q / runs;
    const int k0 = (int)(q - outer * runs) * kSplRun;
    const size_t line = (size_t)blockIdx.y * vol_stride + (size_t)outer * (size_t)n * stride + inner;      // the line's first voxel
    const float *__restrict__ c = src + line;
    float v[kSplRun + 2 * kSplReach];
    if (k0 >= kSplReach && k0 <= n - kSplRun - kSplReach) {
        const float *__restrict__ p = c + (size_t)(k0 - kSplReach) * stride;
#pragma unroll
        for (int m = 0; m < kSplRun + 2 * kSplReach; m++) v[m] = p[(size_t)m * stride];
    } else {
#pragma unroll
        for (int m = 0; m < kSplRun + 2 * kSplReach; m++) v[m] = c[(size_t)spl_mirror((long long)k0 - kSplReach + m, n) * stride];
    }
    float *__restrict__ o = dst + line + (size_t)k0 * stride;
#pragma unroll
    for (int r = 0; r < kSplRun; r++) {
        if (r >= n - k0) break;
        float acc = 0.f;
#pragma unroll
        for (int j = kSplReach; j >= 1; j--) acc = fmaf(t.h[j], v[kSplReach + r - j] + v[kSplReach + r + j], acc);
        o[(size_t)r * stride] = fmaf(t.h[0], v[kSplReach + r], acc);
    }
}

// mg: the SAMPLED lattice and the scales (the host fills in the target's own and ones where the caller gave none).  chan_stride: sampled voxels
// between channels.  theta NULL: the flow-only chain; flow NULL: zero flow.
template <int ND, int ORDER>
__global__ __launch_bounds__(TRX_BLOCK) void transform_resample_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta,
                                                                       const float *__restrict__ flow, int channels, size_t chan_stride, float *__restrict__ out)
{
    constexpr int NT = ND * (ND + 1);
    const int b = blockIdx.y;
    const int D = vol.D, H = vol.H, W = vol.W;
    const int S[3] = {mg.W, mg.H, mg.D};      // x, y, z: the order of the coordinate
    const size_t nvox = (size_t)D * H * W;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    float te[NT];
    if (theta) {
        ami_theta_eff<ND>(theta + (size_t)b * TRX_PSTRIDE, mg, te);
    } else {
#pragma unroll
        for (int k = 0; k < NT; k++) te[k] = 0.f;
    }
    const size_t i = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= nvox) return;
    const unsigned row = (unsigned)i / (unsigned)W, zz = row / (unsigned)H;
    const int x = (int)((unsigned)i - row * (unsigned)W), y = (int)(row - zz * (unsigned)H), z = (int)zz;
    float f[ND], ic[ND];
#pragma unroll
    for (int c = 0; c < ND; c++) f[c] = flow ? __builtin_nontemporal_load(flow + ((size_t)b * ND + c) * nvox + i) : 0.f;
    if (theta) {
        af_coord<ND>(te, f, x, y, z, D, H, W, S[2], S[1], S[0], ic);
    } else {
        ic[0] = (float)x + f[ND - 1];
        ic[1] = (float)y + f[ND - 2];
        if constexpr (ND == 3) ic[2] = (float)z + f[0];
    }
    float *__restrict__ o = out + (size_t)b * channels * nvox + i;

    spl_sample_store<ND, ORDER>(mov, chan_stride, channels, ic, S, o, nvox);
}

// what both coefficient entry points refuse about a geometry
static int spl_check(int ndim, int N, int D, int H, int W)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (N < 1 || D < 1 || H < 1 || W < 1 || N > 65535) return TRX_ERR_ARG;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if ((double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    return TRX_OK;
}

// passes over the volume: x always (a copy when W == 1), y and z where the axis has more than one voxel
static int spl_passes(int ndim, int D, int H) { return 1 + (H > 1) + (ndim == 3 && D > 1); }

static size_t spl_workspace(int ndim, int N, int D, int H, int W)
{
    return spl_passes(ndim, D, H) >= 2 ? (size_t)N * D * H * W * sizeof(float) : 0;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_spline_workspace_bytes(int ndim, int N, int D, int H, int W)
{
    return spl_check(ndim, N, D, H, W) == TRX_OK ? spl_workspace(ndim, N, D, H, W) : SIZE_MAX;
}

extern "C" int trx_spline_coefficients(const float *src, float *coef, int ndim, int N, int D, int H, int W, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    if (!src || !coef || src == coef) return TRX_ERR_ARG;
    const int rc = spl_check(ndim, N, D, H, W);
    if (rc != TRX_OK) return rc;
    const size_t need = spl_workspace(ndim, N, D, H, W);
    if (need && (!workspace || workspace_bytes < need)) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    SplTaps t;
    const double z = std::sqrt(3.0) - 2.0;
    for (int j = 0; j <= kSplReach; j++) t.h[j] = (float)(std::sqrt(3.0) * std::pow(z, j));
    const size_t nvox = (size_t)D * H * W;
    const int rows = D * H, passes = spl_passes(ndim, D, H);
    float *ws = (float *)workspace;
    // the last pass writes coef, the ones before it alternate between the workspace and coef
    float *dst = (passes & 1) ? coef : ws;
    const float *cur = src;
    const unsigned tiles = ((unsigned)W + kSplTile - 1) / kSplTile, rblocks = ((unsigned)rows + kSplRows - 1) / kSplRows;
    hipLaunchKernelGGL(spl_x_kernel, dim3(tiles * rblocks, (unsigned)N), dim3(kSplTile * kSplRows), 0, s, cur, dst, rows, W, nvox, t);
    const int axis_n[2] = {H, ndim == 3 ? D : 1}, axis_outer[2] = {D, 1};
    const unsigned axis_stride[2] = {(unsigned)W, (unsigned)H * (unsigned)W};
    for (int a = 0; a < 2; a++) {
        if (axis_n[a] <= 1) continue;
        cur = dst;
        dst = dst == coef ? ws : coef;
        const size_t threads = (size_t)axis_outer[a] * (((size_t)axis_n[a] + kSplRun - 1) / kSplRun) * axis_stride[a];      // <= nvox
        hipLaunchKernelGGL(spl_axis_kernel, dim3((unsigned)((threads + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)N), dim3(TRX_BLOCK), 0, s, cur, dst, (unsigned)threads,
                           axis_n[a], axis_stride[a], nvox, t);
    }
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_transform_resample(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, int channels, int order,
                                      float *out, void *stream)
{
    int rc = check_vol(vol, false);
    if (rc == TRX_OK && mg) rc = ami_grid_check(vol->ndim, mg);
    if (rc != TRX_OK) return rc;
    if (!out || (!theta && !flow) || (mg && !theta) || channels < 1 || (order != 0 && order != 3)) return TRX_ERR_ARG;
    MovingLattice g;      // (mg->overlap / mask are not read: a resampler pads)
    if (mg) {
        g = *mg;
    } else {
        g.D = vol->D; g.H = vol->H; g.W = vol->W;
        for (int k = 0; k < TRX_PSTRIDE; k++) g.scale[k] = 1.0f;
    }
    const size_t nvox = (size_t)vol->D * vol->H * vol->W, nsrc = (size_t)g.D * g.H * g.W;
    const dim3 grid((unsigned)((nvox + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)vol->B), block(TRX_BLOCK);   // one thread per voxel: < 2^23 blocks (check_vol)
    hipStream_t s = (hipStream_t)stream;
    with_ndim(vol->ndim, [&](auto nd) {
        constexpr int ND = decltype(nd)::value;
        if (order == 3) hipLaunchKernelGGL((transform_resample_kernel<ND, 3>), grid, block, 0, s, *vol, g, theta, flow, channels, nsrc, out);
        else hipLaunchKernelGGL((transform_resample_kernel<ND, 0>), grid, block, 0, s, *vol, g, theta, flow, channels, nsrc, out);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
