// Intensity moments of N volumes: trx_image_moments (include/trx.h; DESIGN.md section 4.17 - the centre-of-mass initialiser of world-geometry registration).
//
//   moments_partial_kernel   a block takes kMomChunk consecutive voxels of one volume (waves along x: VoxelWalk), reads the mask byte first where there is a
//                            mask, forms w = v - offset in fp64 and adds (w, w x, w y(, w z)) to the thread's four fp64 sums in ascending voxels; the block's
//                            sum is a fixed shuffle tree per wave and the four waves in order -> one partial row of four doubles.  4 B/voxel read (5 with a
//                            mask; a voxel outside the mask costs its byte), 32 B per block written.
//   moments_reduce_kernel    one wave per volume: lane l sums rows l, l + 64, ... in ascending order, then the same shuffle tree -> out[n][1 + nd].
// A volume gets ceil(N / kMomChunk) blocks whatever the batch, every sum has a fixed order, nothing is atomic: the same bits on every call.
#include "trx_common.h"

namespace trx {

constexpr int kMomChunk = 16384;      // voxels per block (64 per thread), as the mutual-information passes.  Measured at 1 x 256^3 (profiles/affine_mi_world_bench.txt): 40 us raw /
                                      // 67 us masked per call against 8.4 / 10.5 us of traffic - the per-voxel fp64 conversions and FMAs bind, not HBM; 4096-voxel blocks (four
                                      // times the waves in flight) gave 44 / 57 us, so occupancy is not what limits it.  An initialiser that runs twice per registration
constexpr int kMomCols = 4;           // doubles per partial row: w, w x, w y, w z (2-D: the last stays 0)

static int moments_geom(int ndim, int N, int D, int H, int W, unsigned *nvox, unsigned *nchunk)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && D != 1) return TRX_ERR_NDIM;
    if (N < 1 || N > 65535 || D < 1 || H < 1 || W < 1 || (double)D * H * W >= 2147483648.0) return TRX_ERR_ARG;
    *nvox = (unsigned)D * (unsigned)H * (unsigned)W;
    *nchunk = (*nvox + kMomChunk - 1) / kMomChunk;
    return TRX_OK;
}

__device__ __forceinline__ double mom_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <bool MASKED>
__global__ __launch_bounds__(TRX_BLOCK) void moments_partial_kernel(const float *__restrict__ x, const unsigned char *__restrict__ mask, const float *__restrict__ offset,
                                                                      unsigned N, int H, int W, double *__restrict__ partials)
{
    __shared__ double wsum[TRX_WAVES][kMomCols];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *__restrict__ v = x + (size_t)n * N;
    const unsigned char *mk = MASKED ? mask + (size_t)n * N : nullptr;
    const double off = offset ? (double)offset[n] : 0.0;
    double s[kMomCols] = {0.0, 0.0, 0.0, 0.0};
    const unsigned first = blockIdx.x * (unsigned)kMomChunk, last = min(N, first + (unsigned)kMomChunk);
    for (VoxelWalk vw(first + tid, TRX_BLOCK, H, W); vw.i < last; vw.next(H, W)) {
        if constexpr (MASKED) {
            if (!mk[vw.i]) continue;
        }
        const double w = (double)__builtin_nontemporal_load(v + vw.i) - off;
        s[0] += w;
        s[1] = fma(w, (double)vw.x, s[1]);
        s[2] = fma(w, (double)vw.y, s[2]);
        s[3] = fma(w, (double)vw.z, s[3]);
    }
#pragma unroll
    for (int k = 0; k < kMomCols; k++) {
        const double t = mom_wave_sum(s[k]);
        if (lane == 0) wsum[wave][k] = t;
    }
    __syncthreads();
    if (tid < kMomCols) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < TRX_WAVES; w++) t += wsum[w][tid];
        partials[((size_t)n * gridDim.x + blockIdx.x) * kMomCols + tid] = t;
    }
}

__global__ __launch_bounds__(64) void moments_reduce_kernel(const double *__restrict__ partials, int nchunk, int ncol, double *__restrict__ out)
{
    const int n = blockIdx.x, lane = threadIdx.x;
    const double *__restrict__ p = partials + (size_t)n * nchunk * kMomCols;
    double s[kMomCols] = {0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < nchunk; r += 64) {
#pragma unroll
        for (int k = 0; k < kMomCols; k++) s[k] += p[(size_t)r * kMomCols + k];
    }
#pragma unroll
    for (int k = 0; k < kMomCols; k++) {
        const double t = mom_wave_sum(s[k]);
        if (lane == 0 && k < ncol) out[(size_t)n * ncol + k] = t;
    }
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_image_moments_workspace_bytes(int ndim, int N, int D, int H, int W)
{
    unsigned nvox, nchunk;
    if (moments_geom(ndim, N, D, H, W, &nvox, &nchunk) != TRX_OK) return 0;
    return (size_t)N * nchunk * kMomCols * sizeof(double);
}

extern "C" int trx_image_moments(const float *x, const unsigned char *mask, const float *offset, int ndim, int N, int D, int H, int W, double *out, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!x || !out || !workspace) return TRX_ERR_ARG;
    unsigned nvox, nchunk;
    const int rc = moments_geom(ndim, N, D, H, W, &nvox, &nchunk);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < (size_t)N * nchunk * kMomCols * sizeof(double)) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partials = (double *)workspace;
    const dim3 grid(nchunk, (unsigned)N), block(TRX_BLOCK);
    if (mask) hipLaunchKernelGGL((moments_partial_kernel<true>), grid, block, 0, s, x, mask, offset, nvox, H, W, partials);
    else hipLaunchKernelGGL((moments_partial_kernel<false>), grid, block, 0, s, x, mask, offset, nvox, H, W, partials);
    TRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((unsigned)N), dim3(64), 0, s, (const double *)partials, (int)nchunk, 1 + ndim, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
