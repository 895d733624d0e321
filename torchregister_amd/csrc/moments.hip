// Intensity moments of N volumes: trx_image_moments (include/trx.h; DESIGN.md section 4.17 - the centre-of-mass initialiser of world-geometry registration)
// and trx_image_moments2 (DESIGN.md section 4.21 - the second moments behind the principal-axes initialiser).
//
//   moments_partial_kernel   a block takes kMomChunk consecutive voxels of one volume (waves along x: VoxelWalk), reads the mask byte first where there is a
//                            mask, forms w = v - offset in fp64 and adds (w, w x, w y(, w z)) to the thread's four fp64 sums in ascending voxels; the block's
//                            sum is a fixed shuffle tree per wave and the four waves in order -> one partial row of four doubles.  4 B/voxel read (5 with a
//                            mask; a voxel outside the mask costs its byte), 32 B per block written.
//   moments_reduce_kernel    one wave per volume: lane l sums rows l, l + 64, ... in ascending order, then the same shuffle tree -> out[n][1 + nd].
// A volume gets ceil(N / kMomChunk) blocks whatever the batch, every sum has a fixed order, nothing is atomic: the same bits on every call.
// Both kernels are templates on the ORDER of the moments.  ORDER 1 is the code above as it was; ORDER 2 carries six more sums per thread - w xx, w xy,
// w yy, w xz, w yz, w zz, each one fma with an index product formed in fp64 (exact while an index stays below 2^26) - through the same walk, the same
// tree and the same row reduction, in rows of kMom2Cols doubles: its first four columns see the operations of ORDER 1 in the same order, hence its bits.
#include "trx_common.h"

namespace trx {

constexpr int kMomChunk = 16384;      // voxels per block (64 per thread), as the mutual-information passes.  Measured at 1 x 256^3 (profiles/affine_mi_world_bench.txt): 40 us raw /
                                      // 67 us masked per call against 8.4 / 10.5 us of traffic - the per-voxel fp64 conversions and FMAs bind, not HBM; 4096-voxel blocks (four
                                      // times the waves in flight) gave 44 / 57 us, so occupancy is not what limits it.  An initialiser that runs twice per registration
constexpr int kMomCols = 4;           // doubles per partial row: w, w x, w y, w z (2-D: the last stays 0)
constexpr int kMom2Cols = 10;         // ORDER 2: ... w xx, w xy, w yy, w xz, w yz, w zz (2-D: every column with a z stays 0 and is not handed out).  Measured at 1 x 256^3
                                      // (profiles/world_search_bench.txt): 47.5 us raw / 73.3 us masked beside ORDER 1's 42.0 / 68.0 in the same process

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

template <bool MASKED, int ORDER>
__global__ __launch_bounds__(TRX_BLOCK) void moments_partial_kernel(const float *__restrict__ x, const unsigned char *__restrict__ mask, const float *__restrict__ offset,
                                                                      unsigned N, int H, int W, double *__restrict__ partials)
{
    constexpr int NC = ORDER == 1 ? kMomCols : kMom2Cols;
    __shared__ double wsum[TRX_WAVES][NC];
    const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *__restrict__ v = x + (size_t)n * N;
    const unsigned char *mk = MASKED ? mask + (size_t)n * N : nullptr;
    const double off = offset ? (double)offset[n] : 0.0;
    double s[NC] = {};
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
        if constexpr (ORDER == 2) {
            const double px = (double)vw.x, py = (double)vw.y, pz = (double)vw.z;
            s[4] = fma(w, px * px, s[4]);
            s[5] = fma(w, px * py, s[5]);
            s[6] = fma(w, py * py, s[6]);
            s[7] = fma(w, px * pz, s[7]);
            s[8] = fma(w, py * pz, s[8]);
            s[9] = fma(w, pz * pz, s[9]);
        }
    }
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const double t = mom_wave_sum(s[k]);
        if (lane == 0) wsum[wave][k] = t;
    }
    __syncthreads();
    if (tid < NC) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < TRX_WAVES; w++) t += wsum[w][tid];
        partials[((size_t)n * gridDim.x + blockIdx.x) * NC + tid] = t;
    }
}

// The output column of partial column k: ORDER 1 and 3-D hand the row out as it is; ORDER 2 in 2-D (ncol 6) drops w z and the three products with a z.
template <int ORDER>
__device__ __forceinline__ int mom_out_col(int k, int ncol)
{
    if constexpr (ORDER == 2) {
        if (ncol != kMom2Cols) return k < 3 ? k : (k >= 4 && k <= 6) ? k - 1 : ncol;
    }
    return k;
}

template <int ORDER>
__global__ __launch_bounds__(64) void moments_reduce_kernel(const double *__restrict__ partials, int nchunk, int ncol, double *__restrict__ out)
{
    constexpr int NC = ORDER == 1 ? kMomCols : kMom2Cols;
    const int n = blockIdx.x, lane = threadIdx.x;
    const double *__restrict__ p = partials + (size_t)n * nchunk * NC;
    double s[NC] = {};
    for (int r = lane; r < nchunk; r += 64) {
#pragma unroll
        for (int k = 0; k < NC; k++) s[k] += p[(size_t)r * NC + k];
    }
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const double t = mom_wave_sum(s[k]);
        const int col = mom_out_col<ORDER>(k, ncol);
        if (lane == 0 && col < ncol) out[(size_t)n * ncol + col] = t;
    }
}

template <int ORDER>
static int moments_launch(const float *x, const unsigned char *mask, const float *offset, int ndim, int N, int D, int H, int W, double *out, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    constexpr int NC = ORDER == 1 ? kMomCols : kMom2Cols;
    if (!x || !out || !workspace) return TRX_ERR_ARG;
    unsigned nvox, nchunk;
    const int rc = moments_geom(ndim, N, D, H, W, &nvox, &nchunk);
    if (rc != TRX_OK) return rc;
    if (workspace_bytes < (size_t)N * nchunk * NC * sizeof(double)) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partials = (double *)workspace;
    const dim3 grid(nchunk, (unsigned)N), block(TRX_BLOCK);
    if (mask) hipLaunchKernelGGL((moments_partial_kernel<true, ORDER>), grid, block, 0, s, x, mask, offset, nvox, H, W, partials);
    else hipLaunchKernelGGL((moments_partial_kernel<false, ORDER>), grid, block, 0, s, x, mask, offset, nvox, H, W, partials);
    TRX_CHECK_LAUNCH();
    const int ncol = ORDER == 1 ? 1 + ndim : 1 + ndim + ndim * (ndim + 1) / 2;
    hipLaunchKernelGGL((moments_reduce_kernel<ORDER>), dim3((unsigned)N), dim3(64), 0, s, (const double *)partials, (int)nchunk, ncol, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

template <int ORDER>
static size_t moments_workspace(int ndim, int N, int D, int H, int W)
{
    unsigned nvox, nchunk;
    if (moments_geom(ndim, N, D, H, W, &nvox, &nchunk) != TRX_OK) return 0;
    return (size_t)N * nchunk * (ORDER == 1 ? kMomCols : kMom2Cols) * sizeof(double);
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_image_moments_workspace_bytes(int ndim, int N, int D, int H, int W) { return moments_workspace<1>(ndim, N, D, H, W); }

extern "C" int trx_image_moments(const float *x, const unsigned char *mask, const float *offset, int ndim, int N, int D, int H, int W, double *out, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return moments_launch<1>(x, mask, offset, ndim, N, D, H, W, out, workspace, workspace_bytes, stream);
}

extern "C" size_t trx_image_moments2_workspace_bytes(int ndim, int N, int D, int H, int W) { return moments_workspace<2>(ndim, N, D, H, W); }

extern "C" int trx_image_moments2(const float *x, const unsigned char *mask, const float *offset, int ndim, int N, int D, int H, int W, double *out, void *workspace,
                                  size_t workspace_bytes, void *stream)
{
    return moments_launch<2>(x, mask, offset, ndim, N, D, H, W, out, workspace, workspace_bytes, stream);
}
