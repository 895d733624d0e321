// What csrc/bspline.hip needs of csrc/jacobian.hip: the folding penalty of a dense flow as two launches inside a loop iteration, and the
// fixed-order sum of its per-block partials for the kernel that decides on the pair's total.  Definitions: include/trx.h (trx_flow_jacobian).
#pragma once
#include "trx_common.h"

namespace trx {

constexpr int kFoldChunk = 2048;   // voxels of one pair per block of the map / partial-sum pass (8 per thread): 8192 blocks at 256^3

struct FoldGeom {
    int ndim, B, D, H, W;
    unsigned nvox, nchunk;          // voxels per pair, blocks (= fp64 partials) per pair
    size_t part_offset, ws_bytes;   // workspace: det [B][nvox] fp32, then partials [B][nchunk] fp64
};

// [host] TRX_OK or the refusal of trx_flow_jacobian / trx_flow_folding for this geometry
int fold_geom(int ndim, int B, int D, int H, int W, FoldGeom *g);

// [host] det(flow) -> workspace, the partial sums of max(0, threshold - det)^2 behind it
int fold_forward_impl(const FoldGeom &g, const float *flow, float threshold, void *workspace, hipStream_t s);

// [host] dflow = (accumulate ? dflow : 0) + weight dP/dflow from the map fold_forward_impl left in the workspace (same flow, same threshold)
int fold_backward_impl(const FoldGeom &g, const float *flow, float threshold, float weight, float *dflow, int accumulate, const void *workspace, hipStream_t s);

// P_b of one pair from its partials, by the 64 lanes of one wave: lane l adds rows l, l + 64, ... in ascending order, then a fixed shuffle tree; fp64,
// rounded once.  Lane 0 holds the result.  The rows are loaded 16 at a time before they are added (a row past the end counts as +0, which changes no
// bit): with one load per add the 128 rows a lane has at 256^3 were 128 dependent trips to L2, 35 us on a single wave.
__device__ __forceinline__ float fold_penalty_from_partials(const double *__restrict__ p, int nchunk, unsigned nvox)
{
    constexpr int kAhead = 16;
    double s = 0.0;
    for (int r = threadIdx.x & 63; r < nchunk; r += 64 * kAhead) {
        double v[kAhead];
#pragma unroll
        for (int k = 0; k < kAhead; k++) {
            const double x = p[min(r + 64 * k, nchunk - 1)];      // the index is clamped, the value selected: no load is predicated
            v[k] = r + 64 * k < nchunk ? x : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kAhead; k++) s += v[k];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return (float)(s / (double)nvox);
}

}  // namespace trx
