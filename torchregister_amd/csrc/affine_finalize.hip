// The finalise kernels behind a loss evaluation (affine_loss_finalize_kernel) and behind a warp backward, full-volume or lattice
// (affine_bwd_finalize_kernel), each with its host launcher (declared in affine_host.h).  The row reduction and the loss they share with the
// step's finalise are in affine_finalize.h.  The step's own finalise kernel (affine_finalize_kernel) stays in affine.hip: compiled in a unit
// without the step kernels' carry prologue its register allocation came out different, and this split changes no kernel's code.
#include "affine_finalize.h"

namespace trx {

__global__ __launch_bounds__(TRX_FIN_THREADS) void affine_loss_finalize_kernel(const float *__restrict__ partials, int nblk,
                                                                               double nvox, trx_loss_cfg lc,
                                                                               float *__restrict__ terms)
{
    __shared__ double S[64];
    const int b = blockIdx.x;
    reduce_partials<5>(partials + (size_t)b * nblk * 5, nblk, S);
    if (threadIdx.x != 0) return;
    const LossCoef L = loss_from_moments(S, nvox, lc);
    terms[b * 4 + 0] = (float)L.total; terms[b * 4 + 1] = (float)L.mse;
    terms[b * 4 + 2] = (float)L.ncc;   terms[b * 4 + 3] = (float)L.ssd;
}

template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void affine_bwd_finalize_kernel(const float *__restrict__ partials, int nblk,
                                                                              int D, int H, int W, float *__restrict__ dtheta)
{
    constexpr int NT = ND * (ND + 1);
    __shared__ double S[64];
    const int b = blockIdx.x;
    reduce_partials<NT>(partials + (size_t)b * nblk * NT, nblk, S);
    if (threadIdx.x >= NT) return;
    const double scale[3] = {0.5 * W, 0.5 * H, 0.5 * D};
    dtheta[(size_t)b * TRX_PSTRIDE + threadIdx.x] = (float)(scale[threadIdx.x / (ND + 1)] * S[threadIdx.x]);
}

// Behind a loss evaluation (trx_affine_loss): the five moments of every row -> the loss terms
int launch_loss_finalize(const trx_volumes *vol, const trx_loss_cfg *loss, const float *partials, int nblk, float *terms, hipStream_t s)
{
    const double nvox = (double)vol->D * vol->H * vol->W;
    hipLaunchKernelGGL(affine_loss_finalize_kernel, dim3(vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, nblk, nvox, *loss, terms);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// Behind a warp backward (trx_affine_warp_backward, trx_affine_warp_lattice_backward): nblk rows of sum(go * J) per pair -> dL/dtheta
int launch_bwd_finalize(const trx_volumes *vol, const float *partials, int nblk, float *dtheta, hipStream_t s)
{
    with_ndim(vol->ndim, [&](auto nd) {
        hipLaunchKernelGGL((affine_bwd_finalize_kernel<decltype(nd)::value>), dim3(vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, nblk, vol->D, vol->H, vol->W, dtheta);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx
