// Host-side declarations shared by affine.hip, affine_finalize.hip, affine_lattice.hip, affine_mi.hip and affine_flow.hip.  Every kernel is instantiated and launched in
// exactly one of the three (the library is built without relocatable device code), so a kernel another unit needs is reached through the
// host launcher of the unit that owns it.  The cross-unit functions have hidden visibility: libtrx.so exports the trx_* entry points only.
#pragma once
#include <cmath>
#include <type_traits>

#include "trx_common.h"

#define TRX_FIN_THREADS 1024
#define TRX_HIDDEN __attribute__((visibility("hidden")))

namespace trx {

constexpr int kTargetBlocks = 2048;

// affine.hip: the volume checks every affine entry point starts with
TRX_HIDDEN int check_vol(const trx_volumes *v, bool need_target);

// affine_finalize.hip: one launcher per finalise kernel it holds (one block of TRX_FIN_THREADS threads per pair)
TRX_HIDDEN int launch_loss_finalize(const trx_volumes *vol, const trx_loss_cfg *loss, const float *partials, int nblk, float *terms, hipStream_t s);
TRX_HIDDEN int launch_bwd_finalize(const trx_volumes *vol, const float *partials, int nblk, float *dtheta, hipStream_t s);

// what the cross-lattice entry points (trx_affine_*_grids in affine_mi.hip, trx_affine_flow_* in affine_flow.hip) refuse on top of the others
// (ndim: 2 or 3, already checked).  world_ok: the entry point honours mg->world (the rigid / affine mutual-information pair); every other one refuses it,
// and with it the scale is not read
static inline int ami_grid_check(int ndim, const trx_moving_grid *mg, bool world_ok = false)
{
    if (!mg) return TRX_ERR_ARG;
    if (mg->world && !world_ok) return TRX_ERR_ARG;
    if (mg->D < 1 || mg->H < 1 || mg->W < 1 || (double)mg->D * mg->H * mg->W >= 2147483648.0) return TRX_ERR_ARG;
    if (ndim == 2 && mg->D != 1) return TRX_ERR_NDIM;
    for (int k = 0; k < ndim * (ndim + 1) && !mg->world; k++) {
        if (!std::isfinite(mg->scale[k])) return TRX_ERR_ARG;
        if (k % (ndim + 1) < ndim && !(mg->scale[k] > 0.f)) return TRX_ERR_ARG;      // the matrix part: a ratio of extents
    }
    return TRX_OK;
}

// The 2-D or 3-D instance of a kernel template, chosen on the host: f(std::integral_constant<int, ND>{}) with ND = ndim (2 or 3: check_vol).
template <class F>
static void with_ndim(int ndim, F &&f)
{
    if (ndim == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 2>{});
}

}  // namespace trx
