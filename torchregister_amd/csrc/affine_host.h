// Host-side declarations shared by affine.hip, affine_finalize.hip and affine_lattice.hip.  Every kernel is instantiated and launched in
// exactly one of the three (the library is built without relocatable device code), so a kernel another unit needs is reached through the
// host launcher of the unit that owns it.  The cross-unit functions have hidden visibility: libtrx.so exports the trx_* entry points only.
#pragma once
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

// The 2-D or 3-D instance of a kernel template, chosen on the host: f(std::integral_constant<int, ND>{}) with ND = ndim (2 or 3: check_vol).
template <class F>
static void with_ndim(int ndim, F &&f)
{
    if (ndim == 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 2>{});
}

}  // namespace trx
