// What csrc/bspline.hip needs of csrc/ngf.hip: the normalised-gradient-field criterion of (target, warped) as the data term of a loop iteration.
// Definitions: include/trx.h (trx_ngf_loss_grad).
#pragma once
#include "trx_common.h"

namespace trx {

constexpr int kNgfChunk = 2048;   // voxels of one pair per block of the forward pass (8 per thread), as kFoldChunk

struct NgfGeom {
    int ndim, B, D, H, W;
    unsigned nvox, nchunk;                                   // voxels per pair, blocks (= fp64 partials and mask counts) per pair
    size_t part_offset, count_offset, scale_offset, ws_bytes;   // workspace: q [B][ndim][nvox] fp32, partials [B][nchunk] fp64, counts [B][nchunk] u32, scale [B] fp32
    float hinv[3];                                           // 1 / voxel size per axis of the tensor (2-D: y, x, unused)
};

// [host] TRX_OK or the refusal of trx_ngf_loss_grad for this geometry (voxel sizes not included)
int ngf_geom(int ndim, int B, int D, int H, int W, NgfGeom *g);

// [host] cfg's own refusals (alpha, eps, voxel) and g->hinv from cfg->voxel
int ngf_cfg_check(const trx_ngf_cfg *cfg, NgfGeom *g);

// [host] forward, reduce and (grad_warped != nullptr) backward launches; everything validated by the two calls above
int ngf_loss_grad_impl(const NgfGeom &g, const float *target, const float *warped, const trx_ngf_cfg *cfg, float *loss, float *grad_warped, void *workspace,
                       hipStream_t s);

}  // namespace trx
