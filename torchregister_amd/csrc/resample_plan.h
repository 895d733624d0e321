// [host] What the separable resampling entry points share (trx_resample: csrc/pyramid.hip, trx_gaussian_resample: csrc/gaussian.hip): the geometry
// check, and the plan - which axes get a pass, in which order, and how many volumes go through the workspace at a time.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/trx.h"

namespace trx {

static const size_t RESAMPLE_CHUNK_BYTES = (size_t)96 << 20;

struct ResamplePlan {
    int npass;        // axes that get a pass (0 -> one copy pass)
    int axis[3];      // 0 = D, 1 = H, 2 = W, in pass order
    size_t t1, t2;    // floats per volume after pass 1 / pass 2 (intermediates only where another pass follows)
    size_t t2_offset; // floats from the workspace's start to the chunk's t2
    int chunk;        // volumes per round of passes
    size_t ws_bytes;  // workspace the call needs
};

static int resample_check(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo)
{
    if (ndim != 2 && ndim != 3) return TRX_ERR_NDIM;
    if (ndim == 2 && (D != 1 || Do != 1)) return TRX_ERR_NDIM;
    if (N < 1 || D < 1 || H < 1 || W < 1 || Do < 1 || Ho < 1 || Wo < 1) return TRX_ERR_ARG;
    if ((double)D * H * W >= 2147483648.0 || (double)Do * Ho * Wo >= 2147483648.0) return TRX_ERR_ARG;
    return TRX_OK;
}

// An axis gets a pass when its size changes, or when `also` (nullable, [3]) names it (a filter along an axis that keeps its size).
static ResamplePlan resample_plan(int N, int D, int H, int W, int Do, int Ho, int Wo, const bool *also = nullptr)
{
    ResamplePlan pl{};
    const int S[3] = {D, H, W}, So[3] = {Do, Ho, Wo};
    // strongest shrink first (smallest So/S); ties: the inner axis first
    for (int a = 2; a >= 0; a--)
        if (S[a] != So[a] || (also && also[a])) pl.axis[pl.npass++] = a;
    for (int i = 1; i < pl.npass; i++)
        for (int k = i; k > 0; k--) {
            const int a = pl.axis[k], b = pl.axis[k - 1];
            if ((long long)So[a] * S[b] < (long long)So[b] * S[a]) { pl.axis[k] = b; pl.axis[k - 1] = a; }
        }
    int cur[3] = {D, H, W};
    size_t after[3] = {0, 0, 0};
    for (int i = 0; i < pl.npass; i++) {
        cur[pl.axis[i]] = So[pl.axis[i]];
        after[i] = (size_t)cur[0] * cur[1] * cur[2];
    }
    pl.t1 = pl.npass >= 2 ? after[0] : 0;
    pl.t2 = pl.npass >= 3 ? after[1] : 0;
    const size_t per_vol = (pl.t1 + pl.t2) * sizeof(float);
    pl.chunk = per_vol == 0 ? N : (int)std::max<size_t>(1, std::min<size_t>((size_t)N, RESAMPLE_CHUNK_BYTES / per_vol));
    pl.t2_offset = ((size_t)pl.chunk * pl.t1 + 63) / 64 * 64;   // t2 of the chunk starts on a 256-byte boundary
    pl.ws_bytes = std::max<size_t>(256, (pl.t2_offset + (size_t)pl.chunk * pl.t2) * sizeof(float));
    return pl;
}

}  // namespace trx
