// Device side of the Parzen joint histogram shared by mi.hip (histogram and gradient of a warped volume) and affine_mi.hip (the same two passes with
// the affine warp inside them): scales and bins of a voxel, the fixed-point accumulate into a block's LDS tables and their flush, the gather of
// d loss / d warped from the table G.  Definition: include/trx.h (trx_mi_loss_grad).  Device functions only; mi_table_kernel is instantiated in
// mi.hip (the library is built without relocatable device code) and reached from other units through launch_mi_table.
#pragma once
#include <algorithm>

#include "affine_host.h"   // TRX_HIDDEN
#include "trx_common.h"

namespace trx {

constexpr int kMiChunk = 16384;              // voxels per block of the histogram and gradient passes (64 per thread)
#define TRX_MI_ONE 2147483648u              // fixed-point units per voxel (2^31)

// K x K tables of 64-bit cells a block of the histogram pass keeps in LDS: one per wave while they fit into 64 KB
static inline int mi_tables(int K) { return std::min(TRX_WAVES, 8192 / (K * K)); }

struct MiScale {
    float lo_t, s_t, lo_w, s_w;
};

// (lo_t, hi_t, lo_w, hi_w) -> offsets and scales, fp32 division
__device__ __forceinline__ MiScale mi_scale(const float *__restrict__ range, int b, int K)
{
#pragma clang fp contract(off)
    const float lo_t = range[b * 4], hi_t = range[b * 4 + 1], lo_w = range[b * 4 + 2], hi_w = range[b * 4 + 3];
    MiScale m;
    m.lo_t = lo_t; m.lo_w = lo_w;
    m.s_t = hi_t > lo_t ? (float)K / (hi_t - lo_t) : 0.f;
    m.s_w = hi_w > lo_w ? (float)(K - 3) / (hi_w - lo_w) : 0.f;
    return m;
}

// One voxel: target bin a in [0, K - 1], first warped bin c - 1 with c in [1, K - 3], r = u - c in [0, 1], and whether x lies inside [0, K - 3].
// The index arithmetic is a subtract and a multiply in fp32, never contracted; NaN falls into bin 0.
struct MiVoxel {
    int a, c;
    float r;
    bool inside;
};

__device__ __forceinline__ MiVoxel mi_voxel(float t, float w, const MiScale &m, int K)
{
#pragma clang fp contract(off)
    MiVoxel v;
    const float at = floorf((t - m.lo_t) * m.s_t);
    v.a = (int)fminf(fmaxf(at, 0.f), (float)(K - 1));
    const float x = (w - m.lo_w) * m.s_w, top = (float)(K - 3);
    v.inside = x >= 0.f && x <= top;
    const float u = 1.f + fminf(fmaxf(x, 0.f), top);
    v.c = min((int)floorf(u), K - 3);
    v.r = u - (float)v.c;
    return v;
}

// The block's T tables [T][K][K] of 64-bit cells in LDS, zeroed; every thread has passed a barrier behind it
__device__ __forceinline__ void mi_lds_clear(unsigned long long *lds, int cells)
{
    for (int i = threadIdx.x; i < cells; i += TRX_BLOCK) lds[i] = 0ull;
    __syncthreads();
}

// One voxel into a K x K table in LDS: its four cubic B-spline weights in fixed point (three converted from fp32, the largest - a middle one - as the
// remainder: the voxel adds exactly TRX_MI_ONE), integer adds
__device__ __forceinline__ void mi_accumulate(unsigned long long *table, const MiVoxel &v, int K)
{
    const float r = v.r, r2 = r * r, r3 = r2 * r, u = 1.f - r;
    const float w0 = u * u * u * (1.f / 6.f), w3 = r3 * (1.f / 6.f);
    const float w1 = (3.f * r3 - 6.f * r2 + 4.f) * (1.f / 6.f), w2 = (-3.f * r3 + 3.f * r2 + 3.f * r + 1.f) * (1.f / 6.f);
    const unsigned q0 = __float2uint_rn(w0 * (float)TRX_MI_ONE), q3 = __float2uint_rn(w3 * (float)TRX_MI_ONE);   // each <= 2^31 / 6
    unsigned q1, q2;
    if (r < 0.5f) {
        q2 = __float2uint_rn(w2 * (float)TRX_MI_ONE);
        q1 = TRX_MI_ONE - q0 - q2 - q3;
    } else {
        q1 = __float2uint_rn(w1 * (float)TRX_MI_ONE);
        q2 = TRX_MI_ONE - q0 - q1 - q3;
    }
    unsigned long long *cell = table + v.a * K + v.c - 1;
    atomicAdd(cell, (unsigned long long)q0);
    atomicAdd(cell + 1, (unsigned long long)q1);
    atomicAdd(cell + 2, (unsigned long long)q2);
    if (q3) atomicAdd(cell + 3, (unsigned long long)q3);
}

// Behind a barrier: the block's T tables summed, the non-empty cells added to the pair's table in global memory (integer atomics: any order, the same bits)
__device__ __forceinline__ void mi_flush(const unsigned long long *lds, int T, int KK, unsigned long long *__restrict__ dst)
{
    for (int i = threadIdx.x; i < KK; i += TRX_BLOCK) {
        unsigned long long s = 0;
        for (int tb = 0; tb < T; tb++) s += lds[tb * KK + i];
        if (s) atomicAdd(dst + i, s);
    }
}

// d loss / d warped of one voxel from the pair's table G (K x K floats, in LDS): sum_j G[a][c - 1 + j] beta'_j(r), 0 outside the range
__device__ __forceinline__ float mi_voxel_grad(const float *G, const MiVoxel &v, int K)
{
    const float r = v.r, r2 = r * r, u = 1.f - r;
    const float *g = G + v.a * K + v.c - 1;
    float acc = -0.5f * u * u * g[0];
    acc = fmaf(0.5f * (3.f * r2 - 4.f * r), g[1], acc);
    acc = fmaf(0.5f * (-3.f * r2 + 2.f * r + 1.f), g[2], acc);
    acc = fmaf(0.5f * r2, g[3], acc);
    return v.inside ? acc : 0.f;
}

// The region-of-interest mask (trx_mi_cfg.mask: one byte per voxel of the target lattice, non-zero = the voxel counts), read like t and w:
// thread-strided within the chunk, non-temporal.  A pass is instantiated with and without it; the unmasked instance has no mask code at all.
template <bool MASKED>
__device__ __forceinline__ bool mi_counts(const unsigned char *__restrict__ mask, unsigned i)
{
    if constexpr (MASKED) return __builtin_nontemporal_load(mask + i) != 0;
    else return true;
}

// mi.hip: mi_table_kernel, one block per pair - counts [B][K][K] -> loss [B] (nullable) and G [B][K][K] = d loss / d P scaled by s_w / N (nullable).
// With cfg->mask set, or from_counts (the overlap rule of the fused affine passes selects voxels without a target mask), N is ignored: the kernel takes
// N_m = (sum of the pair's counts) / TRX_MI_ONE, an exact integer, from the table itself.
TRX_HIDDEN int launch_mi_table(const unsigned long long *counts, unsigned N, int B, const trx_mi_cfg *cfg, bool from_counts, float *loss, float *G, hipStream_t s);

}  // namespace trx
