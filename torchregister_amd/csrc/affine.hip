// Affine / rigid hot path for gfx950: fused forward warp + loss moments + analytic backward
// accumulation (F1, one pass over moving and target), device-side finalise (loss, dL/dtheta,
// Theta chain, SGD/Adam, best-theta tracking), forward warp and generic warp backward.
//
// Replaces, per iteration, the ATen chain behind ref:warpings.py:67-93 / :138-159:
//   affine_grid_generator -> grid_sampler_{2,3}d -> mse/NCC reductions -> grid_sampler backward
//   -> affine_grid backward -> SGD.step -> .item()
// with ONE streaming kernel (8 algorithmic bytes / voxel) + one tiny finalise kernel.
//
// Math: with J_p = (d out/d g_c)_p * (xn, yn, zn, 1)_p and dL/dw_p affine in
// (y_p, w_p) given the global moments,  dL/dw_p = cy*y_p + cw*w_p + c0, hence
//   dL/dtheta = cy * sum(y J) + cw * sum(w J) + c0 * sum(J).
// The streaming kernel accumulates {Sy, Sw, Syy, Sww, Syw} and sum(q J) for q in {1, y, w};
// the coefficients only exist after the pass, in the finalise kernel.
//
// This file: the un-tiled gather kernel, the step kernels around the three F1 bodies (affine_tile.h, affine_zstream.h, affine_eft.h), the
// step's finalise kernel, the launch plan and the step / run / loss / warp entry points.  The device functions of the finalise and the carry
// prologue of the step kernels are in affine_finalize.h, the loss and backward finalise kernels in affine_finalize.hip, the lattice warp and
// the NMI loop's kernels in affine_lattice.hip.
#ifdef TRX_DEV
#include <cstdlib>   // getenv: development builds only (tools/kbench.hip); the product library reads no environment variable
#endif
#include "trx_dev.h"   // development instrumentation (in-kernel stamps, LDS padding): no-ops unless tools/kbench.hip asks for them

#include "trx_common.h"
#include "affine_host.h"       // check_vol, the loss / backward finalise launchers (affine_finalize.hip)
#include "affine_finalize.h"   // partial-row and carry-buffer layout, carry_prologue

namespace trx {

struct AffineGeom {
    int TX, TY, logTX, RPT, nxseg, nychunk, nblk;  // nblk = blocks per pair
};

static AffineGeom affine_geom(const trx_volumes &v, int target_blocks_total)
{
    AffineGeom g;
    int tx = 16, l = 4;
    while (tx < v.W && tx < TRX_BLOCK) { tx <<= 1; l++; }
    g.TX = tx; g.logTX = l; g.TY = TRX_BLOCK / tx;
    g.nxseg = (v.W + tx - 1) / tx;
    long rows = (long)v.D * v.H * g.nxseg * v.B;
    long rpt = rows / ((long)g.TY * target_blocks_total);
    if (rpt < 1) rpt = 1;
    if (rpt > 64) rpt = 64;
    g.RPT = (int)rpt;
    int rows_per_blk = g.TY * g.RPT;
    g.nychunk = (v.H + rows_per_blk - 1) / rows_per_blk;
    g.nblk = v.D * g.nychunk * g.nxseg;
    return g;
}

// MODE 0: moments + sum(qJ), q in {1,y,w}   (the optimiser step)
// MODE 1: moments only                       (loss evaluation)
// MODE 2: sum(go*J) over channels            (generic warp backward; `tgt` = grad_out)
template <int ND, int MODE>
__global__ __launch_bounds__(TRX_BLOCK) void affine_accum_kernel(trx_volumes vol, const float *__restrict__ theta,
                                                                 AffineGeom g, int channels, size_t chan_stride,
                                                                 float *__restrict__ partials)
{
    constexpr int NC = ND;                 // gradient components (x, y[, z])
    constexpr int NQ = (MODE == 0) ? 3 : (MODE == 2 ? 1 : 0);
    constexpr int NP = (MODE == 0) ? np_full(ND) : (MODE == 1 ? 5 : ND * (ND + 1));
    const int b = blockIdx.y;
    int id = blockIdx.x;
    const int xs = id % g.nxseg; id /= g.nxseg;
    const int yc = id % g.nychunk;
    const int z = id / g.nychunk;
    const int tid = threadIdx.x;
    const int lx = tid & (g.TX - 1), ly = tid >> g.logTX;
    const int x = xs * g.TX + lx;
    const int D = vol.D, H = vol.H, W = vol.W;

    const float *__restrict__ th = theta + (size_t)b * TRX_PSTRIDE;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ tgt = vol.target + (size_t)b * vol.target_stride;

    float A[NQ > 0 ? NQ : 1][NC], Bq[NQ > 0 ? NQ : 1][NC], m[5];
#pragma unroll
    for (int q = 0; q < (NQ > 0 ? NQ : 1); q++)
#pragma unroll
        for (int c = 0; c < NC; c++) A[q][c] = Bq[q][c] = 0.f;
#pragma unroll
    for (int i = 0; i < 5; i++) m[i] = 0.f;

    float xn = 0.f, zn = 0.f;
    if (x < W) {
        xn = base_coord(vol.xn, x, W);
        // hoisted: everything that does not depend on the row
        float bx, by, bz = 0.f, t_x1, t_y1, t_z1 = 0.f;
        if constexpr (ND == 3) {
            zn = base_coord(vol.zn, z, D);
            bx = fmaf(th[0], xn, fmaf(th[2], zn, th[3]));
            by = fmaf(th[4], xn, fmaf(th[6], zn, th[7]));
            bz = fmaf(th[8], xn, fmaf(th[10], zn, th[11]));
            t_x1 = th[1]; t_y1 = th[5]; t_z1 = th[9];
        } else {
            bx = fmaf(th[0], xn, th[2]);
            by = fmaf(th[3], xn, th[5]);
            t_x1 = th[1]; t_y1 = th[4];
        }
        const float fW = (float)W, fH = (float)H, fD = (float)D;
        const int y0 = yc * g.TY * g.RPT + ly;
        for (int j = 0; j < g.RPT; j++) {
            const int y = y0 + j * g.TY;
            if (y >= H) break;
            const float yn = base_coord(vol.yn, y, H);
            const float ix = unnorm<ND>(fmaf(t_x1, yn, bx), fW);
            const float iy = unnorm<ND>(fmaf(t_y1, yn, by), fH);
            const size_t vox = ((size_t)z * H + y) * W + x;
            float gq[NC];
            float w;
            if constexpr (MODE == 2) {
#pragma unroll
                for (int c = 0; c < NC; c++) gq[c] = 0.f;
                for (int ch = 0; ch < channels; ch++) {
                    const float go = tgt[ch * chan_stride + vox];
                    if constexpr (ND == 3) {
                        const float iz = unnorm<ND>(fmaf(t_z1, yn, bz), fD);
                        Samp3 s = sample3(mov + ch * chan_stride, D, H, W, ix, iy, iz);
                        gq[0] = fmaf(go, s.dx, gq[0]); gq[1] = fmaf(go, s.dy, gq[1]); gq[2] = fmaf(go, s.dz, gq[2]);
                    } else {
                        Samp2 s = sample2(mov + ch * chan_stride, H, W, ix, iy);
                        gq[0] = fmaf(go, s.dx, gq[0]); gq[1] = fmaf(go, s.dy, gq[1]);
                    }
                }
                w = 0.f;
            } else {
                if constexpr (ND == 3) {
                    const float iz = unnorm<ND>(fmaf(t_z1, yn, bz), fD);
                    Samp3 s = sample3(mov, D, H, W, ix, iy, iz);
                    w = s.v; gq[0] = s.dx; gq[1] = s.dy; gq[2] = s.dz;
                } else {
                    Samp2 s = sample2(mov, H, W, ix, iy);
                    w = s.v; gq[0] = s.dx; gq[1] = s.dy;
                }
            }
            if constexpr (MODE != 2) {
                const float yv = tgt[vox];
                m[0] += yv; m[1] += w;
                m[2] = fmaf(yv, yv, m[2]); m[3] = fmaf(w, w, m[3]); m[4] = fmaf(yv, w, m[4]);
                if constexpr (MODE == 0) {
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const float u = yn * gq[c];
                        A[0][c] += gq[c];            Bq[0][c] += u;
                        A[1][c] = fmaf(yv, gq[c], A[1][c]); Bq[1][c] = fmaf(yv, u, Bq[1][c]);
                        A[2][c] = fmaf(w, gq[c], A[2][c]);  Bq[2][c] = fmaf(w, u, Bq[2][c]);
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < NC; c++) { A[0][c] += gq[c]; Bq[0][c] = fmaf(yn, gq[c], Bq[0][c]); }
            }
        }
    }

    // thread-level fold: x and z are fixed per thread, so the xn / zn columns are A scaled
    float vals[NP];
    int o = 0;
    if constexpr (MODE != 2) {
#pragma unroll
        for (int i = 0; i < 5; i++) vals[o++] = m[i];
    }
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int c = 0; c < NC; c++) {
            vals[o++] = xn * A[q][c];
            vals[o++] = Bq[q][c];
            if constexpr (ND == 3) vals[o++] = zn * A[q][c];
            vals[o++] = A[q][c];
        }
    block_reduce_store<NP>(vals, partials + ((size_t)b * g.nblk + blockIdx.x) * NP);
}

#include "affine_tile.h"      // LDS-tiled F1 body: the tile geometries and tile_body, the first four per-pair choices of the step kernels
#include "affine_zstream.h"   // z-streaming F1 body for transforms near the identity: the fifth per-pair choice of the step kernels
#include "affine_eft.h"       // exact-footprint F1 body for rotated transforms: the sixth per-pair choice of the step kernels
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"

// The primary kernel: one geometry (GeomA) for every block.
template <int MODE>
__global__ __launch_bounds__(GeomA::Threads, TRX_TILE_MIN_WAVES) void affine_tile_kernel(trx_volumes vol, const float *__restrict__ theta,
                                                                                          TileGeom tg, int channels, float *__restrict__ partials)
{
    __shared__ __attribute__((aligned(16))) float box[GeomA::BoxAlloc + TRX_DEV_LDS_PAD];
    tile_body<MODE, GeomA>(vol, theta, tg, channels, partials, box, blockIdx.x, blockIdx.y, gridDim.x, trx_wave_index());
}

// Does geometry G's box hold the pre-image of one of its tiles for this theta?  (theta-only: the tile-independent maximum extent, the same
// bound the fast loop fetches.)  NaN / huge theta compare false: GeomR, whose own per-tile test then sends everything to the fallback.
template <class G>
__device__ __forceinline__ bool dual_fits(const float *__restrict__ th, float fD, float fH, float fW)
{
    const float slope[3][3] = {{th[0], th[1] * fW / fH, th[2] * fW / fD}, {th[4] * fH / fW, th[5], th[6] * fH / fD}, {th[8] * fD / fW, th[9] * fD / fH, th[10]}};
    const float ex[3] = {(float)(G::TX - 1), (float)(G::TY - 1), (float)(G::TZ - 1)};
    float span[3];
#pragma unroll
    for (int c = 0; c < 3; c++) span[c] = fabsf(slope[c][0]) * ex[0] + fabsf(slope[c][1]) * ex[1] + fabsf(slope[c][2]) * ex[2];
    return (span[0] < 1.0e6f) && (span[1] < 1.0e6f) && (span[2] < 1.0e6f) &&
           ((((int)floorf(span[0] + 0.1f) + 5) >> 2) + 1 <= G::BW4) && ((int)floorf(span[1] + 0.1f) + 3 <= G::BH) &&
           ((int)floorf(span[2] + 0.1f) + 3 <= G::BD);
}
// The geometry a pair's blocks run (0 = GeomD, the deep tile, step kernels only; 1 = GeomA; 2 = GeomR; 3 = GeomRD, step kernels only): evaluated identically by every
// block of the pair and by the step's finalise kernel.
__device__ __forceinline__ int dual_choice(const float *__restrict__ th, float fD, float fH, float fW, bool with_deep, bool with_rd = false, int zs_planes = 0)
{
    if (zs_planes > 0 && zs_nsub<ZS64>(th, fD, fH, fW, zs_planes) > 0) return 4;   // 4 = the z-streaming body (step kernels only, transforms next to the identity)
    if (with_deep && dual_fits<GeomD>(th, fD, fH, fW)) return 0;
    if (dual_fits<GeomA>(th, fD, fH, fW)) return 1;
    return (with_rd && dual_fits<GeomRD>(th, fD, fH, fW)) ? 3 : 2;   // 3 = GeomRD: GeomR's box under a 16 x 16 x 16 tile, where the pre-image still fits it
}

// The dual kernel: per pair, GeomA where its box holds the pre-image of a GeomA tile for this theta (decided from the
// tile-independent maximum extent, the same bound the fast loop fetches), GeomR otherwise.  The grid is sized for the geometry
// with more blocks; the surplus blocks of the other one write a zero partial row and leave.
// WHICH = 0: every body in one kernel (3: only GeomA and GeomR, whatever the mode).  (Removed alternative: the GeomA and GeomR bodies as two
// launches of single-body kernels, bench.py 0.328 ms per step against 0.323 ms for the two-body kernel)
__device__ __forceinline__ bool eft_wants(int choice, const float *__restrict__ th, float fD, float fH, float fW)
{
    if (choice == 2) return true;
    if (choice != 3) return false;
    const float tilt = fabsf(th[8] * fD / fW) + fabsf(th[9] * fD / fH);                 // how far the tile's pre-image leans out of its z planes
    const float zspan = (tilt + fabsf(th[10])) * (float)(ECfg::TZ - 1);
    // (removed alternative, round 4's first rule: zspan > 17 alone - profiles/r05d_eft_offer_rule.txt)
    if (zspan > 17.0f || tilt > 0.07f) return true;
    const float s = fmaxf(fabsf(th[1] * fW / fH), fabsf(th[4] * fH / fW));              // in-plane rotation (its sine, in voxels)
    return s > 0.15f && s < 0.37f;   // GeomRD's rows are at their longest just past GeomD's window (NaN compares false: GeomRD)
}

// The kernel arguments of affine_tile_dual_kernel as one struct: the kernel reads its arguments THROUGH THE KERNARG SEGMENT at the point
// of use (a few scalar loads in front of the body that needs them) instead of through its parameters, which the compiler loads at entry
// and keeps in SGPRs across the dispatch to five inlined bodies: that cost ~60 SGPRs, pushed the bodies' own scalars into VGPR lanes
// and the work-item id into scratch, whose reload (a memory round trip in front of everything) made every launch 5-6 us longer -
// 1 x 64^3: 15.5 -> 10 us per launch (tools/kbench.hip).  Field order and types = the parameter list (same layout rules).
struct DualKArgs {
    trx_volumes vol;
    const float *theta;
    TileGeom tgA, tgR;
    int channels;
    float *partials;
    int zero_surplus;
    TileGeom tgD, tgRD;
    ZGeom zg;
    int *rows_used;
    int rows_stride;
    int eft;
    CarryKArgs carry;
};

template <int MODE, int WHICH = 0>
__global__ __launch_bounds__(512, TRX_DUAL_MIN_WAVES) void affine_tile_dual_kernel(trx_volumes vol_, const float *__restrict__ theta_, TileGeom tgA_,
                                                                                   TileGeom tgR_, int channels_, float *__restrict__ partials_,
                                                                                   int zero_surplus_ = 1, TileGeom tgD_ = TileGeom{}, TileGeom tgRD_ = TileGeom{},
                                                                                   ZGeom zg_ = ZGeom{}, int *__restrict__ rows_used_ = nullptr, int rows_stride_ = 0,
                                                                                   int eft_ = 0, CarryKArgs carry_ = CarryKArgs{})
{
    static_assert(GeomA::Threads == 512 && GeomR::Threads == 512 && GeomD::Threads == 512 && GeomRD::Threads == 512, "every geometry runs 512-thread blocks");
    static_assert(GeomRD::BoxAlloc <= GeomR::BoxAlloc, "GeomRD lives in GeomR's box");
    // the step kernels (MODE 0 / 4) of the one-launch form also carry the deep tile for transforms next to the identity
    // WHICH = 4: the same without the z-streaming body - behind affine_zs_step_kernel, which has taken the pairs next to the identity
    // (removed alternative: the exact-footprint body merged into WHICH = 4 - headline unchanged, rotated poses -5.5 %: profiles/r05a_eft_merged.txt)
    // WHICH = 6: WHICH = 3 (GeomA / GeomR, classic grid) in the CARRY form - the block's prologue finalises the previous iteration of its pair and theta comes from LDS
    constexpr bool kCarry = WHICH == 6;
    static_assert(!kCarry || MODE == 0 || MODE == 4, "the carry form exists for the step kernels");
    constexpr bool kDeep = (WHICH == 0 || WHICH == 4) && (MODE == 0 || MODE == 4);
    constexpr bool kZs = kDeep && WHICH == 0;
    constexpr int kAllocAR = GeomA::BoxAlloc > GeomR::BoxAlloc ? GeomA::BoxAlloc : GeomR::BoxAlloc;
    constexpr int kAllocD = (kDeep && GeomD::BoxAlloc > kAllocAR) ? GeomD::BoxAlloc : kAllocAR;
    constexpr int kAlloc = (kZs && ZS64::Alloc > kAllocD) ? ZS64::Alloc : kAllocD;
    __shared__ __attribute__((aligned(16))) float box[kAlloc];
    constexpr bool kPerChannel = (MODE == 2) || (MODE == 3);
    constexpr int NP = (MODE == 0) ? np_full(3) : (MODE == 2 ? 12 : (MODE == 4 ? kNpMse : 5));
    // a fresh view of the arguments: the empty asm hides the pointer's identity, so loads through it stay where they are written
    typedef const __attribute__((address_space(4))) DualKArgs *KArgs;
    auto args = [&]() {
        KArgs p = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return p;
    };
    typedef const __attribute__((address_space(4))) TileGeom *KTile;
    auto tile_of = [](KTile t) { return TileGeom{t->ntx, t->nty, t->ntz, t->ntiles, t->blocks_per_pair, t->ysplit, t->tiles_per_seg}; };   // (field by field: scalar loads)
    float fD, fH, fW;
    bool with_d, with_rd;
    int zs_planes, rows_stride, nA, nR, nD, nRD, nZ;
    bool with_ef;
    const float *theta;
    {
        KArgs a = args();
        fD = (float)a->vol.D; fH = (float)a->vol.H; fW = (float)a->vol.W;
        nA = a->tgA.blocks_per_pair; nR = a->tgR.blocks_per_pair; nD = a->tgD.blocks_per_pair; nRD = a->tgRD.blocks_per_pair; nZ = a->zg.blocks_per_pair;
        with_d = kDeep && nD > 0; with_rd = kDeep && nRD > 0;
        zs_planes = kZs && nZ > 0 ? a->zg.planes_per_seg : 0;   // (WHICH = 4: the z-streaming test is the kernel's in front - never repeated here, where it could round differently)
        rows_stride = a->rows_stride;
        theta = a->theta;
        with_ef = kDeep && a->rows_used != nullptr && (a->eft != 0 || WHICH == 4);   // pairs with rows_used < 0 belong to a kernel that ran in front
        if constexpr (WHICH == 4) {   // the kernels in front left the number of pairs they did NOT take: none - the usual case next to the identity - and this launch is over
            const int *plan = a->rows_used + a->vol.B;
            if (__builtin_amdgcn_readfirstlane(*plan) == 0) return;
        }
    }
    // 6 = taken by the exact-footprint kernel (affine_eft_step_kernel, launched IN FRONT of this one: it left rows_used[b] = -(its row
    // count) for the pairs it took - rotated pairs that GeomR would run and whose plan fits its buffers): no block here
    // (7 = the exact-footprint body inside this kernel, a removed alternative: its case stays here because the instructions of every instance depend on it)
    auto blocks_of = [&](int choice) { return choice == 6 ? 0 : (choice == 7 ? nRD : (choice == 4 ? nZ : (choice == 0 ? nD : (choice == 3 ? nRD : (choice == 1 ? nA : nR))))); };
    // Work items of this block: (pair / slab `by`, block index v of that pair's geometry).  Classic grid: exactly one, from blockIdx.
    // FLAT grid (rows_stride > 0; the launcher's choice for big batches of the step kernels): gridDim.x persistent blocks share one list
    // of work items - pair 0's blocks, then pair 1's, ... each pair with the block count of the body ITS theta selects - and block p runs
    // items p, p + gridDim.x, ...  Why: a (blocks of the largest geometry) x (pairs) grid makes every pair of a smaller geometry dispatch
    // hundreds of blocks that exit at once, in front of the next pair's working blocks (3584 of them cost the 8 x 256^3 launch 33 us); a
    // per-pair loop over x removes them but runs all pairs side by side on every XCD, and the halo re-reads of the rotated geometries
    // then miss the L2 (GeomR: +28 %).  Pair-major items keep the dispatcher's order: all blocks on one pair, each XCD on its slab of
    // columns (block counts are multiples of 8, so item % 8 is the XCD of v as before).
    const bool flat = kDeep && rows_stride > 0;
    const int wave_idx = trx_wave_index();   // the only use of threadIdx in this kernel
    const int lane = trx_lane_id();
    const int tid_ = wave_idx * 64 + lane;
    // flat path: per pair (lane) the body its theta selects and the inclusive prefix sum of the block counts - kept in LDS, not in
    // registers, across the item loop (two more live VGPRs are two spilled ones in the bodies that sit at the register limit)
    __shared__ int s_choice[64], s_pre[64];
    __shared__ float s_th[16];   // (carry) theta of this block's pair
    if constexpr (kCarry) {
        carry_prologue<MODE>(&args()->carry, (int)blockIdx.y, blockIdx.x == 0, args()->vol.D, args()->vol.H, args()->vol.W, box, s_th, wave_idx, lane);
        theta = s_th - (size_t)blockIdx.y * TRX_PSTRIDE;   // (the choice below indexes by pair; the bodies take s_th itself)
    }
    int my_choice = 2, total = 1;
    if (flat) {
        KArgs a = args();
        const int B = a->vol.B;
        int *rows_used = a->rows_used;
        int cnt = 0, ch = 2;
        if (lane < B) ch = dual_choice(theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW, with_d, with_rd, zs_planes);
        if (with_ef && lane < B && rows_used[lane] < 0) ch = 6;   // taken by the exact-footprint kernel, which ran in front of this one
        if (lane < B) {
            cnt = blocks_of(ch);
            if (rows_used && blockIdx.x == 0 && wave_idx == 0 && ch != 6) rows_used[lane] = ch == 7 ? -rows_note(cnt, 7) : rows_note(cnt, 1 + ch);   // for the step's finalise kernel
        }
        int pre = cnt;   // inclusive prefix sum over the lanes (pairs)
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(pre, d, 64);
            if (lane >= d) pre += t;
        }
        total = __builtin_amdgcn_readlane(pre, 63);
        if (wave_idx == 0) { s_choice[lane] = ch; s_pre[lane] = pre; }
        __syncthreads();
    } else {
        KArgs a = args();
        const int channels = a->channels;
        const int b = kPerChannel ? blockIdx.y / channels : blockIdx.y;
        my_choice = __builtin_amdgcn_readfirstlane(dual_choice(theta + (size_t)b * TRX_PSTRIDE, fD, fH, fW, with_d, with_rd, zs_planes));
        if (with_ef && a->rows_used[b] < 0) my_choice = 6;   // taken by the exact-footprint kernel, which ran in front of this one
        const int mine = blocks_of(my_choice);
        // zero_surplus = 0: surplus blocks write nothing; the reader (the step's finalise kernel) learns the pair's row count from
        // rows_used[], written here by the pair's first block - it does not repeat the choice (two inlined copies of a float test could
        // disagree by an ulp)
        int *rows_used = a->rows_used;
        if (rows_used && blockIdx.x == 0 && tid_ == 0 && my_choice != 6) rows_used[blockIdx.y] = rows_note(mine, 1 + my_choice);
        if ((int)blockIdx.x >= mine) {
            if (MODE != 3 && a->zero_surplus && tid_ < NP) a->partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NP + tid_] = 0.f;
            return;
        }
    }
    total = __builtin_amdgcn_readfirstlane(total);
    const int it0 = flat ? (int)blockIdx.x : 0, it_step = flat ? (int)gridDim.x : 1;
    for (int item = __builtin_amdgcn_readfirstlane(it0); item < total; item += it_step) {
        int choice, v, by, stride;
        if (flat) {
            const int pre = *(volatile int *)&s_pre[lane];
            // (round 5) odd iterations of a run (TRX_FLAG_WALK_DOWN) take the list backwards, in groups of 8 (item % 8 stays the XCD): they start on the pairs the Infinity Cache still holds
            const int it = (WHICH == 4 && (args()->vol.flags & TRX_FLAG_WALK_DOWN) && (total & 7) == 0) ? total - 8 - (item & ~7) + (item & 7) : item;
            const int pair = __builtin_amdgcn_readfirstlane(__builtin_popcountll(__builtin_amdgcn_ballot_w64(pre <= it)));   // lanes >= B hold the total: never counted
            const int off = pair > 0 ? __builtin_amdgcn_readlane(pre, pair - 1) : 0;
            choice = *(volatile int *)&s_choice[pair];
            v = __builtin_amdgcn_readfirstlane(it - off); by = pair; stride = rows_stride;
            if (item != it0) __syncthreads();   // the previous body's reduction scratch aliases the box
        } else {
            choice = __builtin_amdgcn_readfirstlane(my_choice); v = blockIdx.x; by = blockIdx.y; stride = gridDim.x;   // (my_choice is per-lane on the flat path: keep this one provably uniform)
        }
        choice = __builtin_amdgcn_readfirstlane(choice); v = __builtin_amdgcn_readfirstlane(v);   // all four ARE wave-uniform; say so to the
        by = __builtin_amdgcn_readfirstlane(by); stride = __builtin_amdgcn_readfirstlane(stride);  // compiler (the bodies pin them to SGPRs)
        KArgs a = args();   // this item's view of the arguments: the volumes and ONE geometry
        const trx_volumes vol = {a->vol.moving, a->vol.target, a->vol.moving_stride, a->vol.target_stride, a->vol.ndim, a->vol.B, a->vol.D, a->vol.H, a->vol.W,
                                 a->vol.xn, a->vol.yn, a->vol.zn, a->vol.flags};
        float *partials = a->partials;
        const int channels = a->channels;
        if constexpr (kZs) {
            if (choice == 4) {
                const ZGeom zg = {a->zg.ntx, a->zg.nty, a->zg.nzseg, a->zg.planes_per_seg, a->zg.blocks_per_pair};
                zstream_body<MODE, ZS64>(vol, theta, zg, partials, box, v, by, stride, wave_idx,
                                         (int)((blockIdx.y * gridDim.x + blockIdx.x) * 2 >= gridDim.x * gridDim.y));   // (second half of the grid = the later block of its CU)
                continue;
            }
        }
        if constexpr (kDeep) {
            if (choice == 0) {
                const TileGeom t = tile_of(&a->tgD);
                tile_body<MODE, GeomD>(vol, theta, t, channels, partials, box, v, by, stride, wave_idx);
                continue;
            }
            if (choice == 3) {
                const TileGeom t = tile_of(&a->tgRD);
                tile_body<MODE, GeomRD>(vol, theta, t, channels, partials, box, v, by, stride, wave_idx);
                continue;
            }
        }
        if (choice != 1) {
            const TileGeom t = tile_of(&a->tgR);
            if constexpr (kCarry) tile_body<MODE, GeomR, true>(vol, s_th, t, channels, partials, box, v, by, stride, wave_idx);
            else tile_body<MODE, GeomR>(vol, theta, t, channels, partials, box, v, by, stride, wave_idx);
            continue;
        }
        const TileGeom t = tile_of(&a->tgA);
        if constexpr (kCarry) tile_body<MODE, GeomA, true>(vol, s_th, t, channels, partials, box, v, by, stride, wave_idx);
        else tile_body<MODE, GeomA>(vol, theta, t, channels, partials, box, v, by, stride, wave_idx);
    }
}

// The exact-footprint kernel of a step, launched IN FRONT of affine_tile_dual_kernel.  It decides which pairs are its own - those that
// kernel would give to GeomR or (eft_wants) GeomRD (dual_choice, same arguments) and whose plan fits its buffers (counted exactly, one pair per wave) - leaves
// rows_used[b] = -(partial rows it writes) for them and 0 for the others (the step kernel behind it skips the negative ones; so does the
// finalise kernel's reading of the count: |rows_used|), and runs them.  Why a kernel of its own: inlined into affine_tile_dual_kernel as a
// sixth body - or called from it, or with only this decision in its prologue - it changed the code the compiler makes of the z-streaming
// loop (a reload and a vmcnt(0) per step): the headline lost 7-12 % (profiles/r04c_eft_placement_ab.txt).
// stride > 0: FLAT grid of persistent blocks over the pair-major list of those pairs' blocks (partial rows of stride `stride` per pair);
// stride < 0: block (x, pair) of a (blocks_per_pair, pairs) grid, rows of stride -stride.  No pair of its own: every block leaves at once.
// Which of the fused kernel's choices this kernel takes over: GeomR's pairs (2) always; GeomRD's (3) when the tile's pre-image leans out of its z
// planes (zspan > 17 source planes per 16^3 tile, or a tilt of more than 0.07 voxels per voxel: GeomRD's rows get long), or when the in-plane rotation
// lies between the end of GeomD's window and a sine of 0.37 - pure rotations about z beyond that stay with GeomRD.  Measured, 8 x 256^3, us per
// pair-iteration, GeomRD -> this kernel: R_x(0.6) 63.7 -> 47.6, R(.3,.3,.3) 63.8 -> 53.3, R_z(0.25) 54.3 -> 48.6, R(.1,0,.3) 55.5 -> 48.1, but
// R_z(0.6) 50.3 -> 54.5, R_z(1.0) 50.7 -> 56.2 (profiles/r04g_rotation_sweep.txt, profiles/r04h_eft_offer_rule.txt).
// The z-streaming body as a kernel of its OWN for launches that fill the chip (flat grid), IN FRONT of the exact-footprint kernel and the
// tile kernel (round 5).  Inside affine_tile_dual_kernel its loop shared the register allocation of four other bodies: the same source
// measured 253-262 us stand-alone and 261-318 us fused, by which way the allocator fell (profiles/r05a_zstream_fused_vs_alone.txt).  This
// kernel takes every pair whose theta passes zs_nsub - the ONLY place that test is evaluated for such a launch -, leaves
// rows_used[b] = -(its rows) for them and 0 for the rest, the number of pairs it did NOT take in rows_used[B] and the bit mask of those it
// took in rows_used[B + 1, B + 2]: the two kernels behind it return at once when the count is zero (a launch boundary each, ~1.5 us), and
// otherwise skip the pairs of the mask.
// The z-streaming kernel also carries the FLAT tile (ZSF: 64 x 16 voxels per plane, ring of 8 planes of 80 x 30) for pairs the 64 x 32 tile
// does not take: poses of the convergence basin (rotations up to ~0.15 rad about z, zooms to 1.15, 3.7 planes of tilt) run 10-11 %
// faster on it than on the deep tile kernel (profiles/r05a_zs_flat_tile.txt).
// FB (round 6): the ONE-KERNEL form of a step (TRX_FLAG_ONE_KERNEL) - nothing is launched behind this kernel, so the pairs its two streaming tiles do
// not take run HERE, on GeomR's body (the tile whose box holds the pre-image under any rotation; 78.6 KB, inside the ring's allocation): a pair that
// leaves the window costs ~2 x its usual time for as long as it stays outside, instead of two launches that find nothing to do on every step of every
// run: 3.2-3.5 us per step, measured (profiles/r06a_one_kernel_ab.txt; their traced durations, 5.3 + 4.8 us, overstate it).  FB = 0 is the kernel of
// round 5: the FB code is compiled out of it (same instructions: tools/isa_loops.py).
struct ZsOneKArgs {   // the kernel arguments of affine_zs_one_kernel as one struct (field order and types = its parameter list)
    trx_volumes vol;
    const float *theta;
    ZGeom zg, zgf;
    float *partials;
    int *rows_used;
    int stride;
    TileGeom tgR;
};
template <int MODE, int FB>
__device__ __forceinline__ void zs_step_main(const trx_volumes &vol, const float *__restrict__ theta, const ZGeom &zg, const ZGeom &zgf, float *__restrict__ partials,
                                             int *__restrict__ rows_used, int stride, const int fb_blocks, float *ring)
{
    const int wave = trx_wave_index(), lane = trx_lane_id();
    const float fD = (float)vol.D, fH = (float)vol.H, fW = (float)vol.W;
    // per pair (lane): 1 = the 64 x 32 tile takes it, 2 = the flat tile does, 0 = left to the kernels behind (FB: 3 = GeomR's body, here)
    int which = 0;
    if (lane < vol.B) {
        if (zs_nsub<ZS64>(theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW, zg.planes_per_seg) > 0) which = 1;
        else if (zgf.blocks_per_pair > 0 && zs_nsub<ZSF>(theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW, zgf.planes_per_seg) > 0) which = 2;
        else if (FB) which = 3;
    }
    const unsigned long long take = __builtin_amdgcn_ballot_w64(which != 0), take1 = __builtin_amdgcn_ballot_w64(which == 1);
    const int mine = which == 1 ? zg.blocks_per_pair : (which == 2 ? zgf.blocks_per_pair : ((FB && which == 3) ? fb_blocks : 0));
    if (blockIdx.x == 0 && wave == 0) {
        if (lane < vol.B) rows_used[lane] = -rows_note(mine, which == 3 ? 3 : (which == 2 ? 8 : 6));
        if (lane == 0) {
            rows_used[vol.B] = vol.B - __builtin_popcountll(take);
            rows_used[vol.B + 1] = (int)(unsigned)take; rows_used[vol.B + 2] = (int)(unsigned)(take >> 32);   // which pairs: nobody rewrites this
        }
        if (lane < 8) rows_used[vol.B + 3 + lane] = 0;   // work tickets of the exact-footprint kernel behind this one (one queue per XCD)
    }
    if (take == 0) return;
    int pre = mine;   // inclusive prefix sum over the lanes (pairs)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(pre, d, 64);
        if (lane >= d) pre += t;
    }
    const int total = __builtin_amdgcn_readlane(pre, 63);
    const int second = (int)(blockIdx.x * 2 >= gridDim.x);   // the later of the two blocks of a CU (zstream_body's fair sharing)
    if constexpr (FB != 0) {
        // the pair's body rides in the low two bits of its prefix sum: the masks of the FB = 0 form (two scalar-register pairs, live across the streaming
        // loops, which have none to spare) would be three here
        const int prew = (pre << 2) | which;
        for (int item = blockIdx.x; item < total; item += gridDim.x) {
            const int pair = __builtin_amdgcn_readfirstlane(__builtin_popcountll(__builtin_amdgcn_ballot_w64((prew >> 2) <= item)));
            const int off = pair > 0 ? (__builtin_amdgcn_readlane(prew, pair - 1) >> 2) : 0;
            const int w = __builtin_amdgcn_readlane(prew, pair) & 3;
            const int v = __builtin_amdgcn_readfirstlane(item - off);
            if (item != (int)blockIdx.x) __syncthreads();   // the previous item's reduction scratch aliases the ring
            if (__builtin_expect(w == 3, 0)) {
                // (the tile geometry is read through the kernarg segment HERE, as affine_tile_dual_kernel reads its arguments: loaded at the kernel's entry
                // its seven scalars stay live across the streaming loops.  Inlined: as a function of its own - __noinline__, arguments through the kernarg
                // segment - the call's register conventions cost the streaming loops 25 more scalar reloads per two planes than the inlined body's 2)
                typedef const __attribute__((address_space(4))) ZsOneKArgs *KArgs;
                KArgs a = (KArgs)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(a));
                const TileGeom t = {a->tgR.ntx, a->tgR.nty, a->tgR.ntz, a->tgR.ntiles, a->tgR.blocks_per_pair, a->tgR.ysplit, a->tgR.tiles_per_seg};
                tile_body<MODE, GeomR>(vol, theta, t, 1, partials, ring, v, pair, stride, wave);
            } else if (w == 1) zstream_body<MODE, ZS64>(vol, theta, zg, partials, ring, v, pair, stride, wave, second);
            else zstream_body<MODE, ZSF>(vol, theta, zgf, partials, ring, v, pair, stride, wave, second);
        }
        return;
    }
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int pair = __builtin_amdgcn_readfirstlane(__builtin_popcountll(__builtin_amdgcn_ballot_w64(pre <= item)));
        const int off = pair > 0 ? __builtin_amdgcn_readlane(pre, pair - 1) : 0;
        const int v = __builtin_amdgcn_readfirstlane(item - off);
        if (item != (int)blockIdx.x) __syncthreads();   // the previous item's reduction scratch aliases the ring
        if ((take1 >> pair) & 1ull) zstream_body<MODE, ZS64>(vol, theta, zg, partials, ring, v, pair, stride, wave, second);
        else zstream_body<MODE, ZSF>(vol, theta, zgf, partials, ring, v, pair, stride, wave, second);
    }
}

template <int MODE>
__global__ __launch_bounds__(ZS64::Threads, TRX_ZS_MIN_WAVES) void affine_zs_step_kernel(trx_volumes vol, const float *__restrict__ theta, ZGeom zg, ZGeom zgf, float *__restrict__ partials,
                                                                                         int *__restrict__ rows_used, int stride)
{
    constexpr int kAlloc = ZSF::Alloc > ZS64::Alloc ? ZSF::Alloc : ZS64::Alloc;
    __shared__ __attribute__((aligned(16))) float ring[kAlloc];
    zs_step_main<MODE, 0>(vol, theta, zg, zgf, partials, rows_used, stride, 0, ring);
}

template <int MODE>
__global__ __launch_bounds__(ZS64::Threads, TRX_ZS_MIN_WAVES) void affine_zs_one_kernel(trx_volumes vol, const float *__restrict__ theta, ZGeom zg, ZGeom zgf, float *__restrict__ partials,
                                                                                        int *__restrict__ rows_used, int stride, TileGeom tgR)
{
    constexpr int kAllocZ = ZSF::Alloc > ZS64::Alloc ? ZSF::Alloc : ZS64::Alloc;
    constexpr int kAlloc = GeomR::BoxAlloc > kAllocZ ? GeomR::BoxAlloc : kAllocZ;
    __shared__ __attribute__((aligned(16))) float ring[kAlloc];
    zs_step_main<MODE, 1>(vol, theta, zg, zgf, partials, rows_used, stride, tgR.blocks_per_pair, ring);
}

template <int MODE>
__global__ __launch_bounds__(ECfg::Threads, 4) void affine_eft_step_kernel(trx_volumes vol, const float *__restrict__ theta, TileGeom tg, float *__restrict__ partials,
                                                                           int *__restrict__ rows_used, int stride, int with_d, int with_rd, int zs_planes_)
{
    const bool zs_first = zs_planes_ < 0;   // (flat launches behind affine_zs_step_kernel: the z-streaming test is not repeated here)
    const int zs_planes = zs_first ? 0 : zs_planes_;
    __shared__ __attribute__((aligned(16))) float lds[ECfg::Alloc];
    __shared__ int s_ef[64];
    const int wave = trx_wave_index(), lane = trx_lane_id();
    const float fD = (float)vol.D, fH = (float)vol.H, fW = (float)vol.W;
    if (stride < 0) {   // (small launches: the body is offered by TRX_FLAG_EFT only)
        if ((int)blockIdx.x >= tg.blocks_per_pair) return;
        const int b = blockIdx.y;
        const float *th = theta + (size_t)b * TRX_PSTRIDE;
        bool take = __builtin_amdgcn_readfirstlane((int)eft_wants(dual_choice(th, fD, fH, fW, with_d != 0, with_rd != 0, zs_planes), th, fD, fH, fW)) &&
                    __builtin_amdgcn_readfirstlane((int)ef_candidate(th, fD, fH, fW));
        if (take) {   // (block-uniform) the plan's granules, counted by the whole block: two rows per thread
            const EfMap m = ef_map(th, fD, fH, fW);
            const EfDims d = ef_dims(m);
            int cnt = 0;
#pragma unroll
            for (int h = 0; h < (ECfg::NY * ECfg::NZ) / ECfg::Threads; h++) {
                const int r = wave * 64 + lane + h * ECfg::Threads, iy = r & (ECfg::NY - 1), iz = r >> 5;
                int wlo;
                if (iy < d.ny && iz < d.nz) cnt += ef_row_window(m, d.dy0 + iy, d.dz0 + iz, wlo);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0) s_ef[wave] = cnt;
            __syncthreads();
            int g = 0;
#pragma unroll
            for (int w = 0; w < ECfg::Waves; w++) g += s_ef[w];
            g = __builtin_amdgcn_readfirstlane(g);
            take = d.ok && g > 0 && g <= ECfg::GCap;
            __syncthreads();   // s_ef is not touched again, but the body's prologue reuses LDS right away: keep the phases apart
        }
        if (blockIdx.x == 0 && wave == 0 && lane == 0) rows_used[b] = take ? -rows_note(tg.blocks_per_pair, 7) : 0;
        if (!take) return;
    }
    // ONE call site of the body for both grids (as in affine_tile_dual_kernel): with a second inlined copy behind the classic grid's branch the
    // compiler produced a kernel whose classic-grid launches faulted as soon as round 5 touched the flat branch (tools/repro_eft2.py)
    const bool flat = stride >= 0;
#if TRX_EF_STAMP
    if (flat && wave == 0 && lane == 0) { for (int k = 1; k < 8; k++) trx_ef_blocks[blockIdx.x * 8 + k] = 0; trx_ef_blocks[blockIdx.x * 8] = __builtin_amdgcn_s_memrealtime(); }
#endif
    int pre = 0, total = 1;
    if (flat) {
    // flat: per pair (lane) the decision, one candidate pair per wave and round
    // zs_first: affine_zs_step_kernel ran in front - no pair left (rows_used[B] = 0): done; else its pairs are those of the mask in rows_used[B + 1, B + 2]
    if (zs_first && __builtin_amdgcn_readfirstlane(rows_used[vol.B]) == 0) return;
    unsigned long long zs_mask = 0;   // pairs of the kernel in front (its mask is not rewritten by anybody: block 0 of THIS kernel rewrites rows_used[b] of the free pairs)
    if (zs_first) zs_mask = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(rows_used[vol.B + 1]) | ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(rows_used[vol.B + 2]) << 32);
    const bool free_l = lane < vol.B && !((zs_mask >> lane) & 1ull);
    const bool cand_l = free_l && eft_wants(dual_choice(theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW, with_d != 0, with_rd != 0, zs_planes),
                                                  theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW) &&
                        ef_candidate(theta + (size_t)lane * TRX_PSTRIDE, fD, fH, fW);
    const unsigned long long cand = __builtin_amdgcn_ballot_w64(cand_l);
    unsigned long long fit = 0;
    if (cand) {
        if (wave == 0) s_ef[lane] = 0;
        __syncthreads();
        unsigned long long rest = cand;
        for (int k = 0; rest; k++) {
            const int pb = __builtin_ctzll(rest);
            rest &= rest - 1;
            if ((k & (ECfg::Waves - 1)) != wave) continue;
            const EfMap m = ef_map(theta + (size_t)pb * TRX_PSTRIDE, fD, fH, fW);
            const EfDims d = ef_dims(m);
            const int g = ef_plan_granules_wave(m, d, lane);
            if (lane == 0) s_ef[pb] = (d.ok && g > 0 && g <= ECfg::GCap) ? 1 : 0;
        }
        __syncthreads();
        fit = __builtin_amdgcn_ballot_w64(s_ef[lane] != 0) & cand;
    }
    const int mine = ((fit >> lane) & 1ull) ? tg.blocks_per_pair : 0;
    if (blockIdx.x == 0 && wave == 0 && free_l) rows_used[lane] = -rows_note(mine, 7);
    if (fit == 0) return;
    pre = mine;   // inclusive prefix sum over the lanes (pairs)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(pre, d, 64);
        if (lane >= d) pre += t;
    }
    total = __builtin_amdgcn_readlane(pre, 63);
    }
    total = __builtin_amdgcn_readfirstlane(total);
    const int rows_stride = __builtin_amdgcn_readfirstlane(flat ? stride : -stride);
    // A block's items (pair-major index blockIdx + k gridDim) would be the SAME column in pair after pair - and columns differ widely in
    // cost (those that leave the source volume early are cheap): the column index is rotated per pair (by a multiple of 8: blocks b, b + 8,
    // ... still share an XCD's L2 with the neighbouring columns), which evens the blocks' loads without any shared counter.
    // Tickets (round 5): behind affine_zs_step_kernel (which zeroes them) the flat grid's blocks DRAW their items - items cost 43 k ... 345 k ticks, and
    // with every gridDim-th item a launch waited 460 us for blocks whose median finished at 349 (profiles/r05c_eft_item_timeline.txt).  One queue per XCD
    // (block b draws from queue b & 7: the columns v = b & 7 (mod 8) of every pair, pair-major - the slab of its XCD's L2, as before); a block's first item is the
    // one it had (no draw), the ticket of the next item is drawn when the current one is done.  Removed alternatives (same profile): the ticket drawn at
    // the START of an item (every block then holds an item nobody else can take: worse), and a block's items CONSECUTIVE - one plan per block - 12 % slower.
    const bool tickets = flat && zs_first && (tg.blocks_per_pair & 7) == 0 && (gridDim.x & 7) == 0 && (total % tg.blocks_per_pair) == 0;
    const int it0 = flat ? (int)blockIdx.x : 0, it_step = flat ? (int)gridDim.x : 1;
    const int it_end = flat ? total : 1;
    EfPlanRegs pr;
    int planned = -1;   // the pair the registers and the row table in LDS belong to
    int q = blockIdx.x & 7;                                                                   // (tickets) the queue the current item came from: this block's XCD's, at the end any
    const int qlen = total >> 3, per_pair_q = tg.blocks_per_pair >> 3;                        // (tickets) a queue's length, a pair's items in it
    int qk = (int)blockIdx.x >> 3;                                                            // (tickets) position in the queue of the current item
    for (int item = __builtin_amdgcn_readfirstlane(it0); tickets ? (qk < qlen) : (item < it_end); item += it_step) {
        int v = blockIdx.x, pair = blockIdx.y;   // classic grid: the one item of this block
        if (flat) {
            if (tickets) {
                // (order of a queue: pair-major.  The pairs' inner columns first and their columns on a face of the volume - the cheap items - last was measured
                // worse, 429 against 408 us: profiles/r05c_eft_item_timeline.txt)
                int ord = qk / per_pair_q;                                    // the ord-th pair of those that fit ...
                const int j = qk - ord * per_pair_q;                          // ... position in the XCD's slab
                if (vol.flags & TRX_FLAG_WALK_DOWN) ord = total / tg.blocks_per_pair - 1 - ord;   // odd iterations of a run take the pairs in the opposite order: they start on what the Infinity Cache still holds
                pair = __builtin_popcountll(__builtin_amdgcn_ballot_w64(pre <= ord * tg.blocks_per_pair));
                v = q + 8 * j;
            } else {
                pair = __builtin_popcountll(__builtin_amdgcn_ballot_w64(pre <= item));
                const int off = pair > 0 ? __builtin_amdgcn_readlane(pre, pair - 1) : 0;
                v = (item - off + 104 * pair) % tg.blocks_per_pair;
            }
        }
        v = __builtin_amdgcn_readfirstlane(v); pair = __builtin_amdgcn_readfirstlane(pair);
        if (item != it0) __syncthreads();   // the previous item's reduction scratch aliases the buffers
        eft_body<MODE>(vol, theta, tg, partials, lds, v, pair, rows_stride, wave, pr, pair != planned);
        planned = pair;
#if TRX_EF_STAMP
        if (flat && wave == 0 && lane == 0) { trx_ef_blocks[blockIdx.x * 8 + 1 + min((item - it0) / it_step, 5)] = __builtin_amdgcn_s_memrealtime(); }
#endif
        if (tickets) {   // the next item: a ticket, counted behind the (gridDim / 8) items the queue's blocks started with
            if (wave == 0 && lane == 0) {
                const int first = (int)gridDim.x >> 3;
                int nq = blockIdx.x & 7, k = qlen;
                for (int t = 0; t < 8 && k >= qlen; t++) {   // own queue first; when it is empty the others in turn (the XCDs' slabs differ in cost: edge slabs leave the source volume early)
                    nq = ((int)blockIdx.x + t) & 7;
                    k = __hip_atomic_fetch_add(rows_used + vol.B + 3 + nq, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + first;
                }
                s_ef[63] = k < qlen ? ((nq << 24) | k) : -1;
            }
            __syncthreads();
            const int nx = __builtin_amdgcn_readfirstlane(s_ef[63]);
            if (nx < 0) break;
            q = nx >> 24; qk = nx & 0xffffff;
        }
    }
}

#pragma clang diagnostic pop

// closed-form base coordinates for callers that pass no tables: (2i+1)/S - 1
__global__ void fill_tables_kernel(float *__restrict__ tab, int W, int H, int D)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W) tab[i] = (float)(2 * i + 1) / (float)W - 1.0f;
    if (i < H) tab[W + i] = (float)(2 * i + 1) / (float)H - 1.0f;
    if (i < D) tab[W + H + i] = (float)(2 * i + 1) / (float)D - 1.0f;
}

// ------------------------------------------------------------------------------------------
// Finalise: reduce the per-block partials in fp64, then (MODE 0) loss, gradient, optimiser and
// best tracking for one pair; one 1024-thread block per pair.
// ------------------------------------------------------------------------------------------
// state_in != nullptr: the pair's state is read from a carry buffer (the flush behind the last one-launch iteration of a run) instead of the caller's arrays
template <int ND>
__global__ __launch_bounds__(TRX_FIN_THREADS) void affine_finalize_kernel(const float *__restrict__ partials, int nblk,
                                                                          double nvox, int D, int H, int W,
                                                                          trx_loss_cfg lc, trx_opt_cfg oc,
                                                                          trx_affine_state st, const int *__restrict__ rows_used = nullptr, int mse_rows = 0,
                                                                          const float *__restrict__ state_in = nullptr)
{
    constexpr int NP = np_full(ND);
    constexpr int NT = ND * (ND + 1);
    constexpr int NPOSE = (ND == 3) ? 6 : 3;
    __shared__ double S[64];
    const int b = blockIdx.x;
    // Lane-parallel epilogue: lane i owns parameter i.  Every load of the per-pair state is issued up front
    // by all lanes at once (ONE memory round trip; a single thread looping over the 12 parameters paid a
    // dependent load->store chain per parameter, ~20 us) and BEFORE the partial rows, so that the state and the rows share
    // one wait; the scalar fp64 math is computed redundantly.
    __shared__ double sh_dth[NT];
    __shared__ float sh_pose[NPOSE];
    const int i = threadIdx.x;
    const bool rigid = st.mode == TRX_PARAM_RIGID;
    float *param = st.param + (size_t)b * TRX_PSTRIDE;
    float *theta = st.theta + (size_t)b * TRX_PSTRIDE;
    FinRegs<ND> r;
    if (i < 64) {
        if (state_in) {
            const float *sb = state_in + (size_t)b * kCarryStride;
            r = fin_load<ND>(sb + kCarryParam, sb + kCarryTheta, sb + kCarryM, sb + kCarryV, reinterpret_cast<const int *>(sb + kCarryStep), st.best_loss + b,
                             oc.kind == TRX_OPT_ADAM, rigid, i);
        } else {
            r = fin_load<ND>(param, theta, st.adam_m ? st.adam_m + (size_t)b * TRX_PSTRIDE : nullptr, st.adam_v ? st.adam_v + (size_t)b * TRX_PSTRIDE : nullptr, st.step + b,
                             st.best_loss + b, oc.kind == TRX_OPT_ADAM, rigid, i);
        }
    }
    {
        // rows the F1 pass wrote for this pair: the dual kernel lays a pair's rows out with stride nblk and fills the first
        // blocks_per_pair of the geometry it chose for the pair - it left that count in rows_used[b]
        int rows = nblk;
        if (rows_used) rows = min(abs(rows_used[b]) & kRowsMask, nblk);   // (negative: the pair was left to the exact-footprint kernel, which wrote |rows_used| rows)
        if (ND == 3 && mse_rows) reduce_partials<kNpMse>(partials + (size_t)b * nblk * kNpMse, rows, S);   // rows of the MSE / SSD-only step kernel
        else reduce_partials<NP>(partials + (size_t)b * nblk * NP, rows, S);
    }
    if (i >= 64) return;
    fin_apply<ND>(S, r, b, i, nvox, D, H, W, lc, oc, st, mse_rows, param, theta, st.adam_m ? st.adam_m + (size_t)b * TRX_PSTRIDE : nullptr,
                  st.adam_v ? st.adam_v + (size_t)b * TRX_PSTRIDE : nullptr, st.step + b, true, nullptr, sh_dth, sh_pose);
}

// ------------------------------------------------------------------------------------------
// Forward warp (Register.__call__): one thread per output voxel, channels share coordinates.
// ------------------------------------------------------------------------------------------
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void affine_warp_kernel(trx_volumes vol, const float *__restrict__ theta,
                                                                int channels, size_t chan_stride,
                                                                float *__restrict__ out)
{
    const int b = blockIdx.y;
    const int D = vol.D, H = vol.H, W = vol.W;
    const size_t nvox = (size_t)D * H * W;
    const float *__restrict__ th = theta + (size_t)b * TRX_PSTRIDE;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    float *__restrict__ o = out + (size_t)b * channels * nvox;
    const float fW = (float)W, fH = (float)H, fD = (float)D;
    for (VoxelWalk vw(blockIdx.x * TRX_BLOCK + threadIdx.x, gridDim.x * TRX_BLOCK, H, W); vw.i < nvox; vw.next(H, W)) {
        const size_t i = vw.i;
        const int x = vw.x, y = vw.y, z = vw.z;
        const float xn = base_coord(vol.xn, x, W), yn = base_coord(vol.yn, y, H);
        if constexpr (ND == 3) {
            const float zn = base_coord(vol.zn, z, D);
            const float ix = unnorm<3>(fmaf(th[1], yn, fmaf(th[0], xn, fmaf(th[2], zn, th[3]))), fW);
            const float iy = unnorm<3>(fmaf(th[5], yn, fmaf(th[4], xn, fmaf(th[6], zn, th[7]))), fH);
            const float iz = unnorm<3>(fmaf(th[9], yn, fmaf(th[8], xn, fmaf(th[10], zn, th[11]))), fD);
            for (int ch = 0; ch < channels; ch++) o[ch * nvox + i] = sample3(mov + ch * chan_stride, D, H, W, ix, iy, iz).v;
        } else {
            const float ix = unnorm<2>(fmaf(th[1], yn, fmaf(th[0], xn, th[2])), fW);
            const float iy = unnorm<2>(fmaf(th[4], yn, fmaf(th[3], xn, th[5])), fH);
            for (int ch = 0; ch < channels; ch++) o[ch * nvox + i] = sample2(mov + ch * chan_stride, H, W, ix, iy).v;
        }
    }
}

int check_vol(const trx_volumes *v, bool need_target)
{
    if (!v || !v->moving || (need_target && !v->target)) return TRX_ERR_ARG;
    if (v->ndim != 2 && v->ndim != 3) return TRX_ERR_NDIM;
    if (v->B < 1 || v->D < 1 || v->H < 1 || v->W < 1) return TRX_ERR_ARG;
    if (v->ndim == 2 && v->D != 1) return TRX_ERR_NDIM;
    if (v->B > 65535) return TRX_ERR_ARG;
    if ((size_t)v->D * v->H * v->W >= ((size_t)1 << 31)) return TRX_ERR_ARG;   // 32-bit voxel indices inside one volume
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

// false: the single-geometry kernel only (TRX_FLAG_SINGLE_GEOM); true: GeomA / GeomR (and the step kernels' extra bodies) chosen per pair
static bool use_dual(const trx_volumes *vol) { return !(vol->flags & TRX_FLAG_SINGLE_GEOM); }

// Block slots of the device for the 512-thread step kernels: two per CU (LDS and registers allow exactly two) - 512 on MI355X (256 CUs).
// The size of the flat grid and the yardstick of the offer rules in f1_plan; queried once per launch (the runtime caches device attributes).
static int persistent_blocks()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        return TRX_PERSISTENT_BLOCKS;
    return 2 * cus;
}

// What a launch of the 3-D dual path consists of, decided from sizes and flags alone (f1_plan): launch_f1 launches what it says, the workspace
// is sized from the same list of geometries, and trx_affine_near_identity asks it which z-streaming tiles a step offers.
enum DualInstance { kTwoBody = 3, kFiveBody = 0, kBehindZs = 4, kCarry = 6 };   // (the values are affine_tile_dual_kernel's WHICH)
template <int W> struct Which { static constexpr int value = W; };
struct F1Plan {
    TileGeom ta, tr, td, trd, tef;   // the geometries offered to the pairs; blocks_per_pair == 0: not offered (tef: the exact-footprint kernel's 16^3 tiling - GeomRD's)
    ZGeom zg, zgf;                   // ... the z-streaming body's 64 x 32 tile and its flat tile
    int rows, slots;                 // partial rows per pair: the row stride the kernels and the finalise get (nblk); block slots of the device = the flat grid
    bool flat;                       // a flat grid of persistent blocks over a pair-major work list (else the classic grid rows x pairs)
    bool zs_first, one_kernel;       // the z-streaming body runs as a kernel of its own in front (affine_zs_step_kernel); ... and alone (affine_zs_one_kernel)
    int eft;                         // the exact-footprint kernel runs in front of the tile kernel: its partial rows per pair (0: it does not)
    DualInstance dual;               // the instance of affine_tile_dual_kernel that runs behind them
};

// Every geometry a launch may choose from.  The ONE list: the workspace reserves rows for all of them, a plan offers a subset.
static F1Plan f1_candidates(const trx_volumes &v)
{
    F1Plan p = F1Plan{};
    p.ta = tile_geom<GeomA>(v); p.tr = tile_geom<GeomR>(v); p.td = tile_geom<GeomD>(v); p.trd = p.tef = tile_geom<GeomRD>(v);
    if (zs_shape_ok<ZS64>(v)) p.zg = zs_geom<ZS64>(v);
    if (zs_shape_ok<ZSF>(v)) p.zgf = zs_geom<ZSF>(v);
    return p;
}

// partial rows per pair that a launch of these geometries may write (the grid is sized for the geometry with the most blocks)
static int f1_rows(const F1Plan &p)
{
    return max(max(max(p.ta.blocks_per_pair, p.tr.blocks_per_pair), max(p.td.blocks_per_pair, p.trd.blocks_per_pair)),
               max(p.tef.blocks_per_pair, max(p.zg.blocks_per_pair, p.zgf.blocks_per_pair)));
}

// The plan of one launch.  No HIP call, nothing launched.  slots: persistent_blocks().  step: a step kernel (MODE 0 / 4) whose reader knows which
// rows were written (the step's finalise kernel reads the row count of every pair from rows_used) - every other launch is GeomA / GeomR on the
// classic grid.  carry: trx_affine_run asks for the carry form.
static F1Plan f1_plan(const trx_volumes &v, int slots, bool step, bool carry)
{
    if (!step) {
        F1Plan p = F1Plan{tile_geom<GeomA>(v), tile_geom<GeomR>(v)};
        p.rows = f1_rows(p); p.dual = kTwoBody;
        return p;
    }
    F1Plan p = f1_candidates(v);
    p.slots = slots;
    // the deep tile joins the choice only where the reader of the partial rows knows which rows were written (the step's finalise
    // kernel) and where its 128-row slabs still fill the chip (8192 voxels per tile: big batches)
    // big batches as before; smaller ones where the deep tiling still fills every block slot with blocks of at least four tiles
    // (1 or 2 pairs of 256^3: -3 %; never where it would leave slots empty - 2 x 128^3 measured +29 % with it)
    const long blocks_d = (long)p.td.blocks_per_pair * v.B, slots_d = slots;   // block slots of these 512-thread kernels (MI355X: 512) - the same number the flat grid and the z-streaming / exact-footprint rules use
    const long rem_d = blocks_d % slots_d;  // a last round that is less than ~60 % full costs more than the deeper tile saves (6 x 256^3: +6 %)
    const bool small_ok = blocks_d >= slots_d && p.td.tiles_per_seg >= 4 && (rem_d == 0 || rem_d >= slots_d * 5 / 8);
    if (!(blocks_d >= 2 * slots_d || small_ok || (v.flags & TRX_FLAG_DEEP_TILE))) p.td = TileGeom{};
    // GeomRD (GeomR's box under a 16 x 16 x 16 tile) joins under the same condition: rotations whose pre-image still fits that box
    // tiny volumes (<= 64^3: at most 64 of these tiles) stay with GeomR's smaller tiles: measured +5 ... +14 % otherwise; and a launch
    // of fewer than 1024 of these tiles (one pair up to 128^3) is a step of ~15 us, of which the five-body kernel's entry is 2-3
    const bool big_rd = p.trd.ntiles >= 128 && (long)p.trd.ntiles * v.B >= 2l * slots;
    if ((v.flags & TRX_FLAG_NO_ROT_DEEP_TILE) || !(big_rd || (v.flags & TRX_FLAG_DEEP_TILE))) p.trd = TileGeom{};
    // the z-streaming body: pairs next to the identity (zs_fits on the device) in launches that fill the chip.  Sizes only here: the shape
    // must tile (f1_candidates), and the launch must fill the chip with blocks of useful length (small problems stay with the tile kernels)
    if (v.flags & TRX_FLAG_NO_ZSTREAM) p.zg = ZGeom{};
    else if (p.zg.blocks_per_pair > 0 && !(v.flags & TRX_FLAG_ZSTREAM)) {
        const long zb = (long)p.zg.blocks_per_pair * v.B;
        if (zb < TRX_ZS_MIN_BLOCKS || p.zg.planes_per_seg < TRX_ZS_MIN_PLANES) p.zg = ZGeom{};
        // between one block per CU and a full round the streaming blocks share CUs unevenly; where the tile kernels fit ONE round of block
        // slots they win that case (3 x 192^3: 62 us against 69), everywhere else measured the streaming body is ahead
        else if (zb > slots / 2 && zb < slots && (long)p.ta.blocks_per_pair * v.B <= slots) p.zg = ZGeom{};
    }
    if (p.zg.blocks_per_pair == 0) p.zgf = ZGeom{};   // (the flat tile belongs to the z-streaming kernel)
    const TileGeom tef = p.tef;
    p.tef = TileGeom{};
    p.rows = f1_rows(p);
    // big batches of the step kernels: a flat grid of persistent blocks over a pair-major work list (no surplus blocks; see the kernel)
    // (B <= 64: the flat grid keeps one pair's state per lane)
    p.flat = v.B <= 64 && (long)p.rows * v.B >= 2 * slots;
    // the exact-footprint kernel (rotated pairs that GeomR would take) behind launches that fill the chip: columns of at most 64 of its tiles
    // (sizes: its row / plane pitches are 24-bit multiplier operands, its byte offsets 32-bit)
    const bool eft_sizes = (long)v.H * v.W * 4 < (1l << 24) && (size_t)v.D * v.H * v.W < ((size_t)1 << 29);
    if (tef.tiles_per_seg <= 64 && eft_sizes && !(v.flags & TRX_FLAG_NO_EFT) && (p.flat || (v.flags & TRX_FLAG_EFT))) {
        p.tef = tef;
        p.eft = tef.blocks_per_pair;   // = the partial rows per pair of that kernel
        p.rows = f1_rows(p);
    }
    // the row stride above counts the flat z-streaming tile wherever its shape fits; the tile handed to the kernels respects TRX_FLAG_NO_ZS_FLAT
    if (v.flags & TRX_FLAG_NO_ZS_FLAT) p.zgf = ZGeom{};
    // flat launches that offer the z-streaming body run it as a kernel of its own, FIRST (affine_zs_step_kernel): it alone evaluates the
    // test, the kernels behind it skip its pairs and return at once when it has taken them all
    p.zs_first = p.flat && p.zg.blocks_per_pair > 0 && !(v.flags & TRX_FLAG_ZS_FUSED);
    // the one-kernel form of a step: the streaming kernel also runs the pairs outside its window (GeomR's body), nothing behind it
    p.one_kernel = p.zs_first && (v.flags & TRX_FLAG_ONE_KERNEL);
    // the two-body (GeomA / GeomR) instance for launches that offer nothing else - the five-body kernel's entry costs 2-3 us
    // more (its arguments are fetched in front of the body that needs them), which is what a step of a small volume takes in all
    // (and no exact-footprint kernel in front: the two-body instance does not read its marks and would run its pairs a second time - ADVICE r4)
    const bool two_body = !p.flat && p.td.blocks_per_pair == 0 && p.trd.blocks_per_pair == 0 && p.zg.blocks_per_pair == 0 && p.eft == 0;
    // (the carry form of a step is the two-body launch with theta from the block's own prologue: trx_affine_run)
    p.dual = p.zs_first ? kBehindZs : !two_body ? kFiveBody : carry ? kCarry : kTwoBody;
    return p;
}

// Workspace of the affine entry points: [B][rows][41] partial sums | coordinate tables (callers that pass none) | rows_used[B + 11]
// ... | (3-D) second partial buffer | second rows_used[B + 11] | two carry buffers [B][64] floats  (the parity buffers of trx_affine_run's one-launch iterations)
struct AffineWs {
    size_t rows, off_tab, off_rows_used, off_part2, off_rows_used2, off_carry, bytes;
};
static AffineWs affine_ws(const trx_volumes &v)
{
    AffineWs w;
    AffineGeom g = affine_geom(v, kTargetBlocks);
    w.rows = (size_t)g.nblk;
    if (v.ndim == 3) w.rows = max(w.rows, (size_t)f1_rows(f1_candidates(v)));   // whatever a plan offers, its rows fit
    w.off_tab = ((size_t)v.B * w.rows * np_full(3) * sizeof(float) + 255) & ~(size_t)255;
    w.off_rows_used = w.off_tab + (((size_t)(v.W + v.H + v.D) * sizeof(float) + 255) & ~(size_t)255);
    const size_t notes = ((size_t)(v.B + 11) * sizeof(int) + 255) & ~(size_t)255;   // rows_used[B] | pairs left by the z-streaming kernel | its pair mask (2) | the exact-footprint kernel's work tickets, one per XCD (8)
    w.off_part2 = w.off_rows_used + notes;
    w.off_rows_used2 = w.off_part2 + (v.ndim == 3 ? w.off_tab : 0);
    w.off_carry = w.off_rows_used2 + (v.ndim == 3 ? notes : 0);
    w.bytes = w.off_carry + (v.ndim == 3 ? (((size_t)2 * v.B * kCarryStride * sizeof(float) + 255) & ~(size_t)255) : 0);
    return w;
}

extern "C" size_t trx_affine_workspace_bytes(const trx_volumes *vol)
{
    if (check_vol(vol, false) != TRX_OK) return 0;
    return affine_ws(*vol).bytes;
}

extern "C" size_t trx_affine_workspace_rows_offset(const trx_volumes *vol)
{
    if (check_vol(vol, false) != TRX_OK) return 0;
    return affine_ws(*vol).off_rows_used;
}

extern "C" size_t trx_affine_workspace_carry_offset(const trx_volumes *vol)
{
    if (check_vol(vol, false) != TRX_OK || vol->ndim != 3) return 0;
    return affine_ws(*vol).off_carry;
}

// [host] Would a step of this batch run entirely on the z-streaming kernel's two tiles at these (HOST) thetas?  The same test the kernel
// evaluates per pair on the device (zs_nsub), for callers that decide about TRX_FLAG_ONE_KERNEL from values they hold on the host.
extern "C" int trx_affine_near_identity(const trx_volumes *vol, const float *theta_host)
{
    if (check_vol(vol, false) != TRX_OK || !theta_host || vol->ndim != 3) return 0;
    const F1Plan p = f1_plan(*vol, persistent_blocks(), true, false);
    if (p.zg.blocks_per_pair == 0) return 0;
    const float fD = (float)vol->D, fH = (float)vol->H, fW = (float)vol->W;
    for (int b = 0; b < vol->B; b++) {
        const float *th = theta_host + (size_t)b * TRX_PSTRIDE;
        if (zs_nsub<ZS64>(th, fD, fH, fW, p.zg.planes_per_seg) > 0) continue;
        if (p.zgf.blocks_per_pair > 0 && zs_nsub<ZSF>(th, fD, fH, fW, p.zgf.planes_per_seg) > 0) continue;
        return 0;
    }
    return 1;
}

// (TRX_FLAG_GATHER_PATH: the un-tiled kernel stays reachable so that the tests can compare the two)
static bool use_tile_path(const trx_volumes *vol) { return vol->ndim == 3 && !(vol->flags & TRX_FLAG_GATHER_PATH); }

struct CarryLaunch {   // trx_affine_run's request for the carry form of a step launch: which parity buffers it writes, the kernel's carry arguments; `used` = it was launched
    int parity;
    CarryKArgs args;
    bool used;
    float *partials_out;   // where the launch wrote its rows (the parity buffer), whether or not the carry form was used
};

template <int MODE>
static int launch_accum(const trx_volumes *vol, const float *theta, const AffineGeom &g, int channels, size_t chan_stride,
                        float *partials, hipStream_t s)
{
    dim3 grid(g.nblk, vol->B), block(TRX_BLOCK);
    if (vol->ndim == 3)
        hipLaunchKernelGGL((affine_accum_kernel<3, MODE>), grid, block, 0, s, *vol, theta, g, channels, chan_stride, partials);
    else
        hipLaunchKernelGGL((affine_accum_kernel<2, MODE>), grid, block, 0, s, *vol, theta, g, channels, chan_stride, partials);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// GeomA / GeomR (and the step kernels' extra bodies) per pair in one launch: the instance of affine_tile_dual_kernel that the plan names, on the
// plan's grid.  rows_used == nullptr: the reader of `out` reads every row, so surplus blocks zero theirs.
template <int MODE>
static void launch_dual(const F1Plan &p, hipStream_t s, const trx_volumes &v, const float *theta, int channels, float *out, int *rows_used = nullptr,
                        const CarryKArgs *carry = nullptr)
{
    const dim3 grid = p.flat ? dim3(p.slots, 1) : dim3(p.rows, v.B * channels);
    const int zero_surplus = rows_used == nullptr, rows_stride = p.flat ? p.rows : 0;
    auto launch = [&](auto which, auto... carry_args) {
        hipLaunchKernelGGL((affine_tile_dual_kernel<MODE, decltype(which)::value>), grid, dim3(512), 0, s, v, theta, p.ta, p.tr, channels, out, zero_surplus, p.td, p.trd, p.zg,
                           rows_used, rows_stride, p.eft, carry_args...);
    };
    if constexpr (MODE == 0 || MODE == 4)   // (the step kernels)
        if (p.dual == kCarry) return launch(Which<kCarry>{}, *carry);
    if constexpr (MODE == 0 || MODE == 1 || MODE == 4)   // (the F1 modes: the warp modes 2 / 3 never run behind a z-streaming kernel)
        if (p.dual == kBehindZs) return launch(Which<kBehindZs>{});
    p.dual == kTwoBody ? launch(Which<kTwoBody>{}) : launch(Which<kFiveBody>{});
}

// MODE 0 / 1 / 4 dispatch: LDS-tiled kernels for 3-D, row-walking gather kernel otherwise.  Returns the number of partial rows per pair through *nblk.
// rows_used != nullptr: the caller's reduction reads the row count of every pair from the device array returned through it (the
// step's finalise kernel): surplus blocks of the dual grid then write nothing, and the step kernels may offer their extra bodies.
template <int MODE>
static int launch_f1(const trx_volumes *vol, const float *theta, float *partials, int *nblk, hipStream_t s, const int **rows_used = nullptr, CarryLaunch *cl = nullptr)
{
    if (rows_used) *rows_used = nullptr;
    if (cl) cl->used = false;
    if (!use_tile_path(vol)) {
        if constexpr (MODE == 4) return TRX_ERR_ARG;   // (the MSE-only rows exist in the tile kernels only; trx_affine_step asks for them on the tile path)
        else {
            AffineGeom g = affine_geom(*vol, kTargetBlocks);
            *nblk = g.nblk;
            return launch_accum<MODE>(vol, theta, g, 1, 0, partials, s);
        }
    }
    trx_volumes v = *vol;
    const AffineWs ws = affine_ws(*vol);
    float *const ws_base = partials;   // (tables and notes sit at fixed offsets from the workspace's start; the rows go to the parity buffer)
    const bool odd = cl != nullptr && cl->parity != 0;
    if (odd) partials = (float *)((char *)ws_base + ws.off_part2);
    if (cl) cl->partials_out = partials;
    if (!v.xn || !v.yn || !v.zn) {
        // tables live behind the partials (trx_affine_workspace_bytes reserves the room)
        float *tab = (float *)((char *)ws_base + ws.off_tab);
        const int n = max(v.W, max(v.H, v.D));
        hipLaunchKernelGGL(fill_tables_kernel, dim3((n + 255) / 256), dim3(256), 0, s, tab, v.W, v.H, v.D);
        TRX_CHECK_LAUNCH();
        v.xn = tab; v.yn = tab + v.W; v.zn = tab + v.W + v.H;
    }
    if (!use_dual(vol)) {
        const TileGeom t = tile_geom(*vol);
        hipLaunchKernelGGL((affine_tile_kernel<MODE>), dim3(t.blocks_per_pair, vol->B), dim3(kTileThreads), 0, s, v, theta, t, 1, partials);
        TRX_CHECK_LAUNCH();
        *nblk = t.blocks_per_pair;
        return TRX_OK;
    }
    int *const ru = rows_used ? (int *)((char *)ws_base + (odd ? ws.off_rows_used2 : ws.off_rows_used)) : nullptr;
    const F1Plan p = f1_plan(*vol, persistent_blocks(), ru != nullptr && (MODE == 0 || MODE == 4), cl != nullptr);
    if constexpr (MODE == 0 || MODE == 4) {
        if (p.one_kernel) hipLaunchKernelGGL((affine_zs_one_kernel<MODE>), dim3(p.slots, 1), dim3(ZS64::Threads), 0, s, v, theta, p.zg, p.zgf, partials, ru, p.rows, p.tr);
        else {
            if (p.zs_first) {
                hipLaunchKernelGGL((affine_zs_step_kernel<MODE>), dim3(p.slots, 1), dim3(ZS64::Threads), 0, s, v, theta, p.zg, p.zgf, partials, ru, p.rows);
                TRX_CHECK_LAUNCH();
            }
            if (p.eft) {   // in front of the tile kernel: takes its pairs and marks them rows_used < 0 (none - the usual case next to the identity - costs ~3 us, ~1.5 behind the z-streaming kernel)
                const int wd = p.td.blocks_per_pair > 0, wrd = p.trd.blocks_per_pair > 0, zp = p.zs_first ? -1 : (p.zg.blocks_per_pair > 0 ? p.zg.planes_per_seg : 0);   // (-1: the z-streaming kernel ran in front)
                if (p.flat) hipLaunchKernelGGL((affine_eft_step_kernel<MODE>), dim3(p.slots, 1), dim3(ECfg::Threads), 0, s, v, theta, p.tef, partials, ru, p.rows, wd, wrd, zp);
                else hipLaunchKernelGGL((affine_eft_step_kernel<MODE>), dim3(p.tef.blocks_per_pair, vol->B), dim3(ECfg::Threads), 0, s, v, theta, p.tef, partials, ru, -p.rows, wd, wrd, zp);
                TRX_CHECK_LAUNCH();
            }
        }
    }
    if (!p.one_kernel) launch_dual<MODE>(p, s, v, theta, 1, partials, ru, cl ? &cl->args : nullptr);
    TRX_CHECK_LAUNCH();
    if (cl) cl->used = p.dual == kCarry;
    *nblk = p.rows;
    if (rows_used) *rows_used = ru;
    return TRX_OK;
}

// The finalise kernel behind a step launch (trx_affine_step, and the flush behind the last carry launch of trx_affine_run: state_in = its carry buffer)
static int launch_finalize(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_affine_state *st, const float *partials, int nblk,
                           const int *rows_used, bool mse_only, const float *state_in, hipStream_t s)
{
    const double nvox = (double)vol->D * vol->H * vol->W;
    // rows_used, mse_only and state_in belong to the 3-D tile path: a 2-D caller holds nullptr / false / nullptr, the kernel's defaults
    if (vol->ndim != 3 && (rows_used || mse_only || state_in)) return TRX_ERR_ARG;
    with_ndim(vol->ndim, [&](auto nd) {
        hipLaunchKernelGGL((affine_finalize_kernel<decltype(nd)::value>), dim3(vol->B), dim3(TRX_FIN_THREADS), 0, s, partials, nblk, nvox,
                           vol->D, vol->H, vol->W, *loss, *opt, *st, rows_used, mse_only ? 1 : 0, state_in);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

// The arguments of a step: what trx_affine_step refuses, and what the carry form of trx_affine_run needs to hold before it launches anything
static int check_step_args(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_affine_state *st, const void *workspace, size_t workspace_bytes)
{
    int rc = check_vol(vol, true);
    if (rc) return rc;
    if (!loss || !opt || !st || !workspace) return TRX_ERR_ARG;
    if (!st->param || !st->theta || !st->best_theta || !st->best_loss || !st->best_idx || !st->step) return TRX_ERR_ARG;
    if (opt->kind != TRX_OPT_SGD && opt->kind != TRX_OPT_ADAM) return TRX_ERR_ARG;
    if (opt->kind == TRX_OPT_ADAM && (!st->adam_m || !st->adam_v)) return TRX_ERR_ARG;
    if (st->mode != TRX_PARAM_AFFINE && st->mode != TRX_PARAM_RIGID) return TRX_ERR_ARG;
    if (workspace_bytes < trx_affine_workspace_bytes(vol)) return TRX_ERR_WORKSPACE;
    return TRX_OK;
}

// without an NCC term only d = warped - target matters: the step kernel then keeps 13 sums instead of 41 (3-D tile path)
static bool step_mse_only(const trx_volumes *vol, const trx_loss_cfg *loss) { return (loss->w_ncc == 0.f) && use_tile_path(vol); }

// the F1 launch of a step (launch_f1's arguments): the MSE-only rows are MODE 4 of the same kernels
template <class... Args>
static int launch_step_f1(bool mse_only, Args... args) { return mse_only ? launch_f1<4>(args...) : launch_f1<0>(args...); }

// odd iterations of a run walk the z-streaming columns downward: the tail of one pass is the head of the next (TRX_FLAG_WALK_DOWN)
static unsigned iteration_flags(const trx_volumes *vol, int k) { return ((k & 1) && !(vol->flags & TRX_FLAG_NO_PINGPONG)) ? vol->flags ^ TRX_FLAG_WALK_DOWN : vol->flags; }

extern "C" int trx_affine_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                               const trx_affine_state *st, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_step_args(vol, loss, opt, st, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *partials = (float *)workspace;
    int nblk = 0;
    // Every step picks GeomA / GeomR per pair in the kernel (TRX_FLAG_SINGLE_GEOM: the primary geometry only).  Rigid runs start from a
    // random pose (reference: torch.rand, up to 1 rad) and live at large rotations; affine runs start at the identity, where the
    // GeomA body is all that runs, but may rotate away from it: the single-geometry kernel then gathers from L2 at 3.2x the cost.
    const int *rows_used = nullptr;
    const bool mse_only = step_mse_only(vol, loss);
    rc = launch_step_f1(mse_only, vol, st->theta, partials, &nblk, s, &rows_used);
    if (rc) return rc;
    return launch_finalize(vol, loss, opt, st, partials, nblk, rows_used, mse_only, nullptr, s);
}

extern "C" int trx_affine_accumulate(const trx_volumes *vol, const float *theta, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_vol(vol, true);
    if (rc) return rc;
    if (!theta || !workspace) return TRX_ERR_ARG;
    if (workspace_bytes < trx_affine_workspace_bytes(vol)) return TRX_ERR_WORKSPACE;
    int nblk = 0;
    const int *rows_used = nullptr;
    return launch_f1<0>(vol, theta, (float *)workspace, &nblk, (hipStream_t)stream, &rows_used);   // exactly the launch of a step (profiling aid)
}

extern "C" int trx_affine_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                              const trx_affine_state *st, int iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (iters < 0 || !st) return TRX_ERR_ARG;
    if (st->losses && iters > st->losses_capacity) return TRX_ERR_CAPACITY;
    if (!vol) return TRX_ERR_ARG;
    trx_volumes v = *vol;
    int first = 0;
    // CARRY (CarryKArgs): launch-bound 3-D steps - one (GeomA / GeomR) kernel and a finalise kernel behind it - run as ONE launch per iteration: the finalise
    // of iteration k rides in the prologue of iteration k + 1's kernel, and one finalise kernel behind the last launch flushes the run.  The launches alternate
    // between the workspace's two partial / note / carry buffers; the LAST one writes the primary set (what trx_affine_workspace_rows_offset describes).
    // (arguments a step would refuse: the loop below reports them)
    if (iters >= 2 && !(vol->flags & TRX_FLAG_NO_CARRY) && use_tile_path(vol) && check_step_args(vol, loss, opt, st, workspace, workspace_bytes) == TRX_OK) {
        hipStream_t s = (hipStream_t)stream;
        const bool mse_only = step_mse_only(vol, loss);
        float *const base = (float *)workspace;
        float *const carry_buf = (float *)((char *)workspace + affine_ws(*vol).off_carry);
        const float *prev_partials = nullptr;
        const int *prev_notes = nullptr;
        int prev_nblk = 0;
        for (int k = 0; k < iters; k++) {
            CarryLaunch cl = CarryLaunch{};
            cl.parity = (iters - 1 - k) & 1;
            cl.args = CarryKArgs{prev_partials, prev_notes, prev_nblk, mse_only ? 1 : 0, k > 0 ? carry_buf + (size_t)(cl.parity ^ 1) * vol->B * kCarryStride : nullptr,
                                 carry_buf + (size_t)cl.parity * vol->B * kCarryStride, (double)vol->D * vol->H * vol->W, *loss, *opt, *st};
            v.flags = iteration_flags(vol, k);
            int nblk = 0;
            const int *notes = nullptr;
            int rc = launch_step_f1(mse_only, &v, st->theta, base, &nblk, s, &notes, &cl);
            if (rc) return rc;
            if (!cl.used) {
                // not a launch the carry form exists for (only possible at k = 0: the choice depends on sizes and flags alone): the launch above was an
                // ordinary step launch - finish that step and run the rest the ordinary way
                rc = launch_finalize(vol, loss, opt, st, cl.partials_out, nblk, notes, mse_only, nullptr, s);
                if (rc) return rc;
                first = 1;
                prev_partials = nullptr;
                break;
            }
            prev_partials = cl.partials_out; prev_notes = notes; prev_nblk = nblk;
        }
        if (prev_partials != nullptr)   // every launch was a carry launch: flush the last iteration (its buffers are the primary set: parity 0)
            return launch_finalize(vol, loss, opt, st, prev_partials, prev_nblk, prev_notes, mse_only, carry_buf, s);
    }
    for (int i = first; i < iters; i++) {
        v.flags = iteration_flags(vol, i);
        int rc = trx_affine_step(&v, loss, opt, st, workspace, workspace_bytes, stream);
        if (rc) return rc;
    }
    return TRX_OK;
}

extern "C" int trx_affine_loss(const trx_volumes *vol, const trx_loss_cfg *loss, const float *theta, float *terms,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_vol(vol, true);
    if (rc) return rc;
    if (!loss || !theta || !terms || !workspace) return TRX_ERR_ARG;
    if (workspace_bytes < trx_affine_workspace_bytes(vol)) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float *partials = (float *)workspace;
    int nblk = 0;
    rc = launch_f1<1>(vol, theta, partials, &nblk, s);
    if (rc) return rc;
    return launch_loss_finalize(vol, loss, partials, nblk, terms, s);
}

extern "C" int trx_affine_warp(const trx_volumes *vol, const float *theta, int channels, float *out, void *stream)
{
    int rc = check_vol(vol, false);
    if (rc) return rc;
    if (!theta || !out || channels < 1) return TRX_ERR_ARG;
    if ((long)vol->B * channels > 65535) return TRX_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W;
    if (use_tile_path(vol) && vol->xn && vol->yn && vol->zn) {
        // LDS-tiled forward warp (same staging as the F1 pass); needs the caller's coordinate tables
        trx_volumes v = *vol;
        v.B = vol->B * channels;                       // geometry: every (pair, channel) is one slab of blocks
        TileGeom t = tile_geom(v);
        if (use_dual(vol)) {
            const F1Plan p = f1_plan(v, 0, false, false);   // (GeomA / GeomR on the classic grid)
            v.B = vol->B;
            launch_dual<3>(p, s, v, theta, channels, out);
            TRX_CHECK_LAUNCH();
            return TRX_OK;
        }
        v.B = vol->B;
        hipLaunchKernelGGL((affine_tile_kernel<3>), dim3(t.blocks_per_pair, vol->B * channels), dim3(kTileThreads), 0, s, v, theta, t, channels, out);
        TRX_CHECK_LAUNCH();
        return TRX_OK;
    }
    size_t nb = (nvox + TRX_BLOCK - 1) / TRX_BLOCK;
    if (nb > 8192) nb = 8192;
    dim3 grid((unsigned)nb, vol->B), block(TRX_BLOCK);
    if (vol->ndim == 3)
        hipLaunchKernelGGL((affine_warp_kernel<3>), grid, block, 0, s, *vol, theta, channels, nvox, out);
    else
        hipLaunchKernelGGL((affine_warp_kernel<2>), grid, block, 0, s, *vol, theta, channels, nvox, out);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

extern "C" int trx_affine_warp_backward(const trx_volumes *vol, const float *theta, int channels, const float *grad_out,
                                        float *dtheta, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_vol(vol, false);
    if (rc) return rc;
    if (!theta || !grad_out || !dtheta || !workspace || channels < 1) return TRX_ERR_ARG;
    if (workspace_bytes < trx_affine_workspace_bytes(vol)) return TRX_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    AffineGeom g = affine_geom(*vol, kTargetBlocks);
    float *partials = (float *)workspace;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W;
    trx_volumes v = *vol;
    v.target = grad_out;
    v.target_stride = (size_t)channels * nvox;
    if (use_tile_path(vol) && vol->xn && vol->yn && vol->zn && channels == 1) {
        // LDS-tiled kernel (same staging as the F1 pass); one partial row per block, 12 sums each.  (Several channels or
        // caller-less tables: the row-walking gather kernel below; the workspace is sized for single-channel tiles.)
        TileGeom t = tile_geom(*vol);
        int rows = t.blocks_per_pair;
        if (use_dual(vol)) {
            const F1Plan p = f1_plan(*vol, 0, false, false);   // (GeomA / GeomR on the classic grid)
            rows = p.rows;
            launch_dual<2>(p, s, v, theta, 1, partials);
        } else {
            hipLaunchKernelGGL((affine_tile_kernel<2>), dim3(t.blocks_per_pair, vol->B), dim3(kTileThreads), 0, s, v, theta, t, 1, partials);
        }
        TRX_CHECK_LAUNCH();
        return launch_bwd_finalize(vol, partials, rows, dtheta, s);
    }
    rc = launch_accum<2>(&v, theta, g, channels, nvox, partials, s);
    if (rc) return rc;
    return launch_bwd_finalize(vol, partials, g.nblk, dtheta, s);
}
