// LDS-TILED variant of the fused F1 pass (3-D): the tile geometries, their launch shapes and the tile body.  Included by affine.hip inside namespace trx,
// in front of affine_zstream.h and affine_eft.h, which use its accumulators and its lane / wave / reduce helpers (and by the bench harnesses
// through affine.hip).  Needs np_full and kNpMse (affine_finalize.h).  The kernels that run tile_body are in affine.hip.
//
// ------------------------------------------------------------------------------------------
// LDS-tiled 3-D variant of the F1 pass (the path the headline number runs).
//
// A block owns one (32 x, 8 z) COLUMN of the volume and walks it along y in tiles of 16 rows.  The pre-image
// of a tile under the affine map is a small parallelepiped; its bounding box (x origin aligned to 4 voxels)
// is staged into LDS by LDS-DMA (global_load_lds_dwordx4, masked to the needed, in-volume float4 slots; cells
// outside the volume are zero-filled, which IS grid_sample's zero padding), then all 8-corner gathers are
// ds_read2_b32 from LDS with fixed strides and no bounds checks.  Full tiles whose box fits run in the fast
// loop; partial tiles, tiles whose box exceeds the LDS budget (large rotations / zoom-out) and the one tile per
// pair that holds the volume's last row when W % 4 != 0 run in the generic loop behind it, which also holds
// the global-gather fallback - results never depend on which path ran beyond fp32 rounding.
// Thread (x, z) is fixed for the whole column, so only sum(q grad) and sum(q grad yn) live in registers and
// the xn / zn columns of the 41 sums are one multiply at the very end.
// ------------------------------------------------------------------------------------------
// Every geometry: 512-thread blocks, ONE box, 2 blocks per CU (staging of one block overlaps the gather of the other).  Removed
// alternative ("cfg 1"): 1024-thread blocks with two 81.3 KB boxes, one block per CU, 324-331 us against 315.
// LDS box (floats), kBW % 4 == 0.  One LDS-DMA piece (one global_load_lds_dwordx4 per wave) covers kPP z planes of the
// box - at most one float4 slot per thread - so piece k of a thread is its piece-0 slot shifted by k * kPP planes: one VGPR
// offset + one packed slot id per thread instead of one per piece.
template <int TX_, int TZ_, int THREADS_, int BW_, int BH_, int BD_, int PP_, int TY_ = 16>
struct TileCfg {
    static constexpr int TX = TX_, TY = TY_, TZ = TZ_, Threads = THREADS_;
    static constexpr int BW = BW_, BH = BH_, BD = BD_, PP = PP_;
    static constexpr int NH = Threads / (TX * TZ);          // y groups of a tile (2 halves of 8 rows, or 4 quarters of 4)
    static constexpr int Rows = TY / NH;                    // rows per thread
    static constexpr int Waves = Threads / 64;
    static constexpr int BW4 = BW / 4;
    static constexpr int PlaneSlots = BH * BW4;             // float4 slots per box plane
    static constexpr int Pieces = (BD + PP - 1) / PP;       // DMA pieces per tile
    static constexpr int PieceFloats = PP * BH * BW;        // floats of LDS per piece
    static constexpr int BoxFloats = BW * BH * BD;          // one box; lanes of the last piece past it are always masked
    static constexpr int ReduceScratch = Waves * 16 * 65 + Waves * 16;   // floats block_reduce_store_nw needs (aliases the box)
    static constexpr int BoxAlloc = (BoxFloats > ReduceScratch) ? BoxFloats : ReduceScratch;
    static_assert(BW % 4 == 0 && PP * PlaneSlots <= Threads && (PP == 2 || PP == 4), "one DMA piece: at most one slot per thread");
};
using GeomA = TileCfg<32, 8, 512, 44, 23, TRX_GEOMA_BD, 2>;      // near-identity transforms: 32 x 16 x 8 tile, 44 x 23 x 14 box (56.7 KB)
// Rotated transforms: the pre-image of a 32-wide tile grows by 31 sin(angle) rows / planes and stops fitting any box beyond
// ~0.1 rad.  A more cubic tile (16 x 16 x 8, four y-quarters of 4 rows per thread) with a 28 x 27 x 26 box (78.6 KB, still two blocks
// per CU): the pre-image of the tile under ANY rotation (span <= |(15,15,7)| = 22.3 voxels per axis) fits, i.e. every pose the reference's
// rigid mode can draw (angles uniform in [0,1) rad, ref:utils.py:316-330); only the needed extent is fetched, so small angles cost what
// they cost with a 28 x 26 x 16 box (the removed alternative: rotations about one axis up to ~0.5 rad, 55 us per 256^3 pair).
#ifndef TRX_GEOMR_BH
#define TRX_GEOMR_BH 27
#define TRX_GEOMR_BD 26
#endif
using GeomR = TileCfg<16, 8, 512, 28, TRX_GEOMR_BH, TRX_GEOMR_BD, 2>;
// (Removed alternative, GeomW: a 64 x 8 x 8 tile with a 76 x 13 x 14 box, -3 % at the identity, fits |rotation| < ~0.04 rad only: profiles/HISTORY.md.)
// Deep tile on 512 threads (32 x 16 x 16, sixteen rows per thread, ONE 44 x 23 x 19 box = 76.9 KB, two blocks per CU): per-tile work and the two
// barriers are paid once per 8192 voxels instead of 4096 and the z halo is 18 / 16 instead of 10 / 8; the box has one plane of slack, so it
// serves |theta - I| up to ~0.03 rad about x / y only.
using GeomD = TileCfg<32, 16, 512, 44, 23, 19, 2>;
// GeomR's box under a 16 x 16 x 16 tile (eight rows per thread): per-tile work is paid once per 4096 voxels instead of 2048 and the z halo is
// 18 / 16 instead of 10 / 8; the pre-image fits the 26-plane box for rotations about z of any size GeomR serves and for general rotations up to
// ~0.4 rad per axis.
using GeomRD = TileCfg<16, 16, 512, 28, TRX_GEOMR_BH, TRX_GEOMR_BD, 2>;
// The single-geometry kernel (affine_tile_kernel, TRX_FLAG_SINGLE_GEOM) runs GeomA.

struct TileGeom {
    int ntx, nty, ntz, ntiles, blocks_per_pair, ysplit, tiles_per_seg;
};

template <class G = GeomA>
static TileGeom tile_geom(const trx_volumes &v)
{
    TileGeom t;
    t.ntx = (v.W + G::TX - 1) / G::TX; t.nty = (v.H + G::TY - 1) / G::TY; t.ntz = (v.D + G::TZ - 1) / G::TZ;
    t.ntiles = t.ntx * t.nty * t.ntz;
    // One block per (x-tile, z-tile) column walking y; columns are split into y segments where that fills the chip better
    // (512 block slots: 2 blocks on each of 256 CUs).  Measured with tools/kbench.hip (TRX_TILE_TARGET_BLOCKS sweeps):
    //  - few columns (<= 512 blocks): one round of ~512 blocks, but at least 2 tiles per block
    //    (1 x 256^3: 47 us at 512 blocks, 53 at 256 and 1024; 1 x 128^3: 12.1 us at 256 blocks x 2 tiles, 13.6 at 512 x 1);
    //  - many columns: the split (1..4) that minimises  (slot rounds * 512 / blocks) * (1 + 1.5 / tiles per block)  - the
    //    idle tail of the last round against the per-block prologue / epilogue (8 x 182^3: 181 us unsplit, 173 us split in 2).
    const int ncol = t.ntx * t.ntz;
#ifdef TRX_DEV
    static const int target = [] { const char *e = getenv("TRX_TILE_TARGET_BLOCKS"); return e ? atoi(e) : 0; }();   // development override (kbench sweeps)
#else
    constexpr int target = 0;
#endif
    const long cols = (long)v.B * ncol;
    int ys = 1;
    if (target > 0) {
        ys = (int)((target + cols - 1) / cols);
    } else if (cols * t.nty > 1024) {
        // Occupancy model of one launch, in units of "one tile on a CU that runs a single block": 512 block slots (two per CU); a block
        // costs its tiles + 1.5 of prologue / epilogue, times 1.6 when it shares its CU (the pair together: 1.25x a lone block); blocks
        // beyond the slots run in further rounds, a last round of <= 256 blocks has the CUs to itself.  Reproduces the sweeps the
        // round-1 rules were fitted to by hand (1 x 256^3: 512 blocks 47 us, 256 or 1024 blocks 53 us; 8 x 182^3: split in two 173 us,
        // unsplit 181) and fixes what they missed - a second round that is nearly empty (1 x 192^3: 576 blocks 39 us, 432 blocks 32 us;
        // 2 x 182 x 218 x 182: 552 blocks 77 us, 828 blocks 66 us).  Many columns: at most four segments, as before (every segment of
        // every geometry enlarges the dual kernel's grid, whose surplus blocks cost their dispatch).
        double best = 1e30;
        int last_tps = 0;
        const int cmax = cols > 512 ? (t.nty < 4 ? t.nty : 4) : t.nty;
        for (int c = 1; c <= cmax; c++) {
            const int tps = (t.nty + c - 1) / c, segs = (t.nty + tps - 1) / tps;
            if (tps == last_tps) continue;   // same split as the previous c
            last_tps = tps;
            const long blocks = cols * segs, full = blocks / 512, rem = blocks % 512;
            double cost = (double)full * 1.6 * (tps + 1.5);
            if (rem > 0) cost += (rem <= 256 ? 1.0 : 1.6) * (tps + 1.5);
            if (cost < best - 1e-9) { best = cost; ys = c; }
        }
    } else if (cols <= 512) {   // (launches of at most two tiles per block slot, where fixed costs decide and the model does not resolve them: the round-1 rules)
        ys = (int)((512 + cols - 1) / cols);
        const int cap = t.nty / 2 > 1 ? t.nty / 2 : 1;
        if (ys > cap && cols * cap >= 256) ys = cap;   // (tiny volumes: as many blocks as there are tiles - 1 x 64^3: 8.9 vs 12.1 us)
    } else {
        double best = 1e30;
        for (int c = 1; c <= 4 && c <= t.nty; c++) {
            const int tps = (t.nty + c - 1) / c, segs = (t.nty + tps - 1) / tps;
            const double blocks = (double)cols * segs;
            const double rounds = (double)(((long)blocks + 511) / 512);
            const double waste = rounds * 512.0 / blocks * (1.0 + 1.5 / tps);
            if (waste < best - 1e-9) { best = waste; ys = c; }
        }
    }
    if (ys < 1) ys = 1;
    if (ys > t.nty) ys = t.nty;
    t.tiles_per_seg = (t.nty + ys - 1) / ys;
    t.ysplit = (t.nty + t.tiles_per_seg - 1) / t.tiles_per_seg;
    t.blocks_per_pair = ncol * t.ysplit;
    return t;
}

// packed running sums of the tile kernel: AB[q][c] = (sum q*g_c, sum q*g_c*yn), M01 = (Sy, Sw), M23 = (Syy, Sww)
struct F1Acc {
    f2 AB[3][3], M01, M23;
    float M4;
};

template <int MODE>
__device__ __forceinline__ void f1_accumulate_pk(const Samp3 &sm, float yv, float yn, F1Acc &a)
{
    if constexpr (MODE == 2) {   // generic warp backward: yv = grad_out of this voxel, only sum(go * grad) and sum(go * grad * yn)
        const float gq[3] = {sm.dx, sm.dy, sm.dz};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const f2 gu = {gq[c], yn * gq[c]};
            a.AB[0][c] = gu * yv + a.AB[0][c];
        }
        return;
    }
    if constexpr (MODE == 4) {   // MSE / SSD only (no NCC term): d = w - y carries everything - sum d^2 and sum(d * grad), sum(d * grad * yn)
        const float d = sm.v - yv;
        a.M4 = fmaf(d, d, a.M4);
        const float gq[3] = {sm.dx, sm.dy, sm.dz};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const f2 gu = {gq[c], yn * gq[c]};
            a.AB[0][c] = gu * d + a.AB[0][c];
        }
        return;
    }
    const f2 yw = {yv, sm.v};
    a.M01 += yw;
    a.M23 = yw * yw + a.M23;
    a.M4 = fmaf(yv, sm.v, a.M4);
    if constexpr (MODE == 0) {
        const float gq[3] = {sm.dx, sm.dy, sm.dz};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const f2 gu = {gq[c], yn * gq[c]};
            a.AB[0][c] += gu;
            a.AB[1][c] = gu * yv + a.AB[1][c];
            a.AB[2][c] = gu * sm.v + a.AB[2][c];
        }
    }
}

constexpr int kTileThreads = GeomA::Threads;   // block size of the primary kernel (the dual kernel: 512)

// Work-item id of a 1-D block WITHOUT keeping v0 (the packed ids the hardware delivers) alive: lane id from v_mbcnt, wave index read once
// at kernel entry into an SGPR (trx_wave_index).  With five bodies inlined behind a dispatch the allocator spilled v0 to scratch at entry and
// every body paid a memory round trip to get it back.
__device__ __forceinline__ int trx_lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int trx_wave_index() { return __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); }

// F64 = false: the 64 lane partials of a wave, then the NW wave sums, are summed in one fp32 chain each (the z-streaming and exact-footprint kernels:
// they run only in launches of hundreds of blocks, whose rows the finalise sums in fp64, so the chains' errors average out).
// F64 = true (the tile bodies, the only step kernels a small volume runs): fp64 accumulators in eight independent chains, the wave sums handed over
// as a float pair (hi + lo), so that only the threads' own sums and one rounding of the row are fp32.  Where a volume is ONE block the fp64 row
// sums behind this have nothing to average: 8 x 16 x 32 at NCC = 0.99 had its loss off by 2.8e-5 with the fp32 chains, 8.6e-6 with these
// (tests/test_gpu_carry.py [one-tile]).  Cost and the A/B against the fp32 chains: DESIGN.md 4.1f (3).
template <int NV, int NW, bool F64 = false>
__device__ __forceinline__ void block_reduce_store_nw(const float (&vals)[NV], float *__restrict__ out, float *smem, int wave)
{
    // smem: >= NW*16*65 + NW*16 floats of scratch (aliases the tile box); wave: this wave's index in the block (uniform)
    constexpr int CH = 16;
    float(*red)[CH][65] = reinterpret_cast<float(*)[CH][65]>(smem);
    float(*wsum)[CH] = reinterpret_cast<float(*)[CH]>(smem + NW * CH * 65);
    const int lane = trx_lane_id(), tid = wave * 64 + lane;
#pragma unroll
    for (int c0 = 0; c0 < NV; c0 += CH) {
#pragma unroll
        for (int j = 0; j < CH; j++)
            if (c0 + j < NV) red[wave][j][lane] = vals[c0 + j];
        __syncthreads();
        if (lane < CH && c0 + lane < NV) {
            if constexpr (F64) {
                double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // (one chain of 64 fp64 adds: measured +1 us per block)
#pragma unroll
                for (int i = 0; i < 64; i += 8)
#pragma unroll
                    for (int k = 0; k < 8; k++) a[k] += (double)red[wave][lane][i + k];
                const double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
                const float hi = (float)s;
                wsum[wave][lane] = hi;
                red[wave][lane][64] = (float)(s - (double)hi);   // (column 64 of a row: the padding of the 65-float pitch, read by nobody else)
            } else {
                float s = 0.f;
#pragma unroll 16
                for (int i = 0; i < 64; i++) s += red[wave][lane][i];
                wsum[wave][lane] = s;
            }
        }
        __syncthreads();
        if (tid < CH && c0 + tid < NV) {
            if constexpr (F64) {
                double hi = 0.0, lo = 0.0;
#pragma unroll
                for (int w = 0; w < NW; w++) { hi += (double)wsum[w][tid]; lo += (double)red[w][tid][64]; }
                out[c0 + tid] = (float)(hi + lo);
            } else {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < NW; w++) s += wsum[w][tid];
                out[c0 + tid] = s;
            }
        }
        __syncthreads();
    }
}

// value is identical in every lane: pin it to an SGPR so it does not occupy a VGPR
__device__ __forceinline__ float uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// wave-uniform pointer pinned to an SGPR pair (a no-op when the compiler already knows it is uniform); the asm blocks of the
// tile kernel take their base addresses as "s" operands
template <class T>
__device__ __forceinline__ T *uni_ptr(T *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return (T *)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float lane_bcast(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// Requires vol.xn / vol.yn / vol.zn != NULL (the launcher materialises them when the caller passes NULL).
//
// Work decomposition: a 512-thread block owns one (x-tile, z-tile) COLUMN of the volume and walks it
// along y, 16 rows per tile.  Thread (lx, lz, half) keeps its voxel column (x, z) for the whole block, so
// only sum(q grad) and sum(q grad yn) live in registers (23 accumulators); the xn / zn columns of the 41
// sums are one multiply at the very end.
//
// Sample coordinates are formed as  (ATen's identity coordinate of this voxel) + (deviation of theta
// from identity): i_x = id_x(x) + (W/2)((t00-1) xn + t01 yn + t02 zn + t03), etc.  id_c uses ATen's exact
// un-normalisation roundings (unnorm<3>), so at theta = identity the coordinates are BITWISE those of
// the reference (every sample sits on a voxel there and the one-sided derivative depends on the last
// bit); for any other theta this is the same affine map to within fp32 rounding, at 4 VALU ops / voxel.
// s[100:101] (the DMA base walker of the fast loop) are outside the compiler's allocatable SGPR range on gfx950 - it warns
// that it will not preserve them, which is exactly why they are safe to use; LDS addresses are 32-bit integers by construction.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#pragma clang diagnostic ignored "-Wint-to-pointer-cast"
// LTH (round 6, the carry form of a step): `theta` points at the 12 floats of THIS pair in LDS (the block's prologue has just computed them) instead of at the
// batch's theta array in global memory.
template <int MODE, class G, bool LTH = false>
__device__ __forceinline__ void tile_body(const trx_volumes &vol, const float *__restrict__ theta, const TileGeom &tg, int channels,
                                          float *__restrict__ partials, float *box, const int bx, const int by, const int rows_stride, const int wave_in)
{
    // geometry of this instantiation (bx, by: the block's index in the (blocks_per_pair, pairs x channels) grid)
    constexpr int kTX = G::TX, kTY = G::TY, kTZ = G::TZ, kBW = G::BW, kBH = G::BH, kBD = G::BD, kPP = G::PP;
    // One box per block in every geometry.  The two-box form of the fast loop (kBufs == 2: the removed 1024-thread "cfg 1") stays below:
    // deleting it changes the instructions of the kernels that remain.
    constexpr int kBufs = 1;
    constexpr int kNH = G::NH, kRows = G::Rows, kTileWaves = G::Waves, kBW4 = G::BW4, kPlaneSlots = G::PlaneSlots, kPieces = G::Pieces;
    constexpr int kPieceFloats = G::PieceFloats, kBoxFloats = G::BoxFloats;
    (void)kNH; (void)kBD; (void)kPlaneSlots;
    // MODE 0: F1 sums, MODE 1: moments only, MODE 2: generic warp backward (`vol.target` = grad_out [B][channels][D][H][W],
    // 12 sums per (pair, channel)), MODE 3: forward warp (writes the warped volume to `partials` = out[B][channels][D][H][W])
    // MODE 4: the step kernel for losses without an NCC term (MSE and / or SSD - what the reference's rigid / affine drivers always run,
    // SURVEY Q2): 13 sums per block (sum d^2, 12 x sum d J with d = warped - target) instead of 41, 8 accumulation instructions per
    // voxel instead of 15
    constexpr int NQ = (MODE == 0) ? 3 : ((MODE == 2 || MODE == 4) ? 1 : 0);
    constexpr int NP = (MODE == 0) ? np_full(3) : (MODE == 2 ? 12 : (MODE == 4 ? kNpMse : 5));
    constexpr bool kGrad = (MODE == 0) || (MODE == 2) || (MODE == 4);
    constexpr bool kPerChannel = (MODE == 2) || (MODE == 3);   // blockIdx.y enumerates (pair, channel); channels share theta
    const int b = kPerChannel ? by / channels : by;
    const int ch = kPerChannel ? by - b * channels : 0;
    const int D = vol.D, H = vol.H, W = vol.W;
    const float *__restrict__ th = LTH ? theta : uni_ptr(theta + (size_t)b * TRX_PSTRIDE);
    const float *__restrict__ mov = uni_ptr(vol.moving + (size_t)b * vol.moving_stride + (size_t)ch * D * H * W);
    // MODE 3 has no target: `tgt` is the OUTPUT volume of this (pair, channel)
    float *__restrict__ wout = uni_ptr(partials + (size_t)by * D * H * W);
    const float *__restrict__ tgt = (MODE == 3) ? wout : uni_ptr(vol.target + (size_t)b * vol.target_stride + (MODE == 2 ? (size_t)ch * D * H * W : 0));
    const float *__restrict__ xtab = uni_ptr(vol.xn), *__restrict__ ytab = uni_ptr(vol.yn), *__restrict__ ztab = uni_ptr(vol.zn);
    const int lane = trx_lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(wave_in);          // provably wave-uniform (SGPR)
    const int tid = wave * 64 + lane;
    const int lx = tid & (kTX - 1), lz = (tid / kTX) & (kTZ - 1), lh = wave / (kTileWaves / kNH);
    const float fW = (float)W, fH = (float)H, fD = (float)D;
    const float hW = 0.5f * fW, hH = 0.5f * fH, hD = 0.5f * fD;
    auto thv = [&](int k) { return LTH ? uni(th[k]) : th[k]; };   // (LDS reads are vector loads: pin the uniform values to scalar registers as the scalar loads do)
    const float t00 = thv(0), t01 = thv(1), t02 = thv(2), t03 = thv(3);
    const float t10 = thv(4), t11 = thv(5), t12 = thv(6), t13 = thv(7);
    const float t20 = thv(8), t21 = thv(9), t22 = thv(10), t23 = thv(11);
    const float sx = uni(hW * t01), sy = uni(hH * (t11 - 1.0f)), sz = uni(hD * t21);

    // XCD-aware column order: blocks b, b+8, b+16, ... share an XCD (and its L2); give each XCD a
    // contiguous slab of columns so that the halo re-reads of neighbouring columns hit the same L2.
    const int ncol = tg.ntx * tg.ntz;
    const int yseg = bx / ncol, cb = bx - yseg * ncol;
    int col = cb;
    if ((ncol & 7) == 0) col = (cb & 7) * (ncol >> 3) + (cb >> 3);
    const int X0 = (col % tg.ntx) * kTX, Z0 = (col / tg.ntx) * kTZ;
    const int nx = min(kTX, W - X0), nz = min(kTZ, D - Z0);
    // per-thread voxel column (x, z); idle lanes are clamped so every load stays in bounds
    const bool act = (lx < nx) && (lz < nz);
    const int x = X0 + (act ? lx : 0), z = Z0 + (act ? lz : 0);
    const float xn = xtab[x], zn = ztab[z];
    const float base_x = unnorm<3>(xn, fW) + hW * fmaf(t00 - 1.0f, xn, fmaf(t02, zn, t03));
    const float base_y = hH * fmaf(t10, xn, fmaf(t12, zn, t13));
    const float base_z = unnorm<3>(zn, fD) + hD * fmaf(t20, xn, fmaf(t22 - 1.0f, zn, t23));

    // Pre-image bounding box of a tile = image of its (X0, Y0, Z0) corner + a tile-independent extent:
    // the map is affine, so extremes sit at corners; d(i_c)/d(voxel step along axis a) = t_ca * S_c / S_a.
    float ext_lo[3], ext_hi[3];
    {
        const float ex[3] = {(float)(kTX - 1), (float)(kTY - 1), (float)(kTZ - 1)};
        const float slope[3][3] = {{t00, t01 * fW / fH, t02 * fW / fD}, {t10 * fH / fW, t11, t12 * fH / fD}, {t20 * fD / fW, t21 * fD / fH, t22}};
#pragma unroll
        for (int c = 0; c < 3; c++) {
            ext_lo[c] = ext_hi[c] = 0.f;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float e = slope[c][a] * ex[a];
                ext_lo[c] += fminf(e, 0.f); ext_hi[c] += fmaxf(e, 0.f);
            }
            ext_lo[c] = uni(ext_lo[c]); ext_hi[c] = uni(ext_hi[c]);
        }
    }
    const float cxn = xtab[X0], czn = ztab[Z0];
    const float corner_x = uni(unnorm<3>(cxn, fW) + hW * fmaf(t00 - 1.0f, cxn, fmaf(t02, czn, t03)));
    const float corner_y = uni(hH * fmaf(t10, cxn, fmaf(t12, czn, t13)));
    const float corner_z = uni(unnorm<3>(czn, fD) + hD * fmaf(t20, cxn, fmaf(t22 - 1.0f, czn, t23)));

    // LDS-DMA slot of a thread in piece 0 (tile independent): box float4 (pz, dy, dx4), pz = 0 .. kPP-1.
    // rb0 = its byte offset from the box origin voxel inside the volume, d0 = packed (dz << 16 | dy << 8 | dx4).
    // Piece k: d = d0 + (kPP k << 16), byte offset rb0 + k * (kPP H W 4).  Spare lanes get dz = 100 (never needed).
    auto slot_geom = [&](int ln, unsigned &rb0, int &d0) {
        const int q = wave * 64 + ln;
        const int pz = q / kPlaneSlots, r = q - pz * kPlaneSlots;
        const int dy = r / kBW4, dx4 = r - dy * kBW4;
        const bool valid = q < kPP * kPlaneSlots;
        rb0 = valid ? (unsigned)((pz * H + dy) * W + dx4 * 4) * 4u : 0u;
        d0 = valid ? ((pz << 16) | (dy << 8) | dx4) : (100 << 16);
    };
    const unsigned piece_stride = (unsigned)(kPP * H * W) * 4u;   // bytes between the pieces of one thread inside the volume
    constexpr int kDShift = (kPP == 2) ? 17 : 18;                  // d of piece k = d0 + (k << kDShift)
    // A needed float4 slot that the DMA does not fetch - outside the volume, or straddling its +x face when W % 4 != 0
    // (global_load_lds_dwordx4 itself takes any 4-byte aligned address) - is filled element by element with zero padding.
    auto fill_slot = [&](float *dst, int gz, int gy, int gx) {
        const bool rowin = ((unsigned)gz < (unsigned)D) && ((unsigned)gy < (unsigned)H);
        const float *row = mov + ((size_t)(rowin ? gz : 0) * H + (rowin ? gy : 0)) * W;
        float4 v;
        v.x = (rowin && (unsigned)(gx + 0) < (unsigned)W) ? row[gx + 0] : 0.f;
        v.y = (rowin && (unsigned)(gx + 1) < (unsigned)W) ? row[gx + 1] : 0.f;
        v.z = (rowin && (unsigned)(gx + 2) < (unsigned)W) ? row[gx + 2] : 0.f;
        v.w = (rowin && (unsigned)(gx + 3) < (unsigned)W) ? row[gx + 3] : 0.f;
        *reinterpret_cast<float4 *>(dst) = v;
    };
    static_assert(kPP == 2 || kPP == 4, "piece planes");

    F1Acc acc;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc.AB[q][c] = (f2)(0.f);
    acc.M01 = acc.M23 = (f2)(0.f);
    acc.M4 = 0.f;
    const int j0 = lh * kRows;                              // first row of this thread's half
    const int toff = (z * H + j0) * W + x;                  // this thread's target offset inside a tile's row block

    // Geometry of up to 64 tiles at a time, ONE TILE PER LANE (the per-tile cost is then a few
    // v_readlane instead of ~40 VALU instructions): box origin, needed extent, fits / interior flags.
    const int ty_begin = yseg * tg.tiles_per_seg, ty_end = min((yseg + 1) * tg.tiles_per_seg, tg.nty);
    int g_ox = 0, g_oy = 0, g_oz = 0, g_pk = 0;
    auto lane_geometry = [&](int ty_first) {
        const int ty = min(ty_first + lane, tg.nty - 1);
        const float yn0 = ytab[ty * kTY], yid0 = unnorm<3>(yn0, fH);
        const float cx = fmaf(sx, yn0, corner_x), cy = yid0 + fmaf(sy, yn0, corner_y), cz = fmaf(sz, yn0, corner_z);
        const float slack = 0.05f;   // fp32 rounding + table non-uniformity of interior points vs the corner + extent bound
        bool fits = (fabsf(cx) < 1.0e6f) && (fabsf(cy) < 1.0e6f) && (fabsf(cz) < 1.0e6f);   // also rejects NaN
        int ox = 0, oy = 0, oz = 0, ex4 = 0, ey = 0, ez = 0;
        bool interior = false;
        if (fits) {
            const int lx0 = (int)floorf(cx + ext_lo[0] - slack), hx1 = (int)floorf(cx + ext_hi[0] + slack) + 1;
            oy = (int)floorf(cy + ext_lo[1] - slack); const int hy1 = (int)floorf(cy + ext_hi[1] + slack) + 1;
            oz = (int)floorf(cz + ext_lo[2] - slack); const int hz1 = (int)floorf(cz + ext_hi[2] + slack) + 1;
            ox = lx0 & ~3;
            ex4 = ((hx1 - ox) >> 2) + 1; ey = hy1 - oy + 1; ez = hz1 - oz + 1;
            fits = (ex4 <= kBW4) && (ey <= kBH) && (ez <= kBD);
            // the whole box capacity lies inside the volume: no zero padding needed for this tile
            interior = (ox >= 0) && (oy >= 0) && (oz >= 0) && (ox + kBW <= W) && (oy + kBH <= H) && (oz + kBD <= D);
        }
        g_ox = ox; g_oy = oy; g_oz = oz;
        g_pk = fits ? ((ex4 - 1) | ((ey - 1) << 8) | ((ez - 1) << 16) | (1 << 24) | ((interior ? 1 : 0) << 25)) : 0;
    };
    int ty = ty_begin;
    // ================= fast loop: full 16-row tiles whose box fits =================
    // No per-lane branch around the accumulation: lanes outside a partial x / z tile work on the clamped
    // column (x, z) = (X0, Z0) - every address stays valid - and their sums are discarded after the loop, so
    // the 23 packed accumulators live in one set of registers with no copies at control-flow joins.
    // The VALU is the busiest unit of this kernel (rocprof: ~70 % issue utilisation), so the loop is written to
    // the instruction: addresses that are (uniform base + per-thread 32-bit offset) use the SGPR-base form of
    // global_load (no VALU address arithmetic), per-row constants stay in SGPRs, the LDS address is a
    // shift-add + two mad24 with SGPR strides.
    {
        const unsigned toffb = (unsigned)toff * 4u;
        const unsigned lane7b = (unsigned)(lane & (kRows - 1)) * 4u;
        float sxv, syv, szv;   // VGPR copies of the uniform slopes: the per-row yn can then be the (single) SGPR operand
        asm("v_mov_b32 %0, %1" : "=v"(sxv) : "s"(sx));
        asm("v_mov_b32 %0, %1" : "=v"(syv) : "s"(sy));
        asm("v_mov_b32 %0, %1" : "=v"(szv) : "s"(sz));
        int ys_s, zs_s;        // LDS strides (bytes) pinned in SGPRs: gfx9 VOP3 takes no literal operand
        asm("s_mov_b32 %0, %1" : "=s"(ys_s) : "i"(kBW * 4));
        asm("s_mov_b32 %0, %1" : "=s"(zs_s) : "i"(kBW * kBH * 4));
        const unsigned box_lds = (unsigned)(uintptr_t)box;   // LDS byte address of the box
        unsigned rb0;                                        // byte offset of this thread's piece-0 DMA slot
        {
            int d0;
            slot_geom(lane, rb0, d0);
        }
        // More than 8 pieces (GeomR's deep box): one exec mask per piece would not fit the SGPR file (the reloads cost 18 %), but the
        // masks are structured - lane (pz, dy, dx4) of piece k fetches iff its (dy, dx4) is wanted and plane 2k + pz is: two masks
        // (pz = 0 / 1 lanes with a wanted (dy, dx4)) and one bit per box plane rebuild each piece's mask with scalar instructions.
        constexpr bool kZMask = kPieces > 8;
        static_assert(!kZMask || (kPP == 2 && kBD <= 32), "plane-bit masks: pieces of two planes");
        constexpr int kNM = kZMask ? 1 : kPieces;
        unsigned long long m_ld[kNM];                        // cached exec masks of the DMA pieces (wave-uniform)
#pragma unroll
        for (int k = 0; k < kNM; k++) m_ld[k] = 0;
        unsigned long long m_a0 = 0, m_a1 = 0;               // kZMask: lanes of plane 0 / 1 of a piece whose (dy, dx4) is fetched
        unsigned m_zb = 0;                                   // kZMask: bit z = box plane z is fetched
        unsigned m_oob = 0;                                  // bit k: slot k of this thread is needed but outside the volume
        unsigned m_part = 0;                                 // bit k: slot k straddles x = W (W % 4 != 0): zero its tail after landing
        // Fetched extent = the LARGEST pre-image extent any tile of this theta can have (capped at the box): the exact
        // extent of a tile flips between two values with the fractional position of its corner, and every change
        // would invalidate the cached masks; one extra row / plane / float4 of DMA is cheaper than that.
        int lim_blk;
        {
            const float slack2 = 0.1f;
            const int ex4m = (((int)floorf(ext_hi[0] - ext_lo[0] + slack2) + 5) >> 2) + 1;   // hx1 - lx0 <= floor(span) + 2, + 3 of alignment
            const int eym = (int)floorf(ext_hi[1] - ext_lo[1] + slack2) + 3, ezm = (int)floorf(ext_hi[2] - ext_lo[2] + slack2) + 3;
            lim_blk = __builtin_amdgcn_readfirstlane(((min(ezm, kBD) - 1) << 16) | ((min(eym, kBH) - 1) << 8) | (min(ex4m, kBW4) - 1));
        }
        int m_lim = -1, m_lo = -1, m_hi = -1, m_px = -2;
        TRX_TM_INIT();
        typedef const __attribute__((address_space(3))) f2u *lds_f2;
        // Tiles come in chunks of 64 (geometry: one tile per lane); the leading run of fast tiles of a chunk is a plain
        // counted loop - no exit in the middle, so the accumulators stay in one register set.
        while (ty < ty_end) {
          lane_geometry(ty);
          const int chunk = min(64, ty_end - ty);
          // W % 4 != 0: a tile whose needed extent reaches the float4 that straddles x = W (only columns at the +x face)
          // (the straddling float4 of a row is fetched whole, i.e. up to 12 bytes into the next row - except on the last row
          // of the volume, where that would leave the allocation: that one tile per pair goes to the generic loop)
          const bool xpart = ((W & 3) != 0) && (g_ox + 4 * ((lim_blk & 0xff) + 1) > W - (W & 3)) &&
                             (g_oy + ((lim_blk >> 8) & 0xff) >= H - 1) && (g_oz + (lim_blk >> 16) >= D - 1);
          const bool ok = (lane < chunk) && ((g_pk >> 24) & 1) && ((ty + lane + 1) * kTY <= H) && !xpart;
          const unsigned long long bad = ~__builtin_amdgcn_ballot_w64(ok);
          const int nf = bad ? __builtin_ctzll(bad) : 64;
          // ---- box of fast tile `g` of this chunk -> LDS buffer `buf`: refresh the cached exec masks if the tile's slot
          // range changed, issue the DMA pieces (no wait), zero-fill needed cells that lie outside the volume.
          const char *dma_base = nullptr;   // of the box prepared last by issue_box (for piece-wise issue)
          unsigned dma_lds = 0;
          auto issue_box = [&](int g, int buf, bool spread) {
              const int ox = __builtin_amdgcn_readlane(g_ox, g), oy = __builtin_amdgcn_readlane(g_oy, g), oz = __builtin_amdgcn_readlane(g_oz, g);
              const int lim = lim_blk;         // (ez-1) << 16 | (ey-1) << 8 | (ex4-1)
              const int loz = max(0, -oz), loy = max(0, -oy), lox = max(0, -(ox >> 2));
              const int hiz = min(lim >> 16, D - 1 - oz), hiy = min((lim >> 8) & 0xff, H - 1 - oy), hix = min(lim & 0xff, ((W - ox + 3) >> 2) - 1);   // includes the float4 straddling x = W (W % 4 != 0)
              const bool none = (hiz < loz) || (hiy < loy) || (hix < lox);   // the whole pre-image lies outside the volume
              const int lo = none ? 0x7f7f7f : ((loz << 16) | (loy << 8) | lox);
              const int hi = none ? 0 : ((hiz << 16) | (hiy << 8) | hix);
              // float4 index of the slot straddling x = W (W % 4 != 0) if this tile fetches it.  It moves with ox, so it is part of
              // the cache key: two tiles of a column can share (lim, lo, hi) while the straddler sits in different slots.
              const int part_x = ((W & 3) && !none && ((W - ox) >> 2) <= hix) ? ((W - ox) >> 2) : -1;
              if (lim != m_lim || lo != m_lo || hi != m_hi || part_x != m_px) {
                  m_lim = lim; m_lo = lo; m_hi = hi; m_px = part_x;
                  m_oob = 0;
                  m_part = 0;
                  int ln = lane;   // opaque copy: keeps the slot decode inside this (rarely taken) branch
                  asm volatile("" : "+v"(ln));
                  unsigned rbx;
                  int d0;
                  slot_geom(ln, rbx, d0);
#pragma unroll
                  for (int k = 0; k < kPieces; k++) {   // per-field compares on the packed (dz, dy, dx4): no field may borrow
                      const int d = d0 + (k << kDShift);
                      const bool need = (((lim - d) & 0x80808080) == 0);
                      const bool ld = need && (((hi - d) & 0x80808080) == 0) && (((d - lo) & 0x80808080) == 0);
                      if constexpr (!kZMask) m_ld[k] = __builtin_amdgcn_ballot_w64(ld);
                      if (need && !ld) m_oob |= 1u << k;
                      if (ld && (d & 0xff) == part_x) m_part |= 1u << k;   // fetched whole; its tail past x = W is zeroed after landing
                  }
                  if constexpr (kZMask) {
                      const int dyx = d0 & 0xffff;
                      const bool xy = (((((lim & 0xffff) - dyx) | ((hi & 0xffff) - dyx) | (dyx - (lo & 0xffff))) & 0x8080) == 0);
                      m_a0 = __builtin_amdgcn_ballot_w64(xy && (d0 >> 16) == 0);
                      m_a1 = __builtin_amdgcn_ballot_w64(xy && (d0 >> 16) == 1);
                      m_zb = (unsigned)__builtin_amdgcn_readfirstlane((int)(none ? 0u : (((2u << hiz) - 1u) & ~((1u << loz) - 1u))));   // hiz <= the needed depth by construction
                  }
              }
              dma_base = reinterpret_cast<const char *>(mov + (ptrdiff_t)((oz * H + oy) * W + ox));   // uniform; may point below `mov` (those lanes are masked)
              dma_lds = box_lds + (unsigned)buf * (kBoxFloats * 4u) + (unsigned)wave * 1024u;
              if (TRX_DBG_SKIP != 2 && !spread) {
                  const float *mbase = reinterpret_cast<const float *>(dma_base);
                  const unsigned lds0 = dma_lds;
                  unsigned long long sv;
                  unsigned m0s;
                  static_assert((kPieces >= 6 && kPieces <= 8) || (kPieces >= 9 && kPieces <= 13), "the DMA block below is written for 6, 7, 8 or 9..13 pieces");
                  // one exec mask + one SGPR-base load per piece; s[100:101] walks the volume by kPP planes per piece
#define TRX_DMA_SKIP "s_cbranch_execz 1f\n\t"   // a piece none of whose lanes fetch is branched over (an LDS-DMA with exec = 0 still costs its issue)
#define TRX_DMA_NEXT(K)                                  \
    "s_add_u32 s100, s100, %[vstr]\n\t"                  \
    "s_addc_u32 s101, s101, 0\n\t"                       \
    "s_add_u32 m0, m0, %[pstr]\n\t"                      \
    "s_mov_b64 exec, %[k" #K "]\n\t"                     \
    TRX_DMA_SKIP                                         \
    "global_load_lds_dwordx4 %[off], s[100:101]" TRX_BOX_POLICY "\n\t" \
    "1:\n\t"
#define TRX_DMA_HEAD                                     \
    "s_mov_b64 %[sv], exec\n\t"                          \
    "s_mov_b32 %[m0s], m0\n\t"                           \
    "s_mov_b64 s[100:101], %[base]\n\t"                  \
    "s_mov_b32 m0, %[lds]\n\t"                           \
    "s_mov_b64 exec, %[k0]\n\t"                          \
    TRX_DMA_SKIP                                         \
    "global_load_lds_dwordx4 %[off], s[100:101]" TRX_BOX_POLICY "\n\t"     \
    "1:\n\t"                                             \
    TRX_DMA_NEXT(1) TRX_DMA_NEXT(2) TRX_DMA_NEXT(3) TRX_DMA_NEXT(4) TRX_DMA_NEXT(5)
#define TRX_DMA_TAIL "s_mov_b64 exec, %[sv]\n\t" "s_mov_b32 m0, %[m0s]"
                  if constexpr (kZMask) {
                      static_assert(kPieces <= 13, "plane-bit DMA block: up to 13 pieces (the plane bits of pieces a shallower box lacks are never set)");
                      unsigned long long t0, t1;
#define TRX_DMA_ZSEL(B0, B1)                             \
    "s_bitcmp1_b32 %[zb], " #B0 "\n\t"                   \
    "s_cselect_b64 %[t0], %[a0], 0\n\t"                 \
    "s_bitcmp1_b32 %[zb], " #B1 "\n\t"                   \
    "s_cselect_b64 %[t1], %[a1], 0\n\t"                 \
    "s_or_b64 exec, %[t0], %[t1]\n\t"                   \
    "s_cbranch_execz 1f\n\t"                            \
    "global_load_lds_dwordx4 %[off], s[100:101]" TRX_BOX_POLICY "\n\t" \
    "1:\n\t"
#define TRX_DMA_ZNEXT(B0, B1)                            \
    "s_add_u32 s100, s100, %[vstr]\n\t"                 \
    "s_addc_u32 s101, s101, 0\n\t"                      \
    "s_add_u32 m0, m0, %[pstr]\n\t" TRX_DMA_ZSEL(B0, B1)
                      asm volatile("s_mov_b64 %[sv], exec\n\t"
                                   "s_mov_b32 %[m0s], m0\n\t"
                                   "s_mov_b64 s[100:101], %[base]\n\t"
                                   "s_mov_b32 m0, %[lds]\n\t" TRX_DMA_ZSEL(0, 1)
                                   TRX_DMA_ZNEXT(2, 3) TRX_DMA_ZNEXT(4, 5) TRX_DMA_ZNEXT(6, 7) TRX_DMA_ZNEXT(8, 9) TRX_DMA_ZNEXT(10, 11)
                                   TRX_DMA_ZNEXT(12, 13) TRX_DMA_ZNEXT(14, 15) TRX_DMA_ZNEXT(16, 17) TRX_DMA_ZNEXT(18, 19)
                                   TRX_DMA_ZNEXT(20, 21) TRX_DMA_ZNEXT(22, 23) TRX_DMA_ZNEXT(24, 25) TRX_DMA_TAIL
                                   : [sv] "=&s"(sv), [m0s] "=&s"(m0s), [t0] "=&s"(t0), [t1] "=&s"(t1)
                                   : [lds] "s"(lds0), [base] "s"(mbase), [pstr] "i"(kPieceFloats * 4), [vstr] "s"(piece_stride), [off] "v"(rb0),
                                     [a0] "s"(m_a0), [a1] "s"(m_a1), [zb] "s"(__builtin_amdgcn_readfirstlane((int)m_zb))
                                   : "memory", "scc", "s100", "s101");
#undef TRX_DMA_ZSEL
#undef TRX_DMA_ZNEXT
                  } else if constexpr (kPieces == 8) {
                      asm volatile(TRX_DMA_HEAD TRX_DMA_NEXT(6) TRX_DMA_NEXT(7) TRX_DMA_TAIL
                                   : [sv] "=&s"(sv), [m0s] "=&s"(m0s)
                                   : [lds] "s"(lds0), [base] "s"(mbase), [pstr] "i"(kPieceFloats * 4), [vstr] "s"(piece_stride), [off] "v"(rb0),
                                     [k0] "s"(m_ld[0]), [k1] "s"(m_ld[1]), [k2] "s"(m_ld[2]), [k3] "s"(m_ld[3]), [k4] "s"(m_ld[4]),
                                     [k5] "s"(m_ld[5]), [k6] "s"(m_ld[kPieces > 6 ? 6 : 0]), [k7] "s"(m_ld[kPieces - 1])
                                   : "memory", "scc", "s100", "s101");
                  } else if constexpr (kPieces == 7) {
                      asm volatile(TRX_DMA_HEAD TRX_DMA_NEXT(6) TRX_DMA_TAIL
                                   : [sv] "=&s"(sv), [m0s] "=&s"(m0s)
                                   : [lds] "s"(lds0), [base] "s"(mbase), [pstr] "i"(kPieceFloats * 4), [vstr] "s"(piece_stride), [off] "v"(rb0),
                                     [k0] "s"(m_ld[0]), [k1] "s"(m_ld[1]), [k2] "s"(m_ld[2]), [k3] "s"(m_ld[3]), [k4] "s"(m_ld[4]),
                                     [k5] "s"(m_ld[5]), [k6] "s"(m_ld[kPieces - 1])
                                   : "memory", "scc", "s100", "s101");
                  } else {
                      asm volatile(TRX_DMA_HEAD TRX_DMA_TAIL
                                   : [sv] "=&s"(sv), [m0s] "=&s"(m0s)
                                   : [lds] "s"(lds0), [base] "s"(mbase), [pstr] "i"(kPieceFloats * 4), [vstr] "s"(piece_stride), [off] "v"(rb0),
                                     [k0] "s"(m_ld[0]), [k1] "s"(m_ld[1]), [k2] "s"(m_ld[2]), [k3] "s"(m_ld[3]), [k4] "s"(m_ld[4]),
                                     [k5] "s"(m_ld[5])
                                   : "memory", "scc", "s100", "s101");
                  }
#undef TRX_DMA_NEXT
#undef TRX_DMA_SKIP
#undef TRX_DMA_HEAD
#undef TRX_DMA_TAIL
              }
              if (m_oob) {   // zero padding: needed cells outside the volume (tiles at a volume face only)
                  float zero;
                  asm volatile("v_mov_b32 %0, 0" : "=v"(zero));   // materialised here, not kept live across the loop
#pragma unroll
                  for (int k = 0; k < kPieces; k++)
                      if (m_oob & (1u << k))
                          *reinterpret_cast<float4 *>(box + buf * kBoxFloats + k * kPieceFloats + (wave * 64 + lane) * 4) = make_float4(zero, zero, zero, zero);
              }
          };
          // W % 4 != 0: the float4 that straddles the +x face was fetched whole (its tail belongs to the next row): zero the tail
          auto zero_tails = [&](int buf) {
#pragma unroll
              for (int k = 0; k < kPieces; k++)
                  if (m_part & (1u << k)) {
                      float *sl = box + buf * kBoxFloats + k * kPieceFloats + (wave * 64 + lane) * 4;
                      for (int e = W & 3; e < 4; e++) sl[e] = 0.f;
                  }
          };
          // one DMA piece of the box prepared by issue_box(.., spread = true): issued between the rows of the gather so that
          // the TA drains the pieces (64 B/clk per CU) while the VALU works, instead of every wave queueing all of them first
          auto issue_piece = [&](int k) {
              if (TRX_DBG_SKIP == 2) return;
              unsigned long long sv;
              unsigned m0s;
              asm volatile("s_mov_b64 %[sv], exec\n\t"
                           "s_mov_b32 %[m0s], m0\n\t"
                           "s_mov_b32 m0, %[lds]\n\t"
                           "s_mov_b64 exec, %[mk]\n\t"
                           "global_load_lds_dwordx4 %[off], %[base]\n\t"
                           "s_mov_b64 exec, %[sv]\n\t"
                           "s_mov_b32 m0, %[m0s]"
                           : [sv] "=&s"(sv), [m0s] "=&s"(m0s)
                           : [lds] "s"(dma_lds + (unsigned)k * (kPieceFloats * 4u)), [base] "s"(dma_base + (size_t)k * piece_stride), [off] "v"(rb0),
                             [mk] "s"(kZMask ? ((((m_zb >> (2 * k)) & 1u) ? m_a0 : 0ull) | (((m_zb >> (2 * k + 1)) & 1u) ? m_a1 : 0ull)) : m_ld[kZMask ? 0 : k])
                           : "memory");
          };
          // ---- the 8 rows of this thread in fast tile `g`, gathered from LDS buffer `buf`.  tnext != nullptr: after row j is
          // consumed, row j of the tile at `tnext` is fetched into the same register (target prefetch without extra VGPRs).
          auto gather_tile = [&](int g, int buf, float yn_l, float yid_l, float (&tv)[kRows], const float *tnext, bool dma_next) {
              const int Y0 = (ty + g) * kTY;
              const int ox = __builtin_amdgcn_readlane(g_ox, g), oy = __builtin_amdgcn_readlane(g_oy, g), oz = __builtin_amdgcn_readlane(g_oz, g);
              float yn_r[kRows], yid_r[kRows];
#pragma unroll
              for (int j = 0; j < kRows; j++) { yn_r[j] = lane_bcast(yn_l, j); yid_r[j] = lane_bcast(yid_l, j); }
              if (TRX_DBG_SKIP == 1) return;
              const int bpb = (int)box_lds + buf * (kBoxFloats * 4) - ((oz * kBH + oy) * kBW + ox) * 4;   // LDS byte address of voxel (0,0,0) of the volume
              // software pipeline: the 4 LDS reads of row j+1 are issued before the arithmetic of row j
              struct Fetch { f2 r00, r01, r10, r11; float fx, fy, fz; };
              auto fetch = [&](int j) -> Fetch {
                  const float yn = yn_r[j];
                  const float ix = fmaf(sxv, yn, base_x);
                  const float iy = yid_r[j] + fmaf(syv, yn, base_y);
                  const float iz = fmaf(szv, yn, base_z);
                  int a0, a1, a2, a3;
                  asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a0) : "v"(floor_to_int(ix)), "s"(bpb));
                  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(a1) : "v"(floor_to_int(iy)), "s"(ys_s), "v"(a0));
                  asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(a2) : "v"(floor_to_int(iz)), "s"(zs_s), "v"(a1));
                  asm("v_add_u32 %0, %1, %2" : "=v"(a3) : "s"(zs_s), "v"(a2));
                  Fetch f;
                  f.r00 = *(lds_f2)(unsigned)a2; f.r01 = *(lds_f2)(unsigned)(a2 + kBW * 4);
                  f.r10 = *(lds_f2)(unsigned)a3; f.r11 = *(lds_f2)(unsigned)(a3 + kBW * 4);
                  f.fx = __builtin_amdgcn_fractf(ix); f.fy = __builtin_amdgcn_fractf(iy); f.fz = __builtin_amdgcn_fractf(iz);
                  return f;
              };
              Fetch cur = fetch(0);
#pragma unroll
              for (int j = 0; j < kRows; j++) {
                  Fetch nxt;
                  if (j + 1 < kRows) nxt = fetch(j + 1);
                  if (kBufs == 2 && j < kPieces && dma_next) issue_piece(j);
                  const Samp3 sm = lerp3_pairs<kGrad>(cur.r00, cur.r01, cur.r10, cur.r11, cur.fx, cur.fy, cur.fz);
                  if constexpr (MODE == 3) { if (act) wout[(size_t)Y0 * W + (unsigned)(toff + j * W)] = sm.v; }
                  else f1_accumulate_pk<MODE>(sm, tv[j], yn_r[j], acc);
                  if (kBufs == 2 && TRX_DBG_SKIP != 3 && MODE != 3)
                      asm volatile("global_load_dword %0, %1, %2" : "=v"(tv[j]) : "v"(toffb), "s"(tnext + (size_t)j * W));
                  if (j + 1 < kRows) cur = nxt;
              }
          };
          auto load_targets = [&](int g, float (&tv)[kRows]) {
              const float *trow = tgt + (size_t)(ty + g) * kTY * W;   // uniform (toffb holds the row offset of this half)
#pragma unroll
              for (int j = 0; j < kRows; j++) {
                  if (TRX_DBG_SKIP == 3 || MODE == 3) tv[j] = 1.f;
                  else asm volatile("global_load_dword %0, %1, %2" TRX_TGT_POLICY : "=v"(tv[j]) : "v"(toffb), "s"(trow + (size_t)j * W) : "memory");
              }
          };
          float tv[kRows];
          if constexpr (kBufs == 1) {
            // one box, two blocks per CU: burst - wait - barrier - gather - barrier
            for (int gl = 0; gl < nf; gl++) {
              TRX_TM_STAMP(tm0);
              // row tables of this wave's 8 rows in lanes 0..7 (broadcast in gather_tile with constant-lane v_readlane)
              float yn_l;
              asm volatile("global_load_dword %0, %1, %2" : "=v"(yn_l) : "v"(lane7b), "s"(ytab + (ty + gl) * kTY + j0) : "memory");
              __builtin_amdgcn_s_setprio(TRX_STAGE_PRIO);
              load_targets(gl, tv);
              issue_box(gl, 0, false);
              __builtin_amdgcn_s_setprio(0);
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // box pieces and the target column have landed
              if (m_part) zero_tails(0);
              {
#pragma unroll
                  for (int j = 0; j < kRows; j++) asm volatile("" : "+v"(tv[j]));
                  asm volatile("" : "+v"(yn_l));
              }
              const float yid_l = unnorm<3>(yn_l, fH);
              TRX_TM_STAMP(tm1);
              __syncthreads();
              TRX_TM_STAMP(tm2);
              gather_tile(gl, 0, yn_l, yid_l, tv, nullptr, false);
              TRX_TM_STAMP(tm3);
              __syncthreads();   // the box is overwritten by the next tile
              TRX_TM_TILE_DONE();
            }
          } else {
            // two boxes, one block per CU: the DMA of tile g+1 (and, row by row, its target column) is in flight while
            // tile g is gathered; one barrier per tile (it also tells that every wave is done with the other box)
            if (nf > 0) {
                load_targets(0, tv);
                issue_box(0, 0, false);
            }
            for (int gl = 0; gl < nf; gl++) {
              TRX_TM_STAMP(tm0);
              float yn_l;
              asm volatile("global_load_dword %0, %1, %2" : "=v"(yn_l) : "v"(lane7b), "s"(ytab + (ty + gl) * kTY + j0) : "memory");
              asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this tile's box pieces (issued one tile ago) and target column
              if (m_part) zero_tails(gl & 1);
              {
#pragma unroll
                  for (int j = 0; j < kRows; j++) asm volatile("" : "+v"(tv[j]));
                  asm volatile("" : "+v"(yn_l));
              }
              const float yid_l = unnorm<3>(yn_l, fH);
              TRX_TM_STAMP(tm1);
              __syncthreads();
              TRX_TM_STAMP(tm2);
              const int gn = (gl + 1 < nf) ? gl + 1 : gl;
              if (gl + 1 < nf) issue_box(gl + 1, (gl + 1) & 1, true);
              TRX_TM_STAMP(tm3);
              gather_tile(gl, gl & 1, yn_l, yid_l, tv, tgt + (size_t)(ty + gn) * kTY * W, gl + 1 < nf);
              TRX_TM_TILE_DONE();
            }
            // the prefetch issued during the last tile is still in flight: its destination registers must not be reused,
            // and the generic loop below must not overwrite box 0 while a slower wave still gathers from it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < kRows; j++) asm volatile("" : "+v"(tv[j]));
            __syncthreads();
          }
          ty += nf;
          if (nf < chunk) break;   // the generic loop takes over at tile ty (same 64-tile chunking, geometry already in g_*)
        }
        TRX_TM_STORE();
        if (!act) {
#pragma unroll
            for (int q = 0; q < 3; q++)
#pragma unroll
                for (int c = 0; c < 3; c++) acc.AB[q][c] = (f2)(0.f);
            acc.M01 = acc.M23 = (f2)(0.f);
            acc.M4 = 0.f;
        }
    }

    // slot geometry for the generic loop, recomputed here from an opaque copy of the lane id so that it is not
    // live across the fast loop
    unsigned rb0;
    int d0;
    {
        int ln = lane;
        asm volatile("" : "+v"(ln));
        slot_geom(ln, rb0, d0);
    }
    int prev_lim = -1;
    unsigned needmask = 0;    // bit k: DMA slot k of this thread lies inside the needed extent of the current tile

    // ---- box of one tile straight into LDS (LDS-DMA, no staging VGPRs); returns after the data has landed (this
    // wave's part: the caller still needs the block barrier).  Only the float4 slots inside the tile's actual pre-image
    // extent (ex4 x ey x ez) are fetched: lanes outside it are masked off, so the bytes a CU ingests track the need,
    // not the box capacity.
    auto stage_box = [&](int pk, int ox, int oy, int oz) {
        const bool interior = (pk >> 25) & 1;
        const int lim = pk & 0xffffff;   // (ez-1) << 16 | (ey-1) << 8 | (ex4-1)
        if (lim != prev_lim) {           // extents rarely change along a column: refresh the slot mask only then
            prev_lim = lim;
            needmask = 0;
#pragma unroll
            for (int k = 0; k < kPieces; k++)   // per-field compare (dz,dy,dx4) <= lim: no field of lim-d may borrow
                if (((lim - (d0 + (k << kDShift))) & 0x80808080) == 0) needmask |= 1u << k;
        }
        const int obase = (oz * H + oy) * W + ox;
        unsigned oob = 0;   // bit k: slot k of this thread is needed but lies outside the volume
        if (interior) {
            const char *__restrict__ mbase = reinterpret_cast<const char *>(mov + obase);    // uniform; obase >= 0 here
#pragma unroll
            for (int k = 0; k < kPieces; k++)
                if ((needmask & (1u << k)) && TRX_DBG_SKIP != 2)
                    __builtin_amdgcn_global_load_lds(reinterpret_cast<const float *>(mbase + (size_t)k * piece_stride + rb0),
                                                     box + k * kPieceFloats + wave * 256, 16, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < kPieces; k++)
                if ((needmask & (1u << k)) && TRX_DBG_SKIP != 2) {
                    const int d = d0 + (k << kDShift);
                    const int gz = oz + (d >> 16), gy = oy + ((d >> 8) & 0xff), gx = ox + (d & 0xff) * 4;
                    const bool inb = ((unsigned)gz < (unsigned)D) && ((unsigned)gy < (unsigned)H) && (gx >= 0) && (gx + 4 <= W);   // whole slot inside
                    const unsigned idx = inb ? (unsigned)(obase + (int)((rb0 + k * piece_stride) >> 2)) : 0u;
                    if (!inb) oob |= 1u << k;
                    __builtin_amdgcn_global_load_lds(mov + idx, box + k * kPieceFloats + wave * 256, 16, 0, 0);
                }
        }
        __builtin_amdgcn_s_setprio(0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (oob) {   // slots the DMA skipped (boundary tiles only): zero padding / partial rows
#pragma unroll
            for (int k = 0; k < kPieces; k++)
                if (oob & (1u << k)) {
                    const int d = d0 + (k << kDShift);
                    fill_slot(box + k * kPieceFloats + (wave * 64 + lane) * 4, oz + (d >> 16), oy + ((d >> 8) & 0xff), ox + (d & 0xff) * 4);
                }
        }
    };
    // ---- one voxel gathered from the LDS box: coordinates, 4 paired reads, trilinear value (+ gradient)
    auto gather = [&](const float *bp, float yn, float yid) -> Samp3 {
        const float ix = fmaf(sx, yn, base_x);
        const float iy = yid + fmaf(sy, yn, base_y);
        const float iz = fmaf(sz, yn, base_z);
        const int a = __mul24(floor_to_int(iz), kBH * kBW) + __mul24(floor_to_int(iy), kBW) + floor_to_int(ix);
        const float *p = bp + a;
        const f2 r00 = *reinterpret_cast<const f2u *>(p), r01 = *reinterpret_cast<const f2u *>(p + kBW);
        const f2 r10 = *reinterpret_cast<const f2u *>(p + kBW * kBH), r11 = *reinterpret_cast<const f2u *>(p + kBW * kBH + kBW);
        return lerp3_pairs<kGrad>(r00, r01, r10, r11, __builtin_amdgcn_fractf(ix), __builtin_amdgcn_fractf(iy), __builtin_amdgcn_fractf(iz));
    };

    // ================= generic loop: partial last tile, tiles whose box does not fit, W % 4 != 0 =================
    for (; ty < ty_end; ty++) {
        const int gl = (ty - ty_begin) & 63;
        if (gl == 0) lane_geometry(ty);
        const int Y0 = ty * kTY;
        const int ny = min(kTY, H - Y0);
        // row tables of this tile, one row per lane (lanes 0..15), broadcast later with v_readlane
        const float yn_l = ytab[Y0 + min(lane & (kTY - 1), ny - 1)];
        const float yid_l = unnorm<3>(yn_l, fH);
        const int pk = __builtin_amdgcn_readlane(g_pk, gl);
        const int ox = __builtin_amdgcn_readlane(g_ox, gl), oy = __builtin_amdgcn_readlane(g_oy, gl), oz = __builtin_amdgcn_readlane(g_oz, gl);
        const bool fits = (pk >> 24) & 1;
        const float *__restrict__ trow = tgt + (size_t)Y0 * W;   // uniform base of this tile's target rows

        if (fits) {
            // staging waves outrank the co-resident block's gather waves: their loads should enter the memory
            // system as early as possible, the VALU work they displace is short
            __builtin_amdgcn_s_setprio(TRX_STAGE_PRIO);
            float tv[kRows];
#pragma unroll
            for (int j = 0; j < kRows; j++)
                tv[j] = (TRX_DBG_SKIP == 3 || MODE == 3) ? 1.f : trow[(unsigned)(toff + (min(j0 + j, ny - 1) - j0) * W)];
            stage_box(pk, ox, oy, oz);
            __syncthreads();
            // wave-uniform row constants of this wave's half (rows j0 .. j0+7) -> SGPRs.  The v_readlane MUST
            // run here, in uniform control flow: inside `if (act)` lanes 0..15 may be inactive (partial x tile)
            // and the compiler is free to sink the computation of yn_l / yid_l into that branch.
            float yn_r[kRows], yid_r[kRows];
#pragma unroll
            for (int j = 0; j < kRows; j++) { yn_r[j] = lane_bcast(yn_l, j0 + j); yid_r[j] = lane_bcast(yid_l, j0 + j); }
            if (act && TRX_DBG_SKIP != 1) {
                const float *bp = box - ((oz * kBH + oy) * kBW + ox);
#pragma unroll
                for (int j = 0; j < kRows; j++)
                    if (j0 + j < ny) {
                        const Samp3 sm = gather(bp, yn_r[j], yid_r[j]);
                        if constexpr (MODE == 3) wout[(size_t)Y0 * W + (unsigned)(toff + j * W)] = sm.v;
                        else f1_accumulate_pk<MODE>(sm, tv[j], yn_r[j], acc);
                    }
            }
            __syncthreads();   // the box is overwritten by the next tile
        } else if (act) {
            // large deformation (or W % 4 != 0): gather straight from global memory (L2), two rows in flight:
            // the 4 pair loads + the target of row j+1 are issued before the arithmetic of row j
            struct GFetch { f2 r00, r01, r10, r11; float fx, fy, fz, yn, yv; };
            auto gfetch = [&](int j) -> GFetch {
                GFetch g;
                g.yn = ytab[Y0 + j];
                const float ix = fmaf(sx, g.yn, base_x);
                const float iy = unnorm<3>(g.yn, fH) + fmaf(sy, g.yn, base_y);
                const float iz = fmaf(sz, g.yn, base_z);
                const float flx = floorf(ix), fly = floorf(iy), flz = floorf(iz);
                g.fx = ix - flx; g.fy = iy - fly; g.fz = iz - flz;
                const int x0 = (int)flx, y0 = (int)fly, z0 = (int)flz;
                const bool interior = ((unsigned)x0 < (unsigned)(W - 1)) & ((unsigned)y0 < (unsigned)(H - 1)) & ((unsigned)z0 < (unsigned)(D - 1));
                if (__all(interior)) {
                    const float *p = mov + ((size_t)z0 * H + y0) * W + x0, *q = p + (size_t)H * W;
                    g.r00 = *reinterpret_cast<const f2u *>(p); g.r01 = *reinterpret_cast<const f2u *>(p + W);
                    g.r10 = *reinterpret_cast<const f2u *>(q); g.r11 = *reinterpret_cast<const f2u *>(q + W);
                } else {
                    const int x1 = x0 + 1, y1 = y0 + 1, z1 = z0 + 1;
                    const bool bx0 = (unsigned)x0 < (unsigned)W, bx1 = (unsigned)x1 < (unsigned)W;
                    const bool by0 = (unsigned)y0 < (unsigned)H, by1 = (unsigned)y1 < (unsigned)H;
                    const bool bz0 = (unsigned)z0 < (unsigned)D, bz1 = (unsigned)z1 < (unsigned)D;
                    const int cx0 = min(max(x0, 0), W - 1), cx1 = min(max(x1, 0), W - 1);
                    const int cy0 = min(max(y0, 0), H - 1), cy1 = min(max(y1, 0), H - 1);
                    const int cz0 = min(max(z0, 0), D - 1), cz1 = min(max(z1, 0), D - 1);
                    const float *a00 = mov + ((size_t)cz0 * H + cy0) * W, *a01 = mov + ((size_t)cz0 * H + cy1) * W;
                    const float *a10 = mov + ((size_t)cz1 * H + cy0) * W, *a11 = mov + ((size_t)cz1 * H + cy1) * W;
                    g.r00 = f2{(bz0 & by0 & bx0) ? a00[cx0] : 0.f, (bz0 & by0 & bx1) ? a00[cx1] : 0.f};
                    g.r01 = f2{(bz0 & by1 & bx0) ? a01[cx0] : 0.f, (bz0 & by1 & bx1) ? a01[cx1] : 0.f};
                    g.r10 = f2{(bz1 & by0 & bx0) ? a10[cx0] : 0.f, (bz1 & by0 & bx1) ? a10[cx1] : 0.f};
                    g.r11 = f2{(bz1 & by1 & bx0) ? a11[cx0] : 0.f, (bz1 & by1 & bx1) ? a11[cx1] : 0.f};
                }
                g.yv = (MODE == 3) ? 0.f : trow[(unsigned)(toff + (j - j0) * W)];
                return g;
            };
            const int jend = min(j0 + kRows, ny);
            if (j0 < jend) {
                GFetch cur = gfetch(j0);
#pragma unroll 1
                for (int j = j0; j < jend; j++) {
                    GFetch nxt = cur;
                    if (j + 1 < jend) nxt = gfetch(j + 1);
                    const Samp3 sm = lerp3_pairs<kGrad>(cur.r00, cur.r01, cur.r10, cur.r11, cur.fx, cur.fy, cur.fz);
                    if constexpr (MODE == 3) wout[(size_t)Y0 * W + (unsigned)(toff + (j - j0) * W)] = sm.v;
                    else f1_accumulate_pk<MODE>(sm, cur.yv, cur.yn, acc);
                    cur = nxt;
                }
            }
        }
    }

    if constexpr (MODE == 3) return;
    float vals[NP];
    int o = 0;
    if constexpr (MODE == 4) {
        vals[0] = acc.M4;
        o = 1;
    } else if constexpr (MODE != 2) {
        vals[0] = acc.M01.x; vals[1] = acc.M01.y; vals[2] = acc.M23.x; vals[3] = acc.M23.y; vals[4] = acc.M4;
        o = 5;
    }
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float a = acc.AB[q][c].x;
            vals[o++] = xn * a; vals[o++] = acc.AB[q][c].y; vals[o++] = zn * a; vals[o++] = a;
        }
    block_reduce_store_nw<NP, kTileWaves, true>(vals, partials + ((size_t)by * rows_stride + bx) * NP, box, wave);
}
#pragma clang diagnostic pop
