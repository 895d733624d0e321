// Two kinds of macros of the tile kernels live here:
//  * TUNING CONSTANTS (first block): numbers, not code paths; the defaults ARE the product, and tools/build_variant.sh A/B runs override
//    them with -D...  The code forms that lost their measurements are gone from the sources; DESIGN.md and profiles/ keep the numbers;
//  * development INSTRUMENTATION (second block: TRX_DEV builds of tools/kbench.hip, -DTRX_TIMING=1 / -DTRX_LDS_PAD=n): in the product
//    library every one of those expands to nothing, so the kernels in affine.hip and affine_tile.h read without #if blocks.
#pragma once

// ---- tuning constants of the tile kernels
#ifndef TRX_GEOMA_BD
#define TRX_GEOMA_BD 14   // (13 = 52.6 KB: three blocks per CU fit the LDS; measured with TRX_TILE_MIN_WAVES=6)
#endif
#ifndef TRX_DBG_SKIP
#define TRX_DBG_SKIP 0   // development ablation (tools/kbench.hip): 1 = no gather/compute, 2 = no box staging, 3 = no target loads
#endif
#ifndef TRX_TGT_POLICY
#define TRX_TGT_POLICY ""   // cache policy suffix of the target loads (development)
#endif
#ifndef TRX_ZS_TGT_POLICY
#define TRX_ZS_TGT_POLICY " nt"   // the z-streaming body's target loads: read once per launch, kept out of the moving planes' way (+1 % on the headline; the same hint on the exact-footprint body costs 6 %, on the tile kernels nothing)
#endif
#ifndef TRX_ZS_RING_POLICY
#define TRX_ZS_RING_POLICY ""    // cache policy suffix of the z-streaming body's ring DMA (development: " nt", " sc1")
#endif
#ifndef TRX_EF_DMA_POLICY
#define TRX_EF_DMA_POLICY ""     // ... of the exact-footprint kernel's granule DMA
#endif
#ifndef TRX_BOX_POLICY
#define TRX_BOX_POLICY ""   // cache policy suffix of the box DMA (development: " nt", " sc1")
#endif
#ifndef TRX_CARRY_BATCH
#define TRX_CARRY_BATCH 16   // carry prologue: partial rows a lane has in flight per batch (32: measured alternative, +-0: profiles/r06b_carry.txt)
#endif
#ifndef TRX_PERSISTENT_BLOCKS
#define TRX_PERSISTENT_BLOCKS 512   // block slots for the 512-thread step kernels if the device cannot be queried (MI355X: 2 x 256 CUs); persistent_blocks() asks the device
#endif
#ifndef TRX_ZS_MIN_BLOCKS
#define TRX_ZS_MIN_BLOCKS 200   // the z-streaming body is offered to launches of at least this many of its blocks (measured, profiles/r03f_zstream_small_batches.txt:
                                // 216 blocks - 2 x 192^3 - gain 20 %, 128 blocks - 4 x 128^3 - lose a factor of two) ...
#endif
#ifndef TRX_ZS_MIN_PLANES
#define TRX_ZS_MIN_PLANES 32    // ... of at least this many planes each (a block pays ~7 planes of pipeline fill; zs_geom never cuts segments shorter)
#endif
#ifndef TRX_STAGE_PRIO
#define TRX_STAGE_PRIO 3
#endif
#ifndef TRX_TILE_MIN_WAVES
#define TRX_TILE_MIN_WAVES 4   // waves per SIMD the register allocator must allow (16 waves per CU)
#endif
#ifndef TRX_DUAL_MIN_WAVES
#define TRX_DUAL_MIN_WAVES 4   // the dual kernel's LDS (GeomR's 78.6 KB box) allows two blocks per CU whatever the registers
#endif

// ---- instrumentation

#ifndef TRX_TIMING
#define TRX_TIMING 0      // 1: per-block staging / barrier / gather cycle counts of the tile kernel's fast loop into trx_timing[]
#endif
#ifdef TRX_LDS_PAD        // inflate the primary tile kernel's LDS footprint (floats) to force one block per CU
#define TRX_DEV_LDS_PAD (TRX_LDS_PAD)
#else
#define TRX_DEV_LDS_PAD 0
#endif

#if TRX_TIMING
namespace trx {
__device__ unsigned long long trx_timing[4 * 8192];
}
#define TRX_TM_INIT() unsigned long long tm_acc[4] = {0, 0, 0, 0} /* wave 0: stage-wait, barrier-1 wait, gather, barrier-2 wait */
#define TRX_TM_STAMP(name) const unsigned long long name = __builtin_amdgcn_s_memtime()
#define TRX_TM_TILE_DONE()                                                                                              \
    do {                                                                                                                \
        const unsigned long long tm4 = __builtin_amdgcn_s_memtime();                                                   \
        tm_acc[0] += tm1 - tm0; tm_acc[1] += tm2 - tm1; tm_acc[2] += tm3 - tm2; tm_acc[3] += tm4 - tm3;                 \
    } while (0)
#define TRX_TM_STORE()                                                                                                  \
    do {                                                                                                                \
        if (tid == 0) {                                                                                                 \
            const size_t bi = (size_t)by * gridDim.x + bx;                                                              \
            if (bi < 8192) for (int i = 0; i < 4; i++) trx::trx_timing[bi * 4 + i] = tm_acc[i];                        \
        }                                                                                                               \
    } while (0)
#else
#define TRX_TM_INIT() ((void)0)
#define TRX_TM_STAMP(name) ((void)0)
#define TRX_TM_TILE_DONE() ((void)0)
#define TRX_TM_STORE() ((void)0)
#endif
