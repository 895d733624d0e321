/*
 * trx.h — C ABI of the MI355X-native TorchRegister hot path (libtrx.so).
 *
 * The reference (AgamChopra/TorchRegister v0.2.3, ref: = src/TorchRegister/) is pure Python and
 * has NO plugin / operator / FFI interface; its hot path is a chain of ATen ops inside three
 * Python loops.  These entry points are what a binding for that path would call instead; each
 * one names the reference code it replaces.  All pointers are DEVICE pointers unless marked
 * [host]; `stream` is a hipStream_t passed as void*.  No entry point allocates, synchronises
 * or calls back into the host: everything is enqueued on `stream` and is graph-capturable.
 * Return value: 0 (TRX_OK) or a negative trx_status; nothing throws.
 * Thread-compatible: no global state (the library reads no environment variable and keeps no settings: every choice a
 * caller can make travels in the argument structs), one host thread per GPU/stream may call concurrently.
 *
 * Data layout (fp32, contiguous): volumes [B][D][H][W] (2-D: D = 1, ndim = 2), pair p of a
 * batch at base + p * stride elements (stride 0 = one volume shared by all pairs).
 * theta: row-major [ndim][ndim+1] per pair, row 0 -> x (W axis), row 1 -> y (H), row 2 -> z (D),
 * exactly F.affine_grid's convention; per-pair small vectors are padded to TRX_PSTRIDE floats.
 * flow: [B][ndim][D][H][W], channel i displaces along spatial dim i in voxel units
 * (ref:utils.py:343-351).
 */
#ifndef TRX_H
#define TRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history (trx_version() returns TRX_VERSION; the first two digits follow the reference package version whose API the host layer mirrors):
 *   200  round 2: flags in trx_volumes (no environment variables), trx_nmi_from_pdfs, trx_theta_chain, the flow loop's device-side early stop
 *   220  round 3: TRX_FLAG_ZSTREAM / NO_ZSTREAM, TRX_FLAG_NEAREST, trx_flow_lncc_run, trx_peer_* (first form)
 *   230  round 4: TRX_FLAG_SAVE_LAST (slab updates store flow_last only on request), TRX_FLAG_EFT / TRX_FLAG_NO_EFT, trx_peer_alloc / export /
 *        import on raw HIP IPC handles, sticky peer time-outs
 *   231  round 5: trx_affine_workspace_bytes grows by three ints (the z-streaming kernel's note to the kernels behind it), the rows_used array the
 *        step kernels leave in the workspace carries the kernel body in bits 24-27, TRX_FLAG_ZS_FUSED.  No entry point changed its signature.
 *   232  round 5: trx_affine_workspace_bytes reserves eight more ints (work tickets of the exact-footprint kernel, zeroed by the z-streaming kernel in
 *        front of it on every launch: the workspace still needs no initialisation by the caller).  No entry point changed its signature.
 *   240  round 6: TRX_FLAG_ONE_KERNEL (a step of a chip-filling launch next to the identity is ONE streaming launch + the finalise), trx_affine_near_identity;
 *        trx_affine_run folds the finalise of an iteration into the next iteration's kernel for launch-bound 3-D steps (TRX_FLAG_NO_CARRY keeps two launches);
 *        trx_affine_workspace_bytes grows by a second partial / note buffer and two carry buffers (3-D).  No entry point changed its signature.
 *        Later addition under the same number: trx_resample / trx_resample_workspace_bytes (the levels of a coarse-to-fine pyramid and the flow
 *        hand-over between them) - new entry points only, no existing signature or struct changed.
 *        Later addition under the same number: trx_bspline_* and trx_bspline_state (cubic B-spline free-form deformation: control lattice <-> dense
 *        flow, its adjoint, and the device-side loop over them) - new entry points and one new struct only.
 *        Later addition under the same number: trx_mi_* , trx_flow_mi_* , trx_bspline_mi_* and trx_mi_cfg (Parzen joint-histogram mutual information
 *        and the two device-side loops over it) - new entry points and one new struct only.
 *        Later addition under the same number: trx_affine_mi_workspace_bytes, trx_affine_mi_loss_grad, trx_affine_mi_run (rigid / affine registration under
 *        the mutual information, the warp fused into the histogram and gradient passes) - new entry points only.
 *        Later addition under the same number: trx_svf_workspace_bytes, trx_svf_exp, trx_svf_exp_backward, trx_bspline_svf_workspace_bytes,
 *        trx_bspline_svf_run (stationary velocity field: the exponential by scaling and squaring, its exact adjoint, and the diffeomorphic form of the
 *        free-form-deformation loop) - new entry points only.
 *        Later addition under the same number: trx_mi_cfg grows by one trailing field, `mask` (a region of interest on the target lattice for every
 *        mutual-information entry point; NULL = every voxel, the launches and bits of before) - no entry point changed its signature.
 *        Later addition under the same number: trx_moving_grid, trx_affine_mi_loss_grad_grids, trx_affine_mi_run_grids, trx_affine_warp_grids (rigid /
 *        affine mutual information and the forward warp for a moving image on a lattice and voxel size of its own) - new entry points and one new
 *        struct only.
 *        Later addition under the same number: trx_affine_flow_warp, trx_affine_flow_warp_backward, trx_bspline_mi_run_grids (a flow composed with an
 *        initial affine and sampled once in a moving image on its own lattice; the B-spline mutual-information loop over it) - new entry points only.
 *        Later addition under the same number: trx_spline_workspace_bytes, trx_spline_coefficients, trx_transform_resample (nearest-neighbour and cubic
 *        B-spline resampling through the final transform) - new entry points only.
 *        Later addition under the same number: trx_moving_grid grows by one trailing field, `world` (voxel-to-world geometry for the rigid / affine
 *        mutual-information entry points; NULL = the scale, the launches and bits of before), trx_affine_world_theta, trx_image_moments and its
 *        workspace query - no entry point changed its signature.
 *        Later addition under the same number: trx_flow_jacobian, trx_flow_folding and its workspace query, trx_fold_cfg, trx_bspline_run_fold,
 *        trx_bspline_mi_run_fold and their workspace queries (the Jacobian determinant map of a dense flow and a folding penalty on it, alone and
 *        inside the free-form deformation loops) - new entry points and one new struct only.
 *        Later addition under the same number: trx_flow_compose, trx_flow_invert (composition of two dense flows and the fixed-point inverse of one) -
 *        new entry points only.
 *        Later addition under the same number: trx_transform_points, trx_affine_then_flow_resample (points and target-space images through the whole
 *        transform, in both chain orders) - new entry points only.
 *        Later addition under the same number: trx_affine_workspace_carry_offset (diagnostics: where the carry buffers of trx_affine_run's one-launch
 *        iterations sit in the workspace) - one new host-only entry point, no device code, no existing signature or struct changed.
 *        Later addition under the same number: trx_image_moments2 and its workspace query (the second intensity moments behind the principal-axes
 *        initialiser) - new entry points only.
 *        Later addition under the same number: trx_distance_transform and its workspace query, trx_mask_surface, trx_label_overlap (the exact Euclidean
 *        distance transform of a binary mask in millimetres, the surface voxels of a mask and the overlap counts of two label maps: what Dice and
 *        the surface distances are computed from) - new entry points only.
 *        Later addition under the same number: trx_ngf_cfg, trx_ngf_loss_grad, trx_bspline_ngf_run and their workspace queries (the normalised gradient
 *        field criterion, alone and as the data term of the free-form deformation loop) - new entry points and one new struct only. */
#define TRX_VERSION 240
#define TRX_PSTRIDE 12  /* floats per pair in theta / param / adam / best_theta arrays */

typedef enum {
    TRX_OK = 0,
    TRX_ERR_ARG = -1,       /* null pointer / non-positive size / bad enum / B > 65535 / a volume of >= 2^31 voxels */
    TRX_ERR_NDIM = -2,      /* ndim not 2 or 3 (or D != 1 with ndim 2) */
    TRX_ERR_WORKSPACE = -3, /* workspace too small: see trx_*_workspace_bytes */
    TRX_ERR_HIP = -4,       /* a HIP launch failed (hipGetLastError) */
    TRX_ERR_CAPACITY = -5   /* trx_*_run: `iters` exceeds losses_capacity (the per-pair device counters cannot be read without a
                               sync, so callers that split a run over several calls keep the running total themselves) */
} trx_status;

/* trx_volumes.flags: per-call path selection (0 = the library picks; the others exist so that every path can be tested
 * against the others through the same entry points - results never depend on the path beyond fp32 rounding). */
#define TRX_FLAG_GATHER_PATH 1u    /* affine entry points: the un-tiled row-walking kernel instead of the LDS-tiled ones */
#define TRX_FLAG_SINGLE_GEOM 2u    /* affine entry points: one tile geometry for every pair (no per-pair choice among GeomD / GeomA / GeomRD / GeomR) */
#define TRX_FLAG_TWO_PASS_FLOW 4u  /* trx_flow_run: keep the moments pass of every iteration (no fusion into the previous update) */
#define TRX_FLAG_DEEP_TILE 8u      /* affine steps: offer the deep tiles (GeomD, GeomRD) to every pair they fit, whatever the batch and volume size
                                      (by default only where their larger tiles still fill the chip) */
#define TRX_FLAG_SAVE_LAST 256u      /* trx_flow_slab_update[_fused]: also store the flow this update starts from into st->flow_last (+12 B/voxel written);
                                      callers set it on the LAST iteration of a run - the iteration that meets stop_crit stores it by itself */
#define TRX_FLAG_NEAREST 128u        /* trx_flow_warp: nearest-neighbour sampling (SpatialTransformer(mode='nearest'), ref:utils.py:339-365) instead of bi/trilinear */
#define TRX_FLAG_NO_ZSTREAM 32u     /* affine steps: never use the z-streaming body (pairs next to the identity run GeomD / GeomA like the others) */
#define TRX_FLAG_ZSTREAM 64u        /* affine steps: offer the z-streaming body whatever the batch size (by default only to launches that fill the chip).
                                     * The body re-checks its window per block from the block's own corners and would publish NaN rows for a pair whose
                                     * pre-image left it; the offer rule (theta and sizes only) is that test's worst case with 0.3 voxels to spare, and
                                     * tests/test_gpu_zstream.py::test_zstream_offer_boundary_never_trips bisects to the rule's edge in 60 directions of
                                     * theta space on three shapes without reaching it: a NaN loss from this path would be a bug, not an input property */
#define TRX_FLAG_NO_EFT 512u        /* affine steps: never use the exact-footprint body (rotated pairs run GeomR as before) */
#define TRX_FLAG_EFT 1024u          /* affine steps: offer the exact-footprint body whatever the batch size (by default only to launches that fill the chip) */
#define TRX_FLAG_ZS_FUSED 2048u      /* affine steps on launches that fill the chip: keep the z-streaming body inside the tile kernel (the round 3-4 form) instead of
                                      * running it as a kernel of its own in front (measured alternative; tests compare the two) */
#define TRX_FLAG_WALK_DOWN 8192u      /* affine steps: the z-streaming kernel walks its columns from the last plane to the first (same sums up to rounding); the exact-footprint
                                      * and tile kernels behind it take the pairs in the opposite order (same sums bit for bit).  trx_affine_run
                                      * toggles this bit on every second iteration (unless TRX_FLAG_NO_PINGPONG): the planes (pairs) a pass read last are the ones the next pass
                                      * starts with, and the 256 MiB Infinity Cache still holds them.  Callers that step one iteration per call may alternate it themselves */
#define TRX_FLAG_NO_PINGPONG 16384u   /* trx_affine_run: every iteration walks in the direction the caller's flags say (measured alternative) */
#define TRX_FLAG_NO_ZS_FLAT 4096u     /* affine steps: the z-streaming kernel never uses its flat 64 x 16 tile (pairs beyond the 64 x 32 tile's window run the tile kernels) */
#define TRX_FLAG_ONE_KERNEL 32768u     /* affine steps of launches that fill the chip: the caller EXPECTS every pair to stay next to the identity (inside the z-streaming kernel's
                                      * windows: |theta - I| up to ~0.03 on its 64 x 32 tile, rotations to ~0.15 rad / zooms to 1.15 on its flat tile), so the step launches that
                                      * kernel ALONE - no exact-footprint kernel, no tile kernel behind it (two launches that find nothing to do: 3.2-3.5 us per step,
                                      * profiles/r06a_one_kernel_ab.txt - worth it up to ~4 x 256^3 voxels per launch).  Always correct: a pair that leaves the windows is run by the same kernel
                                      * on GeomR's body, at about twice its usual cost while it stays outside - a hint about speed, never about results (fp32 rounding between
                                      * bodies as with every other path flag).  trx_affine_near_identity() evaluates the expectation for thetas the caller holds on the host;
                                      * torchregister_amd.AffineSolver sets the flag by itself from the initial thetas and from the bodies the previous run() call ended on */
#define TRX_FLAG_NO_CARRY 65536u      /* trx_affine_run: every iteration is a step kernel plus a finalise kernel, also where the run would fold the finalise into the next
                                      * iteration's kernel (launch-bound 3-D registrations: one pair up to ~128^3) - measured alternative; results differ by fp32 rounding at most
                                      * (the folded finalise sums a pair's partial rows in another fixed order) */
#define TRX_FLAG_NO_ROT_DEEP_TILE 16u /* affine steps: never use GeomRD (the 16 x 16 x 16 tile in GeomR's box) - rotated pairs all run GeomR */

/* A batch of B independent (moving, target) pairs. */
typedef struct {
    const float *moving;   /* [B][D][H][W] */
    const float *target;   /* [B][D][H][W] (may be NULL for warp-only calls) */
    size_t moving_stride;  /* elements between pairs */
    size_t target_stride;
    int ndim, B, D, H, W;
    /* Optional base-coordinate tables of affine_grid(align_corners=False): xn[W], yn[H], zn[D] =
     * fp32 linspace(-1,1,S)*(S-1)/S as ATen builds them.  NULL -> closed form (2i+1)/S-1. */
    const float *xn, *yn, *zn;
    unsigned flags;        /* TRX_FLAG_* (0 for normal use) */
} trx_volumes;

/* L = w_mse*MSE + w_ncc*ncc_alpha*(1-NCC) + w_ssd*ssd_alpha*SSD
 * replaces nn.MSELoss call sites (ref:warpings.py:37,39,124,126,179), NCCLoss.forward
 * (ref:utils.py:197-205, EPSILON=1e-10), SSDLoss.forward (ref:utils.py:218-221) and the weighted
 * sum (ref:warpings.py:78-79,144-145,213-214).  Argument order (target, warped) as in the loops. */
typedef struct {
    float w_mse, w_ncc, ncc_alpha, w_ssd, ssd_alpha;
} trx_loss_cfg;

typedef enum { TRX_OPT_SGD = 0, TRX_OPT_ADAM = 1 } trx_opt_kind;
/* SGD replaces torch.optim.SGD(params, lr) (ref:warpings.py:58,131,192); Adam is an extension
 * (torch.optim.Adam defaults beta=(0.9,0.999), eps=1e-8, bias-corrected). */
typedef struct {
    int kind;
    float lr, beta1, beta2, eps;
} trx_opt_cfg;

typedef enum { TRX_PARAM_AFFINE = 0, TRX_PARAM_RIGID = 1 } trx_param_mode;

/* Per-pair optimisation state, all device memory, all [B][TRX_PSTRIDE] unless noted.
 * AFFINE: param IS theta (ref:warpings.py:42-55,70-74: the regressor MLP is dead, theta == its
 *         bias).  RIGID: param is the pose vector of Theta (ref:utils.py:287-310,
 *         6 floats in 3-D, 3 in 2-D) and theta = Theta(param). */
typedef struct {
    int mode;           /* trx_param_mode */
    float *param;       /* in/out: optimised parameters */
    float *theta;       /* in/out: theta of the NEXT forward (caller initialises consistently) */
    float *adam_m;      /* in/out, may be NULL for SGD */
    float *adam_v;
    float *best_theta;  /* out: theta of the first strict loss minimum (ref:warpings.py:85-93) */
    float *best_loss;   /* [B] out */
    int *best_idx;      /* [B] out */
    float *losses;      /* [B][losses_capacity] out: L_t per iteration (ref:warpings.py:83) */
    int losses_capacity;
    int *step;          /* [B] in/out: iteration counter t (device-resident; 0 before the run) */
    float *grad;        /* optional out [B][TRX_PSTRIDE]: dL/dparam of the last step (may be NULL) */
} trx_affine_state;

int trx_version(void);
const char *trx_status_string(int status);

/* Bytes of scratch the affine entry points need for this batch geometry. */
size_t trx_affine_workspace_bytes(const trx_volumes *vol /*[host]*/);

/* Diagnostics: byte offset, inside the affine workspace, of int rows_used[B] - the number of partial rows the last 3-D step's streaming
 * launch wrote for each pair.  The step kernels pick a kernel body per pair from theta (tile geometry / z-streaming) and each body has its
 * own row count, so this tells a test or a profiler which body ran; the step's own reduction reads the same array. */
size_t trx_affine_workspace_rows_offset(const trx_volumes *vol /*[host]*/);

/* Diagnostics: byte offset, inside the affine workspace, of the two carry buffers float[2][B][64] that the one-launch iterations of
 * trx_affine_run alternate between (per pair theta[12] | param[12] | Adam m[12] | Adam v[12] | step (int) | 15 unused floats).  Nothing else writes
 * them, so a test that fills them with a sentinel before a run reads afterwards whether the run took the one-launch form.  0 for a refused
 * volume and for 2-D (the form does not exist there).  No device work. */
size_t trx_affine_workspace_carry_offset(const trx_volumes *vol /*[host]*/);

/* [host] 1 if a step of this batch at the given thetas (HOST memory, [B][TRX_PSTRIDE]) would run entirely on the z-streaming kernel's tiles - the
 * test that kernel evaluates per pair on the device - i.e. if TRX_FLAG_ONE_KERNEL costs nothing at these poses; 0 otherwise (also for 2-D and
 * for batches the z-streaming kernel is not offered).  No device work. */
int trx_affine_near_identity(const trx_volumes *vol /*[host]*/, const float *theta_host);

/* ONE optimiser iteration for all B pairs: fused forward warp + loss + analytic backward
 * (single pass over moving/target), then loss/gradient/optimiser/best-tracking on device.
 * Replaces one trip of the loop bodies ref:warpings.py:67-93 (affine) / :138-159 (rigid):
 * get_affine_warp (ref:warpings.py:18-26) -> criterions -> error.backward() -> optimizer.step()
 * -> losses_train.append(error.item()) -> best tracking. */
int trx_affine_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                    const trx_affine_state *st, void *workspace, size_t workspace_bytes, void *stream);

/* Pass 1 of trx_affine_step alone (the streaming kernel: per-block partial sums into `workspace`,
 * no finalise, no state change).  Exposed so that the dominant kernel can be timed in isolation
 * (bench.py roofline leg) and for callers that want to overlap their own finalise. */
int trx_affine_accumulate(const trx_volumes *vol, const float *theta, void *workspace, size_t workspace_bytes, void *stream);

/* `iters` iterations enqueued back to back (no host sync in between; replaces the whole loop). */
int trx_affine_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                   const trx_affine_state *st, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* Loss only (forward), theta untouched: terms[B][4] = {total, MSE, NCC-loss, SSD-loss}. */
int trx_affine_loss(const trx_volumes *vol, const trx_loss_cfg *loss, const float *theta, float *terms,
                    void *workspace, size_t workspace_bytes, void *stream);

/* get_affine_warp forward (ref:warpings.py:18-26; used by Register.__call__, ref:torchregister.py:123-128):
 * out[B][C][D][H][W] = warp(moving[B][C][D][H][W], theta[B]); vol->moving_stride is the stride
 * between BATCH items (C*D*H*W for a dense tensor); channels share theta. */
int trx_affine_warp(const trx_volumes *vol, const float *theta, int channels, float *out, void *stream);

/* Generic backward of the warp wrt theta: dtheta[B][TRX_PSTRIDE] = sum_p,c grad_out * d warp/d theta
 * (grid_sampler backward + affine_grid backward of the autograd chain behind error.backward(),
 * ref:warpings.py:80,146) — lets any torch loss drive the HIP warp. */
int trx_affine_warp_backward(const trx_volumes *vol, const float *theta, int channels, const float *grad_out,
                             float *dtheta, void *workspace, size_t workspace_bytes, void *stream);

/* The warp and its theta-backward on a sub-lattice of the output grid: out[B][nz][ny][nx] = warp(moving, theta) at the output voxels
 * (iz[kz], iy[ky], ix[kx]) (device int32 tables; 2-D: nz = 1, iz ignored) - what the NMI loss's
 * F.interpolate(warped, size, mode="nearest") keeps of a full-volume warp (ref:utils.py:236-252: 100^3 of a 256^3 volume) when the
 * tables hold that call's source indices - and dtheta[B][TRX_PSTRIDE] = sum_k grad_out[B][k] * d out_k / d theta (replaces the
 * nearest-interpolate backward + grid_sampler backward + affine_grid backward of the same chain).  Single channel.
 * workspace (backward): at least max(trx_affine_workspace_bytes(vol), B * 1024 * 12 * sizeof(float)) bytes. */
int trx_affine_warp_lattice(const trx_volumes *vol, const float *theta, const int *iz, int nz, const int *iy, int ny, const int *ix, int nx,
                            float *out, void *stream);
int trx_affine_warp_lattice_backward(const trx_volumes *vol, const float *theta, const int *iz, int nz, const int *iy, int ny, const int *ix,
                                     int nx, const float *grad_out, float *dtheta, void *workspace, size_t workspace_bytes, void *stream);

/* Theta (ref:utils.py:287-310: pose vector -> affine matrix, 6 floats in 3-D / 3 in 2-D) and its vector-Jacobian product, for
 * callers that assemble dL/dtheta themselves: theta_out[B][TRX_PSTRIDE] = Theta(pose[B][TRX_PSTRIDE]) and / or
 * dpose_out[B][TRX_PSTRIDE] = J(pose)^T dtheta[B][TRX_PSTRIDE] (fp64 inside, as in trx_affine_step's rigid branch). */
int trx_theta_chain(const float *pose, const float *dtheta, int ndim, int B, float *theta_out, float *dpose_out, void *stream);

/* ------------------------------------------------------------------ dense flow (SpatialTransformer) */
typedef struct {
    float *flow;        /* [B][ndim][D][H][W] in/out */
    float *flow_tmp;    /* same size; required only when smooth_weight != 0 (double buffer) */
    float *adam_m;      /* same size, Adam only */
    float *adam_v;
    float *losses;      /* [B][losses_capacity] */
    int losses_capacity;
    int *step;          /* [B] */
    float smooth_weight; /* extension: lambda * mean squared forward differences of the flow */
    /* Early stop of ref:warpings.py:231-233 (`if losses_train[-1] <= self.stop_crit: break`), decided on the device, per pair, with
     * no host sync: once the recorded loss of iteration k is <= stop_crit the update of iteration k is still applied (the reference
     * steps before it tests) and every later iteration of this and of later calls is a no-op for that pair - step[b] stays k + 1 =
     * the number of recorded losses.  stopped == NULL disables the test. */
    float stop_crit;
    int *stopped;        /* [B] in/out, 0 before the run; non-zero once pair b has stopped */
    /* optional [B][ndim][D][H][W]: the flow of the LAST FORWARD (the one the last recorded loss was computed from, i.e. before
     * that iteration's update) - what the reference's flow_register.flow holds after optimize() (ref:warpings.py:194-196,211). */
    float *flow_last;
} trx_flow_state;

size_t trx_flow_workspace_bytes(const trx_volumes *vol);

/* SpatialTransformer.forward (ref:utils.py:350-365), C channels sharing the flow
 * (flow_register.deform, ref:warpings.py:238-242; Register.__call__, ref:torchregister.py:123-126). */
int trx_flow_warp(const trx_volumes *vol, const float *flow, int channels, float *out, void *stream);

/* One iteration of direct flow-field optimisation (pass A moments, pass B gradient + optimiser):
 * the warp + loss + backward + step span of ref:warpings.py:208-220 with the flow itself as parameter. */
int trx_flow_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                  const trx_flow_state *st, void *workspace, size_t workspace_bytes, void *stream);
int trx_flow_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                 const trx_flow_state *st, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* Loss + dL/dflow for a given flow (the autograd.Function backward for U-Net-generated flows):
 * terms[B][4]; dflow may be NULL (loss only). */
int trx_flow_loss_grad(const trx_volumes *vol, const trx_loss_cfg *loss, const float *flow, float *terms,
                       float *dflow, void *workspace, size_t workspace_bytes, void *stream);

/* Z-slab partition of ONE 3-D volume over ranks (BASELINE config 5): `vol` describes the rank's slab — target,
 * flow and optimiser state hold planes [z_offset, z_offset + vol->D) — while vol->moving is the WHOLE moving
 * volume [B][D_full][H][W] (replicated, constant: no halo of it is exchanged).  One iteration =
 *   (if smooth_weight != 0) exchange one flow plane with each Z neighbour (xGMI P2P): halo_lo / halo_hi =
 *        the neighbour's flow plane just below / above the slab, [ndim][H][W], NULL at the ends of the volume;
 *   trx_flow_slab_moments: pass A -> this rank's 8 raw fp64 sums {Sy,Sw,Syy,Sww,Syw, smooth_z,smooth_y,smooth_x};
 *   the caller all-reduces `moments` over ranks (RCCL; 64 bytes);
 *   trx_flow_slab_update: loss of the whole volume into losses[t], pass B on the slab.  With the regulariser the
 *        new flow is written to st->flow_tmp (it reads neighbours of the old flow): the caller swaps the two.
 * Same span of the reference as trx_flow_step (ref:warpings.py:208-220). */
int trx_flow_slab_moments(const trx_volumes *vol, int z_offset, int D_full, const float *flow, int smooth, const float *halo_hi, double *moments,
                          void *workspace, size_t workspace_bytes, void *stream);
int trx_flow_slab_update(const trx_volumes *vol, int z_offset, int D_full, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                         const trx_flow_state *st, const double *global_moments, const float *halo_lo, const float *halo_hi,
                         void *workspace, size_t workspace_bytes, void *stream);
/* The cross-slab part of trx_flow_slab_moments' smoothness sums on its own: sum over the slab's top plane of (halo_hi - flow)^2, added to
 * moments[b][5].  trx_flow_slab_moments(..., halo_hi = NULL, ...) followed by this equals trx_flow_slab_moments with the halo - and lets
 * the first run while the neighbour's plane is still travelling over xGMI (SlabFlowSolver.run puts the exchange on a side stream). */
int trx_flow_slab_boundary_smooth(const trx_volumes *vol, const float *flow, const float *halo_hi, double *moments, void *stream);

/* Peer-mapped transport of the slab partition (not in the reference, which is single-device): the halo planes and
 * the 64-byte sum of moments as direct writes into a PEER rank's mailbox - device memory of another GPU of the node (or of another
 * process on the same GPU), mapped by the caller through HIP IPC / peer access - instead of torch.distributed.batch_isend_irecv and
 * all_reduce (RCCL).  Flags are 32-bit iteration numbers that only increase; waits poll with system-scope loads in a one-thread
 * kernel, give up after timeout_us and OR a bit into *status (1: trx_peer_wait, 2: trx_peer_gather) instead of hanging the device.
 *   trx_peer_signal : *flag = value, ordered after everything enqueued on `stream` before it (e.g. the copy of a plane into the
 *                     peer's halo slot);
 *   trx_peer_wait   : returns (on the stream) once *flag >= value;
 *   trx_peer_publish: sums[0..8) -> slot_ptrs[r][0..8) for r < n, then *flag_ptrs[r] = value (slot_ptrs / flag_ptrs: DEVICE arrays of n
 *                     device pointers, one per peer: this rank's slot and flag inside that peer's mailbox);
 *   trx_peer_gather : waits until flags[r] >= value for all r < n (this rank's own mailbox), then out[k] = sum over r in rank order of
 *                     slots[r * 8 + k] - the same fp64 additions in the same order on every rank.
 * torchregister_amd.SlabPeers wraps them (mailbox layout, IPC exchange of the handles, double buffering by iteration parity). */
int trx_peer_signal(unsigned *flag, unsigned value, void *stream);
int trx_peer_wait(const unsigned *flag, unsigned value, unsigned timeout_us, int *status, void *stream);
int trx_peer_publish(const double *sums, const void *slot_ptrs, const void *flag_ptrs, int n, unsigned value, void *stream);
int trx_peer_gather(const double *slots, const unsigned *flags, int n, unsigned value, unsigned timeout_us, double *out, int *status, void *stream);
/* Mailbox memory.  A flag that a RUNNING kernel polls while another device (or process) writes it must live in memory whose remote
 * writes become visible without a kernel boundary: fine-grained device memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained)), not
 * the coarse-grained memory of an ordinary hipMalloc / caching allocator.
 *   trx_peer_alloc  : `bytes` of zeroed fine-grained memory on the CURRENT device;          trx_peer_free releases it;
 *   trx_peer_export : the 64-byte HIP IPC handle of such an allocation (hipIpcGetMemHandle) - to be sent to the peers by any channel;
 *   trx_peer_import : maps a peer's handle into this process (hipIpcOpenMemHandle with hipIpcMemLazyEnablePeerAccess: enables peer
 *                     access between the current device and the allocation's device); trx_peer_close unmaps it.
 * They return TRX_ERR_HIP when the runtime refuses (IPC unavailable, device not visible, no peer access): the caller then keeps
 * torch.distributed (SlabPeers.try_exchange decides that on all ranks together). */
#define TRX_PEER_HANDLE_BYTES 64
int trx_peer_alloc(size_t bytes, void **ptr);
int trx_peer_free(void *ptr);
int trx_peer_export(void *ptr, void *handle);
int trx_peer_import(const void *handle, void **ptr);
int trx_peer_close(void *ptr);
/* Without the smoothness term (3-D): the update that also leaves the slab's block partials of the UPDATED flow in the workspace, and the
 * reduction of those partials to the 8 sums - together they replace trx_flow_slab_moments from the second iteration on (one pass over
 * the slab per iteration instead of two; same numbers). */
int trx_flow_slab_update_fused(const trx_volumes *vol, int z_offset, int D_full, const trx_loss_cfg *loss, const trx_opt_cfg *opt,
                               const trx_flow_state *st, const double *global_moments, void *workspace, size_t workspace_bytes, void *stream);
int trx_flow_slab_moments_ready(const trx_volumes *vol, int z_offset, int D_full, double *moments, void *workspace, size_t workspace_bytes,
                                void *stream);

/* Generic backward of the flow warp: dflow[B][ndim][...] = sum_c grad_out[B][c][...] * d warp/d flow. */
int trx_flow_warp_backward(const trx_volumes *vol, const float *flow, int channels, const float *grad_out,
                           float *dflow, void *stream);

/* ---- local-window NCC (extension; not in the reference: no such criterion exists in src/TorchRegister/utils.py, whose
 * NCCLoss (utils.py:182-205) is global.  Definition = the box-window NCC of VoxelMorph-style registration; CPU restatement:
 * oracle/compose.py::local_ncc_loss).  target / warped: [B][D][H][W] fp32 (D = 1 for ndim 2), contiguous.
 *   loss[b] = alpha * (1 - mean_q cc_b(q)),  cc = c^2 / (a b + eps) over the window^ndim box around q (zero padding),
 *   grad[b] = d loss[b] / d warped[b]   (same shape as warped).  Either output may be NULL.
 * window: 3, 5, 7 or 9.  Workspace: trx_lncc_workspace_bytes (12 B per voxel of intermediate fields + block partials). */
size_t trx_lncc_workspace_bytes(int ndim, int B, int D, int H, int W);
int trx_lncc_loss_grad(const float *target, const float *warped, int ndim, int B, int D, int H, int W, int window, float alpha,
                       float eps, float *loss, float *grad, void *workspace, size_t workspace_bytes, void *stream);

/* Direct flow field + LOCAL-window NCC (+ smoothness regulariser st->smooth_weight) as one device-side loop: `iters` iterations of
 *   warp at the current flow -> window sums, loss, dL/dwarped (the kernels behind trx_lncc_loss_grad) -> loss curve / early stop / optimiser
 *   scalars -> dL/dflow through the trilinear derivative + smoothness gradient + SGD / Adam in place
 * with no autograd, no torch optimiser and no host sync (3-D only; 2-D callers compose trx_flow_warp / trx_lncc_loss_grad /
 * trx_flow_warp_backward).  Recorded loss of pair b: lncc_alpha * (1 - mean cc) + smooth_weight / ndim * sum_d mean (forward difference)^2,
 * both of the flow the iteration STARTS from.  State, early stop and flow_last as for trx_flow_run.  vol->target: dense [B][D][H][W].
 * Extension (the reference has neither a local NCC nor a direct flow mode): arbiter = oracle/compose.py under torch autograd. */
size_t trx_flow_lncc_workspace_bytes(const trx_volumes *vol);
int trx_flow_lncc_run(const trx_volumes *vol, int window, float lncc_alpha, float lncc_eps, const trx_opt_cfg *opt,
                      const trx_flow_state *st, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Parzen-window PDF of the reference's NMI loss (ref:utils.py:18-37 K_gauss / PDF_xis / PDF).
 * signals [N][S], xis [N][bins] (bins <= 1024), h > 0:
 *   pdf[n][k] = (1/h) * mean_i K((signals[n][i] - xis[n][k]) / h),  K(u) = exp(-u*u/2) / (2 pi)   (the reference's constant)
 * trx_kde_pdf_backward: grad_signals[n][i] = sum_k grad_pdf[n][k] * d pdf[n][k] / d signals[n][i]  (xis carry no gradient:
 * the reference builds them from .item() values, ref:utils.py:40-48).  No [N][S][bins] tensor is ever formed. */
size_t trx_kde_workspace_bytes(int N, long S, int bins);
int trx_kde_pdf(const float *signals, const float *xis, int N, long S, int bins, float h, float *pdf, void *workspace,
                size_t workspace_bytes, void *stream);
int trx_kde_pdf_backward(const float *signals, const float *xis, const float *grad_pdf, int N, long S, int bins, float h,
                         float *grad_signals, void *stream);
/* The same two functions as a series in (s - x)^2 / (2 h^2) (thirteen terms, 2e-14): the S x bins exponentials become 25 fp64 power
 * sums of the samples and a polynomial per bin.  VALID ONLY when |signals[n][i] - xis[n][k]| <= h for every pair of the call (the NMI
 * loss's bandwidth 3 on intensities normalised to [0, 1]); the caller checks that and passes `center`, the middle of the value range
 * of signals and xis.  One workspace size serves both. */
size_t trx_kde_series_workspace_bytes(int N, long S, int bins);
int trx_kde_pdf_series(const float *signals, const float *xis, int N, long S, int bins, float h, double center, float *pdf,
                       void *workspace, size_t workspace_bytes, void *stream);
int trx_kde_pdf_series_backward(const float *signals, const float *xis, const float *grad_pdf, int N, long S, int bins, float h,
                                double center, float *grad_signals, void *workspace, size_t workspace_bytes, void *stream);
/* The PDF of the SAME signals on another sample line without a second pass over them: `sums` = the workspace an earlier
 * trx_kde_pdf_series(signals, ..., N, S, ..., center, ...) call left behind (the power sums live at its start; same N, S, center).  The NMI
 * loss's pooled sample line moves with the warped image every iteration while the target's samples do not. */
int trx_kde_pdf_series_cached(const void *sums, const float *xis, int xis_stride /* floats between rows of xis, >= bins */, int N, long S, int bins,
                              float h, double center, float *pdf, void *stream);

/* The 256-bin algebra of the NMI loss behind the three PDFs (ref:utils.py:53-79 NMI, :224-259 NMILoss.forward) in one kernel, value and
 * gradient: h1 / h2 / hj [N][bins] = the Parzen "histograms" of target, warped and of the pooled samples (get_pdf, ref:utils.py:40-51).
 *   p = h / sum(h),  E = sum p log2(p + 1e-10)  (the reference's sign convention),  MI = E1 + E2 - Ej,  NMI = 2 MI / (E1 + E2),
 *   loss = alpha * mean_n |NMI_n - 1|  =  sum_n loss_terms[n].
 * Outputs (each may be NULL): nmi [N], mi [N], loss_terms [N], grad_h* [N][bins] = d loss / d h*. */
int trx_nmi_from_pdfs(const float *h1, const float *h2, const float *hj, int N, int bins, float alpha, float *nmi, float *mi,
                      float *loss_terms, float *grad_h1, float *grad_h2, float *grad_hj, void *stream);

/* The same algebra for the loop that evaluates the warped image's PDFs as ONE 2 x bins call (its own line | the pooled line): pdf_w
 * [N][2 bins], pdf_t [N][bins] = the target's PDF on the pooled line; the pooled histogram is 0.5 (pdf_w[:, bins:] + pdf_t) (fp32, like
 * the torch composition) and grad_w [N][2 bins] = [d loss / d h2 | 0.5 d loss / d hj] is what trx_kde_pdf_series_backward takes. */
int trx_nmi_from_pdfs_pooled(const float *h1, const float *pdf_w, const float *pdf_t, int N, int bins, float alpha, float *nmi, float *mi,
                             float *loss_terms, float *grad_w, void *stream);

/* trx_affine_warp_lattice plus the NMI loss's two sample lines in the same call (ref:utils.py:40-48 get_pdf: linspace(max, min, bins)
 * of the samples): out as trx_affine_warp_lattice; xis[B * patches][2 bins] = per pair the line between the extrema of ITS lattice
 * values, then the line between the extrema of those and of minmax_target[B][2] = (min, max) of the target's samples;
 * minmax_warped[B][2] (nullable) receives the warped extrema.  Replaces torch.aminmax + 2 lerp + maximum + minimum + cat per iteration.
 * workspace: B * 8192 * 2 * sizeof(float) bytes. */
int trx_nmi_lattice_lines(const trx_volumes *vol, const float *theta, const int *iz, int nz, const int *iy, int ny, const int *ix, int nx,
                          float *out, const float *minmax_target, int patches, int bins, float *xis, float *minmax_warped, void *workspace,
                          size_t workspace_bytes, void *stream);

/* Tail of one iteration of a loop that assembles dL/dtheta itself (ref:warpings.py:80-93 / :146-159 after error.backward()), one pair:
 * *hist_loss_t = sum(loss_terms[0 .. n_terms)) + *loss_b (nullable); hist_theta_t[TRX_PSTRIDE] = theta (of this forward);
 * g = grad_a + grad_b (nullable); pose == NULL: theta -= lr g (affine SGD), else pose -= lr J(pose)^T g and theta = Theta(pose)
 * (rigid, as trx_theta_chain); param_copy[TRX_PSTRIDE] (nullable) = the new theta. */
int trx_nmi_loop_update(int ndim, float *theta, float *pose, const float *grad_a, const float *grad_b, float lr, const float *loss_terms,
                        int n_terms, const float *loss_b, float *hist_loss_t, float *hist_theta_t, float *param_copy, void *stream);

/* ---- Resampling between grid sizes (the levels of a coarse-to-fine pyramid; extension, the reference registers at one resolution).
 * in: N volumes [D][H][W], out: N volumes [Do][Ho][Wo], both contiguous fp32 (2-D: ndim 2, D = Do = 1).  Each axis on its own:
 *   shrinks (So < S): separable 5-tap binomial blur [1,4,6,4,1]/16 along that axis on the input grid (replicate boundary), then linear
 *                     interpolation at the output positions;
 *   same size: identity (no blur);  grows (So > S): linear interpolation only.
 * Output positions are F.interpolate(size=..., mode='bilinear' | 'trilinear', align_corners=...)'s: align_corners 0:
 * u = max((j + 0.5) S / So - 0.5, 0), 1: u = j (S - 1) / (So - 1).  channel_scale [host] (nullable): volume n is multiplied by
 * channel_scale[n % channels] (channels <= 64; a flow field's per-axis unit change when it moves to a finer grid).
 * Deterministic (no atomics).  Workspace: trx_resample_workspace_bytes (0 = arguments rejected) - intermediates of the separable passes,
 * a chunk of volumes at a time. */
size_t trx_resample_workspace_bytes(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo);
int trx_resample(const float *in, float *out, int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo, int align_corners, int channels,
                 const float *channel_scale /*[host]*/, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Cubic B-spline free-form deformation (Rueckert et al. 1999; extension, the reference has dense flows only: ref:warpings.py:178-242).
 * A control lattice with an integer spacing of d voxels per axis parameterises the displacement field.  Per spatial axis of S voxels:
 *   G = (S - 1) / d + 4 control points (integer division), point i at voxel coordinate (i - 1) d;
 *   at voxel x: i0 = x / d, t = (x % d) / d, weights B0 = (1-t)^3/6, B1 = (3t^3 - 6t^2 + 4)/6, B2 = (-3t^3 + 3t^2 + 3t + 1)/6, B3 = t^3/6
 *   (formed in fp64, stored in fp32: there are only d distinct quadruples per axis).
 * ctrl [B][ndim][Gz][Gy][Gx] fp32 contiguous (2-D: [B][2][Gy][Gx], D = 1, sz ignored), units and channel convention of `flow` above.
 *   expand: flow_c(z,y,x) = base_c(z,y,x) + sum_{l,m,n=0..3} B_l(tz) B_m(ty) B_n(tx) ctrl_c[iz0+l][iy0+m][ix0+n]   (base: nullable, shape of flow)
 *   reduce: dctrl_c[k] = sum over voxels of w_k(voxel) dflow_c(voxel), the same weights - the exact adjoint; base receives no gradient.
 * Spacings: 1 .. 1024 per axis (sz, sy, sx; they may differ).  Separable 1-D passes, no atomics, every sum in a fixed order: the same bits on
 * every call, and a pair's result does not depend on the batch around it.  CPU restatement: tests/bspline_ref.py. */

/* [host] (Gz, Gy, Gx) of a geometry and spacing into grid[3] (2-D: Gz = 1).  No device work.  Extension; restatement: tests/bspline_ref.py::grid. */
int trx_bspline_grid(int ndim, int D, int H, int W, int sz, int sy, int sx, int *grid /*[host]*/);

/* Bytes of workspace that trx_bspline_expand, trx_bspline_reduce, trx_bspline_bending and trx_bspline_run / _step each accept for this geometry
 * (one size serves all: the intermediates of the separable passes, for the loop dL/dctrl, the loss terms and trx_flow_loss_grad's workspace,
 * and for the bending energy its Gram bands and one partial sum per lattice tile).  0 = arguments
 * rejected, as trx_resample_workspace_bytes.  Extension. */
size_t trx_bspline_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx);

/* Control lattice -> dense flow (+ base).  Passes z, y, x: only the last touches a full-size array (12 B/voxel written in 3-D, 24 B/voxel moved
 * with a base).  Extension; restatement: tests/bspline_ref.py::expand. */
int trx_bspline_expand(const float *ctrl, const float *base /*nullable*/, float *flow, int ndim, int B, int D, int H, int W, int sz, int sy, int sx,
                       void *workspace, size_t workspace_bytes, void *stream);

/* The adjoint: dL/dflow [B][ndim][D][H][W] -> dL/dctrl [B][ndim][Gz][Gy][Gx].  Passes x, y, z: dflow is read exactly once (12 B/voxel in 3-D).
 * Extension; restatement: tests/bspline_ref.py::reduce. */
int trx_bspline_reduce(const float *dflow, float *dctrl, int ndim, int B, int D, int H, int W, int sz, int sy, int sx, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Bending energy of the control lattice (the regulariser of Rueckert et al. 1999) and its gradient.  Extension.
 * Per axis, the k-th-derivative weights with respect to the voxel coordinate, on control points i0 .. i0 + 3 at voxel x (i0, t as above):
 *   k = 0: B0 .. B3;   k = 1: (1/d) [ -(1-t)^2/2, (3t^2 - 4t)/2, (-3t^2 + 2t + 1)/2, t^2/2 ];   k = 2: (1/d^2) [ 1-t, 3t-2, 1-3t, t ]
 * (formed in fp64, stored in fp32).  M_a^(k) [S][G] holds them in row x, columns i0 .. i0 + 3.  With N = D H W:
 *   E_b = (1/N) sum_c sum_{kz+ky+kx = 2} (2! / (kz! ky! kx!)) sum_voxels [ (ctrl_{b,c} x_z M_z^(kz) x_y M_y^(ky) x_x M_x^(kx))(voxel) ]^2
 * - 3-D: zz, yy, xx once and zy, zx, yx twice; 2-D: yy, xx and 2 yx - exact second derivatives of the B-spline displacement (no `base`), in
 * `flow`'s units, sampled at the voxel centres; an axis of one voxel has its one sample at t = 0.
 * The kernels use the Gram form: R_a^(k) = M_a^(k)^T M_a^(k) ([G][G], banded: |i - j| <= 3; each entry summed in fp64 over its voxels in
 * ascending x, stored in fp32), dE_b/dctrl_{b,c} = (2/N) sum_k mult_k (R_z^(kz) (x) R_y^(ky) (x) R_x^(kx)) ctrl_{b,c},
 * E_b = 1/2 sum_c <ctrl_{b,c}, dE_b/dctrl_{b,c}>.  E is not clamped: for a lattice whose energy is zero (affine), rounding can leave a
 * slightly negative value.
 *   energy[b] = E_b (unweighted);   dctrl (nullable) = (accumulate ? dctrl : 0) + weight dE/dctrl.
 * Three launches (the bands, the lattice tiles, the per-pair sum), no atomics, every sum in a fixed order: the same bits on every call, and a
 * pair's result does not depend on the batch around it.  Status codes before any HIP call.  Workspace: trx_bspline_workspace_bytes.
 * CPU restatement: tests/bspline_bending_ref.py. */
int trx_bspline_bending(const float *ctrl, float *energy /*[B]*/, float *dctrl /*nullable*/, float weight, int accumulate, int ndim, int B, int D, int H,
                        int W, int sz, int sy, int sx, void *workspace, size_t workspace_bytes, void *stream);

/* State of the free-form-deformation loop, all device memory.  Early stop, step and flow_last as in trx_flow_state: the iteration whose recorded
 * loss is <= stop_crit still applies its update, every later iteration is a no-op for that pair, step[b] = number of recorded losses,
 * flow_last = the expanded flow of the pair's last forward.  Extension (no counterpart in the reference). */
typedef struct {
    float *ctrl;        /* [B][ndim][Gz][Gy][Gx] in/out: the parameters */
    float *adam_m;      /* same size, Adam only (may be NULL for SGD) */
    float *adam_v;
    const float *base;  /* [B][ndim][D][H][W] or NULL: a fixed dense flow the lattice adds to (coarse-to-fine hand-over); no gradient */
    float *flow;        /* [B][ndim][D][H][W] scratch the caller owns: the expanded flow of the last forward of the call */
    float *dflow;       /* same size, scratch: dL/dflow of that forward */
    float *losses;      /* [B][losses_capacity] */
    int losses_capacity;
    int *step;          /* [B] in/out, 0 before the run */
    float stop_crit;
    int *stopped;       /* [B] in/out, 0 before the run; NULL disables the early stop */
    float *flow_last;   /* optional [B][ndim][D][H][W]: kept for a pair when it stops and on the last iteration of every call */
    float bending_weight; /* lambda >= 0 of the bending-energy penalty (trx_bspline_bending); 0 = none: today's launches and bits.  Later addition
                           * under TRX_VERSION 240: a caller built against the shorter struct must zero this field */
} trx_bspline_state;

/* One iteration / `iters` iterations back to back, no host sync, no allocation: expand -> trx_flow_loss_grad on the expanded flow (the fused
 * MSE / NCC / SSD loss of trx_loss_cfg and its dL/dflow) -> reduce -> per pair: losses[b][t] = terms[b][0], early stop, SGD or Adam on ctrl
 * (trx_opt_cfg's constants and bias correction).  spacing [host]: (sz, sy, sx).  Status codes before any HIP call; iters > losses_capacity:
 * TRX_ERR_CAPACITY.  With st->bending_weight = lambda > 0 the objective of pair b is L = data term + lambda E_b (trx_bspline_bending): the
 * Gram bands are formed once per call, each iteration has one more launch (after reduce: dctrl += lambda dE/dctrl, the tiles' energies), and
 * losses[b][t] and the early stop see the total; `base` receives nothing.  lambda < 0 or not finite: TRX_ERR_ARG.  Extension: arbiter = tests/bspline_ref.py::expand + oracle/compose.py (flow_warp, weighted_loss) under torch autograd. */
int trx_bspline_step(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st,
                     const int *spacing /*[host]*/, void *workspace, size_t workspace_bytes, void *stream);
int trx_bspline_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st,
                    const int *spacing /*[host]*/, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Mutual information from a Parzen joint histogram (Mattes et al. 2003; extension: the reference's NMILoss, ref:utils.py:224-259, is a Gaussian
 * KDE on a nearest-resampled lattice that its own README rules out in 3-D).  target / warped: [B][D][H][W] fp32 contiguous (D = 1 for ndim 2),
 * N = D H W voxels per pair, K = cfg->bins in 8 .. 64, range [B][4] = (lo_t, hi_t, lo_w, hi_w) per pair.
 *   target bin (box window):   a = clamp((int)floorf((t - lo_t) * s_t), 0, K - 1),  s_t = hi_t > lo_t ? K / (hi_t - lo_t) : 0 - one fp32 subtract, one
 *                              fp32 multiply, never contracted;
 *   warped (cubic B-spline):   x = (w - lo_w) * s_w,  s_w = hi_w > lo_w ? (K - 3) / (hi_w - lo_w) : 0 (fp32 as above),  u = 1 + clamp(x, 0, K - 3),
 *                              c = min((int)floorf(u), K - 3),  r = u - c in [0, 1]; bins c - 1 .. c + 2 receive
 *                              ((1 - r)^3, 3r^3 - 6r^2 + 4, -3r^3 + 3r^2 + 3r + 1, r^3) / 6 (they sum to 1; every index lies in [0, K - 1]);
 *   P[a][k] = (1 / N) sum_v [a_v = a] beta_k(u_v),  p_T = sum_k P,  p_W = sum_a P,  H_T, H_W, H_TW their entropies (natural logarithm, 0 log 0 = 0);
 *   loss[b] = alpha (H_TW - H_W)  [= alpha (H_T - MI): the gradient of -alpha MI]   or, cfg->normalized != 0,   alpha (2 - (H_T + H_W) / H_TW)
 *             (loss and gradient 0 when H_TW = 0).  Both are >= 0 up to rounding, so the loops' `loss <= stop_crit` keeps its meaning;
 *   grad_warped[v] = (s_w / N) [0 <= x_v <= K - 3] sum_{j = 0..3} G[a_v][c_v - 1 + j] beta'_j(r_v),  G = d loss / d P (0 where P = 0),
 *             beta' = (-(1 - r)^2, 3r^2 - 4r, -3r^2 + 2r + 1, r^2) / 2.  The mask is inclusive (torch's clamp backward); at a voxel exactly on an
 *             end of the range the function is only one-sidedly differentiable.  The target receives no gradient.
 * Ranges are the caller's: the hot paths take the target's min / max and the moving image's min / max widened to contain 0 (the value of the
 * zero-padded warp outside the field of view; not widened under the overlap rule of trx_moving_grid, which counts no padded sample) once per optimisation.  Values outside the range fall into the end bins with a zero gradient.
 * The histogram is accumulated in fixed point (2^31 units per voxel, the fp32 weights converted to units, the largest of the four as the remainder so
 * that every voxel adds exactly one) with 64-bit integer adds, LDS and global: beyond the fp32 rounding of the weights,
 * |P[a][k] - exact| <= 1.5 * 2^-31 n[a][k] / N for the n[a][k] voxels that touch the cell, at most 3 * 2^-31 summed over the table.  No float atomics; entropies in fp64 in a fixed order: the same bits on every call, and a pair's result does not depend on
 * the batch around it.  One memset and three launches (histogram 8 B/voxel, the K x K table, gradient 12 B/voxel; grad_warped == NULL: two), no host
 * sync, no allocation; status codes (TRX_ERR_ARG: null pointer, bins outside 8 .. 64, alpha not finite; TRX_ERR_NDIM; TRX_ERR_WORKSPACE) before any
 * HIP call.  CPU restatement: tests/mi_ref.py.
 * Region of interest, cfg->mask != NULL: a binary mask on the target lattice, one per pair, M_b = {v : mask[b][v] != 0}, N_m = |M_b|.
 *   histogram    only voxels v in M_b are accumulated, each adding exactly 2^31 units as above: sum(counts[b]) = N_m 2^31 exactly;
 *   P, G         P = counts / (N_m 2^31), G scaled by s_w / N_m.  N_m is never known to the host and costs no sync: the table kernel sums the pair's
 *                K^2 64-bit cells (integers: exact, any order) and divides by 2^31.  With an all-ones mask N_m = N and every operation behind it is
 *                the unmasked call's: the same bits;
 *   N_m = 0      loss[b] = 0, G = 0, gradient 0: no division by zero, no NaN, the other pairs of the batch untouched;
 *   grad_warped  0 for v outside M_b (the array is fully written); inside, the definition above with N_m for N.
 * Mutual information depends on nothing but the multiset of (t, w) pairs, so this is the unmasked definition applied to the selected voxels (CPU
 * restatement: tests/mi_mask_ref.py).  The masked passes read one byte more per voxel (9 and 9 B/voxel read).  Same bits on every call, a pair
 * does not depend on its batch, no new status code, the workspace sizes do not change.  cfg->mask == NULL: the launches and bits of before.
 * Every entry point that takes a trx_mi_cfg honours it: trx_mi_histogram, trx_flow_mi_run and trx_bspline_mi_run (through trx_mi_loss_grad, once per
 * iteration), trx_affine_mi_loss_grad and trx_affine_mi_run (below). */
typedef struct {
    int bins;            /* K: 8 .. 64 */
    float alpha;
    int normalized;      /* 0: alpha (H_TW - H_W);  otherwise: alpha (2 - (H_T + H_W) / H_TW) */
    const float *range;  /* device [B][4]: lo_t, hi_t, lo_w, hi_w */
    const unsigned char *mask;   /* device [B][D][H][W] (D = 1 for ndim 2), dense, N bytes between pairs; NULL = every voxel (today's launches and bits);
                                    non-zero = the voxel counts.  Read on the device on every evaluation: it must outlive the call / run. */
} trx_mi_cfg;
size_t trx_mi_workspace_bytes(int ndim, int B, int D, int H, int W, int bins);   /* 0 = arguments rejected */
int trx_mi_loss_grad(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_mi_cfg *cfg, float *loss /*[B]*/,
                     float *grad_warped /*nullable, [B][D][H][W]*/, void *workspace, size_t workspace_bytes, void *stream);
/* The histogram pass of trx_mi_loss_grad alone: uint64 counts[B][K][K] (target bin, warped bin; 2^31 units per voxel, so a pair's counts sum to
 * N * 2^31 exactly and P = counts / (N * 2^31)) at the start of the workspace.  Exposed so that the pass can be timed in isolation
 * (tools/bench_mi.py) and its table checked on its own.  Same arguments, checks and workspace. */
int trx_mi_histogram(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_mi_cfg *cfg, void *workspace,
                     size_t workspace_bytes, void *stream);

/* Direct flow field + mutual information (+ smoothness regulariser st->smooth_weight) as one device-side loop: trx_flow_lncc_run with
 * trx_mi_loss_grad in the middle - warp at the current flow -> histogram, loss, dL/dwarped -> loss curve / early stop / optimiser scalars -> dL/dflow
 * through the trilinear derivative + smoothness gradient + SGD / Adam in place.  3-D only (TRX_ERR_NDIM otherwise).  State, early stop and flow_last as
 * for trx_flow_run; vol->target: dense [B][D][H][W]; cfg->range is read on the device, once per iteration, and must outlive the run.
 * Extension: arbiter = oracle/compose.py::flow_warp + tests/mi_ref.py under torch autograd. */
size_t trx_flow_mi_workspace_bytes(const trx_volumes *vol, int bins);
int trx_flow_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_flow_state *st, int iters, void *workspace,
                    size_t workspace_bytes, void *stream);

/* Free-form deformation + mutual information: trx_bspline_run with another data term, 2-D and 3-D.  Per iteration: expand -> trx_flow_warp ->
 * trx_mi_loss_grad -> trx_flow_warp_backward -> reduce -> the bending / decide / update launches of trx_bspline_run.  trx_bspline_state keeps its
 * whole meaning (base, bending_weight, stop_crit, stopped, flow_last, losses = data term + lambda E).  vol->target: dense [B][D][H][W].
 * Extension: arbiter = tests/bspline_ref.py::expand + oracle/compose.py::flow_warp + tests/mi_ref.py (+ tests/bspline_bending_ref.py) under torch autograd. */
size_t trx_bspline_mi_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins);
int trx_bspline_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_bspline_state *st,
                       const int *spacing /*[host]*/, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Rigid / affine registration under the mutual information above, the warp fused into its two passes (no warped volume).
 * 2-D and 3-D.  vol->target: dense [B][D][H][W]; moving_stride and target_stride are honoured; xn / yn / zn as for every affine entry point.  theta
 * [B][TRX_PSTRIDE] and range [B][4]: one of each per pair.  Sampling: the affine warp's (affine_grid + grid_sample, align_corners=False, zero padding, bi- /
 * trilinear), coordinates formed as the row-walking affine kernels form them.  Histogram, loss and G exactly as trx_mi_loss_grad defines them, with
 * w = the sample; dtheta = what trx_affine_warp_backward returns for grad_out = trx_mi_loss_grad's grad_warped (its out-of-bounds corners included).
 * Per evaluation: one memset, pass 1 (sample + histogram, 8 B/voxel read), the K x K table kernel, pass 2 (sample + gradient rows, 8 B/voxel read), one
 * reduction - against 36 B/voxel moved by the chain warp -> trx_mi_loss_grad -> warp backward.  A pair gets ceil(N / 16384) blocks and partial rows, whatever B:
 * its loss and gradient are the same bits on every call and in every batch.  No float atomics, no host sync, no allocation.  cfg->range is read on the
 * device and must outlive the call.  Status codes before any HIP call: TRX_ERR_ARG (null pointer, bins outside 8 .. 64, alpha not finite, B > 65535,
 * >= 2^31 voxels), TRX_ERR_NDIM, TRX_ERR_WORKSPACE.
 * cfg->mask (trx_mi_loss_grad's semantics; dense [B][D][H][W] whatever target_stride / moving_stride say): a voxel outside the mask is not sampled at
 * all, in either pass - it costs its mask byte - and its contribution to the partial rows is exactly zero; dtheta = what trx_affine_warp_backward
 * returns for grad_out = the masked grad_warped.  A pair with an empty mask has loss 0 and dtheta 0, and a run leaves its theta where it was. */

/* [host] bytes of workspace for this geometry (only ndim, B, D, H, W of `vol` are read) and bin count; 0 = rejected.  Pure arithmetic.  Also the
 * query of the *_grids entry points below: their workspace depends on the target lattice (vol) alone, not on the moving one. */
size_t trx_affine_mi_workspace_bytes(const trx_volumes *vol /*[host]*/, int bins);

/* loss[B] and (dtheta != NULL) dtheta[B][TRX_PSTRIDE] at theta[B][TRX_PSTRIDE].  Replaces the chain trx_affine_warp -> trx_mi_loss_grad ->
 * trx_affine_warp_backward (what get_affine_warp + MILoss + backward() enqueue).  Afterwards uint64 counts[B][K][K] lie at the start of the workspace, as
 * after trx_mi_histogram.  dtheta == NULL: pass 2 is not launched, the loss has the same bits.  Extension: arbiter = oracle/compose.py::affine_warp +
 * tests/mi_ref.py under torch autograd (tests/affine_mi_ref.py). */
int trx_affine_mi_loss_grad(const trx_volumes *vol, const trx_mi_cfg *cfg, const float *theta /*[B][TRX_PSTRIDE]*/, float *loss /*[B]*/,
                            float *dtheta /*nullable, [B][TRX_PSTRIDE]*/, void *workspace, size_t workspace_bytes, void *stream);

/* `iters` iterations back to back: trx_affine_run with the mutual information as the criterion.  Per iteration four launches: pass 1, table, pass 2, and one
 * update kernel per pair with trx_affine_step's epilogue - (rigid) dtheta -> dpose through Theta's vector-Jacobian product, SGD or Adam on param, theta of
 * the next forward, losses[b][t] = the loss at the theta of THIS forward, best_theta / best_loss / best_idx by first strict minimum, step, optional grad.
 * State and semantics: trx_affine_state / trx_affine_run (iters > losses_capacity: TRX_ERR_CAPACITY; the other refusals as above plus trx_affine_step's
 * for opt and st).  Replaces the generic loop get_affine_warp -> MILoss -> backward() -> torch optimiser -> .item() per iteration.  Extension: arbiter =
 * tests/affine_mi_ref.py (oracle/compose.py::affine_warp, pose_to_theta + tests/mi_ref.py under torch autograd and torch.optim). */
int trx_affine_mi_run(const trx_volumes *vol, const trx_mi_cfg *cfg, const trx_opt_cfg *opt, const trx_affine_state *st, int iters, void *workspace,
                      size_t workspace_bytes, void *stream);

/* ---- The same three operations for a moving image on a lattice of its own, and in millimetres.  Extension.
 * vol->D / H / W describe the TARGET lattice: the voxels the passes walk, cfg->mask, the base-coordinate tables xn / yn / zn, the output of the warp,
 * the workspace.  vol->moving holds volumes of mg->D x mg->H x mg->W voxels, vol->moving_stride counts moving elements.
 * Sampling: for target voxel (x, y, z) the normalised coordinate (xn, yn, zn) is formed as above; the moving coordinate is
 *   theta_eff . (xn, yn, zn, 1),  theta_eff[k] = theta[k] * scale[k] (one fp32 multiply, k < ndim (ndim + 1), theta's own layout),
 * un-normalised with the MOVING sizes and sampled in the moving volume with zero padding:
 *   grid_sample(moving, affine_grid(theta_eff, target.shape), align_corners=False).
 * World space: with e = size * voxel size / 2 the half extent of an axis in mm, scale[r][c] = e_target[c] / e_moving[r] on the matrix entries and 1 on
 * the translation column give  moving_mm = theta[:, :nd] target_mm + e_moving (.) theta[:, nd]  for two volumes whose centres coincide and whose axes
 * are aligned: with theta = Theta(pose) the map is rigid in millimetres whatever the voxel sizes.  scale == 1 everywhere: the two normalised cubes
 * coincide, and with equal sizes every number below has the bits of the entry point above.
 * theta, dtheta, st->theta, st->param, st->best_theta are the UNSCALED theta: dtheta = dL/dtheta_eff (.) scale (formed in fp64 in the reduction behind pass
 * 2, whose order does not change; the S / 2 per row is the moving size's), so the rigid chain rule and the whole epilogue are trx_affine_mi_run's.
 * Everything else keeps its meaning: losses, best tracking, SGD / Adam, capacity, the mask (target lattice, one byte per target voxel), N_m, the
 * fixed-point histogram, the same bits on every call and in every batch, the launches per evaluation.
 * Workspace: it depends on the target lattice alone - trx_affine_mi_workspace_bytes(vol, bins) is the query.
 * Refusals on top of the entry points above, before any HIP call: TRX_ERR_ARG (mg NULL, a moving size < 1, >= 2^31 moving voxels, a scale entry that
 * is not finite, a matrix scale entry <= 0), TRX_ERR_NDIM (ndim 2 with mg->D != 1). */
typedef struct {
    int D, H, W;                 /* the MOVING lattice (D = 1 for ndim 2) */
    float scale[TRX_PSTRIDE];    /* theta's own layout, row-major [ndim][ndim + 1]; entries past ndim (ndim + 1) are not read */
    int overlap;                 /* 0: every target voxel counts, its sample zero-padded (the launches and bits of before).  Otherwise the overlap rule
                                  * below.  Later addition under TRX_VERSION 240, like `mask`: a caller built against the shorter struct must zero both */
    const unsigned char *mask;   /* device [B][D][H][W] of THIS (moving) lattice, dense, nullable; non-zero = the moving voxel counts.  Needs overlap != 0
                                  * (TRX_ERR_ARG otherwise).  Read on the device on every evaluation: it must outlive the call / run */
    const double *world;         /* device [B][TRX_WORLD_STRIDE], nullable: world geometry (below).  When given, `scale` is not read.  Read on the device on
                                  * every evaluation: it must outlive the call / run.  Later addition under TRX_VERSION 240: a caller built against the
                                  * shorter struct must zero it, like `overlap` and `mask` */
} trx_moving_grid;
/* World geometry (elastix AutomaticTransformInitialization, ITK CenteredTransformInitializer, ANTs -r): each image carries a
 * voxel-to-world matrix A (columns in the tensor's axis order d, h, w; rows world x, y, z, in mm), and theta acts in world millimetres about a centre c
 * behind a fixed world transform T0:  p_moving = T0 Tr(c) Theta Tr(-c) p_target,  Theta = [theta[:, :nd] | l (.) theta[:, nd]] (homogeneous),
 * l_r = sum_a |A_m[r][a]| S_m,a / 2 the half extent of the moving volume's bounding box along world axis r.  With N(S) the map from affine_grid's
 * normalised coordinate (x, y, z order) to the voxel index (d, h, w order), i_a = ((n_a + 1) S_a - 1) / 2:
 *   R = Tr(-c) A_t N(S_t),   L = N(S_m)^-1 A_m^-1 T0 Tr(c),   theta_eff = (L Theta R)[:nd].
 * The record of pair b, TRX_WORLD_STRIDE doubles, made by the caller on the host in fp64: L row-major [nd][nd + 1] at offset 0, R row-major
 * [nd][nd + 1] at offset 12, l [nd] at offset 24; the rest is not read.  One record per pair: every patient has their own origin.
 * theta_eff is formed once per block, where theta (.) scale is formed otherwise, in fp64 with one IEEE multiply and one IEEE add per term (no
 * contraction), each sum in ascending index order with the homogeneous term last:
 *   M[r][j] = sum_{c < nd} theta[r][c] R[c][j]  (+ l_r theta[r][nd] for j = nd),   theta_eff[i][j] = sum_{r < nd} L[i][r] M[r][j]  (+ L[i][nd] for j = nd),
 * rounded once to fp32.  trx_affine_world_theta runs the same device function: its output is, bit for bit, the theta the passes sample at, and a call
 * with that theta, scale 1 and no record gives the same counts and the same loss bits.  The voxel loop is the one of the other instances.
 * Gradient, in fp64 behind reduce_partials (whose order does not change): g[i][j] = (S_m,i / 2) (sum of the partial rows)[i][j] = dL/dtheta_eff;
 *   P[r][j] = sum_i L[i][r] g[i][j];   dtheta[r][c < nd] = sum_{j <= nd} P[r][j] R[c][j];   dtheta[r][nd] = l_r P[r][nd].
 * The state (theta, param, best_theta) stays the unscaled theta, as under `scale`.
 * Honoured by trx_affine_mi_loss_grad_grids and trx_affine_mi_run_grids, alone, with cfg->mask and under the overlap rule (instances of their own,
 * *_world_kernel; the other instances keep their code).  Every other entry point that takes a trx_moving_grid - trx_affine_warp_grids,
 * trx_affine_flow_warp / _backward / _valid, trx_bspline_mi_run_grids, trx_transform_resample - refuses a non-NULL `world` with TRX_ERR_ARG before any HIP call: they take the effective theta
 * (trx_affine_world_theta) and scale 1.  trx_bspline_mi_grids_workspace_bytes is host arithmetic on sizes and ignores it, as it ignores the scale.  The entries of a record
 * are device memory and cannot be checked on the host: a non-finite entry gives a non-finite theta_eff, hence loss, for that pair only. */
#define TRX_WORLD_STRIDE 32
#define TRX_WORLD_L 0
#define TRX_WORLD_R 12
#define TRX_WORLD_EXT 24
/* The overlap rule (elastix -mMask and its discarded samples, NiftyReg -fmask / NaN padding, ITK's Mattes metric): with
 * mg->overlap != 0, target voxel v of pair b with un-normalised moving coordinate i (x, y(, z)), formed exactly as the sampling kernel forms it, is
 *   valid(v) = (cfg->mask at v, if any)  and  0 <= i_a <= S_m,a - 1 on every axis a  and  (mg->mask at rint(i) != 0, if any)
 * (rint per axis, half to even - in range by the second condition; a NaN coordinate is invalid).  All 2^ndim corners of a valid sample lie in the moving
 * volume: no zero is blended into a counted sample.  Histogram, P, G and loss are trx_mi_loss_grad's masked definition with M_b = {v : valid(v)}:
 * sum(counts[b]) = N_valid 2^31 exactly, N_valid = 0 gives loss 0 and gradient 0.  The gradient treats validity as constant (ITK, elastix): dtheta / dflow
 * are the masked chain's with mask = valid at the current transform, so the loss is piecewise smooth and jumps by O(1 / N_valid) when a sample crosses
 * a border plane.  Ranges are the caller's; with the rule on the hot paths take the moving image's own min / max (inside mg->mask), NOT widened to 0.
 * Honoured by trx_affine_mi_loss_grad_grids and trx_affine_mi_run_grids (a third instance of the two fused passes: the sample is rejected after its
 * coordinate is formed and before anything is gathered; the same launches, the same workspace) and by trx_bspline_mi_run_grids (below); every other
 * entry point that takes a trx_moving_grid reads neither member. */
int trx_affine_mi_loss_grad_grids(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const trx_mi_cfg *cfg, const float *theta, float *loss,
                                  float *dtheta /*nullable*/, void *workspace, size_t workspace_bytes, void *stream);
int trx_affine_mi_run_grids(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const trx_mi_cfg *cfg, const trx_opt_cfg *opt,
                            const trx_affine_state *st, int iters, void *workspace, size_t workspace_bytes, void *stream);
/* out[B][channels][target lattice] = the sample of moving[B][channels][moving lattice] at theta_eff; channels share coordinates (trx_affine_warp's
 * layout: vol->moving_stride between batch items).  vol->target is not read.  Equal sizes and scale == 1: trx_affine_warp itself, the same bits.  No
 * backward; the nearest-neighbour and cubic forms are trx_transform_resample. */
int trx_affine_warp_grids(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const float *theta, int channels, float *out, void *stream);
/* theta_eff[B][TRX_PSTRIDE] of theta[B][TRX_PSTRIDE] under mg->world (the device function of the two passes: the same bits; entries past
 * ndim (ndim + 1) are written as 0).  One launch, no workspace; of mg only `world` is read.  Later addition under TRX_VERSION 240.  Refusals before
 * any HIP call: TRX_ERR_ARG (mg, mg->world, theta or theta_eff NULL, B outside 1 .. 65535), TRX_ERR_NDIM. */
int trx_affine_world_theta(const trx_moving_grid *mg /*[host]*/, int ndim, int B, const float *theta, float *theta_eff, void *stream);

/* ---- Intensity moments of N volumes (the centre-of-mass initialiser of DESIGN.md section 4.17).  Extension; later addition under TRX_VERSION 240.
 * x: N volumes [D][H][W] fp32 contiguous (2-D: ndim 2, D = 1); mask: dense uint8 [N][D][H][W], nullable, non-zero = the voxel counts; offset: device
 * [N] fp32, nullable (= 0).  out [N][1 + ndim] fp64: sum w, sum w x, sum w y(, sum w z) over the counted voxels with w = v - offset[n] (formed in
 * fp64) and (x, y, z) the voxel's index along W, H, D - voxel-index units, theta's axis order.  Each block sums kMomChunk consecutive voxels of one
 * volume in fp64 (per thread in ascending voxels, a fixed shuffle tree, the waves in order) into a partial row; one wave per volume then sums the
 * rows in a fixed order.  No atomics: the same bits on every call, and a volume's sums do not depend on N.  4 B/voxel read (5 with a mask), two
 * launches.  Workspace: trx_image_moments_workspace_bytes (the partial rows; 0 = arguments rejected: ndim outside 2 .. 3, D != 1 in 2-D, a size < 1,
 * N outside 1 .. 65535, >= 2^31 voxels per volume).  Refusals before any HIP call: TRX_ERR_ARG (x, out or workspace NULL, the sizes above),
 * TRX_ERR_NDIM, TRX_ERR_WORKSPACE. */
size_t trx_image_moments_workspace_bytes(int ndim, int N, int D, int H, int W);
int trx_image_moments(const float *x, const unsigned char *mask /*nullable*/, const float *offset /*nullable*/, int ndim, int N, int D, int H, int W,
                      double *out /*[N][1 + ndim]*/, void *workspace, size_t workspace_bytes, void *stream);
/* The same with the second moments (the principal-axes initialiser of DESIGN.md section 4.21).  Later addition under TRX_VERSION 240.
 * out [N][ncol] fp64, ncol = 1 + ndim + ndim (ndim + 1) / 2:
 *   3-D  sum w, sum w x, sum w y, sum w z, sum w xx, sum w xy, sum w yy, sum w xz, sum w yz, sum w zz
 *   2-D  sum w, sum w x, sum w y, sum w xx, sum w xy, sum w yy
 * w, x, y, z as above; a product of two indices is formed in fp64, where it is exact, and enters by one fma like a first moment.  The reduction is
 * trx_image_moments' own (the kernel body is shared, a template on the order): the first 1 + ndim columns are its bits on the same input, the same
 * bits on every call, a volume's sums do not depend on N.  Ten fp64 accumulators per thread instead of four; the traffic is the same.  Workspace:
 * trx_image_moments2_workspace_bytes (partial rows of ten doubles; 0 = arguments rejected, as above).  Refusals before any HIP call: those of
 * trx_image_moments. */
size_t trx_image_moments2_workspace_bytes(int ndim, int N, int D, int H, int W);
int trx_image_moments2(const float *x, const unsigned char *mask /*nullable*/, const float *offset /*nullable*/, int ndim, int N, int D, int H, int W,
                       double *out /*[N][ncol]*/, void *workspace, size_t workspace_bytes, void *stream);

/* ---- A deformation composed with an initial affine, sampled ONCE (what elastix, NiftyReg and ANTs do with the transform of the
 * stage before).  Extension.  Later addition under TRX_VERSION 240.  vol describes the TARGET lattice S_t = (D, H, W); vol->moving holds
 * [B][channels][mg->D][mg->H][mg->W] with vol->moving_stride moving elements between batch items (trx_affine_warp_grids' layout); theta [B][TRX_PSTRIDE],
 * theta_eff[k] = theta[k] * mg->scale[k] (one fp32 multiply); flow [B][ndim][*S_t] in TARGET voxels, channel i along spatial dim i (trx_flow_warp's
 * convention).  For target voxel x:
 *   p   = x + flow(x)                        one fp32 add per axis, as trx_flow_warp
 *   n_c = (2 p_c + 1) / S_t,c - 1            closed form (xn / yn / zn are not used: p is not an integer)
 *   m   = theta_eff . (n_x, n_y, n_z, 1)     theta's row order x, y, z
 *   i_r = ((m_r + 1) S_m,r - 1) / 2          with the MOVING sizes
 *   out = bi- / trilinear sample of moving at i, zero padding
 * = grid_sample(moving, composed grid, align_corners=False).  flow == 0: trx_affine_warp_grids on closed-form coordinates; theta_eff = I on equal
 * lattices: trx_flow_warp up to the rounding of the coordinate's round trip through the normalised cube.
 * Backward: dflow_c(x) = sum_ch grad_out_ch(x) sum_r (dsample_ch / di_r) (S_m,r / 2) theta_eff[r][c] (2 / S_t,c), c converted between the flow's
 * z, y, x channel order and theta's x, y, z column order.  A gather per target voxel like the forward: no scatter, no atomics, no workspace, the same
 * bits on every call.  No gradient with respect to theta or the moving image; the nearest-neighbour and cubic forms are trx_transform_resample.  vol->target is not read.  2-D and 3-D.
 * Per voxel in 3-D the forward moves 12 B flow + 4 B out per channel + the gather, the backward 12 B flow + 4 B grad_out per channel + 12 B dflow +
 * the gather.  Refusals before any HIP call: those of trx_flow_warp / trx_flow_warp_backward, those of trx_moving_grid above, theta NULL, channels < 1.
 * CPU restatement: tests/affine_flow_ref.py. */
int trx_affine_flow_warp(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const float *theta, const float *flow, int channels,
                         float *out /*[B][channels][*S_t]*/, void *stream);
int trx_affine_flow_warp_backward(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const float *theta, const float *flow, int channels,
                                  const float *grad_out, float *dflow /*[B][ndim][*S_t]*/, void *stream);
/* trx_bspline_mi_run with the two composed kernels where trx_flow_warp / trx_flow_warp_backward stand: the deformable stage behind a rigid / affine one,
 * the moving image on its own lattice and never resampled in between.  The same loop (expand, trx_mi_loss_grad, reduce, bending, decide, update are the
 * existing launches) and the same workspace: trx_bspline_mi_workspace_bytes is the query, it depends on the target lattice alone.  cfg->mask,
 * bending_weight, base, stop_crit and flow_last keep their meaning; st->flow / ctrl are on the target lattice, in target voxels.  theta
 * [B][TRX_PSTRIDE] is read on the device on every iteration and never written.  Refusals before any HIP call: trx_bspline_mi_run's, trx_moving_grid's,
 * theta NULL.  Arbiter: tests/affine_flow_ref.py (bspline_ref.expand + the composed warp + mi_ref / mi_mask_ref under torch autograd and torch.optim). */
int trx_bspline_mi_run_grids(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const float *theta, const trx_mi_cfg *cfg,
                             const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing /*[host]*/, int iters, void *workspace,
                             size_t workspace_bytes, void *stream);
/* With mg->overlap != 0 each iteration of trx_bspline_mi_run_grids is: composed warp -> trx_affine_flow_valid -> trx_mi_loss_grad with a copy of cfg
 * whose mask is the validity bytes -> composed warp backward (grad_warped is 0 outside a mask, so dflow is 0 at an invalid voxel).  The B N validity
 * bytes lie behind the loop's workspace: trx_bspline_mi_grids_workspace_bytes is then the query (mg == NULL or overlap == 0: it equals
 * trx_bspline_mi_workspace_bytes); one byte short is TRX_ERR_WORKSPACE.  0 = arguments rejected. */
size_t trx_bspline_mi_grids_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins, const trx_moving_grid *mg /*[host]*/);
/* valid [B][*S_t] bytes (1 / 0) of the overlap rule at the composed warp's coordinate: one thread per target voxel forms i with the warp's own statement
 * (bit-identical to trx_affine_flow_warp's) and applies the rule above with target_mask (nullable, dense [B][*S_t]) and mg->mask (nullable); mg->overlap
 * itself is not read.  No workspace, the same bits on every call.  Refusals before any HIP call: trx_affine_flow_warp's, valid NULL. */
int trx_affine_flow_valid(const trx_volumes *vol, const trx_moving_grid *mg /*[host]*/, const float *theta, const float *flow,
                          const unsigned char *target_mask /*nullable*/, unsigned char *valid /*[B][*S_t]*/, void *stream);

/* ---- Nearest-neighbour and cubic B-spline resampling through the final transform (elastix FinalBSplineInterpolationOrder 3,
 * NiftyReg -inter 3 / -inter 0, ANTs BSpline / NearestNeighbor).  Extension.  Later addition under TRX_VERSION 240: new entry points only.
 * Coefficients: c = the coefficients of the interpolating cubic B-spline of s with whole-sample mirror boundaries (index i outside 0 .. n-1 reflects about
 * 0 and n-1, period 2 (n-1)) - per axis of n > 1 voxels, with z = sqrt(3) - 2, the recursive filter
 *   c+[0] = (s[0] + z^(n-1) s[n-1] + sum_{k=1..n-2} (z^k + z^(2n-2-k)) s[k]) / (1 - z^(2n-2)),  c+[k] = s[k] + z c+[k-1],
 *   c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),  c-[k] = z (c-[k+1] - c+[k]),  c = 6 c-
 * which the kernels evaluate as its impulse response, c[k] = sum_{|j| <= 16} sqrt(3) z^|j| s[mirror(k - j)] (the truncation: 4.5e-9 of the range; every
 * output independent of the others).  An axis of one voxel is left alone.  src, coef: N volumes [D][H][W] fp32 contiguous (2-D: ndim 2, D = 1; N = batch x
 * channels, at most 65535); they must not be the same buffer.  One launch per axis longer than one voxel (at least one), each reading and writing every
 * voxel once; the workspace holds the intermediate volume when there is more than one pass, so trx_spline_workspace_bytes may answer 0; SIZE_MAX =
 * arguments rejected (ndim outside 2 .. 3, a size < 1, N outside 1 .. 65535, D != 1 in 2-D, >= 2^31 voxels per volume).
 * Refusals before any HIP call: TRX_ERR_ARG (src or coef NULL, src == coef, the sizes above), TRX_ERR_NDIM, TRX_ERR_WORKSPACE. */
size_t trx_spline_workspace_bytes(int ndim, int N, int D, int H, int W);
int trx_spline_coefficients(const float *src, float *coef, int ndim, int N, int D, int H, int W, void *workspace, size_t workspace_bytes, void *stream);
/* out[B][channels][target lattice] = vol->moving [B][channels][sampled lattice] (vol->moving_stride elements between batch items) sampled at the
 * positions of exactly one of the two existing chains; vol describes the TARGET lattice as for trx_affine_flow_warp, vol->target is not read.
 *   theta == NULL: p = x + flow(x), one fp32 add per axis (trx_flow_warp); the sampled lattice is the target's; mg must be NULL.
 *   theta != NULL: trx_affine_flow_warp's closed form p -> n -> m = theta_eff . (n, 1) -> i with the MOVING sizes, theta_eff = theta (.) mg->scale;
 *                  flow == NULL: zero flow; mg == NULL: the moving lattice is the target's and the scale is 1.  (The plain affine, the two-lattice affine
 *                  and the composed warp.)
 * order 0: out = moving[rint(i)] per axis (half to even), 0 where a rounded index lies outside - trx_flow_warp's TRX_FLAG_NEAREST rule.
 * order 3: vol->moving holds the COEFFICIENTS (trx_spline_coefficients; made once, reusable for any number of transforms).  Per axis i0 = floor(i),
 *          r = i - i0, taps i0 - 1 .. i0 + 2 mirrored as above, weights ((1-r)^3, 3r^3 - 6r^2 + 4, -3r^3 + 3r^2 + 3r + 1, r^3) / 6; out = the
 *          tensor-product sum over the 4^ndim taps; out = 0 where i_a < -0.5 or i_a > S_a - 0.5 on some axis (the zero padding of every other warp
 *          here; a NaN position too).  The spline reproduces the samples at lattice points and overshoots their range near edges: no clamp.
 * Order 1 is deliberately not an order of this entry point: trx_affine_warp / _grids, trx_flow_warp and trx_affine_flow_warp are the linear form.
 * Channels share coordinates and weights.  A gather per target voxel: no atomics, no workspace, no host sync, the same bits on every call, and a
 * pair's result does not depend on its batch.  Not differentiable.  Refusals before any HIP call: those of trx_affine_warp about vol, those of
 * trx_moving_grid when mg is given, TRX_ERR_ARG for out NULL, theta and flow both NULL, mg without theta, channels < 1, order not 0 or 3.
 * CPU restatement: tests/spline_ref.py. */
int trx_transform_resample(const trx_volumes *vol, const trx_moving_grid *mg /*[host], nullable*/, const float *theta /*nullable*/,
                           const float *flow /*nullable*/, int channels, int order, float *out /*[B][channels][*S_t]*/, void *stream);

/* ---- Stationary velocity field (Arsigny et al. 2006; NiftyReg's -vel, VoxelMorph-diff's VecInt; extension: the reference has no such model, its flows
 * are displacements, ref:warpings.py:178-242).  Fields are [B][ndim][D][H][W] fp32 contiguous (2-D: [B][2][H][W], D = 1), voxel units and channel order
 * of `flow` above.  S(f, p) = the bi / trilinear sample of field f at the voxel position p, corners outside the volume contributing zero (the sampler
 * of trx_flow_warp).  With K = squarings in 0 .. 12 and s = inverse ? -1 : +1:
 *   exp:      u_0 = s 2^-K vel (exact);   u_{k+1}(x) = u_k(x) + S(u_k, x + u_k(x)), k = 0 .. K - 1;   flow = u_K   (K = 0: flow = s vel).
 *             A position is ONE fp32 add of the voxel index and the displacement; i0 = floor(p), t = p - i0, corner kappa has the weight
 *             w_kappa(t) = prod_a (kappa_a ? t_a : 1 - t_a) and ok_kappa = whether i0 + kappa lies inside the volume.
 *   adjoint of one squaring (g = dL/du_{k+1}, u = u_k, i0 and t of p = y + u(y)):
 *             dL/du_c(y) = g_c(y) + sum_x sum_kappa [i0(x) + kappa = y] ok_kappa w_kappa(t(x)) g_c(x)
 *                                 + sum_kappa ok_kappa (dw_kappa/dt_c)(t(y)) sum_a g_a(y) u_a(i0(y) + kappa);     dL/dvel = s 2^-K dL/du_0.
 * exp(vel) is a diffeomorphism up to the discretisation, and inverse != 0 gives its inverse for the price of a second integration.
 * Forward: one launch for u_0 and one per squaring (a gather; 24 B/voxel moved in 3-D).  Backward: per squaring a scatter-add (splat) and a
 * finishing pass.  The splat runs in fixed point: with m = max |g| of the pair at that level and m < 2^E, each contribution w g is rounded once to a
 * multiple of 2^(E - 31) and added with 64-bit integer atomics, LDS first (a tile of source voxels and a halo of 2), then global - at most 2^31
 * contributions of magnitude <= 2^31 per voxel, so a sum stays below 2^62; beyond the fp32 rounding of w g the splat's error per voxel is at most
 * 2^(E - 32) per contribution.  No float atomics: the same bits on every call, and a pair's result does not depend on the batch around it.  A
 * non-finite dflow gives a non-finite dvel for that pair only.  No host sync, no allocation; status codes before any HIP call: TRX_ERR_ARG (null
 * pointer, squarings outside 0 .. 12, B > 65535, more than 2^31 voxels), TRX_ERR_NDIM, TRX_ERR_WORKSPACE.
 * Workspace (trx_svf_workspace_bytes; 0 = arguments rejected), each part rounded up to 256 bytes: the levels u_0 .. u_{K-1} (K fields of
 * 4 B ndim D H W bytes), for K > 0 two gradient fields and the int64 accumulator (8 B ndim D H W bytes), and 13 B maxima of 4 bytes - 1 x 256^3 with
 * K = 6: 2.0 GB.  CPU restatement: tests/svf_ref.py (exp, exp_backward). */
size_t trx_svf_workspace_bytes(int ndim, int B, int D, int H, int W, int squarings);
/* flow = exp(+-vel); leaves u_0 .. u_{K-1} in the workspace. */
int trx_svf_exp(const float *vel, float *flow, int ndim, int B, int D, int H, int W, int squarings, int inverse, void *workspace,
                size_t workspace_bytes, void *stream);
/* dvel = (d exp(+-vel) / d vel)^T dflow.  MUST follow a trx_svf_exp call with the same vel, geometry, squarings, inverse and workspace, with nothing
 * else writing to that workspace in between: it reads the levels that call kept (vel itself is not read again).  dvel must not overlap dflow. */
int trx_svf_exp_backward(const float *vel, const float *dflow, float *dvel, int ndim, int B, int D, int H, int W, int squarings, int inverse,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Diffeomorphic free-form deformation: trx_bspline_run with the expanded lattice (+ st->base) read as a stationary VELOCITY.  Per iteration: expand ->
 * trx_svf_exp (phi, in the workspace) -> trx_flow_loss_grad at phi -> trx_svf_exp_backward into st->dflow -> reduce -> the bending / decide / update
 * launches of trx_bspline_run.  trx_bspline_state keeps its whole meaning with `flow` = the velocity: base (a velocity), bending_weight (of the velocity's
 * lattice), stop_crit, stopped, losses, flow_last (the VELOCITY of the last forward; its deformation is trx_svf_exp of it).  squarings == 0: the data term
 * is trx_bspline_run's own and the run is bit-identical to it.  Workspace: trx_bspline_svf_workspace_bytes = trx_bspline_workspace_bytes + two fields +
 * trx_svf_workspace_bytes.  Extension: arbiter = tests/bspline_ref.py::expand + tests/svf_ref.py::exp + oracle/compose.py (flow_warp, weighted_loss) under
 * torch autograd. */
size_t trx_bspline_svf_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int squarings);
int trx_bspline_svf_run(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st,
                        const int *spacing /*[host]*/, int squarings, int iters, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Jacobian determinant of a dense flow and the folding penalty on it.  Extension: the reference has neither.  Later
 * addition under TRX_VERSION 240: new entry points only.  CPU restatement: tests/jacobian_ref.py.
 * flow [B][ndim][D][H][W] fp32 in voxel units, channel a along spatial axis a (trx_svf_exp's convention).  D_b u is the difference along axis b:
 * (u(x + e_b) - u(x - e_b)) / 2 inside, u(1) - u(0) on the first voxel, u(S - 1) - u(S - 2) on the last, 0 on an axis of one voxel.
 *   J(x)[a][b] = delta_ab + (D_b u_a)(x),   det(x) = det J(x)   - a map of the full size [B][D][H][W];
 *   P_b = (1 / N) sum_x max(0, eps - det(x))^2,   N = D H W      - C^1, zero where nothing is near a fold;
 *   dP/dJ(x) = -(2 / N) max(0, eps - det(x)) cof J(x), pulled back to the flow through the adjoint of D with the same one-sided faces.
 * The determinant in voxel units is the determinant in millimetres (the two matrices are similar): nothing here depends on voxel sizes.  Behind an
 * initial affine (trx_bspline_mi_run_grids) the whole transform's local volume change is this map times the constant determinant of the affine.
 * No atomics, every sum in a fixed order (per-block fp64 partials, then a fixed-order second stage): the same bits on every call, and a pair's result does
 * not depend on the batch around it; a non-finite flow in one pair leaves the others alone.  No host sync, no allocation.  Refusals before any HIP
 * call: TRX_ERR_ARG (null pointer, a size < 1, B outside 1 .. 65535, >= 2^31 voxels, threshold or weight not finite, weight < 0), TRX_ERR_NDIM,
 * TRX_ERR_WORKSPACE. */
/* det [B][D][H][W] = the map; one launch, no workspace. */
int trx_flow_jacobian(const float *flow, int ndim, int B, int D, int H, int W, float *det, void *stream);
/* Bytes of workspace trx_flow_folding accepts: the map (4 B N bytes) and one double per 2048 voxels of a pair, each part rounded up to 256.
 * 0 = arguments rejected. */
size_t trx_flow_folding_workspace_bytes(int ndim, int B, int D, int H, int W);
/* penalty[b] = P_b (unweighted) with eps = threshold; dflow (nullable, [B][ndim][D][H][W]) = (accumulate ? dflow : 0) + weight dP/dflow -
 * trx_bspline_bending's convention.  The map is left at the start of the workspace.  dflow must not overlap flow. */
int trx_flow_folding(const float *flow, int ndim, int B, int D, int H, int W, float threshold, float weight, float *penalty /*[B]*/,
                     float *dflow /*nullable*/, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* The folding penalty inside the free-form deformation loops.  It travels in a struct of its own: trx_bspline_state does not grow. */
typedef struct {
    float weight;    /* >= 0, finite; 0: the launches and the bits of the unpenalised entry point */
    float threshold; /* eps, finite */
} trx_fold_cfg;
/* trx_bspline_run / trx_bspline_mi_run / trx_bspline_mi_run_grids (mg and theta both NULL: the one-lattice loop; both given: the composed one, its
 * overlap rule included) with objective L = data term + lambda E_b + weight P_b, P_b on the TOTAL flow st->flow = base + expand(ctrl).  Per iteration,
 * after the data term has written st->dflow and before reduce: the map and the partials (one launch), dflow += weight dP/dflow (one launch); losses[b][t]
 * and the early stop see the total; `base` receives no gradient.  Everything else - state, refusals, capacity - is the unpenalised entry point's; fold
 * NULL, a weight or threshold that is not finite, weight < 0: TRX_ERR_ARG.  Workspace: the *_fold_workspace_bytes query (the unpenalised entry point's bytes,
 * rounded up to 256, + trx_flow_folding_workspace_bytes), whatever the weight; one byte short is TRX_ERR_WORKSPACE.  The diffeomorphic loop
 * (trx_bspline_svf_run) has no such form.  Arbiter: the unpenalised loop's arbiter + weight * tests/jacobian_ref.py::penalty under torch autograd. */
size_t trx_bspline_fold_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx);
int trx_bspline_run_fold(const trx_volumes *vol, const trx_loss_cfg *loss, const trx_opt_cfg *opt, const trx_bspline_state *st,
                         const int *spacing /*[host]*/, const trx_fold_cfg *fold /*[host]*/, int iters, void *workspace, size_t workspace_bytes, void *stream);
size_t trx_bspline_mi_fold_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, int bins, const trx_moving_grid *mg /*[host], nullable*/);
int trx_bspline_mi_run_fold(const trx_volumes *vol, const trx_moving_grid *mg /*[host], nullable*/, const float *theta /*nullable*/, const trx_mi_cfg *cfg,
                            const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing /*[host]*/, const trx_fold_cfg *fold /*[host]*/, int iters,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- Composition and fixed-point inversion of dense flows.  Extension: the reference has neither.  Later addition under
 * TRX_VERSION 240: new entry points only.  CPU restatement: tests/flowops_ref.py.
 * Fields are [B][ndim][D][H][W] fp32 contiguous in voxel units, channel a along spatial axis a (trx_svf_exp's convention; 2-D: D = 1); a warp is
 * warped(x) = image(x + flow(x)).  A position is ONE fp32 add of the voxel index and the displacement.  Two samplers of a field f at a position p:
 *   S0(f, p)  trx_svf_exp's: bi / trilinear, i0 = floor(p), t = p - i0, corners outside the volume contribute zero.
 *   Sb(f, p)  border extension.  Per axis pc = min(max(p, 0), S - 1), i0 = min(floor(pc), max(S - 2, 0)), t = pc - i0, corners i0 and
 *             min(i0 + 1, S - 1), weights 1 - t and t (an axis of one voxel: t = 0).  Sb is continuous in p and its Lipschitz constant is that of f -
 *             the fixed-point iteration below needs that at the faces, where S0 ramps to zero over one voxel.
 * Compose:  c = compose(first, second),  c(x) = second(x) + S(first, x + second(x)),  S = Sb for padding 1, S0 for padding 0.
 *           image(x + c(x)) is flow_warp(flow_warp(image, first), second) up to the second interpolation: one resampling in place of two.  With padding 0,
 *           compose(u, u) is one squaring: the bits of trx_svf_exp(2u, squarings = 1).
 * Invert:   v = invert(u) is the right inverse on the lattice, (id + u) o (id + v) = id, that is v(y) = -Sb(u, y + v(y)).  Per voxel y:
 *             v_0 = init(y) (init NULL: 0);  v_{k+1} = -Sb(u, y + v_k);  r = max_a |v_{k+1,a} - v_{k,a}|;
 *           the voxel stops after the first update with r <= tol, or after `iterations` updates; residual(y) = the r of its last update, so a voxel
 *           has converged exactly when residual <= tol.  tol = 0 runs the fixed count, except for a voxel that reaches a bit-exact fixed point.
 *           Nothing in a voxel's result depends on another voxel's iteration, on the call or on the batch.  A non-finite value, the voxel's own v_k or
 *           a sampled one, ends the voxel at once with NaN in every channel of v and in residual.  A folded u has no inverse where it folds: there
 *           the iteration need not converge, the outputs stay finite and residual says where.  No damping, no convergence guarantee beyond that report.
 * Neither operator is differentiable.  One launch each, a gather per voxel: no workspace, no atomics, no host sync, no allocation.  Refusals before any
 * HIP call: TRX_ERR_NDIM (ndim not 2 or 3; ndim 2 with D != 1); TRX_ERR_ARG (a NULL pointer other than init / residual, a size < 1, B outside
 * 1 .. 65535, more than 2^31 voxels, padding not 0 or 1, iterations outside 1 .. 1000, tol negative or not finite, out == first, inverse == flow). */
/* out = compose(first, second).  out may be `second` itself (second is read at the voxel's own index only); out must not overlap first. */
int trx_flow_compose(const float *first, const float *second, float *out, int ndim, int B, int D, int H, int W, int padding /*0 zeros, 1 border*/,
                     void *stream);
/* inverse = invert(flow) from init (NULL: zero); residual NULL or [B][D][H][W].  inverse may be `init` itself (a voxel reads its own init before it
 * writes), so a run can be continued in place: K1 updates followed by K2 from that result are the bits of K1 + K2 at tol = 0.  inverse and residual
 * must not overlap flow. */
int trx_flow_invert(const float *flow, const float *init /*NULL: zero*/, float *inverse, float *residual /*NULL or [B][N]*/, int ndim, int B, int D, int H,
                    int W, int iterations /*1..1000*/, float tol /*finite, >= 0*/, void *stream);

/* ---- Points and target-space images through the whole transform, both ways.  Extension: the reference moves no point and has no
 * inverse.  Later addition under TRX_VERSION 240: new entry points only.  CPU restatement: tests/chain_ref.py.
 * Lattices have sizes S = (D, H, W), 2-D: D = 1.  Points and flows use the flow convention above: voxel-index units, component a along spatial axis a
 * (tensor order z, y, x in 3-D, y, x in 2-D).  theta is an EFFECTIVE theta [B][TRX_PSTRIDE] between normalised cubes, rows and columns in x, y, z order:
 * what trx_transform_resample takes with mg->scale = 1.  These entry points take no scale and no world record; callers convert on the host.
 * Normalise and un-normalise are trx_affine_flow_warp's closed forms, n_c = (2 p_c + 1) / S_c - 1 and i_r = ((m_r + 1) S_r - 1) / 2.  S(f, p) is a flow
 * sampled at a float position p: Sb (padding 1, border extension) or S0 (padding 0), the pair of trx_flow_compose.  Border is the natural choice: a
 * displacement should continue past the face, S0 ramps to zero there.  Two chains from a start lattice S_a to an end lattice S_b:
 *   chain 0, flow then affine.  The flow lives on S_a.  p' = p + S(flow, p), one fp32 add per axis; out = unnorm_b(theta . (norm_a(p'), 1)).  theta NULL:
 *            out = p' and S_b is not read.  These are the positions trx_affine_flow_warp samples at, for any p, not only at lattice points.
 *   chain 1, affine then flow.  The flow lives on S_b.  q = unnorm_b(theta . (norm_a(p), 1)); out = q + S(flow, q).  flow NULL: out = q.  theta NULL: the
 *            two lattices must be equal and q = p.
 * With T(p) = theta_eff(p + u(p)) the map of a registration (target voxels to moving voxels: chain 0 from the target lattice to the moving one), its
 * inverse is chain 1 from the moving lattice to the target one with theta_eff^-1 and v = trx_flow_invert(u): T^-1(q) = r + v(r), r = theta_eff^-1 q.
 * Both entry points: one launch, a gather per point / output voxel, no workspace, no atomics, no host sync, the same bits on every call, a pair's result
 * does not depend on its batch; every flow gather index is clamped into its axis in float before any conversion to int, every image gather is predicated
 * or clamped by the sampler it reuses, and no unbounded float is converted to an integer.  Not differentiable.  Refusals before any HIP call: TRX_ERR_NDIM
 * (ndim not 2 or 3, checked first; ndim 2 with a lattice whose D != 1); TRX_ERR_ARG (a NULL that is not nullable, theta and flow both NULL, theta NULL with
 * unequal lattices in chain 1, a size < 1, B outside 1 .. 65535, P < 1, a lattice of >= 2^31 voxels, channels < 1, src_stride < channels voxels of S_b,
 * order not 0, 1 or 3, padding not 0 or 1, chain not 0 or 1, out overlapping src or flow, out overlapping points without being points). */
/* out[B][P][ndim] = the chain's image of points[B][P][ndim].  out may be `points` itself (a point is read before it is written).  from_size / to_size:
 * host, {D, H, W} of S_a / S_b; to_size may be NULL in chain 0 without theta.  A non-finite component of a point gives NaN in every component of that
 * point only, and no address is formed from it; a finite point however far outside is sampled by S as the definition says. */
int trx_transform_points(const float *points, float *out, int ndim, int B, int P, const float *theta /*nullable*/, const float *flow /*nullable*/,
                         const int *from_size /*[host] [3]*/, const int *to_size /*[host] [3]*/, int chain /*0 flow then affine, 1 affine then flow*/,
                         int padding /*0 zeros, 1 border*/, void *stream);
/* out[B][channels][*S_a] (S_a = out_size): for every voxel y of the output lattice, the sample of src [B][channels][*S_b] (S_b = src_size; src_stride
 * elements between batch items) at chain 1's position of y, the flow [B][ndim][*S_b] living on src's lattice.  The resampler in the other chain order:
 * trx_transform_resample and trx_affine_flow_warp do the flow first, then the affine.  `order` selects the sampler, zero padding in every order:
 *   order 0: rint per axis, half to even; 0 where a rounded index lies outside (trx_transform_resample's rule).
 *   order 1: trx_flow_warp's bi- / trilinear sampler, corners outside the volume contributing zero, at the position clamped into [-2, S + 1] per axis
 *            (beyond -1 and S every corner lies outside, so every finite position keeps its value).
 *   order 3: src holds trx_spline_coefficients; taps, mirror rule and the 0 beyond half a voxel outside the field of view are trx_transform_resample's.
 * A NaN position (a non-finite theta or flow value) yields 0 in every order: orders 0 and 3 by the existing rule, order 1 because the clamp sends a NaN to
 * -2.  `padding` is the flow sampler's (S above), not the image's.  Channels share positions and weights.  out must not overlap src or flow. */
int trx_affine_then_flow_resample(const float *src, size_t src_stride, const int *src_size /*[host] [3]*/, const float *theta /*nullable*/,
                                  const float *flow /*nullable*/, int ndim, int B, int channels, const int *out_size /*[host] [3]*/, int order /*0, 1, 3*/,
                                  int padding /*0 zeros, 1 border*/, float *out, void *stream);

/* ---- Euclidean distance transform, mask surface and label overlap.  Extension: the reference has none of them.  Later addition
 * under TRX_VERSION 240: new entry points only.  CPU restatement: tests/distance_ref.py.
 * Volumes are [B][D][H][W] contiguous, 2-D: ndim == 2 with D == 1.  A mask is unsigned char, non-zero = set (a feature).
 *   dist2(x) = min over features y of sum_a (voxel_a (x_a - y_a))^2 - the SQUARED distance from the centre of voxel x to the centre of the nearest feature,
 *   in mm^2; voxel NULL: in voxels^2.  0 on a feature.  voxel: host, ndim floats in the tensor's axis order, (dz, dy, dx) or (dy, dx).
 * A pair without any feature gets +inf everywhere (and -1 in `nearest`) and leaves the other pairs of the batch alone.  nearest (nullable,
 * int [B][ndim][D][H][W]): the index of a feature that attains the minimum, channel a along spatial axis a (the flow convention); of several equidistant
 * features the same one on every call (per pass: the smaller axis distance, then the lower index).  The distance recomputed from it is dist2.
 * voxel == NULL: all arithmetic in integers (every size <= 16384 keeps d^2 below 2^30), dist2 is that integer correctly rounded into fp32 - exact below
 * 2^24.  With voxel sizes: fp32, weights w_a = voxel_a^2 rounded once, per pass min_j f(j) + w_a (i - j)^2 with (i - j)^2 an exact integer converted to fp32.
 * The transform is separable, one pass per axis (csrc/distance.hip): a ballot scan along x, an exact outward search along y and z inside the range of rows
 * / planes that hold a feature at all; its cost grows with the distance to the nearest feature within that range, O(n^2) per line at worst.  No atomics, no floating-point sums: the same bits on every call, a
 * pair's bits do not depend on the batch around it.  No host sync, no allocation.  Refusals before any HIP call: TRX_ERR_ARG (a NULL mask, dist2,
 * workspace, surface, label map or counts; a size < 1 or > 16384; B outside 1 .. 65535; >= 2^31 voxels; a voxel size that is not finite or <= 0;
 * L outside 1 .. 4096; label_bytes not 1 or 4), TRX_ERR_NDIM (ndim not 2 or 3, ndim == 2 with D != 1), TRX_ERR_WORKSPACE. */
/* Bytes of workspace trx_distance_transform accepts: one 4-byte value per voxel of the batch (4 B N bytes), ndim - 1 int16 index maps (2 B N bytes each),
 * one byte per row (B D H) and one per plane (B D), each part rounded up to 256, whether or not `nearest` is asked for.  0 = arguments rejected. */
size_t trx_distance_workspace_bytes(int ndim, int B, int D, int H, int W);
/* dist2 [B][D][H][W] fp32 and, if not NULL, nearest [B][ndim][D][H][W].  3 launches in 3-D, 2 in 2-D.  dist2 serves as scratch between the passes; mask
 * must not overlap dist2, nearest or the workspace. */
int trx_distance_transform(const unsigned char *mask, int ndim, int B, int D, int H, int W, const float *voxel /*[host] [ndim], nullable*/, float *dist2,
                           int *nearest /*nullable*/, void *workspace, size_t workspace_bytes, void *stream);
/* surface [B][D][H][W] unsigned char, 0 / 1: 1 where the voxel is set and at least one of its 2 ndim face neighbours is not set or lies outside the volume -
 * mask & ~binary_erosion(mask, border_value = 0) with the face-connected structuring element, MedPy's surface.  (ndim == 3 with D == 1: both z
 * neighbours lie outside, every set voxel is a surface voxel.)  One launch, no workspace.  surface must not overlap mask. */
int trx_mask_surface(const unsigned char *mask, int ndim, int B, int D, int H, int W, unsigned char *surface, void *stream);
/* counts [B][L][3] = |a = l|, |b = l|, |a = l and b = l| for l in [0, L) of two label maps [B][D][H][W], label_bytes 1: unsigned char, 4: int.  A label
 * outside [0, L) counts nowhere.  The entry point zeroes counts itself, on the stream.  Per-block 32-bit counters in LDS, flushed with 64-bit integer
 * adds: integer sums, the same bits on every call.  One memset and one launch, no workspace. */
int trx_label_overlap(const void *a, const void *b, int label_bytes /*1 or 4*/, int ndim, int B, int D, int H, int W, int L /*1 .. 4096*/,
                      unsigned long long *counts, void *stream);

/* ---- Gaussian smoothing and resampling between grid sizes.  Extension: the reference has no image filter.  Later addition
 * under TRX_VERSION 240: new entry points only.  CPU restatement: tests/gaussian_ref.py.
 * in: N volumes [D][H][W], out: N volumes [Do][Ho][Wo], both contiguous fp32 (2-D: ndim 2, D = Do = 1); out must not overlap in or the workspace.
 * sigma: host, ndim floats in VOXELS OF `in`, in the tensor's axis order, (z, y, x) or (y, x).  Separable, one pass per axis whose radius is above 0
 * or whose size changes.  Along an axis of S voxels with sigma > 0:
 *   R = (int)(truncate sigma + 0.5)    (scipy.ndimage.gaussian_filter's radius; R == 0: the axis is not filtered)
 *   g_t = exp(-((t - R) / sigma)^2 / 2) / sum g, t = 0 .. 2R: formed and normalised in fp64 on the host, used as fp32
 *   s(i) = sum_t g_t x(i - R + t), indices clamped to [0, S - 1] (padding 1, scipy's mode 'nearest') or out-of-range taps left out (padding 0,
 *   scipy's mode 'constant': the operator is then symmetric, its own adjoint when no size changes)
 * and output j is (1 - l) s(i0) + l s(i1) at trx_resample's position u (F.interpolate's; u in fp64, i0 = floor(u), i1 = min(i0 + 1, S - 1),
 * l = u - i0); an axis that keeps its size has u = j: out = s.  sigma 0 on every axis and no size change: one copy.
 * TRX_GAUSSIAN_MAX_RADIUS: the largest R (sigma = 32 voxels at truncate 4).  Taps are summed in fp32 in the order t = 0 .. 2R, s(i0) before s(i1), without
 * atomics: the same bits on every call, and a volume's bits do not depend on N.  Passes run strongest shrink first; intermediates go through the
 * workspace a chunk of volumes at a time, as trx_resample's do.  No host sync, no allocation.  Refusals before any HIP call: trx_resample's
 * (TRX_ERR_NDIM; TRX_ERR_ARG: a NULL pointer, a size < 1, >= 2^31 voxels, align_corners not 0 / 1) and TRX_ERR_ARG for sigma NULL, a sigma that is
 * negative or not finite, truncate <= 0 or not finite, R > TRX_GAUSSIAN_MAX_RADIUS, padding not 0 / 1; TRX_ERR_WORKSPACE for a workspace below the
 * query's bytes - one byte short is refused, whatever the sigmas. */
#define TRX_GAUSSIAN_MAX_RADIUS 128
/* Bytes of workspace trx_gaussian_resample accepts for this geometry: the intermediates of up to three passes, whichever axes the sigmas select.
 * 0 = arguments rejected, as trx_resample_workspace_bytes. */
size_t trx_gaussian_workspace_bytes(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo);
int trx_gaussian_resample(const float *in, float *out, int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo,
                          const float *sigma /*[host] [ndim], voxels of `in`*/, float truncate, int align_corners, int padding /*0 zeros, 1 border*/,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- Normalised gradient field criterion (NGF, Haber & Modersitzki 2006): a local multimodal data term - edges of the two images
 * should be parallel or antiparallel, whatever the intensities on either side.  Extension: the reference has none.  Later addition under TRX_VERSION 240:
 * new entry points only.  CPU restatement: tests/ngf_ref.py.
 * target / warped: [B][D][H][W] fp32, dense (D = 1 for ndim 2).  Voxel sizes h_a: cfg->voxel, 1 without.  eps[b] = (eps_t, eps_w): device [B][2], the
 * edge parameters (noise levels) of the two images.  mask: as trx_mi_cfg.mask (NULL = every voxel, N_m = the number of non-zero voxels of the pair).
 *   differences  (D_a I)(n) = sc_a(n) / h_a (I(n + (ip - n_a) e_a) - I(n - (n_a - im) e_a)), ip = min(n_a + 1, S_a - 1), im = max(n_a - 1, 0), sc = 1/2
 *                where ip - im == 2, else 1: central inside, one-sided on the faces, 0 on an axis of one voxel (trx_flow_jacobian's convention and
 *                torch.gradient's).  The kernels form (sc fl(1 / h_a)) (I(+) - I(-)) in fp32.
 *   loss         gT = D target, gW = D warped, s = <gW, gT>, a = |gW|^2 + eps_w^2, b = |gT|^2 + eps_t^2, r = s^2 / (a b), r = 0 where a b == 0 (a select:
 *                no NaN); loss[b] = alpha (1 - (1 / N_m) sum_{v in M} r(v)), in [0, alpha] up to rounding.  N_m == 0: loss and gradient 0, the other
 *                pairs untouched, as for trx_mi_loss_grad.
 *   gradient     q = dr / dgW = 2 s gT / (a b) - 2 s^2 gW / (a^2 b), 0 outside the mask and where a b == 0; grad_warped = -(alpha / N_m) D^T q, in
 *                gather form
 *                  (D^T q)(y) = sum_a (1 / h_a) [ [y_a >= 1] sc_a(y - e_a) q_a(y - e_a) + [y_a = S_a - 1] sc_a(y) q_a(y)
 *                                                - [y_a <= S_a - 2] sc_a(y + e_a) q_a(y + e_a) - [y_a = 0] sc_a(y) q_a(y) ]
 *                (the two face terms cancel on an axis of one voxel).  The target gets no gradient; eps is held constant under the gradient.  With a
 *                mask, q is 0 outside it, so grad_warped is 0 at every voxel none of whose face neighbours (nor itself) lies in the mask; a voxel
 *                just outside the mask is read by the difference at its neighbour inside and has a gradient.
 *   properties   loss(T, c W + d) == loss(T, W) for c != 0 when eps_w is scaled by |c|; in particular loss(T, 1 - W) == loss(T, W): contrast inversion
 *                costs nothing.  The zero padding of a warp outside the moving field of view is an edge like any other: `mask` is the remedy (the
 *                overlap rule of trx_moving_grid is not built for this criterion).
 * Launches: forward (2 ndim loads of each image per voxel, the y / z neighbours cache hits; r summed in fp64 per thread in ascending voxels, a fixed
 * shuffle tree, the waves in order -> one fp64 partial and one mask count per block of 2048 voxels; q [B][ndim][N] into the workspace when a gradient is
 * wanted), reduce (one wave per pair: loss[b] and the scale -alpha / N_m into the workspace - N_m never goes to the host), backward (the gather above
 * times the pair's scale; grad_warped is fully written).  grad_warped == NULL skips the q stores and the backward pass.  No atomics, no floating-point
 * sum in a data-dependent order: the same bits on every call, a pair's bits do not depend on its batch, an all-ones mask gives the bits of no mask, and a
 * loss-only call gives the loss bits of the call with a gradient.  3-D traffic: forward 8 (+ 1 with a mask) B/voxel read and 12 B/voxel written,
 * backward 12 B/voxel read and 4 B/voxel written.  No host sync, no allocation.  Refusals before any HIP call: TRX_ERR_ARG (target, warped, cfg,
 * cfg->eps, loss or workspace NULL, a size < 1, B outside 1 .. 65535, >= 2^31 voxels, alpha not finite, a voxel size that is not finite or not > 0),
 * TRX_ERR_NDIM (ndim not 2 or 3, ndim 2 with D != 1), TRX_ERR_WORKSPACE. */
typedef struct {
    float alpha;
    const float *eps;            /* device [B][2]: eps_t, eps_w; read on every evaluation: it must outlive the call / run */
    const float *voxel;          /* [host] [ndim] in the tensor's axis order, (z, y, x) or (y, x), > 0, finite; NULL = 1 */
    const unsigned char *mask;   /* as trx_mi_cfg.mask */
} trx_ngf_cfg;
size_t trx_ngf_workspace_bytes(int ndim, int B, int D, int H, int W);   /* 0 = arguments rejected */
int trx_ngf_loss_grad(const float *target, const float *warped, int ndim, int B, int D, int H, int W, const trx_ngf_cfg *cfg, float *loss /*[B]*/,
                      float *grad_warped /*nullable, [B][D][H][W]*/, void *workspace, size_t workspace_bytes, void *stream);
/* Free-form deformation + NGF: trx_bspline_mi_run with this criterion where trx_mi_loss_grad stands - per iteration expand -> warp -> trx_ngf_loss_grad ->
 * warp backward -> (folding) -> reduce -> the bending / decide / update launches of trx_bspline_run.  One entry point for every route: mg and theta both
 * NULL - one lattice, trx_flow_warp / _backward; both given - trx_affine_flow_warp / _backward, one interpolation through the initial affine theta, the
 * moving image on a lattice of its own (one of the two alone: TRX_ERR_ARG).  fold NULL or fold->weight == 0: the unpenalised loop, launch for launch;
 * otherwise the folding penalty of trx_bspline_run_fold.  mg->overlap or mg->mask: TRX_ERR_ARG (the overlap rule is not built for this criterion).
 * trx_bspline_state keeps its whole meaning (base, bending_weight, stop_crit, stopped, flow_last, losses = data term + lambda E + w P); the pairs'
 * losses take the place of terms at stride 1, as on the mutual-information route.  vol->target: dense [B][D][H][W].  Workspace: one query whatever the
 * route (the folding penalty's part included); one byte short is TRX_ERR_WORKSPACE; 0 = arguments rejected.  Refusals before any HIP call: those of
 * trx_bspline_run, trx_ngf_loss_grad's, trx_moving_grid's when mg is given, trx_fold_cfg's when fold is given; iters > losses_capacity:
 * TRX_ERR_CAPACITY.  Arbiter: tests/bspline_ref.py::expand + oracle/compose.py::flow_warp + tests/ngf_ref.py under torch autograd. */
size_t trx_bspline_ngf_workspace_bytes(int ndim, int B, int D, int H, int W, int sz, int sy, int sx, const trx_moving_grid *mg /*[host], nullable*/);
int trx_bspline_ngf_run(const trx_volumes *vol, const trx_moving_grid *mg /*[host], nullable*/, const float *theta /*nullable*/, const trx_ngf_cfg *cfg,
                        const trx_opt_cfg *opt, const trx_bspline_state *st, const int *spacing /*[host]*/, const trx_fold_cfg *fold /*[host], nullable*/,
                        int iters, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRX_H */
