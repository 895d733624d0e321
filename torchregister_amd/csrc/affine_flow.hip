// A deformation composed with an initial affine, sampled once: trx_affine_flow_warp and trx_affine_flow_warp_backward.
// The moving image keeps its own lattice (trx_moving_grid); the flow lives on the target lattice, in target voxels.  For target voxel x:
//   p = x + flow(x)                       one fp32 add per axis (trx_flow_warp's position)
//   n_c = (2 p_c + 1) / S_t,c - 1         closed form of affine_grid's base coordinate at a non-integer position (vol's xn / yn / zn tables are not used)
//   m = theta_eff . (n_x, n_y, n_z, 1)    theta_eff = theta (.) scale (ami_theta_eff); this line and the next are affine_coord (trx_common.h),
//   i_r = unnorm<ND>(m_r, S_m,r)          with the MOVING sizes - the call affine_warp_grids_kernel makes
//   out = sample3 / sample2 of moving at i (zero padding)
// With flow == 0 every operation is affine_warp_grids_kernel's on the closed-form coordinates: the same bits.  Backward, per target voxel (a gather like
// the forward: no scatter, no atomics, no workspace, the same bits on every call):
//   dflow_c = sum_r (sum_ch grad_out_ch dsample_ch / di_r) J[r][c],   J[r][c] = theta_eff[r][c] S_m,r / S_t,c   ((S_m,r / 2) (2 / S_t,c): the two halves cancel)
// with c between the flow's z, y, x channel order and theta's x, y, z column order.  theta_eff and J are formed once per block from uniform values and
// pinned to SGPRs; the size ratios S_m,r / S_t,c come from the host as a kernel argument (a uniform fp32 division still runs on the vector unit, per
// lane: nine of them in a thread's prologue were a third of the backward's instructions).  One thread per target voxel, x fastest, blocks in
// memory order: the blocks in flight cover a few consecutive planes of the target, so at a rotated pose their gathers share cache lines (a
// grid-stride walk over 4096 blocks, trx_flow_warp's count, measured 12 % .. 15 % faster at theta = I and 1.6 .. 1.7 x slower at 0.2 rad at
// 1 x 256^3: DESIGN.md section 4.14); flow, grad_out, out and dflow are coalesced streams touched once per call and carry the non-temporal hint; the
// moving gather goes through the caches.  No LDS.
// CPU restatement: tests/affine_flow_ref.py.
#include "affine_host.h"

namespace trx {

// S_m,r / S_t,c in theta's [row r][column c] order (x, y, z), formed on the host in fp32
struct AfRatios {
    float v[3][3];
};

// BWD false: io = out [B][channels][target lattice].  BWD true: io = dflow [B][ND][target lattice], grad_out [B][channels][target lattice].
// chan_stride: moving voxels between channels.
template <int ND, bool BWD>
__global__ __launch_bounds__(TRX_BLOCK) void affine_flow_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, const float *__restrict__ flow,
                                                                int channels, size_t chan_stride, AfRatios ratio, const float *__restrict__ grad_out,
                                                                float *__restrict__ io)
{
    constexpr int NT = ND * (ND + 1);
    const int b = blockIdx.y;
    const int D = vol.D, H = vol.H, W = vol.W, Dm = mg.D, Hm = mg.H, Wm = mg.W;
    const size_t nvox = (size_t)D * H * W;
    const float *__restrict__ mov = vol.moving + (size_t)b * vol.moving_stride;
    const float *__restrict__ fl = flow + (size_t)b * ND * nvox;
    float te[NT];
    ami_theta_eff<ND>(theta + (size_t)b * TRX_PSTRIDE, mg, te);
    float J[ND][ND];   // [theta row r: x, y, z][flow channel c: z, y, x]
    if constexpr (BWD) {
#pragma unroll
        for (int r = 0; r < ND; r++)
#pragma unroll
            for (int c = 0; c < ND; c++) {
                const int col = ND - 1 - c;
                J[r][c] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(te[r * (ND + 1) + col] * ratio.v[r][col])));
            }
    }
    const size_t i = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i < nvox) {
        const unsigned row = (unsigned)i / (unsigned)W, zz = row / (unsigned)H;
        const int x = (int)((unsigned)i - row * (unsigned)W), y = (int)(row - zz * (unsigned)H), z = (int)zz;
        float f[ND], ic[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) f[c] = __builtin_nontemporal_load(fl + c * nvox + i);
        af_coord<ND>(te, f, x, y, z, D, H, W, Dm, Hm, Wm, ic);
        if constexpr (!BWD) {
            float *__restrict__ o = io + (size_t)b * channels * nvox;
            for (int ch = 0; ch < channels; ch++) {
                float v;
                if constexpr (ND == 3) v = sample3(mov + ch * chan_stride, Dm, Hm, Wm, ic[0], ic[1], ic[2]).v;
                else v = sample2(mov + ch * chan_stride, Hm, Wm, ic[0], ic[1]).v;
                __builtin_nontemporal_store(v, o + ch * nvox + i);
            }
        } else {
            const float *__restrict__ go = grad_out + (size_t)b * channels * nvox;
            float *__restrict__ df = io + (size_t)b * ND * nvox;
            float a[ND];   // sum_ch grad_out_ch dsample_ch / di_r, r = x, y, z
#pragma unroll
            for (int r = 0; r < ND; r++) a[r] = 0.f;
            for (int ch = 0; ch < channels; ch++) {
                const float g = __builtin_nontemporal_load(go + ch * nvox + i);
                if constexpr (ND == 3) {
                    const Samp3 s = sample3(mov + ch * chan_stride, Dm, Hm, Wm, ic[0], ic[1], ic[2]);
                    a[0] = fmaf(g, s.dx, a[0]); a[1] = fmaf(g, s.dy, a[1]); a[2] = fmaf(g, s.dz, a[2]);
                } else {
                    const Samp2 s = sample2(mov + ch * chan_stride, Hm, Wm, ic[0], ic[1]);
                    a[0] = fmaf(g, s.dx, a[0]); a[1] = fmaf(g, s.dy, a[1]);
                }
            }
#pragma unroll
            for (int c = 0; c < ND; c++) {
                float acc = a[0] * J[0][c];
#pragma unroll
                for (int r = 1; r < ND; r++) acc = fmaf(a[r], J[r][c], acc);
                __builtin_nontemporal_store(acc, df + c * nvox + i);
            }
        }
    }
}

// The overlap rule at the warp's coordinate (trx_affine_flow_valid; include/trx.h: trx_moving_grid): the prologue of the kernel above
// to af_coord - the same statements on the same values, so the same coordinate bit for bit -, then valid = target mask byte (if any) and overlap_valid
// (bounds, then the moving-mask byte at rint).  One thread per target voxel, one byte written per voxel; a voxel outside the target mask forms no coordinate.
template <int ND>
__global__ __launch_bounds__(TRX_BLOCK) void affine_flow_valid_kernel(trx_volumes vol, MovingLattice mg, const float *__restrict__ theta, const float *__restrict__ flow,
                                                                      const unsigned char *__restrict__ tmask, const unsigned char *__restrict__ mmask,
                                                                      unsigned char *__restrict__ valid)
{
    constexpr int NT = ND * (ND + 1);
    const int b = blockIdx.y;
    const int D = vol.D, H = vol.H, W = vol.W, Dm = mg.D, Hm = mg.H, Wm = mg.W;
    const size_t nvox = (size_t)D * H * W;
    const float *__restrict__ fl = flow + (size_t)b * ND * nvox;
    float te[NT];
    ami_theta_eff<ND>(theta + (size_t)b * TRX_PSTRIDE, mg, te);
    const size_t i = (size_t)blockIdx.x * TRX_BLOCK + threadIdx.x;
    if (i >= nvox) return;
    bool ok = !tmask || tmask[(size_t)b * nvox + i] != 0;
    if (ok) {
        const unsigned row = (unsigned)i / (unsigned)W, zz = row / (unsigned)H;
        const int x = (int)((unsigned)i - row * (unsigned)W), y = (int)(row - zz * (unsigned)H), z = (int)zz;
        float f[ND], ic[ND];
#pragma unroll
        for (int c = 0; c < ND; c++) f[c] = __builtin_nontemporal_load(fl + c * nvox + i);
        af_coord<ND>(te, f, x, y, z, D, H, W, Dm, Hm, Wm, ic);
        ok = overlap_valid<ND>(ic, Dm, Hm, Wm, mmask ? mmask + (size_t)b * Dm * Hm * Wm : nullptr);
    }
    valid[(size_t)b * nvox + i] = ok ? 1 : 0;
}

// what both entry points refuse, before any HIP call
static int af_check(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, int channels)
{
    if (!mg) return TRX_ERR_ARG;
    int rc = check_vol(vol, false);
    if (rc == TRX_OK) rc = ami_grid_check(vol->ndim, mg);
    if (rc != TRX_OK) return rc;
    if (!theta || !flow || channels < 1) return TRX_ERR_ARG;
    return TRX_OK;
}

template <bool BWD>
static int af_launch(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, int channels, const float *grad_out, float *io,
                     hipStream_t s)
{
    const size_t nvox = (size_t)vol->D * vol->H * vol->W, nmov = (size_t)mg->D * mg->H * mg->W;
    const dim3 grid((unsigned)((nvox + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)vol->B), block(TRX_BLOCK);   // one thread per voxel: < 2^23 blocks (check_vol)
    const float St[3] = {(float)vol->W, (float)vol->H, (float)vol->D}, Sm[3] = {(float)mg->W, (float)mg->H, (float)mg->D};
    AfRatios ratio;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) ratio.v[r][c] = Sm[r] / St[c];
    with_ndim(vol->ndim, [&](auto nd) {
        hipLaunchKernelGGL((affine_flow_kernel<decltype(nd)::value, BWD>), grid, block, 0, s, *vol, *mg, theta, flow, channels, nmov, ratio, grad_out, io);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" int trx_affine_flow_warp(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, int channels, float *out,
                                    void *stream)
{
    const int rc = af_check(vol, mg, theta, flow, channels);
    if (rc != TRX_OK) return rc;
    if (!out) return TRX_ERR_ARG;
    return af_launch<false>(vol, mg, theta, flow, channels, nullptr, out, (hipStream_t)stream);
}

extern "C" int trx_affine_flow_warp_backward(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, int channels,
                                             const float *grad_out, float *dflow, void *stream)
{
    const int rc = af_check(vol, mg, theta, flow, channels);
    if (rc != TRX_OK) return rc;
    if (!grad_out || !dflow) return TRX_ERR_ARG;
    return af_launch<true>(vol, mg, theta, flow, channels, grad_out, dflow, (hipStream_t)stream);
}

extern "C" int trx_affine_flow_valid(const trx_volumes *vol, const trx_moving_grid *mg, const float *theta, const float *flow, const unsigned char *target_mask,
                                     unsigned char *valid, void *stream)
{
    const int rc = af_check(vol, mg, theta, flow, 1);
    if (rc != TRX_OK) return rc;
    if (!valid) return TRX_ERR_ARG;
    const size_t nvox = (size_t)vol->D * vol->H * vol->W;
    const dim3 grid((unsigned)((nvox + TRX_BLOCK - 1) / TRX_BLOCK), (unsigned)vol->B), block(TRX_BLOCK);
    with_ndim(vol->ndim, [&](auto nd) {
        hipLaunchKernelGGL((affine_flow_valid_kernel<decltype(nd)::value>), grid, block, 0, (hipStream_t)stream, *vol, *mg, theta, flow, target_mask, mg->mask, valid);
    });
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}
