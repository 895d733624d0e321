// Resampling between grid sizes (trx_resample, include/trx.h): the levels of a coarse-to-fine pyramid and the hand-over of a flow field
// from one level to the next.  Each axis is handled on its own and the operator is separable, so it runs as one 1-D pass per axis whose
// size changes:
//
//     shrink (So < S): 5-tap binomial blur [1,4,6,4,1]/16 on the input grid (replicate boundary), then linear interpolation at the output
//                      positions - folded into ONE 6-tap stencil per output: w_t = (1-l) c_t + l c_(t-1) over i0-2 .. i0+3 (clamped);
//     grow (So > S):   linear interpolation only (2 taps);
//     same size:       no pass.
//
// Output positions are F.interpolate's (area_pixel_compute_source_index): align_corners=0: u = max((j+0.5) S/So - 0.5, 0), 1:
// u = j (S-1)/(So-1); i0 = floor(u), i1 = min(i0+1, S-1), l = u - i0.  u is formed in fp64 (an fp32 u carries ~1.5e-5 of error at
// S = 256, which would show in the weights); the taps are summed in fp32 in a fixed order: no atomics, the same bits on every call.
//
// Passes run in the order of the strongest shrink first, so each later pass reads less.  Intermediates go through the caller's
// workspace, a chunk of volumes at a time: the chunk is sized so that its intermediates (<= 96 MiB) stay in the 256 MiB Infinity
// Cache between the passes, and HBM sees little beyond the input read once and the output written once.
#include "resample_plan.h"
#include "trx_common.h"

namespace trx {

#define TRX_RESAMPLE_MAX_CHANNELS 64

struct ChanScale {
    float s[TRX_RESAMPLE_MAX_CHANNELS];
};

// KIND 0: copy (no axis changes size; only the channel scale), 1: linear, 2: blur + linear.
// A volume is [outer][S][inner] in, [outer][So][inner] out; blockIdx.y walks the volumes of this launch (vol0 = index of the first one in
// the whole call, for the channel of the scale).
template <int KIND>
__global__ __launch_bounds__(TRX_BLOCK) void resample_axis_kernel(const float *__restrict__ in, float *__restrict__ out, int nvol, unsigned outer,
                                                                    int S, int So, unsigned inner, double scale, int align, int vol0, int channels,
                                                                    int use_scale, ChanScale cs)
{
    const unsigned n_out = outer * (unsigned)So * inner;
    const size_t in_vol = (size_t)outer * (unsigned)S * inner;
    for (int v = blockIdx.y; v < nvol; v += gridDim.y) {
        const float *src = in + (size_t)v * in_vol;
        float *dst = out + (size_t)v * n_out;
        const float sc = use_scale ? cs.s[(vol0 + v) % channels] : 1.f;
        for (unsigned e = blockIdx.x * TRX_BLOCK + threadIdx.x; e < n_out; e += gridDim.x * TRX_BLOCK) {
            if constexpr (KIND == 0) {
                dst[e] = src[e] * sc;
                continue;
            } else {
                const unsigned k = e % inner, r = e / inner;
                const unsigned j = r % (unsigned)So, p = r / (unsigned)So;
                const double u = align ? (double)j * scale : fmax(((double)j + 0.5) * scale - 0.5, 0.0);
                const int i0 = min((int)u, S - 1);
                const int i1 = i0 + (i0 < S - 1 ? 1 : 0);
                const float l = (i1 == i0) ? 0.f : (float)(u - (double)i0);
                const float *col = src + (size_t)p * (unsigned)S * inner + k;
                float acc;
                if constexpr (KIND == 1) {
                    acc = (1.f - l) * col[(size_t)i0 * inner] + l * col[(size_t)i1 * inner];
                } else {
                    const float c[5] = {1.f / 16, 4.f / 16, 6.f / 16, 4.f / 16, 1.f / 16};
                    acc = 0.f;
#pragma unroll
                    for (int t = 0; t < 6; t++) {
                        const float w = (t < 5 ? (1.f - l) * c[t] : 0.f) + (t > 0 ? l * c[t - 1] : 0.f);
                        const int i = min(max(i0 - 2 + t, 0), S - 1);
                        acc = fmaf(w, col[(size_t)i * inner], acc);
                    }
                }
                dst[e] = acc * sc;
            }
        }
    }
}

template <int KIND>
static int launch_axis(const float *in, float *out, int nvol, const int shape[3], int axis, int So, int align, int vol0, int channels,
                       int use_scale, const ChanScale &cs, hipStream_t s)
{
    unsigned outer = 1, inner = 1;
    for (int a = 0; a < axis; a++) outer *= (unsigned)shape[a];
    for (int a = axis + 1; a < 3; a++) inner *= (unsigned)shape[a];
    const int S = shape[axis];
    const double scale = align ? (So > 1 ? (double)(S - 1) / (double)(So - 1) : 0.0) : (double)S / (double)So;
    const size_t n_out = (size_t)outer * So * inner;
    const unsigned gy = (unsigned)std::min(nvol, 65535);
    const unsigned gx = (unsigned)std::max<size_t>(1, std::min<size_t>((n_out + TRX_BLOCK - 1) / TRX_BLOCK, std::max<size_t>(1, 8192 / gy)));
    hipLaunchKernelGGL((resample_axis_kernel<KIND>), dim3(gx, gy), dim3(TRX_BLOCK), 0, s, in, out, nvol, outer, S, So, inner, scale, align,
                       vol0, channels, use_scale, cs);
    TRX_CHECK_LAUNCH();
    return TRX_OK;
}

}  // namespace trx

using namespace trx;

extern "C" size_t trx_resample_workspace_bytes(int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo)
{
    if (resample_check(ndim, N, D, H, W, Do, Ho, Wo) != TRX_OK) return 0;
    return resample_plan(N, D, H, W, Do, Ho, Wo).ws_bytes;
}

extern "C" int trx_resample(const float *in, float *out, int ndim, int N, int D, int H, int W, int Do, int Ho, int Wo, int align_corners,
                            int channels, const float *channel_scale, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!in || !out || !workspace) return TRX_ERR_ARG;
    const int rc = resample_check(ndim, N, D, H, W, Do, Ho, Wo);
    if (rc != TRX_OK) return rc;
    if ((align_corners != 0 && align_corners != 1) || channels < 1 || (channel_scale && channels > TRX_RESAMPLE_MAX_CHANNELS)) return TRX_ERR_ARG;
    const ResamplePlan pl = resample_plan(N, D, H, W, Do, Ho, Wo);
    if (workspace_bytes < pl.ws_bytes) return TRX_ERR_WORKSPACE;
    ChanScale cs{};
    const int use_scale = channel_scale != nullptr;
    if (use_scale)
        for (int c = 0; c < channels; c++) cs.s[c] = channel_scale[c];
    hipStream_t s = (hipStream_t)stream;
    const size_t in_vol = (size_t)D * H * W, out_vol = (size_t)Do * Ho * Wo;
    float *t1 = (float *)workspace, *t2 = t1 + pl.t2_offset;
    const int So[3] = {Do, Ho, Wo};
    if (pl.npass == 0) {
        const int shape[3] = {D, H, W};
        return launch_axis<0>(in, out, N, shape, 2, W, align_corners, 0, channels, use_scale, cs, s);
    }
    for (int n0 = 0; n0 < N; n0 += pl.chunk) {
        const int nv = std::min(pl.chunk, N - n0);
        int shape[3] = {D, H, W};
        const float *src = in + (size_t)n0 * in_vol;
        for (int i = 0; i < pl.npass; i++) {
            const bool last = i == pl.npass - 1;
            float *dst = last ? out + (size_t)n0 * out_vol : (i == 0 ? t1 : t2);
            const int a = pl.axis[i];
            const int r = So[a] < shape[a] ? launch_axis<2>(src, dst, nv, shape, a, So[a], align_corners, n0, channels, last && use_scale, cs, s)
                                           : launch_axis<1>(src, dst, nv, shape, a, So[a], align_corners, n0, channels, last && use_scale, cs, s);
            if (r != TRX_OK) return r;
            shape[a] = So[a];
            src = dst;
        }
    }
    return TRX_OK;
}
