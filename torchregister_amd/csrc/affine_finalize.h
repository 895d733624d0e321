// Device side of the affine finalise, shared by the step's finalise kernel and the carry prologue of the step kernels (affine.hip), the loss
// and backward finalise kernels (affine_finalize.hip) and the pose kernels of affine_lattice.hip: the layout constants of the partial rows
// and the carry buffers, loss and coefficients from the moments, Theta and its vector-Jacobian product, the row reduction, the per-pair
// epilogue (fin_load / fin_apply) and the carry prologue.  Device functions only: every kernel is instantiated in exactly one .hip file.
#pragma once
#include "trx_dev.h"
#include "trx_common.h"
#include "affine_host.h"

namespace trx {

constexpr int np_full(int nd) { return 5 + 3 * nd * (nd + 1); }
// rows_used[b] (the step kernels' note to the finalise kernel): low 24 bits = partial rows the pair's kernel wrote, bits 24-27 = which body
// (1 + dual_choice for the tile kernel: 1 GeomD, 2 GeomA, 3 GeomR, 4 GeomRD, 5 z-streaming inside it; 6 = the z-streaming kernel, 7 = the
// exact-footprint kernel, 8 = the z-streaming kernel's flat tile), NEGATIVE when a kernel in front of the tile kernel took the pair.  Read back by AffineSolver.bodies().
constexpr int kRowsMask = 0xFFFFFF;
__host__ __device__ constexpr int rows_note(int rows, int body) { return rows > 0 ? (rows | (body << 24)) : 0; }
constexpr int kNpMse = 13;   // partial-row layout of the MSE / SSD-only step kernel (3-D): sum d^2, then 12 x sum(d J)

struct LossCoef {
    double total, mse, ncc, ssd, cy, cw, c0;
};

__device__ __forceinline__ LossCoef loss_from_moments(const double *S, double n, const trx_loss_cfg &lc)
{
    const double Sy = S[0], Sw = S[1], Syy = S[2], Sww = S[3], Syw = S[4];
    const double my = Sy / n, mw = Sw / n;
    const double Saa = Syy - Sy * my, Sbb = Sww - Sw * mw, Sab = Syw - Sy * mw;
    const double s = sqrt(Saa * Sbb + 1e-10);  // EPSILON, ref:utils.py:15,201
    const double alpha = lc.ncc_alpha;
    const double sq = Syy - 2.0 * Syw + Sww;
    LossCoef r;
    r.mse = sq / n;
    r.ncc = alpha * (1.0 - Sab / s);
    r.ssd = (double)lc.ssd_alpha * sq;
    r.total = (double)lc.w_mse * r.mse + (double)lc.w_ncc * r.ncc + (double)lc.w_ssd * r.ssd;
    // dNCCloss/dw_p = -alpha*(a_p/s - Sab*Saa*b_p/s^3); a = y - my, b = w - mw
    const double k1 = -alpha / s, k2 = alpha * Sab * Saa / (s * s * s);
    const double q = (double)lc.w_mse * 2.0 / n + (double)lc.w_ssd * (double)lc.ssd_alpha * 2.0;
    r.cy = (double)lc.w_ncc * k1 - q;
    r.cw = (double)lc.w_ncc * k2 + q;
    r.c0 = (double)lc.w_ncc * (-k1 * my - k2 * mw);
    return r;
}

template <int ND>
__device__ void theta_from_pose(const float *p, double *th)
{
    if constexpr (ND == 3) {
        double cps, sps;
        sincos((double)p[0], &sps, &cps);
        double cth, sth;
        sincos((double)p[1], &sth, &cth);
        double cph, sph;
        sincos((double)p[2], &sph, &cph);
        th[0] = cps * cth; th[1] = sph * sps * cth - cph * sth; th[2] = cph * sps * cth + sph * sth; th[3] = 0.25 * tanh((double)p[3]);
        th[4] = cps * sth; th[5] = sph * sps * sth + cph * cth; th[6] = cph * sps * sth - sph * cth; th[7] = 0.25 * tanh((double)p[4]);
        th[8] = -sps;      th[9] = sph * cps;                   th[10] = cph * cps;                  th[11] = 0.25 * tanh((double)p[5]);
    } else {
        double c, s;
        sincos((double)p[0], &s, &c);
        th[0] = c; th[1] = -s; th[2] = p[1];
        th[3] = s; th[4] = c;  th[5] = p[2];
    }
}

template <int ND>
__device__ void pose_vjp(const float *p, const double *g, double *dx)
{
    if constexpr (ND == 3) {
        double cps, sps;
        sincos((double)p[0], &sps, &cps);
        double cth, sth;
        sincos((double)p[1], &sth, &cth);
        double cph, sph;
        sincos((double)p[2], &sph, &cph);
        dx[0] = g[0] * (-sps * cth) + g[1] * (sph * cps * cth) + g[2] * (cph * cps * cth) + g[4] * (-sps * sth) +
                g[5] * (sph * cps * sth) + g[6] * (cph * cps * sth) + g[8] * (-cps) + g[9] * (-sph * sps) + g[10] * (-cph * sps);
        dx[1] = g[0] * (-cps * sth) + g[1] * (-sph * sps * sth - cph * cth) + g[2] * (-cph * sps * sth + sph * cth) +
                g[4] * (cps * cth) + g[5] * (sph * sps * cth - cph * sth) + g[6] * (cph * sps * cth + sph * sth);
        dx[2] = g[1] * (cph * sps * cth + sph * sth) + g[2] * (-sph * sps * cth + cph * sth) +
                g[5] * (cph * sps * sth - sph * cth) + g[6] * (-sph * sps * sth - cph * cth) + g[9] * (cph * cps) + g[10] * (-sph * cps);
        for (int i = 0; i < 3; i++) {
            const double t = tanh((double)p[3 + i]);
            dx[3 + i] = g[3 + 4 * i] * 0.25 * (1.0 - t * t);
        }
    } else {
        double c, s;
        sincos((double)p[0], &s, &c);
        dx[0] = g[0] * (-s) + g[1] * (-c) + g[3] * c + g[4] * (-s);
        dx[1] = g[2];
        dx[2] = g[5];
    }
}

template <int NP>
__device__ __forceinline__ void reduce_partials(const float *__restrict__ part, int nblk, double *S /*shared [64]*/)
{
    __shared__ double acc[TRX_FIN_THREADS / 64][64];
    const int tid = threadIdx.x, k = tid & 63, grp = tid >> 6;
    constexpr int NG = TRX_FIN_THREADS / 64;
    double s = 0.0;
    if (k < NP) {
        // batches of 16 independent loads per thread (all in flight together: one memory round trip for up to 256 rows),
        // fixed summation order
        for (int blk0 = grp; blk0 < nblk; blk0 += 16 * NG) {
            float a[16];
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int blk = blk0 + i * NG;
                const float v = part[(size_t)min(blk, nblk - 1) * NP + k];   // clamped, unconditional: a predicated load compiles to
                a[i] = (blk < nblk) ? v : 0.f;                              // branch + s_waitcnt per load (16 serial round trips)
            }
            s += ((((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3])) + (((double)a[4] + (double)a[5]) + ((double)a[6] + (double)a[7]))) +
                 ((((double)a[8] + (double)a[9]) + ((double)a[10] + (double)a[11])) + (((double)a[12] + (double)a[13]) + ((double)a[14] + (double)a[15])));
        }
    }
    acc[grp][k] = s;
    __syncthreads();
    if (tid < 64) {
        double t = 0.0;
#pragma unroll
        for (int i = 0; i < NG; i++) t += acc[i][tid];
        S[tid] = t;
    }
    __syncthreads();
}

// The per-pair epilogue of an iteration, shared by the finalise kernel and by the CARRY prologue of the step kernels (round 6: the finalise of
// iteration t folded into the first kernel of iteration t + 1): lanes 0 .. 63 of ONE wave, lane i owns parameter i.  fin_load issues every load of
// the pair's state at once (callers put the partial rows' reduction between the two, so that state and rows share one wait); fin_apply turns the
// reduced sums S[] into loss, dL/dtheta, (rigid) the pose chain rule, the optimiser update and theta of the next forward.
template <int ND>
struct FinRegs {
    int t;
    float best_prev, theta_old, p_old, m_old, v_old;
    float pose_old[(ND == 3) ? 6 : 3];
};
template <int ND>
__device__ __forceinline__ FinRegs<ND> fin_load(const float *param, const float *theta, const float *am, const float *av, const int *step, const float *best_loss,
                                                bool adam, bool rigid, int i)
{
    constexpr int NT = ND * (ND + 1), NPOSE = (ND == 3) ? 6 : 3;
    FinRegs<ND> r;
    const int ic = min(i, NT - 1);
    r.t = *step;
    r.best_prev = best_loss ? *best_loss : 0.f;
    r.theta_old = theta[ic]; r.p_old = param[ic];
    r.m_old = r.v_old = 0.f;
    if (adam) { r.m_old = am[ic]; r.v_old = av[ic]; }
#pragma unroll
    for (int k = 0; k < NPOSE; k++) r.pose_old[k] = rigid ? param[k] : 0.f;
    return r;
}
// Adam's bias terms of iteration t: 1 - beta1^(t+1) and 1 / sqrt(1 - beta2^(t+1)) (1 and 1 for SGD).  fin_apply keeps its own copy of these lines: calling
// this function there changes the code of the step kernels' carry prologue (compared instruction by instruction), and those kernels are the headline.
__device__ __forceinline__ void fin_bias(const trx_opt_cfg &oc, int t, double &bc1, double &rsbc2)
{
    bc1 = 1.0; rsbc2 = 1.0;
    if (oc.kind == TRX_OPT_ADAM) {   // beta^(t+1) by repeated squaring: a dozen fp64 multiplies instead of two pow() calls
        bc1 = 1.0 - ipow((double)oc.beta1, t + 1);
        rsbc2 = 1.0 / sqrt(1.0 - ipow((double)oc.beta2, t + 1));
    }
}
// The second half of the epilogue, behind whatever produced the pair's loss and lane i's dL/dtheta_i (fin_apply: the moments of the fused MSE / NCC / SSD
// step; the mutual-information loop of affine_mi.hip: its table kernel and its own partial rows): the records, (rigid) the pose chain rule, the
// optimiser update and theta of the next forward.  bc1, rsbc2: fin_bias.  Outputs: the pair's state (param / theta / Adam moments / step: nullable - the
// carry prologue's non-designated blocks write none), the caller-visible per-iteration records (losses[t], best theta / loss / index, grad: `user`), and
// theta of the next forward into LDS (`theta_lds`, nullable).
template <int ND>
__device__ __forceinline__ void fin_update(double total, double dth_i, double bc1, double rsbc2, const FinRegs<ND> &r, int b, int i, const trx_opt_cfg &oc,
                                           const trx_affine_state &st, float *param_out, float *theta_out, float *m_out, float *v_out, int *step_out, bool user,
                                           float *theta_lds, double *sh_dth, float *sh_pose)
{
    constexpr int NT = ND * (ND + 1);
    constexpr int NPOSE = (ND == 3) ? 6 : 3;
    const bool rigid = st.mode == TRX_PARAM_RIGID;
    const int np = rigid ? NPOSE : NT;
    const int t = r.t;
    const float lossf = (float)total;
    // best = first strict minimum, theta of THIS forward (ref:warpings.py:85-93)
    const bool is_best = (t == 0) || (lossf < r.best_prev);
    if (user) {
        if (is_best && i < NT) st.best_theta[(size_t)b * TRX_PSTRIDE + i] = r.theta_old;
        if (i == 0) {
            if (st.losses && t < st.losses_capacity) st.losses[(size_t)b * st.losses_capacity + t] = lossf;
            if (is_best) { st.best_loss[b] = lossf; st.best_idx[b] = t; }
        }
    }
    if (i == 0 && step_out) *step_out = t + 1;

    double g_i = dth_i;
    if (rigid) {
        if (i < NT) sh_dth[i] = dth_i;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        double dth[NT], g[NT];
#pragma unroll
        for (int k = 0; k < NT; k++) dth[k] = sh_dth[k];
        pose_vjp<ND>(r.pose_old, dth, g);
        g_i = 0.0;
#pragma unroll
        for (int k = 0; k < NPOSE; k++) g_i = (k == i) ? g[k] : g_i;
    }
    float p_new = r.p_old;
    if (i < np) {
        const float gf = (float)g_i;
        if (user && st.grad) st.grad[(size_t)b * TRX_PSTRIDE + i] = gf;
        if (oc.kind == TRX_OPT_ADAM) {
            const float mi = r.m_old + (gf - r.m_old) * (1.0f - oc.beta1);
            const float vi = oc.beta2 * r.v_old + (1.0f - oc.beta2) * gf * gf;
            if (m_out) { m_out[i] = mi; v_out[i] = vi; }
            const float denom = (float)(sqrt((double)vi) * rsbc2) + oc.eps;
            p_new = r.p_old - (float)((double)oc.lr / bc1) * (mi / denom);
        } else {
            p_new = r.p_old - oc.lr * gf;
        }
        if (param_out) param_out[i] = p_new;
    }
    float th_new = p_new;
    if (rigid) {
        if (i < NPOSE) sh_pose[i] = p_new;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        float pose_new[NPOSE];
#pragma unroll
        for (int k = 0; k < NPOSE; k++) pose_new[k] = sh_pose[k];
        double thd[NT];
        theta_from_pose<ND>(pose_new, thd);
        double th_i = 0.0;
#pragma unroll
        for (int k = 0; k < NT; k++) th_i = (k == i) ? thd[k] : th_i;
        th_new = (float)th_i;
    }
    if (i < NT) {
        if (theta_out) theta_out[i] = th_new;
        if (theta_lds) theta_lds[i] = th_new;
    }
}

// The fused MSE / NCC / SSD step: loss and lane i's dL/dtheta_i from the reduced moments, then fin_update (outputs: see there).
template <int ND>
__device__ __forceinline__ void fin_apply(const double *S, const FinRegs<ND> &r, int b, int i, double nvox, int D, int H, int W, const trx_loss_cfg &lc, const trx_opt_cfg &oc,
                                          const trx_affine_state &st, int mse_rows, float *param_out, float *theta_out, float *m_out, float *v_out, int *step_out, bool user,
                                          float *theta_lds, double *sh_dth, float *sh_pose)
{
    constexpr int NT = ND * (ND + 1);
    const int ic = min(i, NT - 1);
    const int t = r.t;
    double bc1 = 1.0, rsbc2 = 1.0;
    if (oc.kind == TRX_OPT_ADAM) {   // beta^(t+1) by repeated squaring: a dozen fp64 multiplies instead of two pow() calls
        bc1 = 1.0 - ipow((double)oc.beta1, t + 1);
        rsbc2 = 1.0 / sqrt(1.0 - ipow((double)oc.beta2, t + 1));
    }
    const double scale[3] = {0.5 * W, 0.5 * H, 0.5 * D};
    double dth_i, total;
    if (ND == 3 && mse_rows) {   // S[0] = sum (w - y)^2, S[1 + i] = sum (w - y) J_i:  L = (w_mse / n + w_ssd alpha) S[0],  dL/dw_p = q (w_p - y_p)
        const double q = (double)lc.w_mse * 2.0 / nvox + (double)lc.w_ssd * (double)lc.ssd_alpha * 2.0;
        total = 0.5 * q * S[0];
        dth_i = scale[ic / (ND + 1)] * q * S[1 + ic];
    } else {
        const LossCoef L = loss_from_moments(S, nvox, lc);
        total = L.total;
        dth_i = scale[ic / (ND + 1)] * (L.c0 * S[5 + ic] + L.cy * S[5 + NT + ic] + L.cw * S[5 + 2 * NT + ic]);
    }
    fin_update<ND>(total, dth_i, bc1, rsbc2, r, b, i, oc, st, param_out, theta_out, m_out, v_out, step_out, user, theta_lds, sh_dth, sh_pose);
}

// The carry buffers of trx_affine_run's one-launch iterations (two of them, by iteration parity): per pair 64 floats -
// theta[12] | param[12] | Adam m[12] | Adam v[12] | step (int) - the state the iteration's FIRST kernel computes in its prologue and every block of it reads.
constexpr int kCarryStride = 64;
constexpr int kCarryTheta = 0, kCarryParam = 12, kCarryM = 24, kCarryV = 36, kCarryStep = 48;

// CARRY (round 6): the finalise of iteration t - reduction of the partial rows, loss, dL/dtheta, optimiser, theta of the next forward - folded into the
// prologue of iteration t + 1's step kernel, so that an iteration of a launch-bound registration (one pair up to ~128^3: a 12 us kernel and a 4 us
// finalise launch behind it, profiles/r05e_configs.txt) is ONE launch.  No rendezvous between blocks: EVERY block of a pair reduces that pair's rows of
// the previous launch (other parity of the two partial buffers) in the same fixed order and computes the same theta; the pair's first block alone
// writes the state (into the carry buffer of this parity: blocks of this launch that start later still read the other one), the loss curve and the
// best-theta record.  trx_affine_run enqueues iters such launches and one finalise kernel behind the last (the flush).
struct CarryKArgs {
    const float *prev_partials;   // partial rows of the previous iteration (nullptr: nothing pending - the first launch of a run)
    const int *prev_rows_used;    // ... and its per-pair notes
    int prev_nblk;                // row stride of prev_partials
    int mse_rows;
    const float *state_prev;      // carry buffer the state is read from (nullptr: the caller's arrays - the first launch of a run)
    float *state_next;            // carry buffer the pair's first block writes
    double nvox;
    trx_loss_cfg lc;
    trx_opt_cfg oc;
    trx_affine_state st;
};
typedef const __attribute__((address_space(4))) CarryKArgs *CarryKPtr;

// The carry prologue of a 512-thread step block (3-D): see CarryKArgs.  `scratch`: the block's tile box (free until the body starts); on return s_th[0 .. 11]
// holds theta of this launch's forward and every wave has passed a barrier behind it.
template <int MODE>
__device__ __forceinline__ void carry_prologue(CarryKPtr c, int b, bool designated, int D, int H, int W, float *scratch, float *s_th, int wave, int lane)
{
    constexpr int NP = (MODE == 4) ? kNpMse : np_full(3);
    constexpr int NT = 12;
    const float *prev = c->prev_partials;
    const float *sp = c->state_prev;
    float *sn = c->state_next;
    const trx_affine_state st = {c->st.mode, c->st.param, c->st.theta, c->st.adam_m, c->st.adam_v, c->st.best_theta, c->st.best_loss, c->st.best_idx, c->st.losses,
                                 c->st.losses_capacity, c->st.step, c->st.grad};
    const trx_opt_cfg oc = {c->oc.kind, c->oc.lr, c->oc.beta1, c->oc.beta2, c->oc.eps};
    const bool adam = oc.kind == TRX_OPT_ADAM, rigid = st.mode == TRX_PARAM_RIGID;
    // where the pair's state is read from: the carry buffer of the other parity, or (first launch of a run) the caller's arrays
    const float *src_theta = sp ? sp + (size_t)b * kCarryStride + kCarryTheta : st.theta + (size_t)b * TRX_PSTRIDE;
    const float *src_param = sp ? sp + (size_t)b * kCarryStride + kCarryParam : st.param + (size_t)b * TRX_PSTRIDE;
    const float *src_m = sp ? sp + (size_t)b * kCarryStride + kCarryM : (st.adam_m ? st.adam_m + (size_t)b * TRX_PSTRIDE : nullptr);
    const float *src_v = sp ? sp + (size_t)b * kCarryStride + kCarryV : (st.adam_v ? st.adam_v + (size_t)b * TRX_PSTRIDE : nullptr);
    const int *src_step = sp ? reinterpret_cast<const int *>(sp + (size_t)b * kCarryStride + kCarryStep) : st.step + b;
    float *nxt = (designated && sn) ? sn + (size_t)b * kCarryStride : nullptr;
    if (prev == nullptr) {   // nothing pending: theta of this forward is the state's; the pair's first block seeds the carry buffer
        if (wave == 0) {
            const int ic = min(lane, NT - 1);
            const float th = src_theta[ic], pa = src_param[ic];
            const float m0 = (adam && src_m) ? src_m[ic] : 0.f, v0 = (adam && src_v) ? src_v[ic] : 0.f;
            const int t = *src_step;
            if (lane < NT) {
                s_th[lane] = th;
                if (nxt) { nxt[kCarryTheta + lane] = th; nxt[kCarryParam + lane] = pa; nxt[kCarryM + lane] = m0; nxt[kCarryV + lane] = v0; }
            }
            if (lane == 0 && nxt) *reinterpret_cast<int *>(nxt + kCarryStep) = t;
        }
        __syncthreads();
        return;
    }
    double *acc = reinterpret_cast<double *>(scratch);   // [8][64] | S[64] | dtheta[12] | pose (floats)
    double *S = acc + 8 * 64, *sh_dth = S + 64;
    float *sh_pose = reinterpret_cast<float *>(sh_dth + NT);
    FinRegs<3> r;
    if (wave == 0) r = fin_load<3>(src_param, src_theta, src_m, src_v, src_step, designated ? st.best_loss + b : nullptr, adam, rigid, lane);
    {
        // the pair's rows of the previous launch: wave w sums rows w, w + 8, ... of column `lane` in batches of 16 independent loads, a fixed order, the same
        // in every block of the pair.  (Measured alternatives, profiles/r06b_carry.txt: copying the rows into LDS with float4 loads first, +0.4 ... +1.2 us;
        // a grid without the surplus blocks of the geometry the pair does not run, +-0.)
        const int nblk = c->prev_nblk;
        const int rows = min(abs(c->prev_rows_used[b]) & kRowsMask, nblk);
        const float *part = prev + (size_t)b * nblk * NP;
        double s = 0.0;
        if (lane < NP) {
            constexpr int NB = TRX_CARRY_BATCH;   // loads in flight per lane
            for (int r0 = wave; r0 < rows; r0 += NB * 8) {
                float a[NB];
#pragma unroll
                for (int i = 0; i < NB; i++) {
                    const int row = r0 + i * 8;
                    const float v = part[(size_t)min(row, rows - 1) * NP + lane];   // clamped, unconditional (reduce_partials: a predicated load is a branch + a wait each)
                    a[i] = (row < rows) ? v : 0.f;
                }
                double d[NB];
#pragma unroll
                for (int i = 0; i < NB; i++) d[i] = (double)a[i];
#pragma unroll
                for (int w = 1; w < NB; w <<= 1)   // pairwise tree, fixed order
#pragma unroll
                    for (int i = 0; i + w < NB; i += 2 * w) d[i] += d[i + w];
                s += d[0];
            }
        }
        acc[wave * 64 + lane] = s;
    }
    __syncthreads();
    if (wave == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < 8; w++) t += acc[w * 64 + lane];
        S[lane] = t;
    }
    __syncthreads();
    if (wave == 0) {
        const trx_loss_cfg lc = {c->lc.w_mse, c->lc.w_ncc, c->lc.ncc_alpha, c->lc.w_ssd, c->lc.ssd_alpha};
        fin_apply<3>(S, r, b, lane, c->nvox, D, H, W, lc, oc, st, c->mse_rows, nxt ? nxt + kCarryParam : nullptr, nxt ? nxt + kCarryTheta : nullptr,
                     nxt ? nxt + kCarryM : nullptr, nxt ? nxt + kCarryV : nullptr, nxt ? reinterpret_cast<int *>(nxt + kCarryStep) : nullptr, designated, s_th, sh_dth, sh_pose);
    }
    __syncthreads();
}

}  // namespace trx
