"""CPU restatement of the dense-flow operators of csrc/flowops.hip (include/trx.h: trx_flow_compose, trx_flow_invert) in torch,
any dtype: the border-extension sampler Sb, compose with either padding, the fixed-point inversion with its per-voxel stop, and the cases the tests use.
Fields are [B, nd, *spatial] in voxels, channel a along spatial axis a; a position is ONE add of the voxel index and the displacement in the field's dtype."""
import itertools
import math

import torch

import svf_ref

TOL, ITERATIONS = 1e-3, 30
FIXED_K = 12      # the fixed count of the tol = 0 comparisons: the slowest voxel of any case needs 12 updates at TOL


def sample_border(f, u):
    """Sb(f, x + u(x)) for every voxel x.  Per axis pc = min(max(p, 0), S - 1), i0 = min(floor(pc), max(S - 2, 0)), t = pc - i0, corners i0 and
    min(i0 + 1, S - 1); a NaN position takes the first voxel (the kernel's fmaxf).  The weight of a corner is (t_y-factor * t_x-factor) * t_z-factor and the
    corners are added in the order z, y, x with x fastest, as in the kernel.  f: [B, C, *spatial], u: [B, nd, *spatial]."""
    B, nd = u.shape[:2]
    spatial = u.shape[2:]
    p = (svf_ref.identity(spatial, u.dtype) + u).reshape(B, nd, -1)
    idx, fac = [], []
    for a, S in enumerate(spatial):
        pc = torch.where(torch.isnan(p[:, a]), torch.zeros_like(p[:, a]), p[:, a]).clamp(0, S - 1)
        i0 = torch.floor(pc).clamp(max=max(S - 2, 0))
        t = pc - i0
        i0 = i0.long()
        idx.append((i0, (i0 + 1).clamp(max=S - 1)))
        fac.append((1 - t, t))
    flat = f.reshape(B, f.shape[1], -1)
    acc = torch.zeros_like(flat)
    for kappa in itertools.product((0, 1), repeat=nd):
        lin = torch.zeros_like(idx[0][0])
        for a, k in enumerate(kappa):
            lin = lin * spatial[a] + idx[a][k]
        w = fac[nd - 2][kappa[nd - 2]] * fac[nd - 1][kappa[nd - 1]]
        if nd == 3:
            w = w * fac[0][kappa[0]]
        acc = acc + w[:, None] * torch.gather(flat, 2, lin[:, None].expand(-1, flat.shape[1], -1))
    return acc.reshape(f.shape)


def compose(first, second, padding="border"):
    """c(x) = second(x) + S(first, x + second(x)), S = Sb ('border') or svf_ref.sample ('zeros')."""
    assert padding in ("border", "zeros")
    return second + (sample_border(first, second) if padding == "border" else svf_ref.sample(first, second))


def invert(u, iterations=ITERATIONS, tol=TOL, init=None):
    """(v, residual [B, *spatial], updates [B, *spatial]) in u's dtype: per voxel v_0 = init or 0, v_{k+1} = -Sb(u, y + v_k), r = max_a |v_{k+1,a} - v_{k,a}|;
    the voxel stops after the first update with r <= tol or after `iterations` updates; residual = the r of its last update; a non-finite v_k or sample ends
    the voxel with NaN in every channel and in residual.  updates = how many updates the voxel made."""
    v = torch.zeros_like(u) if init is None else init.to(u.dtype).clone()
    r = torch.zeros(u.shape[:1] + u.shape[2:], dtype=u.dtype)
    n = torch.zeros(r.shape, dtype=torch.long)
    active = torch.ones(r.shape, dtype=torch.bool)
    nan = torch.tensor(float("nan"), dtype=u.dtype)
    for _ in range(iterations):
        if not bool(active.any()):
            break
        vn = -sample_border(u, v)
        bad = ~(torch.isfinite(v).all(1) & torch.isfinite(vn).all(1))
        rk = (vn - v).abs().amax(1)
        v = torch.where(active[:, None], torch.where(bad[:, None], nan, vn), v)
        r = torch.where(active, torch.where(bad, nan, rk), r)
        n = n + active.long()
        active = active & ~bad & ~(rk <= tol)
    return v, r, n


def lipschitz_bound(u):
    """[B] fp64: an upper bound of the Lipschitz constant of p -> Sb(u, p) in the maximum norm.  Sb is multilinear between lattice points and constant
    outside, so along axis a no channel changes faster than the largest difference of two neighbours on that axis, and a step of |dp|_inf <= 1 moves
    every axis at once: the sum over the axes of max_{x, c} |u_c(x + e_a) - u_c(x)|.  Below one, v -> -Sb(u, y + v) is a contraction."""
    u64 = u.double()
    B = u64.shape[0]
    total = torch.zeros(B, dtype=torch.float64)
    for a in range(2, u64.dim()):
        if u64.shape[a] > 1:
            total = total + u64.diff(dim=a).abs().reshape(B, -1).amax(1)
    return total


def right_residual(u, v):
    """|v + Sb(u, y + v)| per voxel (the largest channel) in fp64: how far v is from the right inverse of u.  [B, *spatial]."""
    u64, v64 = u.double(), v.double()
    return (v64 + sample_border(u64, v64)).abs().amax(1)


# id: (B, spatial, amplitude, noise); the fields are svf_ref.smooth_field(B, spatial, amplitude, seed = 11, noise)
CASES = {"a": (1, (13, 18, 23), 1.0, 0.0),      # generic 3-D, W below one wave
         "b": (2, (9, 10, 11), 0.5, 0.01),      # B = 2
         "c": (1, (19, 26), 1.5, 0.0),          # 2-D
         "d": (1, (1, 12, 20), 1.0, 0.0),       # an axis of one voxel
         "e": (1, (7, 19, 37), 1.0, 0.01),      # rows that straddle block boundaries
         "f": (1, (5, 6, 70), 0.5, 0.0),        # W above one wave
         "g": (1, (33, 65, 70), 2.0, 0.0)}      # several blocks
# per case: the updates the slowest voxel needs at TOL, and the largest fp64 |v + Sb(u, y + v)| of the fp32 result (tests/test_flowops_host.py asserts both)
TABLE = {"a": (9, 6.5e-4), "b": (8, 4.3e-4), "c": (8, 4.6e-4), "d": (10, 4.8e-4), "e": (12, 8.3e-4), "f": (9, 4.8e-4), "g": (7, 4.9e-4)}
SLACK = 1.5e-4      # what the fp32 result may add to tol in the fp64 right-inverse residual (cases with a small contraction)
SEED, SECOND_SEED = 11, 29

_CACHE = {}


def field(case, seed=SEED):
    B, spatial, amp, noise = CASES[case]
    return svf_ref.smooth_field(B, spatial, amp, seed, noise)


def second_field(case):
    """The `second` of the compose tests: the case's field at another seed."""
    return field(case, SECOND_SEED)


def reference(case):
    """The restatement's results for a case, computed once and shared (never modified): compose with both paddings and the inversion at tol = 0 for
    FIXED_K updates in fp32 and fp64, and the early-stopping inversion at TOL in fp32."""
    if case not in _CACHE:
        u, s = field(case), second_field(case)
        r = {}
        for pad in ("border", "zeros"):
            r["c32", pad], r["c64", pad] = compose(u, s, pad), compose(u.double(), s.double(), pad)
        r["v32"], r["r32"], _ = invert(u, FIXED_K, 0.0)
        r["v64"], r["r64"], _ = invert(u.double(), FIXED_K, 0.0)
        r["stop32"] = invert(u, ITERATIONS, TOL)
        _CACHE[case] = r
    return _CACHE[case]


FOLD_SHAPE = (13, 18, 23)
FOLD_CONVERGED = 0.89      # share of the fold field's voxels that converge at TOL within ITERATIONS (asserted on the CPU to +-0.01)
CONSTANT = (1.25, -2.5, 0.75)
CONSTANT_SHAPE = (9, 10, 11)


def fold_field():
    """svf_ref.fold_field on FOLD_SHAPE as fp32: id + u folds in the middle of the volume."""
    return svf_ref.fold_field(FOLD_SHAPE).float()


def constant_field():
    return torch.tensor(CONSTANT)[None, :, None, None, None].expand((1, 3) + CONSTANT_SHAPE).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# what composition is for: one interpolation of the image in place of two
# ---------------------------------------------------------------------------------------------------------------------------------------
USE_SHAPE = (20, 24, 28)
USE_MARGIN = 4


def _use_axes(dtype):
    return svf_ref.identity(USE_SHAPE, dtype)[0]


def use_image_at(p):
    """An analytic image at the positions p [3, ...] (voxels): a product of waves with a period of about 6 voxels - fine enough for a linear
    interpolation to blur it."""
    return (torch.sin(1.05 * p[0] + 0.3) * torch.cos(0.95 * p[1] - 0.2) * torch.sin(1.1 * p[2] + 0.5) + 0.5 * torch.cos(0.6 * p[0] + 0.7 * p[1] - 0.8 * p[2]))


def use_flow_at(p, which):
    """Two analytic smooth flows at the positions p [3, ...]: amplitudes of about a voxel, wavelengths of the volume's size."""
    k = [2 * math.pi / s for s in USE_SHAPE]
    if which == "a":
        return torch.stack([0.9 * torch.sin(k[1] * p[1] + 0.4) * torch.cos(k[2] * p[2]), 1.1 * torch.cos(k[0] * p[0]) * torch.sin(k[2] * p[2] + 1.0),
                            0.8 * torch.sin(k[0] * p[0] + 0.2) * torch.cos(k[1] * p[1] - 0.5)])
    return torch.stack([0.7 * torch.cos(k[2] * p[2] - 0.3) * torch.sin(k[0] * p[0] + 0.6), 0.9 * torch.sin(k[1] * p[1] + 1.2) * torch.cos(k[0] * p[0]),
                        1.2 * torch.cos(k[1] * p[1]) * torch.sin(k[2] * p[2] - 0.9)])


def use_inputs(dtype=torch.float64):
    """(image [1,1,*S], a [1,3,*S], b [1,3,*S], truth [1,1,*S]): the image and two flows on the lattice, and the analytically composed image
    image(x + b(x) + a(x + b(x))) = flow_warp(flow_warp(image, a), b) without any interpolation.  Always evaluated in fp64, then cast."""
    x = _use_axes(torch.float64)
    b = use_flow_at(x, "b")
    truth = use_image_at(x + b + use_flow_at(x + b, "a"))
    return tuple(t[None].to(dtype) for t in (use_image_at(x)[None], use_flow_at(x, "a"), b, truth[None]))


def interior_rms(x, y, margin=USE_MARGIN):
    sl = (Ellipsis,) + (slice(margin, -margin),) * 3
    return (x[sl].double() - y[sl].double()).pow(2).mean().sqrt().item()


def use_errors(dtype=torch.float64):
    """(rms of one resampling through compose(a, b), rms of two resamplings) against the analytic image, interior, in the restatement."""
    img, a, b, truth = use_inputs(dtype)
    once = svf_ref.sample(img, compose(a, b))
    twice = svf_ref.sample(svf_ref.sample(img, a), b)
    return interior_rms(once, truth), interior_rms(twice, truth)
