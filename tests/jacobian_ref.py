"""The definition of trx_flow_jacobian / trx_flow_folding (include/trx.h) in torch, on the CPU, in any dtype, the field
cases and loop rows of their tests, and the arbiters of the penalised free-form deformation loops (trx_bspline_run_fold,
trx_bspline_mi_run_fold): bspline_ref.expand followed by the existing data terms, plus weight * penalty, under torch autograd + torch.optim.
Nothing here touches the GPU; tests/test_jacobian_host.py asserts the conditions the GPU tests rest on.  Not a test."""
import functools

import numpy as np
import torch

import affine_flow_ref as fr
import bspline_bending_ref as bref
import bspline_ref
import loop_arbiters as la
import mi_mask_ref as mref
import mi_ref
import svf_ref
from oracle import compose

EPS = 0.3      # the default threshold


def diff(u, dim):
    """D u along tensor dimension `dim`: central inside, one-sided on the first and the last voxel, 0 on an axis of one voxel."""
    S = u.shape[dim]
    if S == 1:
        return torch.zeros_like(u)
    n = lambda a, b: u.narrow(dim, a, b)  # noqa: E731
    parts = [n(1, 1) - n(0, 1)]
    if S > 2:
        parts.append((n(2, S - 2) - n(0, S - 2)) / 2)
    parts.append(n(S - 1, 1) - n(S - 2, 1))
    return torch.cat(parts, dim=dim)


def jacobian(flow):
    """[B, *spatial, nd, nd]: J[a][b] = delta_ab + D_b flow_a."""
    nd = flow.shape[1]
    rows = [torch.stack([diff(flow[:, a], 1 + b) + (1.0 if a == b else 0.0) for b in range(nd)], dim=-1) for a in range(nd)]
    return torch.stack(rows, dim=-2)


def det(flow):
    """[B, *spatial], by the cofactor expansion along the first row (differentiable; torch.linalg.det is not used so that fp32 means fp32)."""
    J = jacobian(flow)
    if flow.shape[1] == 2:
        return J[..., 0, 0] * J[..., 1, 1] - J[..., 0, 1] * J[..., 1, 0]
    c = lambda a1, b1, a2, b2: J[..., a1, b1] * J[..., a2, b2]  # noqa: E731
    return (J[..., 0, 0] * (c(1, 1, 2, 2) - c(1, 2, 2, 1)) + J[..., 0, 1] * (c(1, 2, 2, 0) - c(1, 0, 2, 2))
            + J[..., 0, 2] * (c(1, 0, 2, 1) - c(1, 1, 2, 0)))


def penalty(flow, eps=EPS):
    """[B]: (1 / N) sum_x max(0, eps - det(x))^2."""
    h = torch.clamp(eps - det(flow), min=0)
    return (h * h).reshape(flow.shape[0], -1).mean(1)


def penalty_grad(flow, eps=EPS, dtype=torch.float64):
    """(P [B], dP_b/dflow [B, nd, *spatial]) in `dtype` by autograd (the pairs are independent, so the gradient of the sum is per pair)."""
    fl = flow.to(dtype).clone().requires_grad_()
    p = penalty(fl, eps)
    (g,) = torch.autograd.grad(p.sum(), fl)
    return p.detach(), g


def gather_grad(flow, eps=EPS):
    """dP/dflow in fp64 the way the kernel forms it: dP/dJ = -(2 / N) max(0, eps - det) cof J, and voxel y collects, per axis b, from the lower and
    the upper stencil neighbour n (the clamped index: y itself on a face) the coefficient of u(y) in (D_b u)(n)."""
    fl = flow.double()
    B, nd = fl.shape[:2]
    sp = tuple(fl.shape[2:])
    J = jacobian(fl)
    d = det(fl)
    cof = torch.linalg.inv(J).transpose(-1, -2) * d[..., None, None] if nd == 3 else torch.stack(
        [torch.stack([J[..., 1, 1], -J[..., 1, 0]], -1), torch.stack([-J[..., 0, 1], J[..., 0, 0]], -1)], -2)
    q = -(2.0 / np.prod(sp)) * torch.clamp(eps - d, min=0)
    out = torch.zeros_like(fl)
    for b, S in enumerate(sp):
        j = torch.arange(S)
        sc = lambda k: torch.where((k >= 1) & (k <= S - 2), 0.5, 1.0)  # noqa: E731
        lo, hi = (j - 1).clamp(min=0), (j + 1).clamp(max=S - 1)
        edge = 1.0 if S > 1 else 0.0
        c_lo = torch.where(j >= 1, sc(lo), torch.full_like(sc(lo), -edge))
        c_hi = torch.where(j <= S - 2, -sc(hi), torch.full_like(sc(hi), edge))
        shape = [1] * (1 + nd)
        shape[1 + b] = S
        for a in range(nd):
            w = q * cof[..., a, b]
            out[:, a] += c_lo.reshape(shape) * w.index_select(1 + b, lo) + c_hi.reshape(shape) * w.index_select(1 + b, hi)
    return out


# (B, spatial, amplitude, seed) of svf_ref.smooth_field(..., noise=0.3): an axis of one voxel, of two voxels, W below and above one wave, B = 2, 2-D.
FIELD_CASES = [(1, (5, 6, 7), 2, 1), (2, (9, 10, 11), 4, 2), (1, (13, 18, 23), 6, 3), (1, (1, 12, 20), 5, 4), (1, (2, 3, 70), 3, 5), (1, (19, 26), 8, 6),
               (2, (20, 33, 70), 12, 7), (1, (1, 1, 9), 2, 8), (1, (40, 2), 3, 9)]
FACES_COVERED = 7      # in the first seven cases active voxels lie on both faces of every axis longer than one voxel
# Two more, for the kernels' block boundaries.  A block of the map / gather passes takes kFoldChunk = 2048 consecutive voxels of a pair:
#   (7, 19, 37): 4921 voxels, blocks end at voxels 2048 and 4096 = (z 2, y 17, x 13) and (z 5, y 15, x 26) - in the middle of a row, so the x, y and z
#                neighbours of voxels next to a boundary belong to another block on every axis;
#   (33, 65, 70): 150150 voxels = 74 blocks, more partial sums than the 64 lanes of the second stage.
BLOCK_CASES = [(1, (7, 19, 37), 10, 10), (1, (33, 65, 70), 16, 11)]
KERNEL_CHUNK = 2048
CASES = FIELD_CASES + BLOCK_CASES


def case_id(c):
    return f"{c[0]}x" + "x".join(str(s) for s in c[1])


@functools.lru_cache(maxsize=None)
def field(case):
    """fp32 [B, nd, *spatial] of a CASES row."""
    B, spatial, amp, seed = case
    return svf_ref.smooth_field(B, spatial, amp, seed, noise=0.3)


@functools.lru_cache(maxsize=None)
def reference(case, eps=EPS):
    """dict(det64, det32, p64, p32, g64, g32) as numpy fp64 arrays: computed once per process, shared, never written to."""
    fl = field(case)
    p64, g64 = penalty_grad(fl, eps, torch.float64)
    p32, g32 = penalty_grad(fl, eps, torch.float32)
    out = dict(det64=det(fl.double()), det32=det(fl), p64=p64, p32=p32, g64=g64, g32=g32)
    return {k: v.double().numpy() for k, v in out.items()}


BUMP_SHAPE = (33, 65, 70)


@functools.lru_cache(maxsize=None)
def bump_field():
    """fp32 [1, 3, *BUMP_SHAPE]: a smooth ripple too weak to fold anywhere plus a contraction towards one point, so that the active voxels form a
    ball of a few hundred voxels in a volume of 74 kernel chunks: most blocks of the gather see no active voxel within reach and leave at once,
    those around the ball do not."""
    ax = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in BUMP_SHAPE], indexing="ij")
    c = (14.3, 30.6, 41.2)
    r2 = sum((x - ci) ** 2 for x, ci in zip(ax, c))
    bump = torch.stack([-1.3 * (x - ci) * torch.exp(-r2 / (2 * 4.0 ** 2)) for x, ci in zip(ax, c)])
    ripple = torch.stack([0.2 * torch.sin(0.3 * ax[(k + 1) % 3] + k) for k in range(3)])
    return (bump + ripple)[None].float()


def chunk_activity(d, eps=EPS):
    """bool per kernel chunk of pair 0: whether a voxel of it is active."""
    flat = np.asarray(d)[0].reshape(-1) < eps
    pad = (-flat.size) % KERNEL_CHUNK
    return np.concatenate([flat, np.zeros(pad, dtype=bool)]).reshape(-1, KERNEL_CHUNK).any(1)


def active_share(d, eps=EPS):
    return float(np.mean(np.asarray(d) < eps))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the penalised loops: 10 iterations, eps = 0.3
# ---------------------------------------------------------------------------------------------------------------------------------------
ITERS = 10
NCC_ROW = dict(shape=(20, 24, 28), spacing=(5, 4, 6), amp=10.0, seed=7, optimizer="adam", lr=0.1, weight=2e3)
MI_WEIGHT = 20.0
MI_ROWS = {"adam": 25.0, "masked": 25.0, "bending": 25.0, "sgd": 25.0, "2d": 50.0}      # affine_flow_ref.LOOPS row -> multiplier of its ctrl0


def ncc_setup():
    r = NCC_ROW
    mov, tgt = la.loop_pair(r["shape"])
    return mov, tgt, la.bspline_ctrl0(1, r["shape"], r["spacing"], r["seed"], amp=r["amp"])


def _run(objective, ctrl0, optimizer, lr, dtype, iters=ITERS):
    """objective(p) -> (data term + bending, flow): (losses, penalties, share of active voxels per iteration, final control tensor)."""
    p = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses, pens, shares = [], [], []
    for _ in range(iters):
        opt.zero_grad()
        e, pen, share = objective(p)
        e.backward()
        opt.step()
        losses.append(e.item())
        pens.append(pen)
        shares.append(share)
    return np.asarray(losses), np.asarray(pens), np.asarray(shares), p.detach().numpy().copy()


def _with_penalty(data, flow, weight, eps):
    if not weight:
        d = det(flow.detach())
        return data, 0.0, float((d < eps).double().mean())
    pen = weight * penalty(flow, eps).sum()
    return data + pen, pen.item(), float((det(flow.detach()) < eps).double().mean())


@functools.lru_cache(maxsize=None)
def ncc_loop(weight, dtype, iters=ITERS, eps=EPS):
    r = NCC_ROW
    mov, tgt, ctrl0 = ncc_setup()
    mov, tgt = mov.to(dtype), tgt.to(dtype)

    def objective(p):
        flow = bspline_ref.expand(p, r["shape"], r["spacing"], dtype=dtype)
        return _with_penalty(compose.weighted_loss(tgt, compose.flow_warp(mov, flow), w_ncc=1.0), flow, weight, eps)
    return _run(objective, ctrl0, r["optimizer"], r["lr"], dtype, iters)


def mi_setup(name):
    """affine_flow_ref.loop_setup with the control tensor scaled by the row's multiplier."""
    mov, tgt, theta, mask, rng, ctrl0 = fr.loop_setup(name)
    return mov, tgt, theta, mask, rng, ctrl0 * MI_ROWS[name]


@functools.lru_cache(maxsize=None)
def mi_loop(name, weight, dtype, iters=ITERS, eps=EPS):
    tshape, _, spacing, optimizer, lr, _, lam = fr.LOOPS[name]
    mov, tgt, theta, mask, rng, ctrl0 = mi_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)

    def objective(p):
        flow = bspline_ref.expand(p, tshape, spacing, dtype=dtype)
        warped = fr.warp(mov, theta, flow, None, dtype)
        e = (mi_ref.loss(tgt, warped, rng=rng, dtype=dtype, **mi) if mask is None else mref.loss(tgt, warped, mask, rng=rng, dtype=dtype, **mi)).sum()
        if lam:
            e = e + lam * bref.energy_squares(p, tshape, spacing, dtype=dtype).sum()
        return _with_penalty(e, flow, weight, eps)
    return _run(objective, ctrl0, optimizer, lr, dtype, iters)


def loop_rows():
    """id -> a function (weight, dtype) -> (losses, penalties, shares, ctrl)"""
    rows = {"ncc": lambda w, dt: ncc_loop(w, dt)}
    for name in MI_ROWS:
        rows["mi-" + name] = functools.partial(lambda n, w, dt: mi_loop(n, w, dt), name)
    return rows


def row_weight(row):
    return NCC_ROW["weight"] if row == "ncc" else MI_WEIGHT


# ---------------------------------------------------------------------------------------------------------------------------------------
# what it is for: the two Register runs (40 iterations from zero, Adam 0.3)
# ---------------------------------------------------------------------------------------------------------------------------------------
USE_ITERS, USE_LR = 40, 0.3
USE_NCC = dict(shape=(16, 18, 20), spacing=3, weight=1e4)
USE_MI = dict(tshape=(12, 14, 16), mshape=(15, 13, 18), spacing=2, weight=100.0)


def use_ncc_pair():
    return la.loop_pair(USE_NCC["shape"])


def use_mi_pair():
    import affine_mi_grids_ref as gref
    return gref.pair(USE_MI["tshape"], USE_MI["mshape"])


@functools.lru_cache(maxsize=None)
def use_run(kind, weight, eps=EPS):
    """The fp64 arbiter of a Register run from a zero control tensor: dict(min_det, folded, data, min_det_run) - the minimum determinant and the share
    of voxels with det <= 0 of the LAST FORWARD's flow (what Register hands out as .theta), the data term there, and the smallest minimum over the run."""
    dt = torch.float64
    if kind == "ncc":
        shape, spacing = USE_NCC["shape"], USE_NCC["spacing"]
        mov, tgt = (t.to(dt) for t in use_ncc_pair())
        data = lambda flow: compose.weighted_loss(tgt, compose.flow_warp(mov, flow), w_ncc=1.0)  # noqa: E731
    else:
        shape, spacing = USE_MI["tshape"], USE_MI["spacing"]
        mov, tgt = use_mi_pair()
        theta, rng = fr.loop_theta(3), mi_ref.fit_range(tgt, mov)
        data = lambda flow: mi_ref.loss(tgt, fr.warp(mov, theta, flow, None, dt), rng=rng, dtype=dt, bins=32, alpha=1.0, normalized=False).sum()  # noqa: E731
    p = torch.zeros((1, 3) + bspline_ref.grid(shape, spacing), dtype=dt, requires_grad=True)
    opt = torch.optim.Adam([p], USE_LR)
    mins = []
    for _ in range(USE_ITERS):
        opt.zero_grad()
        flow = bspline_ref.expand(p, shape, spacing, dtype=dt)
        e = data(flow)
        last = dict(data=e.item())
        if weight:
            e = e + weight * penalty(flow, eps).sum()
        e.backward()
        opt.step()
        d = det(flow.detach())
        last.update(min_det=d.min().item(), folded=(d <= 0).double().mean().item())
        mins.append(last["min_det"])
    last["min_det_run"] = min(mins)
    return last
