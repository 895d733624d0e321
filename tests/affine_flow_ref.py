"""The definition of the composed warp (trx_affine_flow_warp, trx_affine_flow_warp_backward, trx_bspline_mi_run_grids)
in torch, on the CPU, in fp64 or fp32.  For target voxel x of a lattice S_t, a flow in target voxels and theta_eff = theta * scale:
  p = x + flow(x);   n_c = (2 p_c + 1) / S_t,c - 1;   m = theta_eff (n_x, n_y, n_z, 1);   out = grid_sample(moving, m, align_corners=False)
(grid_sample un-normalises with the MOVING sizes: i_r = ((m_r + 1) S_m,r - 1) / 2).  The backward is torch autograd; `analytic_backward` is the
closed formula of the kernel, built on a sampler written out corner by corner.  Also here: level_theta restated point by point, and the arbiter
of the loop (bspline_ref.expand + this warp + mi_ref / mi_mask_ref under autograd and torch.optim).  Nothing here touches the GPU;
tests/test_affine_flow_host.py asserts the conditions the GPU tests rely on.  Not a test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import affine_mi_grids_ref as gref
import bspline_bending_ref as bref
import bspline_ref
import mi_mask_ref as mref
import mi_ref
import phantoms as ph


def effective(theta, scale=None):
    """theta [B,nd,nd+1] times the scale as the kernels hold it (fp32), in theta's dtype; scale None = ones."""
    return theta if scale is None else theta * gref.kernel_scale(scale).to(theta.dtype)


def composed_grid(theta_eff, flow):
    """[B, *S_t, nd] (x, y(, z) last - grid_sample's order): theta_eff applied to the normalised positions voxel + flow."""
    B, nd = flow.shape[:2]
    St = tuple(flow.shape[2:])
    idx = torch.meshgrid(*[torch.arange(s, dtype=flow.dtype) for s in St], indexing="ij")
    n = [(2.0 * (idx[c] + flow[:, c]) + 1.0) / St[c] - 1.0 for c in range(nd)]            # tensor axis order (z, y, x)
    hom = torch.stack(n[::-1] + [torch.ones_like(n[0])], dim=-1)                          # (n_x, n_y(, n_z), 1)
    return torch.einsum("b...k,brk->b...r", hom, theta_eff.to(flow.dtype).reshape(-1, nd, nd + 1).expand(B, nd, nd + 1))


def warp(x, theta, flow, scale=None, dtype=torch.float64):
    """[B, C, *S_t]: x [B, C, *S_m] sampled once at the composed positions; differentiable with respect to flow."""
    grid = composed_grid(effective(theta.to(dtype), scale), flow.to(dtype))
    return F.grid_sample(x.to(dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def sample_coords(theta, flow, moving_shape, scale=None):
    """The un-normalised moving coordinate i [B, *S_t, nd] (x, y(, z) last) in fp64."""
    m = composed_grid(effective(theta.double(), scale), flow.double())
    Sm = torch.tensor(tuple(moving_shape)[::-1], dtype=torch.float64)
    return ((m + 1.0) * Sm - 1.0) / 2.0


def backward(x, theta, flow, grad_out, scale=None, dtype=torch.float64):
    """dL/dflow for dL/dout = grad_out, by autograd."""
    fl = flow.to(dtype).clone().requires_grad_()
    (g,) = torch.autograd.grad(warp(x, theta, fl, scale, dtype), fl, grad_out.to(dtype))
    return g


def sample_with_derivatives(x, coords):
    """The bi- / trilinear sample with zero padding written out corner by corner: x [B, C, *S_m], coords [B, *S_t, nd] (x, y(, z) last) ->
    (value [B, C, *S_t], derivative with respect to the un-normalised coordinate [nd][B, C, *S_t] in x, y(, z) order)."""
    B, C = x.shape[:2]
    Sm = tuple(x.shape[2:])
    nd = len(Sm)
    St = tuple(coords.shape[1:-1])
    flat = x.reshape(B, C, -1)
    i0 = torch.floor(coords)
    t = coords - i0
    i0 = i0.long()
    val = torch.zeros((B, C) + St, dtype=x.dtype)
    der = [torch.zeros((B, C) + St, dtype=x.dtype) for _ in range(nd)]
    for corner in range(2 ** nd):
        k = [(corner >> r) & 1 for r in range(nd)]                       # offset along x, y(, z)
        ok = torch.ones((B,) + St, dtype=torch.bool)
        lin = torch.zeros((B,) + St, dtype=torch.long)
        for r in reversed(range(nd)):                                    # z, y, x: the tensor's axis a = nd - 1 - r
            S = Sm[nd - 1 - r]
            i = i0[..., r] + k[r]
            ok &= (i >= 0) & (i < S)
            lin = lin * S + i.clamp(0, S - 1)
        v = torch.gather(flat, 2, lin.reshape(B, 1, -1).expand(-1, C, -1)).reshape((B, C) + St) * ok[:, None].to(x.dtype)
        w = [t[..., r] if k[r] else 1.0 - t[..., r] for r in range(nd)]
        val = val + v * functools.reduce(lambda a, b: a * b, w)[:, None]
        for r in range(nd):
            dw = functools.reduce(lambda a, b: a * b, [(1.0 if k[q] else -1.0) * torch.ones_like(w[q]) if q == r else w[q] for q in range(nd)])
            der[r] = der[r] + v * dw[:, None]
    return val, der


def analytic_backward(x, theta, flow, grad_out, scale=None):
    """dflow_c = sum_ch grad_out_ch sum_r (dsample_ch / di_r) (S_m,r / 2) theta_eff[r][c] (2 / S_t,c) in fp64, c converted between the flow's
    z, y, x channel order and theta's x, y, z column order: the formula of the kernel."""
    B, nd = flow.shape[:2]
    St, Sm = tuple(flow.shape[2:]), tuple(x.shape[2:])
    te = effective(theta.double(), scale).reshape(-1, nd, nd + 1).expand(B, nd, nd + 1)
    _, der = sample_with_derivatives(x.double(), sample_coords(theta, flow, Sm, scale))
    a = [(grad_out.double() * der[r]).sum(1) for r in range(nd)]       # [B, *S_t] per theta row r
    out = torch.zeros_like(flow, dtype=torch.float64)
    for c in range(nd):                                                  # flow channel c (z, y, x) <-> theta column nd - 1 - c
        col = nd - 1 - c
        for r in range(nd):
            out[:, c] += a[r] * (Sm[nd - 1 - r] / 2.0) * te[:, r, col].reshape((B,) + (1,) * nd) * (2.0 / St[c])
    return out


def kept_voxels(theta, flow, moving_shape, scale=None, eps=1e-3):
    """[B, *S_t] bool: the voxels of the backward comparisons - the fp64 sample coordinate is farther than eps from an integer on every axis (the
    trilinear derivative jumps there, and fp32 may land on the other side)."""
    i = sample_coords(theta, flow, moving_shape, scale)
    return ((i - torch.round(i)).abs() > eps).all(-1)


def outside_fraction(theta, flow, moving_shape, scale=None):
    """Share of target voxels whose sample has at least one corner outside the moving volume (the zero-padding paths)."""
    i = sample_coords(theta, flow, moving_shape, scale)
    Sm = torch.tensor(tuple(moving_shape)[::-1], dtype=torch.float64)
    return ((i < 0) | (i > Sm - 1)).any(-1).double().mean().item()


def level_theta_pointwise(theta, target_full, target_level, moving_full, moving_level, points):
    """The chain level_theta folds into one matrix, point by point in fp64: `points` [N, nd] are (fractional) voxel positions of the target LEVEL
    lattice in the tensor's axis order; returns (the normalised level coordinates of those points in x, y(, z) order with a trailing 1 [N, nd+1],
    the normalised coordinates on the moving LEVEL lattice [N, nd] they are sent to through the FULL lattices)."""
    nd = len(target_full)

    def up(j, S, Sl):        # level voxel -> full voxel (align_corners=True pyramids)
        return j if S == Sl else j * (S - 1) / (Sl - 1)

    n_lvl, n_full = [], []
    for a in range(nd):
        j = points[:, a].double()
        n_lvl.append((2.0 * j + 1.0) / target_level[a] - 1.0)
        n_full.append((2.0 * up(j, target_full[a], target_level[a]) + 1.0) / target_full[a] - 1.0)
    hom_full = torch.stack(n_full[::-1] + [torch.ones_like(n_full[0])], dim=-1)
    hom_lvl = torch.stack(n_lvl[::-1] + [torch.ones_like(n_lvl[0])], dim=-1)
    m = hom_full @ theta.double().reshape(nd, nd + 1).T                  # normalised, full moving lattice, (x, y, z)
    out = []
    for r in range(nd):
        S, Sl = moving_full[nd - 1 - r], moving_level[nd - 1 - r]
        i = ((m[:, r] + 1.0) * S - 1.0) / 2.0                            # full moving voxel
        jm = i if S == Sl else i * (Sl - 1) / (S - 1)                    # level moving voxel
        out.append((2.0 * jm + 1.0) / Sl - 1.0)
    return hom_lvl, torch.stack(out, dim=-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the warp cases of the GPU tests: B = 2 with a map per pair, 2 channels, a smooth flow with jitter (off the voxel lattice), for scale = 1 and
# for the world scale of VOXEL_M / VOXEL_T.
# The backward comparisons leave out voxels whose sample coordinate lies within 1e-3 of an integer on some axis, and those may be at most 0.5 %
# of a case.  A coordinate that varies from voxel to voxel is that close with probability 2e-3 per axis: 0.4 % in 2-D, 0.6 % in 3-D.  So in
# 3-D one row of each pair's map follows ONE target axis (z for pair 0, x for pair 1: between them every entry of theta is exercised), and the
# flow channel of that axis depends on that axis alone: that coordinate takes S_t distinct values, none of them near an integer for the seeds
# below, and the other two rows are generic.  tests/test_affine_flow_host.py asserts both conditions and the share of samples that leave the
# moving field of view (5 % .. 50 %) for every case and both scales.
# ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (target shape, moving shape, seed, zoom of the map: below 1 on the short lattices, whose border is a large share of them)
CASES = {
    "9x11x13": ((9, 11, 13), (12, 7, 15), 6, 0.8),
    "20x33x70": ((20, 33, 70), (17, 40, 31), 1, 1.0),
    "17x19": ((17, 19), (14, 23), 14, 1.0),
    "w5": ((11, 9, 5), (8, 10, 7), 12, 0.75),
}
ALIGNED_ROW = (2, 0)      # 3-D, per pair: the row of theta (x, y, z order) that follows one target axis


def case_scale(name, world):
    """ones, or the world scale of VOXEL_M / VOXEL_T of tests/affine_mi_grids_ref.py."""
    tshape, mshape = CASES[name][:2]
    if not world:
        return gref.scale_of(mshape, tshape)
    return gref.scale_of(mshape, tshape, *((gref.VOXEL_M3, gref.VOXEL_T3) if len(tshape) == 3 else (gref.VOXEL_M2, gref.VOXEL_T2)))


def case_thetas(name, world):
    """[2, nd, nd+1] fp32, the UNSCALED thetas: theta * case_scale(name, world) is a rotation-like map with generic entries, zoomed and shifted so
    that part of the target leaves the moving field of view - another one per pair and per scale."""
    tshape, _, seed, zoom = CASES[name]
    nd = len(tshape)
    g = torch.Generator().manual_seed(100 + seed + 1000 * int(world))
    base = torch.tensor(ph.THETA_ROT3 if nd == 3 else ph.THETA_STAR2, dtype=torch.float64)
    out = []
    for b in range(2):
        te = base.clone()
        te[:, :nd] = te[:, :nd] * (zoom + 0.08 * b) + 0.06 * (torch.rand(nd, nd, generator=g, dtype=torch.float64) - 0.5)
        te[:, nd] = 0.12 * (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) + (0.06 if b else -0.06)
        if nd == 3:
            r = ALIGNED_ROW[b]
            te[r, :nd] = 0.0
            te[r, r] = zoom + 0.02 + 0.1 * torch.rand(1, generator=g, dtype=torch.float64).item()
        out.append(te / case_scale(name, world))
    return torch.stack(out).float()


@functools.lru_cache(maxsize=None)
def case(name, world=False):
    """(x [2,2,*S_m], theta [2,nd,nd+1], flow [2,nd,*S_t], grad_out [2,2,*S_t]) fp32 of a CASES row; x, flow and grad_out do not depend on `world`."""
    tshape, mshape, seed, _ = CASES[name]
    nd = len(tshape)
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.cat([ph.blobs(mshape, 10 * seed + 2 * b + c) for c in range(2)], dim=1) for b in range(2)]) + 0.05 * torch.rand((2, 2) + mshape, generator=g)
    lin = [torch.linspace(-1, 1, s, dtype=torch.float64) for s in tshape]
    axes = torch.meshgrid(*lin, indexing="ij")
    flow = torch.stack([torch.stack([(0.9 + 0.3 * b) * torch.sin((1.3 + 0.4 * c) * axes[(c + 1) % nd] + 2.0 * axes[(c + 2) % nd] * (nd == 3) + 0.3 * c + b)
                                     for c in range(nd)]) for b in range(2)])
    flow = flow + 0.13 * (torch.rand(flow.shape, generator=g, dtype=torch.float64) - 0.5)
    if nd == 3:
        for b in range(2):
            a = nd - 1 - ALIGNED_ROW[b]                              # the tensor axis (and flow channel) of the aligned row
            line = 0.8 * torch.sin(2.3 * lin[a] + b) + 0.13 * (torch.rand(tshape[a], generator=g, dtype=torch.float64) - 0.5)
            flow[b, a] = line.reshape([-1 if k == a else 1 for k in range(nd)]).expand(tshape)
    grad_out = (torch.rand((2, 2) + tshape, generator=g) - 0.5).float()
    return x.float(), case_thetas(name, world), flow.float(), grad_out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the arbiter of trx_bspline_mi_run_grids
# ---------------------------------------------------------------------------------------------------------------------------------------
def loop(mov, tgt, theta, rng, spacing, optimizer, lr, iters, ctrl0, mi, dtype, mask=None, lam=0.0, scale=None):
    """`iters` iterations on the control tensor: (losses [iters], final control tensor) as numpy arrays."""
    sp = tuple(tgt.shape[2:])
    p = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        warped = warp(mov, theta, bspline_ref.expand(p, sp, spacing, dtype=dtype), scale, dtype)
        e = (mi_ref.loss(tgt, warped, rng=rng, dtype=dtype, **mi) if mask is None else mref.loss(tgt, warped, mask, rng=rng, dtype=dtype, **mi)).sum()
        if lam:
            e = e + lam * bref.energy_squares(p, sp, spacing, dtype=dtype).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy().copy()


ITERS = 10
# id -> (target shape, moving shape, spacing, optimiser, lr, masked, bending weight).  theta: ph.THETA_STAR3 / THETA_STAR2, the map
# tests/affine_mi_grids_ref.py::pair built the moving image with.  Rates: those of tests/test_gpu_mi.py::BSPLINE_LOOPS (the fp64 loss falls in every
# iteration and the two precisions stay together: asserted in tests/test_affine_flow_host.py).
LOOPS = {
    "adam": ((12, 14, 16), (15, 13, 18), 4, "adam", 0.1, False, 0.0),
    "masked": ((12, 14, 16), (15, 13, 18), 4, "adam", 0.1, True, 0.0),
    "bending": ((12, 14, 16), (15, 13, 18), 4, "adam", 0.1, False, 50.0),
    "2d": ((24, 28), (30, 22), 5, "adam", 0.1, False, 0.0),
    "sgd": ((12, 14, 16), (15, 13, 18), 4, "sgd", 10.0, False, 0.0),
}


def loop_theta(nd):
    return torch.tensor(ph.THETA_STAR3 if nd == 3 else ph.THETA_STAR2)[None]


def loop_setup(name):
    """(mov, tgt, theta [1,nd,nd+1], mask or None, rng, ctrl0) of a LOOPS row; ctrl0: a random control tensor of amplitude 0.2."""
    tshape, mshape, spacing, _, _, masked, _ = LOOPS[name]
    mov, tgt = gref.pair(tshape, mshape)
    mask = mref.loop_mask(tshape) if masked else None
    rng = mi_ref.fit_range(tgt, mov) if mask is None else mref.fit_range(tgt, mov, mask)
    g = torch.Generator().manual_seed(7)
    ctrl0 = (torch.rand((1, len(tshape)) + bspline_ref.grid(tshape, spacing), generator=g) - 0.5) * 0.4
    return mov, tgt, loop_theta(len(tshape)), mask, rng, ctrl0


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    """(r64, r32) of one LOOPS configuration - each (losses, final control tensor) - computed once per process."""
    _, _, spacing, optimizer, lr, _, lam = LOOPS[name]
    mov, tgt, theta, mask, rng, ctrl0 = loop_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    return tuple(loop(mov, tgt, theta, rng, spacing, optimizer, lr, ITERS, ctrl0, mi, dt, mask, lam) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# what it is for: one interpolation against resample-then-deform on the world phantom of tests/affine_mi_grids_ref.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def world_flow(tshape):
    """[1,3,*tshape] fp64, target voxels, on linspace(-1, 1) coordinates of the target lattice: z 0.6 sin(2.1 y + 0.3), y 1.5 sin(1.7 x + 2 z),
    x 1.5 cos(1.9 y - z)."""
    z, y, x = torch.meshgrid(*[torch.linspace(-1, 1, s, dtype=torch.float64) for s in tshape], indexing="ij")
    return torch.stack([0.6 * torch.sin(2.1 * y + 0.3), 1.5 * torch.sin(1.7 * x + 2.0 * z), 1.5 * torch.cos(1.9 * y - z)])[None]


def world_errors():
    """(rms, max) of |one composed interpolation - analytic| and of |resample with theta, then deform - analytic| on world_pair's lattices without
    the intensity map: the moving image is the phantom moved rigidly, the analytic image is the phantom at the composed world positions."""
    (ts, tv), (ms, mv) = gref.WORLD_TARGET, gref.WORLD_MOVING
    e_t, e_m = gref.half_extents(ts, tv), gref.half_extents(ms, mv)
    R, t = gref.rigid_matrix_mm(gref.WORLD_POSE, e_m)
    moving = gref.world_blobs((gref.voxel_centres_mm(ms, mv) - t) @ R)[None, None]          # moving(y) = phantom(R^T (y - t))
    theta = (gref.pose_to_theta(torch.tensor(gref.WORLD_POSE, dtype=torch.float64)) * gref.scale_of(ms, ts, mv, tv))
    flow = world_flow(ts)
    # the analytic image: the phantom at target voxel + flow, in mm
    p_mm = gref.voxel_centres_mm(ts, tv) + flow[0].movedim(0, -1).flip(-1) * torch.tensor(tv[::-1], dtype=torch.float64)
    exact = gref.world_blobs(p_mm)          # moving(R p + t) = phantom(p)
    once = warp(moving, theta, flow)[0, 0]
    from oracle import compose
    twice = compose.flow_warp(gref.warp(theta, torch.ones(3, 4, dtype=torch.float64), moving, ts), flow)[0, 0]
    stats = lambda d: (d.pow(2).mean().sqrt().item(), d.abs().max().item())  # noqa: E731
    return stats(once - exact), stats(twice - exact), (exact.max() - exact.min()).item()
