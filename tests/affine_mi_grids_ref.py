"""The arbiter of the cross-lattice rigid / affine mutual-information entry points (trx_affine_mi_loss_grad_grids, trx_affine_mi_run_grids,
trx_affine_warp_grids): F.affine_grid(theta * scale, [B,1,*target]) -> F.grid_sample on the moving image (its own
lattice; align_corners=False, zero padding) -> tests/mi_ref.py (tests/mi_mask_ref.py under a mask), under torch autograd and torch.optim on the
CPU, in fp32 and fp64.  The mirror of tests/affine_mi_ref.py: `evaluate`, `loop`, a `LOOPS` table - plus a phantom defined in millimetres and
sampled on two lattices, and the registration it is for.  Nothing here touches the GPU; tests/test_affine_mi_grids_host.py asserts the conditions
the GPU tests rely on."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import affine_mi_ref as aref
import mi_mask_ref as mref
import mi_ref
import phantoms as ph

# anisotropic voxels (mm, the tensors' axis order): thick slices against a fine, slightly anisotropic grid
VOXEL_T3, VOXEL_M3 = (3.0, 1.0, 1.0), (1.2, 0.9, 0.8)
VOXEL_T2, VOXEL_M2 = (2.0, 1.0), (0.9, 1.3)


def half_extents(shape, voxel):
    """size * voxel size / 2 per axis, in theta's row order (x, y(, z)), fp64."""
    return torch.tensor([s * v / 2.0 for s, v in zip(shape, voxel)][::-1], dtype=torch.float64)


def scale_of(moving_shape, target_shape, moving_voxel=None, target_voxel=None):
    """The definition grid_scale implements, restated: ones without voxel sizes; e_target[c] / e_moving[r] on the matrix, 1 on the translation."""
    nd = len(target_shape)
    s = torch.ones(nd, nd + 1, dtype=torch.float64)
    if moving_voxel is not None:
        s[:, :nd] = half_extents(target_shape, target_voxel)[None, :] / half_extents(moving_shape, moving_voxel)[:, None]
    return s


def kernel_scale(scale):
    """The scale as the kernels hold it: rounded to fp32 (returned in fp64)."""
    return scale.float().double()


def warp(theta, scale, mov, target_shape):
    """grid_sample(mov, affine_grid(theta * scale, target)) in theta's dtype: [B,C,*target_shape]."""
    nd = mov.dim() - 2
    te = theta.reshape(-1, nd, nd + 1) * scale.to(theta.dtype)
    grid = F.affine_grid(te, [te.shape[0], mov.shape[1], *target_shape], align_corners=False)
    return F.grid_sample(mov.to(theta.dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=False)


@functools.lru_cache(maxsize=None)
def pair(target_shape, moving_shape, seed=5):
    """(moving [1,1,*moving_shape], target [1,1,*target_shape]) fp32: the blob phantom of tests/phantoms.py - a function of the normalised cube -
    sampled on the target lattice; sampled on the moving lattice, warped there by THETA_STAR and sent through the non-monotone map 4w(1 - w)."""
    from oracle import compose
    t = ph.blobs(target_shape, seed)
    w = compose.affine_warp(torch.tensor(ph.THETA_STAR3 if len(moving_shape) == 3 else ph.THETA_STAR2), ph.blobs(moving_shape, seed))
    return (4.0 * w * (1.0 - w)).float(), t


def evaluate(mov, tgt, theta, scale, rng, bins=32, alpha=1.0, normalized=False, dtype=torch.float64, mask=None):
    """One evaluation for B pairs: (loss [B], d loss / d theta [B,nd,nd+1] - the UNSCALED theta -, P [B,K,K]) as fp64 tensors."""
    th = theta.detach().to(dtype).clone().requires_grad_()
    warped = warp(th, kernel_scale(scale), mov, tgt.shape[2:])
    if mask is None:
        loss = mi_ref.loss(tgt, warped, bins, alpha, normalized, rng, dtype)
        P = mi_ref.joint(tgt, warped.detach(), bins, rng, dtype)
    else:
        loss = mref.loss(tgt, warped, mask, bins, alpha, normalized, rng, dtype)
        P = mref.joint(tgt, warped.detach(), mask, bins, rng, dtype)
    (g,) = torch.autograd.grad(loss.sum(), th)
    return loss.detach().double(), g.double(), P.double()


def pose_to_theta(p):
    from oracle import compose
    return compose.pose_to_theta(p)


def loop(mov, tgt, rng, scale, mode, optimizer, lr, iters, start, mi, dtype, mask=None):
    """`iters` iterations for one pair: (losses [iters], final parameter) as numpy arrays; the parameter is the pose (rigid) or the unscaled
    theta (affine), as in tests/affine_mi_ref.py::loop."""
    nd = mov.dim() - 2
    scale = kernel_scale(scale)
    p = start.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        theta = pose_to_theta(p) if mode == "rigid" else p.reshape(1, nd, nd + 1)
        warped = warp(theta, scale, mov, tgt.shape[2:])
        e = (mi_ref.loss(tgt, warped, rng=rng, dtype=dtype, **mi) if mask is None else mref.loss(tgt, warped, mask, rng=rng, dtype=dtype, **mi)).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy().copy()


ITERS = 10
# id -> (target shape, moving shape, mode, optimiser, lr, (moving voxel, target voxel) or None, masked).  Rates: those of affine_mi_ref.LOOPS or
# lower, chosen on the CPU so that the fp64 loss falls in every iteration and the two precisions stay within 1e-5 / 2e-5 (asserted in
# tests/test_affine_mi_grids_host.py).
LOOPS = {
    "rigid-adam": ((12, 14, 16), (15, 13, 18), "rigid", "adam", 0.01, None, False),
    "rigid-sgd": ((12, 14, 16), (15, 13, 18), "rigid", "sgd", 0.03, None, False),
    "affine-adam": ((12, 14, 16), (15, 13, 18), "affine", "adam", 0.005, None, False),
    "2d-rigid": ((24, 28), (30, 22), "rigid", "adam", 0.005, None, False),
    "rigid-voxels": ((12, 14, 16), (20, 18, 16), "rigid", "adam", 0.01, ((1.8, 0.8, 1.0), (3.0, 1.0, 1.0)), False),
    "rigid-masked": ((12, 14, 16), (15, 13, 18), "rigid", "adam", 0.01, None, True),
}


def loop_setup(name):
    """(mov, tgt, scale, mask or None, rng, start) of a LOOPS row."""
    tshape, mshape, mode, _, _, voxels, masked = LOOPS[name]
    mov, tgt = pair(tshape, mshape)
    scale = scale_of(mshape, tshape, *(voxels or (None, None)))
    mask = mref.loop_mask(tshape) if masked else None
    rng = mi_ref.fit_range(tgt, mov) if mask is None else mref.fit_range(tgt, mov, mask)
    return mov, tgt, scale, mask, rng, aref.start_of(tshape, mode)


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    """(r64, r32) of one LOOPS configuration - each (losses, final parameter) - computed once per process."""
    _, _, mode, optimizer, lr, _, _ = LOOPS[name]
    mov, tgt, scale, mask, rng, start = loop_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    return tuple(loop(mov, tgt, rng, scale, mode, optimizer, lr, ITERS, start, mi, dt, mask) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the world phantom: Gaussian blobs defined in millimetres, sampled on any lattice whose centre is the origin
# ---------------------------------------------------------------------------------------------------------------------------------------
WORLD_SEED, WORLD_BLOBS = 11, 8
WORLD_TARGET = ((10, 30, 30), (3.0, 1.0, 1.0))             # shape, voxel (mm): thick slices
WORLD_MOVING = ((26, 22, 18), (1.2, 1.4, 1.7))
WORLD_POSE = (0.18, -0.12, 0.15, 0.10, -0.08, 0.06)       # the rigid motion between the two images, as Theta's pose
WORLD_LR, WORLD_ITERS, WORLD_BINS = 0.01, 120, 32


def voxel_centres_mm(shape, voxel):
    """[*shape, nd] fp64: the world coordinates (x, y(, z)) of the voxel centres of a lattice centred on the origin."""
    axes = [(torch.arange(s, dtype=torch.float64) + 0.5 - s / 2.0) * v for s, v in zip(shape, voxel)]
    return torch.stack(torch.meshgrid(*axes, indexing="ij")[::-1], dim=-1)


def world_blobs(points, seed=WORLD_SEED, nblob=WORLD_BLOBS):
    """The phantom at world points [..., 3] (x, y, z in mm): `nblob` Gaussians, per blob drawn in this order from
    torch.Generator().manual_seed(seed): centre = 16 (rand(3) - 0.5) mm, sigma = 2 + 3 rand(1) mm, amplitude = 0.3 + 0.7 rand(1); scaled to
    a maximum of at most 1 by the sum of the amplitudes."""
    g = torch.Generator().manual_seed(int(seed))
    img, total = torch.zeros(points.shape[:-1], dtype=torch.float64), 0.0
    for _ in range(nblob):
        c = 16.0 * (torch.rand(3, generator=g) - 0.5)
        sig = 2.0 + 3.0 * float(torch.rand(1, generator=g))
        a = 0.3 + 0.7 * float(torch.rand(1, generator=g))
        img += a * torch.exp(-((points - c.double()) ** 2).sum(-1) / (2.0 * sig * sig))
        total += a
    return img / total * 2.0


def rigid_matrix_mm(pose, e_moving):
    """(R [3,3], t [3] mm) of moving_mm = R target_mm + t for theta = Theta(pose) under the world scale: R = theta[:, :3], t = e_moving * theta[:, 3]."""
    th = pose_to_theta(torch.as_tensor(pose, dtype=torch.float64))[0]
    return th[:, :3], th[:, 3] * e_moving


@functools.lru_cache(maxsize=None)
def world_pair():
    """(moving, target) fp32 [1,1,*shape]: the phantom on the target lattice, and on the moving lattice the phantom moved rigidly so that
    theta = Theta(WORLD_POSE) under the world scale brings it back - moving(y) = phantom(R^T (y - t)) - sent through 4w(1 - w)."""
    (ts, tv), (ms, mv) = WORLD_TARGET, WORLD_MOVING
    tgt = world_blobs(voxel_centres_mm(ts, tv)).clamp(max=1.0)
    R, t = rigid_matrix_mm(WORLD_POSE, half_extents(ms, mv))
    w = world_blobs((voxel_centres_mm(ms, mv) - t) @ R).clamp(max=1.0)        # rows: R^T (y - t)
    return (4.0 * w * (1.0 - w)).float()[None, None], tgt.float()[None, None]


@functools.lru_cache(maxsize=None)
def world_run(world, dtype=torch.float64):
    """The registration the feature is for, in the arbiter: rigid, Adam, zero start, WORLD_ITERS iterations under the world scale (world=True)
    or under scale = 1 (False).  Returns (losses, final pose, max |final pose - WORLD_POSE|, best loss)."""
    (ts, tv), (ms, mv) = WORLD_TARGET, WORLD_MOVING
    mov, tgt = world_pair()
    scale = scale_of(ms, ts, mv, tv) if world else scale_of(ms, ts)
    rng = mi_ref.fit_range(tgt, mov)
    losses, pose = loop(mov, tgt, rng, scale, "rigid", "adam", WORLD_LR, WORLD_ITERS, torch.zeros(6), dict(bins=WORLD_BINS, alpha=1.0, normalized=False), dtype)
    return losses, pose, float(np.max(np.abs(pose - np.asarray(WORLD_POSE)))), float(losses.min())
