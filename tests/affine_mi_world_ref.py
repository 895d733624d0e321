"""The arbiter of world-geometry registration (trx_moving_grid.world): an fp64 restatement that builds L, R and l from two
voxel-to-world matrices on its own, forms theta_eff = (L Theta R)[:nd] under torch autograd and hands it to the machinery of
tests/affine_mi_grids_ref.py (F.affine_grid + F.grid_sample on the moving lattice + tests/mi_ref.py / mi_mask_ref.py / mi_overlap_ref.py) with a scale
of ones - so the chain rule is autograd's.  Plus headers (diagonal, oblique with a flipped axis), the layout change of test 3, and the world phantom of
tests/affine_mi_grids_ref.py under two oblique, offset headers with a known rigid world transform.  Nothing here touches the GPU or the package's own
world_geometry: tests/test_affine_mi_world_host.py compares the two."""
import functools
import math

import numpy as np
import torch

import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import mi_mask_ref as mref
import mi_ref

STRIDE, OFF_L, OFF_R, OFF_EXT = 32, 0, 12, 24      # include/trx.h: TRX_WORLD_*


# ---------------------------------------------------------------------------------------------------------------------------------------
# headers
# ---------------------------------------------------------------------------------------------------------------------------------------
def rotation(ax, ay, az):
    """Rz(az) Ry(ay) Rx(ax), fp64 [3,3]."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=torch.float64)
    Ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=torch.float64)
    Rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=torch.float64)
    return Rz @ Ry @ Rx


def header(shape, voxel, rot=None, flip=None, centre=None):
    """A voxel-to-world matrix [nd+1, nd+1] fp64, columns in the tensor's axis order (d, h, w), rows world x, y(, z): tensor axis a runs along world
    axis nd-1-a with its voxel size (the aligned convention of section 4.13), then `flip` (a tensor axis whose direction is reversed), then the
    rotation `rot` [nd,nd]; the origin is placed so that the lattice's geometric centre lies at `centre` (default 0)."""
    nd = len(shape)
    lin = torch.zeros(nd, nd, dtype=torch.float64)
    for a in range(nd):
        lin[nd - 1 - a, a] = voxel[a] * (-1.0 if flip == a else 1.0)
    if rot is not None:
        lin = torch.as_tensor(rot, dtype=torch.float64) @ lin
    mid = torch.tensor([(s - 1) / 2.0 for s in shape], dtype=torch.float64)
    c = torch.zeros(nd, dtype=torch.float64) if centre is None else torch.as_tensor(centre, dtype=torch.float64)
    A = torch.eye(nd + 1, dtype=torch.float64)
    A[:nd, :nd], A[:nd, nd] = lin, c - lin @ mid
    return A


def rot2(a):
    return torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]], dtype=torch.float64)


OBLIQUE = (0.3, -0.2, 0.15)


def oblique_pair(tshape, mshape):
    """(A_m, A_t) of the GPU tests: the moving header rotated by 0.3 / -0.2 / 0.15 rad (2-D: 0.3) with tensor axis 1 flipped, the target's rotated
    slightly; anisotropic voxels of affine_mi_grids_ref; lattice centres a few mm apart so that the volumes overlap, origins tens of mm apart."""
    nd = len(tshape)
    vm, vt = (gref.VOXEL_M3, gref.VOXEL_T3) if nd == 3 else (gref.VOXEL_M2, gref.VOXEL_T2)
    if nd == 3:
        Am = header(mshape, vm, rotation(*OBLIQUE), flip=1, centre=(31.0, -18.5, 12.25))
        At = header(tshape, vt, rotation(-0.05, 0.04, 0.1), centre=(30.0, -18.0, 12.0))
    else:
        Am = header(mshape, vm, rot2(0.3), flip=1, centre=(21.0, -14.5))
        At = header(tshape, vt, rot2(-0.06), centre=(20.5, -14.0))
    return Am, At


# ---------------------------------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------------------------------
def norm_to_voxel(shape):
    """N(S) [nd+1, nd+1]: normalised (x, y(, z)) -> voxel index (d, h, w), i = ((n + 1) S - 1) / 2."""
    nd = len(shape)
    N = torch.zeros(nd + 1, nd + 1, dtype=torch.float64)
    for a, S in enumerate(shape):
        N[a, nd - 1 - a], N[a, nd] = S / 2.0, (S - 1) / 2.0
    N[nd, nd] = 1.0
    return N


def translation(t):
    t = torch.as_tensor(t, dtype=torch.float64)
    T = torch.eye(len(t) + 1, dtype=torch.float64)
    T[:-1, -1] = t
    return T


def centre_of(shape, A):
    nd = len(shape)
    return (A @ torch.tensor([(s - 1) / 2.0 for s in shape] + [1.0], dtype=torch.float64))[:nd]


def geometry(mshape, tshape, Am, At, T0=None, c=None):
    """(L [nd+1,nd+1], R [nd+1,nd+1], l [nd], T0, c) fp64 of one pair, by the definitions of the issue."""
    nd = len(tshape)
    T0 = torch.eye(nd + 1, dtype=torch.float64) if T0 is None else torch.as_tensor(T0, dtype=torch.float64)
    c = centre_of(tshape, At) if c is None else torch.as_tensor(c, dtype=torch.float64)
    R = translation(-c) @ At @ norm_to_voxel(tshape)
    L = torch.linalg.inv(norm_to_voxel(mshape)) @ torch.linalg.inv(Am) @ T0 @ translation(c)
    ext = (Am[:nd, :nd].abs() * torch.tensor(mshape, dtype=torch.float64)[None, :]).sum(1) / 2.0
    return L, R, ext, T0, c


def record(mshape, tshape, Am, At, T0=None, c=None):
    """[1, 32] fp64: the record of include/trx.h."""
    nd = len(tshape)
    L, R, ext, _, _ = geometry(mshape, tshape, Am, At, T0, c)
    rec = torch.zeros(1, STRIDE, dtype=torch.float64)
    rec[0, OFF_L:OFF_L + nd * (nd + 1)] = L[:nd].reshape(-1)
    rec[0, OFF_R:OFF_R + nd * (nd + 1)] = R[:nd].reshape(-1)
    rec[0, OFF_EXT:OFF_EXT + nd] = ext
    return rec


def unpack(rec, nd):
    """(L, R) homogeneous [B,nd+1,nd+1] and l [B,nd] of records [B,32]."""
    rec = rec.double()
    B = rec.shape[0]
    L, R = (torch.eye(nd + 1, dtype=torch.float64).repeat(B, 1, 1) for _ in range(2))
    L[:, :nd] = rec[:, OFF_L:OFF_L + nd * (nd + 1)].reshape(B, nd, nd + 1)
    R[:, :nd] = rec[:, OFF_R:OFF_R + nd * (nd + 1)].reshape(B, nd, nd + 1)
    return L, R, rec[:, OFF_EXT:OFF_EXT + nd]


def theta_eff(theta, rec):
    """(L Theta R)[:nd] in theta's dtype, differentiable: theta [B,nd,nd+1] the UNSCALED theta, rec [B,32]."""
    nd = theta.shape[-1] - 1
    L, R, ext = (x.to(theta.dtype) for x in unpack(rec, nd))
    B = theta.shape[0]
    top = torch.cat([theta[:, :, :nd], (theta[:, :, nd] * ext)[:, :, None]], dim=2)
    last = torch.zeros(B, 1, nd + 1, dtype=theta.dtype)
    last[:, 0, nd] = 1.0
    return (L @ torch.cat([top, last], dim=1) @ R)[:, :nd]


def chain(g_eff, rec):
    """dL/dtheta from dL/dtheta_eff by the issue's steps 2-6, fp64."""
    nd = g_eff.shape[-1] - 1
    L, R, ext = unpack(rec, nd)
    g = g_eff.double()
    P = torch.einsum("bir,bij->brj", L[:, :nd, :nd], g)
    d = torch.zeros_like(g)
    d[:, :, :nd] = torch.einsum("brj,bcj->brc", P, R[:, :nd, :])
    d[:, :, nd] = ext * P[:, :, nd]
    return d


def world_matrix(theta, rec_geom):
    """T = T0 Tr(c) Theta Tr(-c) [nd+1,nd+1] fp64 of one unscaled theta [nd,nd+1]; rec_geom = geometry(...)."""
    _, _, ext, T0, c = rec_geom
    nd = len(c)
    Th = torch.eye(nd + 1, dtype=torch.float64)
    Th[:nd, :nd], Th[:nd, nd] = theta[:, :nd].double(), theta[:, nd].double() * ext
    return T0 @ translation(c) @ Th @ translation(-c)


ONES = lambda nd: torch.ones(nd, nd + 1, dtype=torch.float64)  # noqa: E731


def evaluate(mov, tgt, theta, rec, rng, bins=32, alpha=1.0, normalized=False, dtype=torch.float64, mask=None):
    """(loss [B], dL/dtheta [B,nd,nd+1] of the UNSCALED theta by autograd, P [B,K,K], dL/dtheta_eff) fp64."""
    nd = mov.dim() - 2
    th = theta.detach().to(dtype).clone().requires_grad_()
    te = theta_eff(th, rec)
    te.retain_grad()
    warped = gref.warp(te, ONES(nd), mov, tgt.shape[2:])
    if mask is None:
        loss = mi_ref.loss(tgt, warped, bins, alpha, normalized, rng, dtype)
        P = mi_ref.joint(tgt, warped.detach(), bins, rng, dtype)
    else:
        loss = mref.loss(tgt, warped, mask, bins, alpha, normalized, rng, dtype)
        P = mref.joint(tgt, warped.detach(), mask, bins, rng, dtype)
    loss.sum().backward()
    return loss.detach().double(), th.grad.double(), P.double(), te.grad.double()


def loop(mov, tgt, rng, rec, mode, optimizer, lr, iters, start, mi, dtype, mask=None):
    """affine_mi_grids_ref.loop with theta_eff(theta, rec) where theta * scale stands: (losses [iters], final pose / unscaled theta)."""
    nd = mov.dim() - 2
    p = start.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        theta = gref.pose_to_theta(p) if mode == "rigid" else p.reshape(1, nd, nd + 1)
        warped = gref.warp(theta_eff(theta.reshape(1, nd, nd + 1), rec), ONES(nd), mov, tgt.shape[2:])
        e = (mi_ref.loss(tgt, warped, rng=rng, dtype=dtype, **mi) if mask is None else mref.loss(tgt, warped, mask, rng=rng, dtype=dtype, **mi)).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# pairs of the single-evaluation and loop tests: affine_mi_grids_ref.pair's images under oblique headers.  The images are functions of the
# normalised cube, so the headers only have to keep the overlap large: theta_start is chosen so that theta_eff at the start is the theta the
# grids tests evaluate at (aref.theta0), by solving the linear map theta -> theta_eff.
# ---------------------------------------------------------------------------------------------------------------------------------------
def theta_for(te_want, rec):
    """The unscaled theta [1,nd,nd+1] fp32 whose theta_eff under rec is te_want (fp64 solve, rounded to fp32)."""
    nd = te_want.shape[-1] - 1
    L, R, ext = unpack(rec, nd)
    want = torch.eye(nd + 1, dtype=torch.float64)
    want[:nd] = te_want.double().reshape(nd, nd + 1)
    Th = torch.linalg.inv(L[0]) @ want @ torch.linalg.inv(R[0])
    th = Th[:nd].clone()
    th[:, nd] = th[:, nd] / ext[0]
    return th.float()[None]


ITERS = 10
# id -> (target shape, moving shape, mode, optimiser, lr).  Rates as affine_mi_grids_ref.LOOPS; the host test asserts that the fp64 loss falls in every
# iteration and that the two precisions stay together.
LOOPS = {
    "rigid-adam": ((12, 14, 16), (15, 13, 18), "rigid", "adam", 0.01),
    "rigid-sgd": ((12, 14, 16), (15, 13, 18), "rigid", "sgd", 0.03),
    "affine-adam": ((12, 14, 16), (15, 13, 18), "affine", "adam", 0.005),
    "affine-sgd": ((12, 14, 16), (15, 13, 18), "affine", "sgd", 0.01),
    "2d-rigid": ((24, 28), (30, 22), "rigid", "adam", 0.005),
}


def loop_headers(name):
    """Headers of a LOOPS row: oblique_pair, with T0 chosen so that theta = Theta(0) = identity samples the moving image where the grids loops do at
    scale 1 (theta_eff(I) = I): T0 = A_m N(S_m) N(S_t)^-1 A_t^-1 - `a world transform from anywhere`, handed over as a matrix."""
    tshape, mshape = LOOPS[name][:2]
    Am, At = oblique_pair(tshape, mshape)
    T0 = Am @ norm_to_voxel(mshape) @ torch.linalg.inv(norm_to_voxel(tshape)) @ torch.linalg.inv(At)
    return Am, At, T0


def loop_setup(name):
    """(mov, tgt, rec, rng, start, (A_m, A_t, T0)) of a LOOPS row."""
    tshape, mshape, mode, _, _ = LOOPS[name]
    mov, tgt = gref.pair(tshape, mshape)
    Am, At, T0 = loop_headers(name)
    rec = record(mshape, tshape, Am, At, T0)
    return mov, tgt, rec, mi_ref.fit_range(tgt, mov), aref.start_of(tshape, mode), (Am, At, T0)


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    _, _, mode, optimizer, lr = LOOPS[name]
    mov, tgt, rec, rng, start, _ = loop_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    return tuple(loop(mov, tgt, rng, rec, mode, optimizer, lr, ITERS, start, mi, dt) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# layout change (test 3): the same physical image in another memory layout
# ---------------------------------------------------------------------------------------------------------------------------------------
def relayout(x, A):
    """Flip axis 0 of the volume [B,1,d,h,w] and swap its axes 1 and 2, and the header that describes the same physical image: (x', A')."""
    d = x.shape[2]
    y = x.flip(2).transpose(3, 4).contiguous()
    M = torch.zeros(4, 4, dtype=torch.float64)      # old voxel index from the new one: i0 = d - 1 - j0, i1 = j2, i2 = j1
    M[0, 0], M[0, 3], M[1, 2], M[2, 1], M[3, 3] = -1.0, d - 1.0, 1.0, 1.0, 1.0
    return y, A @ M


# ---------------------------------------------------------------------------------------------------------------------------------------
# what it is for: the world phantom under two headers
# ---------------------------------------------------------------------------------------------------------------------------------------
WORLD_POSE = gref.WORLD_POSE
WORLD_T_CENTRE = (2.0, -3.0, 1.5)          # the target lattice's centre in world mm (the phantom lives around the origin)
WORLD_M_OFFSET = (1.0, -2.0, 1.5)          # the moving lattice's centre against the image of the target's under the true transform


@functools.lru_cache(maxsize=None)
def world_headers():
    """(A_m, A_t, T_true): the target 10x30x30 @ 3x1x1 mm, slightly rotated, centred on WORLD_T_CENTRE; the moving lattice 26x22x18 @ 1.2x1.4x1.7 mm
    under an oblique header (0.3 / -0.2 / 0.15 rad) with tensor axis 1 flipped; T_true = Tr(c) Theta(WORLD_POSE) Tr(-c) with c the target's centre and
    the translation in units of the moving bounding box's half extents - so the header-trusting run (T0 = I) has WORLD_POSE as its answer."""
    (ts, tv), (ms, mv) = gref.WORLD_TARGET, gref.WORLD_MOVING
    At = header(ts, tv, rotation(-0.05, 0.04, 0.1), centre=WORLD_T_CENTRE)
    lin = header(ms, mv, rotation(*OBLIQUE), flip=1)
    ext = (lin[:3, :3].abs() * torch.tensor(ms, dtype=torch.float64)[None, :]).sum(1) / 2.0
    th = gref.pose_to_theta(torch.tensor(WORLD_POSE, dtype=torch.float64))[0]
    c = torch.tensor(WORLD_T_CENTRE, dtype=torch.float64)
    Th = torch.eye(4, dtype=torch.float64)
    Th[:3, :3], Th[:3, 3] = th[:, :3], th[:, 3] * ext
    T = translation(c) @ Th @ translation(-c)
    cm = (T @ torch.cat([c, torch.ones(1, dtype=torch.float64)]))[:3] + torch.tensor(WORLD_M_OFFSET, dtype=torch.float64)
    Am = header(ms, mv, rotation(*OBLIQUE), flip=1, centre=cm)
    return Am, At, T


def lattice_points(shape, A):
    """[*shape, 3] fp64: the world positions of the voxel centres of a lattice under header A."""
    idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij"), dim=-1)
    return idx @ A[:3, :3].T + A[:3, 3]


@functools.lru_cache(maxsize=None)
def world_pair():
    """(moving, target) fp32 [1,1,*shape]: target(p) = phantom(p) on the target lattice; moving(q) = phantom(T_true^-1 q) on the moving lattice, sent
    through 4w(1 - w) - so that moving(T_true p) shows what target(p) shows."""
    (ts, _), (ms, _) = gref.WORLD_TARGET, gref.WORLD_MOVING
    Am, At, T = world_headers()
    tgt = gref.world_blobs(lattice_points(ts, At)).clamp(max=1.0)
    Ti = torch.linalg.inv(T)
    w = gref.world_blobs(lattice_points(ms, Am) @ Ti[:3, :3].T + Ti[:3, 3]).clamp(max=1.0)
    return (4.0 * w * (1.0 - w)).float()[None, None], tgt.float()[None, None]


@functools.lru_cache(maxsize=None)
def world_run(headers, dtype=torch.float64):
    """The registration the feature is for, in the arbiter: rigid, Adam, zero start, WORLD_ITERS iterations - headers=True with the record of the two
    headers (T0 = I), False with the voxel sizes alone (affine_mi_grids_ref's scale: origins and directions ignored).  Returns (losses, final pose,
    max |final pose - WORLD_POSE|, best loss)."""
    (ts, tv), (ms, mv) = gref.WORLD_TARGET, gref.WORLD_MOVING
    mov, tgt = world_pair()
    rng = mi_ref.fit_range(tgt, mov)
    mi = dict(bins=gref.WORLD_BINS, alpha=1.0, normalized=False)
    if headers:
        Am, At, _ = world_headers()
        losses, pose = loop(mov, tgt, rng, record(ms, ts, Am, At), "rigid", "adam", gref.WORLD_LR, gref.WORLD_ITERS, torch.zeros(6), mi, dtype)
    else:
        losses, pose = gref.loop(mov, tgt, rng, gref.scale_of(ms, ts, mv, tv), "rigid", "adam", gref.WORLD_LR, gref.WORLD_ITERS, torch.zeros(6), mi, dtype)
    return losses, pose, float(np.max(np.abs(pose - np.asarray(WORLD_POSE)))), float(losses.min())


# ---------------------------------------------------------------------------------------------------------------------------------------
# two blobs (the world_init modes and the reach test)
# ---------------------------------------------------------------------------------------------------------------------------------------
def two_blobs(shape, A, centres, sigma=(4.0, 5.0), amp=(1.0, 0.6), floor=0.1):
    """[1,1,*shape] fp32: floor + two Gaussians at world centres (mm) on the lattice under header A."""
    p = lattice_points(shape, A)
    img = torch.full(tuple(shape), floor, dtype=torch.float64)
    for c, s, a in zip(centres, sigma, amp):
        img += a * torch.exp(-((p - torch.tensor(c, dtype=torch.float64)) ** 2).sum(-1) / (2.0 * s * s))
    return img.float()[None, None]


def centre_of_mass_world(x, A, mask=None):
    """World centre of mass [nd] fp64 of x [1,1,*shape] with weights v - min over the counted voxels: the definition tr.image_moments implements."""
    v = x[0, 0].double()
    nd = v.dim()
    m = torch.ones_like(v, dtype=torch.bool) if mask is None else (mask.reshape(v.shape) != 0)
    w = torch.where(m, v - v[m].min(), torch.zeros_like(v))
    idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in v.shape], indexing="ij"), dim=-1)
    ctr = (w[..., None] * idx).reshape(-1, nd).sum(0) / w.sum()
    return A[:nd, :nd] @ ctr + A[:nd, nd]


# ---------------------------------------------------------------------------------------------------------------------------------------
# reach (GPU test 6): two images whose contents lie 40 mm apart in the world - beyond 0.25 l of the moving lattice, the rigid loop's cap
# ---------------------------------------------------------------------------------------------------------------------------------------
REACH_SHIFT = (24.0, -32.0, 0.0)                       # |shift| = 40 mm
REACH_TSHAPE, REACH_MSHAPE = (20, 24, 26), (24, 26, 22)
REACH_BLOBS = ((3.0, -2.0, 1.0), (-4.0, 3.0, -2.0))   # world mm, in the target's frame


@functools.lru_cache(maxsize=None)
def reach_pair():
    """(moving, target, A_m, A_t): two blobs on a target lattice @ 1.5x1x1 mm around the origin, and the same blobs moved by REACH_SHIFT (and turned by
    Theta((0.05, -0.04, 0.03, 0, 0, 0)) about their middle) on a moving lattice @ 1x1.2x1.1 mm under an oblique header whose centre lies 1 / -1.5 / 0.5 mm
    off the moved middle."""
    At = header(REACH_TSHAPE, (1.5, 1.0, 1.0), rotation(-0.05, 0.04, 0.1), centre=(0.5, -0.5, 0.25))
    shift = torch.tensor(REACH_SHIFT, dtype=torch.float64)
    Am = header(REACH_MSHAPE, (1.0, 1.2, 1.1), rotation(*OBLIQUE), flip=1, centre=shift + torch.tensor((1.0, -1.5, 0.5), dtype=torch.float64))
    Rm = gref.pose_to_theta(torch.tensor((0.05, -0.04, 0.03, 0.0, 0.0, 0.0), dtype=torch.float64))[0][:, :3]
    moved = [tuple((Rm @ torch.tensor(b, dtype=torch.float64) + shift).tolist()) for b in REACH_BLOBS]
    return two_blobs(REACH_MSHAPE, Am, moved), two_blobs(REACH_TSHAPE, At, REACH_BLOBS), Am, At
