"""The overlap rule of the mutual-information entry points (trx_moving_grid.overlap / .mask, include/trx.h) restated on the
CPU, in fp32 or fp64, without any new maths: the un-normalised moving coordinate i of every target voxel comes from F.affine_grid (the fused
passes) or from tests/affine_flow_ref.py::composed_grid (the composed warp), validity is
    valid(v) = target mask at v  and  0 <= i_a <= S_m,a - 1 on every axis  and  moving mask at rint(i) (half to even)
and the criterion is tests/mi_mask_ref.py::loss with the DETACHED validity as the mask - so autograd treats validity as constant, as the kernels
do.  The loops are tests/affine_mi_grids_ref.py::loop and tests/affine_flow_ref.py::loop with that criterion.  Also here: the cases of the GPU
tests, the border condition they rely on, and the crop phantom that shows what the rule is for.  Nothing here touches the GPU;
tests/test_mi_overlap_host.py asserts the conditions the GPU tests rely on.  Not a test."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as F

import affine_flow_ref as fref
import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import bspline_ref
import mi_mask_ref as mref
import mi_ref
import phantoms as ph

MARGIN = 1e-4      # voxels: the border condition's shift.  A decision is taken at a coordinate of at most S_m - 1 <= 39 (MAX_SIZE = 40 is the largest moving
# size of any case here); the six fp32 operations behind it round by at most 6 * 40 * 2^-24 = 1.4e-5: the margin is 7 x that
MAX_SIZE = 40


# ---------------------------------------------------------------------------------------------------------------------------------------
# coordinates and validity
# ---------------------------------------------------------------------------------------------------------------------------------------
def _sizes(mshape, dtype):
    return torch.tensor(tuple(mshape)[::-1], dtype=dtype)      # x, y(, z)


def affine_coords(theta, scale, mshape, tshape, dtype=torch.float64):
    """[B, *S_t, nd] (x, y(, z) last): grid_sample's un-normalised coordinate of affine_grid(theta * scale, target) in a moving image of mshape."""
    nd = len(tshape)
    te = theta.reshape(-1, nd, nd + 1).to(dtype) * gref.kernel_scale(scale).to(dtype)
    grid = F.affine_grid(te, [te.shape[0], 1, *tshape], align_corners=False)
    return ((grid + 1.0) * _sizes(mshape, dtype) - 1.0) / 2.0


def flow_coords(theta, flow, mshape, scale=None, dtype=torch.float64):
    """The same for the composed warp: affine_flow_ref.composed_grid un-normalised with the moving sizes (fp64: affine_flow_ref.sample_coords)."""
    m = fref.composed_grid(fref.effective(theta.to(dtype), scale), flow.to(dtype))
    return ((m + 1.0) * _sizes(mshape, dtype) - 1.0) / 2.0


def valid_of(i, mshape, tmask=None, mmask=None):
    """[B, 1, *S_t] bool of coordinates i [B, *S_t, nd]; tmask [B,1,*S_t] / mmask [B,1,*S_m] or None.  torch.round is half to even; NaN fails the bounds."""
    nd = i.shape[-1]
    v = ((i >= 0) & (i <= _sizes(mshape, i.dtype) - 1)).all(-1)
    if mmask is not None:
        r = torch.round(i).long()
        idx = torch.zeros_like(r[..., 0])
        for a in range(nd):                                   # tensor axis a <-> coordinate nd - 1 - a
            idx = idx * mshape[a] + r[..., nd - 1 - a].clamp(0, mshape[a] - 1)
        B = i.shape[0]
        v = v & (mmask.reshape(mmask.shape[0], -1).expand(B, -1).gather(1, idx.reshape(B, -1)).reshape(v.shape) != 0)
    v = v[:, None]
    if tmask is not None:
        v = v & (tmask.reshape(tmask.shape[0], 1, *v.shape[2:]) != 0)
    return v


def border_stable(i, mshape, tmask=None, mmask=None, margin=MARGIN):
    """The border condition: the validity set does not change when every coordinate moves by +-margin on one axis, or on all axes at once in any
    combination of signs (the moving-mask lookup at rint included)."""
    nd = i.shape[-1]
    ref = valid_of(i, mshape, tmask, mmask)
    shifts = [tuple(s if a == ax else 0.0 for a in range(nd)) for ax in range(nd) for s in (-1.0, 1.0)] + list(itertools.product((-1.0, 1.0), repeat=nd))
    return all(bool((valid_of(i + margin * torch.tensor(s, dtype=i.dtype), mshape, tmask, mmask) == ref).all()) for s in shifts)


def fit_range(tgt, mov, tmask=None, mmask=None):
    """[B,4] fp32 under the rule: the target's min / max (inside its mask), the moving image's OWN min / max (inside its mask) - not widened to 0."""
    rng = mi_ref.fit_range(tgt, mov) if tmask is None else mref.fit_range(tgt, mov, tmask)
    for b in range(mov.shape[0]):
        m = mov[b].reshape(-1) if mmask is None else mref.select(mov, mmask, b).reshape(-1)
        m = m if m.numel() else mov[b].reshape(-1)
        rng[b, 2], rng[b, 3] = m.min(), m.max()
    return rng


# ---------------------------------------------------------------------------------------------------------------------------------------
# the fused passes: one evaluation and the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def evaluate(mov, tgt, theta, scale, rng, tmask=None, mmask=None, bins=32, alpha=1.0, normalized=False, dtype=torch.float64):
    """(loss [B], dtheta [B,nd,nd+1] - the UNSCALED theta -, P [B,K,K], valid [B,1,*S_t] bool) - gref.evaluate with the detached validity as mask."""
    valid = valid_of(affine_coords(theta.detach(), scale, mov.shape[2:], tgt.shape[2:], dtype), mov.shape[2:], tmask, mmask)
    return gref.evaluate(mov, tgt, theta, scale, rng, bins, alpha, normalized, dtype, valid) + (valid,)


def loop(mov, tgt, rng, scale, mode, optimizer, lr, iters, start, mi, dtype, tmask=None, mmask=None):
    """gref.loop with the rule: (losses [iters], final parameter, [valid per iteration], [coordinates per iteration])."""
    nd = mov.dim() - 2
    ks = gref.kernel_scale(scale)
    p = start.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses, valids, coords = [], [], []
    for _ in range(iters):
        opt.zero_grad()
        theta = gref.pose_to_theta(p) if mode == "rigid" else p.reshape(1, nd, nd + 1)
        i = affine_coords(theta.detach(), scale, mov.shape[2:], tgt.shape[2:], dtype)
        valid = valid_of(i, mov.shape[2:], tmask, mmask)
        e = mref.loss(tgt, gref.warp(theta, ks, mov, tgt.shape[2:]), valid, rng=rng, dtype=dtype, **mi).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
        valids.append(valid)
        coords.append(i)
    return np.asarray(losses), p.detach().numpy().copy(), valids, coords


def flow_loop(mov, tgt, theta, rng, spacing, optimizer, lr, iters, ctrl0, mi, dtype, tmask=None, mmask=None):
    """fref.loop (B-spline through an initial affine) with the rule: the same four results."""
    sp = tuple(tgt.shape[2:])
    p = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses, valids, coords = [], [], []
    for _ in range(iters):
        opt.zero_grad()
        flow = bspline_ref.expand(p, sp, spacing, dtype=dtype)
        i = flow_coords(theta, flow.detach(), mov.shape[2:], None, dtype)
        valid = valid_of(i, mov.shape[2:], tmask, mmask)
        e = mref.loss(tgt, fref.warp(mov, theta, flow, None, dtype), valid, rng=rng, dtype=dtype, **mi).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
        valids.append(valid)
        coords.append(i)
    return np.asarray(losses), p.detach().numpy().copy(), valids, coords


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests.  B = 2, another theta per pair.  A case's thetas are SHIFT / ZOOM applied to affine_mi_ref.theta0 so that 40 % .. 95 %
# of the target samples are valid and the border condition holds (tests/test_mi_overlap_host.py asserts both).
# ---------------------------------------------------------------------------------------------------------------------------------------
# name -> (target shape, moving shape, (moving voxel, target voxel) or None, target mask?, moving mask?, a translation added to POSES' for this case)
CASES = {
    "3d": ((12, 14, 16), (15, 13, 18), None, False, False, 0.0),
    "3d-voxels-mmask": ((12, 14, 16), (20, 18, 16), ((1.8, 0.8, 1.0), (3.0, 1.0, 1.0)), False, True, 0.00814),
    "2d-tmask": ((24, 28), (30, 22), None, True, False, 0.0),
    "3chunks-mmask": ((20, 33, 70), (17, 40, 31), None, False, True, -0.06136),      # 46 200 voxels: three 16384-voxel chunks, the last ragged
}
# per pair: (zoom of the matrix, translation added to every row)
POSES = ((1.13, 0.171), (0.93, -0.143))


def case_scale(name):
    tshape, mshape, voxels = CASES[name][:3]
    return gref.scale_of(mshape, tshape, *(voxels or (None, None)))


def case_thetas(name):
    """[2, nd, nd+1] fp32, the UNSCALED thetas."""
    nd = len(CASES[name][0])
    out = []
    for zoom, shift in POSES:
        th = aref.theta0(nd).double().clone()
        th[:, :nd] *= zoom
        th[:, nd] += shift + CASES[name][5]
        out.append(th)
    return torch.stack(out).float()


@functools.lru_cache(maxsize=None)
def case(name):
    """(mov [2,1,*S_m], tgt [2,1,*S_t], theta [2,nd,nd+1], scale fp64, tmask or None, mmask or None, rng [2,4])."""
    tshape, mshape, _, tm, mm, _ = CASES[name]
    pairs = [gref.pair(tshape, mshape, seed) for seed in (5, 6)]
    mov, tgt = torch.cat([p[0] for p in pairs]) + 0.25, torch.cat([p[1] for p in pairs])      # + 0.25: the background is not 0, the padding value
    tmask = torch.cat([mref.ellipsoid(tshape, 1.1), mref.ellipsoid(tshape, 0.9)]) if tm else None
    mmask = torch.cat([mref.ellipsoid(mshape, 1.05), mref.ellipsoid(mshape, 0.95, (0.1,) * len(mshape))]) if mm else None
    return mov, tgt, case_thetas(name), case_scale(name), tmask, mmask, fit_range(tgt, mov, tmask, mmask)


@functools.lru_cache(maxsize=None)
def case_arbiter(name, bins=32):
    """((loss, dtheta, P, valid) in fp64, the same in fp32) of a case."""
    mov, tgt, theta, scale, tmask, mmask, rng = case(name)
    return tuple(evaluate(mov, tgt, theta, scale, rng, tmask, mmask, bins, dtype=dt) for dt in (torch.float64, torch.float32))


def special_pair(kind, tshape=(12, 14, 16), mshape=(15, 13, 18)):
    """theta [1,3,4] under scale 1 for which every sample ('all') or no sample ('none') is valid: a zoom-in on the moving image's middle; a shift by
    three cube widths."""
    th = torch.eye(3, 4)
    if kind == "all":
        th[:, :3] *= 0.8
    else:
        th[:, 3] = 3.0
    return th[None]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loops of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
ITERS = 10
# id -> (target shape, moving shape, mode, optimiser, lr, voxels, target mask?, moving mask?, (zoom, shift) of the start).  Shapes, modes and optimisers of
# affine_mi_grids_ref.LOOPS; the starts and rates are chosen so that no sample comes within MARGIN of a border plane in 10 iterations of the fp64
# arbiter (asserted in tests/test_mi_overlap_host.py, which also prints what the six rows of affine_mi_grids_ref.LOOPS do as they stand).
LOOPS = {
    "rigid-adam": ((12, 14, 16), (15, 13, 18), "rigid", "adam", 0.01, None, False, False, 0.00999),
    "rigid-sgd": ((12, 14, 16), (15, 13, 18), "rigid", "sgd", 0.03, None, False, False, 0.00703),
    "affine-adam": ((12, 14, 16), (15, 13, 18), "affine", "adam", 0.005, None, False, False, 0.02627),
    "2d-rigid": ((24, 28), (30, 22), "rigid", "adam", 0.005, None, False, False, 0.0),
    "rigid-voxels": ((12, 14, 16), (20, 18, 16), "rigid", "adam", 0.01, ((1.8, 0.8, 1.0), (3.0, 1.0, 1.0)), False, False, 0.00185),
    "rigid-both-masks": ((12, 14, 16), (15, 13, 18), "rigid", "adam", 0.01, None, True, True, 0.01406),
}


def loop_setup(name):
    """(mov, tgt, scale, tmask, mmask, rng, start) of a LOOPS row; the start is affine_mi_ref.start_of plus the row's offset on every parameter."""
    tshape, mshape, mode, _, _, voxels, tm, mm, offset = LOOPS[name]
    mov, tgt = gref.pair(tshape, mshape)
    mov = mov + 0.25
    scale = gref.scale_of(mshape, tshape, *(voxels or (None, None)))
    tmask = mref.loop_mask(tshape) if tm else None
    mmask = mref.ellipsoid(mshape, 1.05) if mm else None
    return mov, tgt, scale, tmask, mmask, fit_range(tgt, mov, tmask, mmask), aref.start_of(tshape, mode) + offset


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    """(r64, r32) of a LOOPS row, each (losses, final parameter, valids, coordinates)."""
    _, _, mode, optimizer, lr = LOOPS[name][:5]
    mov, tgt, scale, tmask, mmask, rng, start = loop_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    return tuple(loop(mov, tgt, rng, scale, mode, optimizer, lr, ITERS, start, mi, dt, tmask, mmask) for dt in (torch.float64, torch.float32))


# id -> (affine_flow_ref.LOOPS row, moving mask?, a value added to the row's starting control tensor)
FLOW_LOOPS = {"bspline": ("adam", False, 0.00259), "bspline-mmask": ("adam", True, 0.0), "bspline-2d": ("2d", False, 0.0)}


def flow_loop_setup(name):
    """(mov, tgt, theta [1,nd,nd+1], mmask, rng, ctrl0, spacing, optimiser, lr) - affine_flow_ref.loop_setup of the row with the rule's range."""
    row, mm, offset = FLOW_LOOPS[name]
    tshape, mshape, spacing, optimizer, lr = fref.LOOPS[row][:5]
    mov, tgt, theta, _, _, ctrl0 = fref.loop_setup(row)
    ctrl0 = ctrl0 + offset
    mov = mov + 0.25
    mmask = mref.ellipsoid(mshape, 1.05) if mm else None
    return mov, tgt, theta, mmask, fit_range(tgt, mov, None, mmask), ctrl0, spacing, optimizer, lr


@functools.lru_cache(maxsize=None)
def flow_loop_pair(name):
    mov, tgt, theta, mmask, rng, ctrl0, spacing, optimizer, lr = flow_loop_setup(name)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    return tuple(flow_loop(mov, tgt, theta, rng, spacing, optimizer, lr, ITERS, ctrl0, mi, dt, None, mmask) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of trx_affine_flow_valid: the warp cases of tests/affine_flow_ref.py (B = 2, a theta per pair, a smooth flow with jitter, off the voxel
# lattice) under scale 1 or the world scale, with a translation added to every row of both thetas - found by search, so that the border condition
# holds with and without the two masks (asserted in tests/test_mi_overlap_host.py).
# ---------------------------------------------------------------------------------------------------------------------------------------
# id -> (affine_flow_ref.CASES row, world scale?, translation)
VALID_CASES = {
    "9x11x13": ("9x11x13", False, -0.00029),
    "9x11x13-world": ("9x11x13", True, 0.0),
    "17x19": ("17x19", False, 0.0),
    "17x19-world": ("17x19", True, 0.0),
    "w5-world": ("w5", True, 0.0),
    "20x33x70": ("20x33x70", False, -0.00203),
}


@functools.lru_cache(maxsize=None)
def valid_case(name):
    """(moving shape, theta [2,nd,nd+1] fp32, flow [2,nd,*S_t] fp32, scale, tmask [2,1,*S_t], mmask [2,1,*S_m])."""
    row, world, shift = VALID_CASES[name]
    tshape, mshape = fref.CASES[row][:2]
    _, theta, flow, _ = fref.case(row, world)
    theta = theta.clone()
    theta[:, :, -1] += shift
    tmask = torch.cat([mref.ellipsoid(tshape, 1.1), mref.checkerboard(tshape)])
    mmask = torch.cat([mref.ellipsoid(mshape, 1.05), mref.ellipsoid(mshape, 0.9)])
    return mshape, theta, flow, fref.case_scale(row, world), tmask, mmask


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the rule is for: a moving image that covers part of the target, with a background that is not 0
# ---------------------------------------------------------------------------------------------------------------------------------------
CROP_SHAPE, CROP_Z = (20, 24, 28), (3, 15)      # the moving image: slices 3 .. 14 of the 20 along z
CROP_LR, CROP_ITERS, CROP_START = 0.002, 150, 0.04


def crop_pair():
    """(moving [1,1,12,24,28], target [1,1,20,24,28], the true theta [3,4] fp64): the target is phantoms.blobs; the moving image 1 + 4w(1 - w) of the
    same phantom (background 1), cropped along z.  Target slice z is moving slice z - 3, so in normalised coordinates z_m = (20 z_t + 14) / 12 - 1:
    theta = diag(1, 1, 5/3) with a z translation of 1/6, exactly."""
    tgt = ph.blobs(CROP_SHAPE, 5)
    mov = (1.0 + 4.0 * tgt * (1.0 - tgt))[:, :, CROP_Z[0]:CROP_Z[1]].contiguous().float()
    truth = torch.eye(3, 4, dtype=torch.float64)
    n = CROP_Z[1] - CROP_Z[0]
    truth[2, 2], truth[2, 3] = CROP_SHAPE[0] / n, (CROP_SHAPE[0] - CROP_Z[0] - CROP_Z[1]) / n
    return mov, tgt, truth


def crop_start(truth):
    """CROP_START off the truth on every entry, signs alternating."""
    sign = torch.tensor([1.0, -1.0] * 6, dtype=torch.float64).reshape(3, 4)
    return truth + CROP_START * sign


@functools.lru_cache(maxsize=None)
def crop_run(overlap):
    """The fp64 arbiter, affine, Adam: (max |theta - truth| at the end, relative z-scale error at the end, share of valid samples at the truth)."""
    mov, tgt, truth = crop_pair()
    ones = torch.ones(3, 4, dtype=torch.float64)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    start = crop_start(truth).reshape(-1)
    if overlap:
        p = loop(mov, tgt, fit_range(tgt, mov), ones, "affine", "adam", CROP_LR, CROP_ITERS, start, mi, torch.float64)[1]
    else:
        p = gref.loop(mov, tgt, mi_ref.fit_range(tgt, mov), ones, "affine", "adam", CROP_LR, CROP_ITERS, start, mi, torch.float64)[1]
    p = torch.as_tensor(p).reshape(3, 4)
    i = affine_coords(truth[None], ones, mov.shape[2:], CROP_SHAPE)      # at the truth the edge slices sit ON the planes 0 and S - 1: counted, up to rounding
    share = ((i >= -1e-9) & (i <= _sizes(mov.shape[2:], i.dtype) - 1 + 1e-9)).all(-1).double().mean().item()
    return (p - truth).abs().max().item(), (p[2, 2] / truth[2, 2] - 1.0).item(), share
