"""Coarse-to-fine pyramids (extension: the reference registers at one resolution).

pyramid_shapes: the level rule, host only.  pyramid / upsample_flow: trx_resample (csrc/pyramid.hip) on the GPU.
theta lives in affine_grid's normalised coordinates (align_corners=False), and a coarse level covers the same extent as its parent, so
one theta is the same mapping at every level: rigid and affine hand their parameters up unchanged.  A flow is in voxel units, so
upsample_flow rescales channel i by the growth of spatial dim i under SpatialTransformer's align_corners=True convention.
"""
import ctypes
import math

import torch

from . import _lib
from ._engine import _require_gpu

MIN_SIZE = 8   # an axis is not halved below this


def pyramid_shapes(spatial, levels):
    """Spatial shapes of a `levels`-level pyramid, coarsest first (the last one is `spatial`).  One level coarser: every axis becomes
    ceil(s / 2) unless that is below MIN_SIZE (then it keeps its size).  ValueError if some level would not shrink at all."""
    spatial = tuple(int(s) for s in spatial)
    levels = int(levels)
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    shapes = [spatial]
    while len(shapes) < levels:
        prev = shapes[-1]
        nxt = tuple(s if math.ceil(s / 2) < MIN_SIZE else math.ceil(s / 2) for s in prev)
        if nxt == prev:
            raise ValueError(f"levels={levels}: no axis of {prev} can be halved without going below {MIN_SIZE} voxels; "
                             f"the largest levels that works for {spatial} is {len(shapes)}")
        shapes.append(nxt)
    return shapes[::-1]


def level_theta(theta, target_full, target_level, moving_full, moving_level):
    """The theta between two LEVEL lattices of align_corners=True pyramids, from the theta between the full ones (pure host arithmetic, fp64,
    returned in theta's dtype; shapes in the tensors' axis order).  A level's voxel j sits at the full voxel j (S - 1) / (S_l - 1), so in
    affine_grid's normalised coordinates n_full = a n_level with a = S_l (S - 1) / (S (S_l - 1)) per axis (1 where the axis keeps its size):
    theta_level[r][c] = theta[r][c] a_t[c] / a_m[r] and theta_level[r][nd] = theta[r][nd] / a_m[r] (rows / columns x, y(, z))."""
    nd = len(target_full)
    if tuple(theta.shape[-2:]) != (nd, nd + 1) or not len(target_level) == len(moving_full) == len(moving_level) == nd:
        raise ValueError(f"expected a theta [..., {nd}, {nd + 1}] and four shapes of {nd} sizes, got {tuple(theta.shape)}, {tuple(target_full)}, "
                         f"{tuple(target_level)}, {tuple(moving_full)}, {tuple(moving_level)}")

    def growth(full, level):      # a per axis, in theta's x, y(, z) order
        return [1.0 if int(S) == int(Sl) else int(Sl) * (int(S) - 1) / (int(S) * (int(Sl) - 1)) for S, Sl in zip(full[::-1], level[::-1])]

    a_t = torch.tensor(growth(tuple(target_full), tuple(target_level)) + [1.0], dtype=torch.float64, device=theta.device)
    a_m = torch.tensor(growth(tuple(moving_full), tuple(moving_level)), dtype=torch.float64, device=theta.device)
    return (theta.double() * a_t / a_m[:, None]).to(theta.dtype)


def resample(x, size, align_corners=False, channel_scale=None):
    """trx_resample of x [B, C, *sp] (fp32, GPU) to [B, C, *size]: per axis a [1,4,6,4,1]/16 blur before a shrink, then linear
    interpolation at F.interpolate's positions; channel_scale: C floats, channel c multiplied by channel_scale[c]."""
    _require_gpu(x, "x")
    nd = x.dim() - 2
    if nd not in (2, 3):
        raise ValueError(f"expected [B,C,H,W] or [B,C,D,H,W], got {tuple(x.shape)}")
    size = tuple(int(s) for s in size)
    if len(size) != nd:
        raise ValueError(f"size {size} does not match the {nd} spatial dims of {tuple(x.shape)}")
    lib = _lib.load()
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    D, H, W = ((1,) + tuple(x.shape[2:])) if nd == 2 else tuple(x.shape[2:])
    Do, Ho, Wo = ((1,) + size) if nd == 2 else size
    out = torch.empty((B, C) + size, dtype=torch.float32, device=x.device)
    args = (nd, B * C, D, H, W, Do, Ho, Wo)
    ws_bytes = lib.trx_resample_workspace_bytes(*args)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_resample_workspace_bytes rejected {tuple(x.shape)} -> {size}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    scale = None
    if channel_scale is not None:
        if len(channel_scale) != C:
            raise ValueError(f"channel_scale needs {C} values, got {len(channel_scale)}")
        scale = (ctypes.c_float * C)(*[float(s) for s in channel_scale])
    with torch.cuda.device(x.device):
        rc = lib.trx_resample(_lib.ptr(x), _lib.ptr(out), *args, int(bool(align_corners)), C, scale, _lib.ptr(ws), ws_bytes,
                              _lib.current_stream(x.device))
    _lib.check(rc, "trx_resample")
    return out


def pyramid(x, levels, align_corners=False, shrink=None, sigma=None):
    """[coarsest, ..., finest] levels of x [B, C, *sp] (GPU): each level is trx_resample of the level directly above it; the finest entry
    is x itself.
    shrink (a schedule: `levels` tuples of per-axis integer factors, coarsest first, the finest all ones - pyramid_schedule makes one from the
    voxel sizes): level k has shape ceil(S / f_k) and is gaussian_resample of the FULL-resolution x, with sigma[k] in x's voxels (None: f / 2
    where f > 1, elastix's default) and border padding; a level with factors all 1 and sigma all 0 is x itself."""
    _require_gpu(x, "x")
    if shrink is not None:
        from .gaussian import scheduled_pyramid
        return scheduled_pyramid(x, levels, align_corners, shrink, sigma)
    if sigma is not None:
        raise ValueError("sigma goes with shrink: the halving pyramid has its fixed [1,4,6,4,1]/16 blur")
    shapes = pyramid_shapes(x.shape[2:], levels)
    out = [x]
    for s in shapes[-2::-1]:
        out.append(resample(out[-1], s, align_corners))
    return out[::-1]


def pyramid_masks(mask, levels, align_corners=False, shrink=None, sigma=None):
    """[coarsest, ..., finest] uint8 masks of a region-of-interest mask [B, 1, *sp] (GPU, non-zero = the voxel counts): the mask as 0.0 / 1.0
    floats through the pyramid() call that makes the target's levels (same blur, same positions, same align_corners), a voxel of a level counting
    where the result is >= 0.5.  ValueError if some pair's mask is empty at some level (level 1 = the coarsest); one host sync per level.
    shrink, sigma: pyramid()'s schedule - the same rule through the same call."""
    out = []
    for k, m in enumerate(pyramid((mask != 0).float(), levels, align_corners, shrink, sigma)):
        m8 = (m >= 0.5).to(torch.uint8).contiguous()
        empty = (m8.flatten(1).amax(1) == 0).nonzero().flatten().tolist()
        if empty:
            raise ValueError(f"mask: pair {empty[0]} has no voxel left at level {k + 1} of {levels} (shape {tuple(m.shape[2:])}); "
                             f"a level's mask is the pyramid of the mask thresholded at 0.5 - use fewer levels or a larger region")
        out.append(m8)
    return out


def upsample_flow(flow, size):
    """A flow [B, nd, *sp] (voxel units, channel i along spatial dim i, SpatialTransformer's align_corners=True convention) moved to
    the grid `size`: linear interpolation with align_corners=True, channel i scaled by (S_i - 1) / (s_i - 1) (1 where the axis keeps
    its size or has one voxel)."""
    nd = flow.dim() - 2
    size = tuple(int(s) for s in size)
    if flow.shape[1] != nd or len(size) != nd:
        raise ValueError(f"expected a flow [B,{nd},*sp] and {nd} sizes, got {tuple(flow.shape)} and {size}")
    sp = tuple(flow.shape[2:])
    scale = [1.0 if (S == s or s == 1) else (S - 1) / (s - 1) for S, s in zip(size, sp)]
    return resample(flow, size, align_corners=True, channel_scale=scale)
