"""Gaussian smoothing in voxels or millimetres, and the voxel-aware pyramid schedule (extension).

gaussian_resample / gaussian_smooth: trx_gaussian_resample (csrc/gaussian.hip) on the GPU.  pyramid_schedule: the per-axis shrink factors and
sigmas of a coarse-to-fine pyramid from the voxel sizes, host only (elastix's ImagePyramidSchedule rule: sigma = factor / 2).
"""
import ctypes
import math

import torch

from . import _lib
from ._engine import _require_gpu
from .pyramid import MIN_SIZE

PADDING = {'zeros': 0, 'border': 1}


def _per_axis(value, nd, name):
    """`nd` floats from a scalar or one value per spatial axis."""
    vals = [float(v) for v in value] if isinstance(value, (list, tuple)) or (torch.is_tensor(value) and value.dim() > 0) else [float(value)] * nd
    if len(vals) != nd:
        raise ValueError(f"{name} needs one value or {nd} (one per spatial axis), got {len(vals)}")
    return vals


def _sigmas(sigma, nd):
    vals = _per_axis(sigma, nd, "sigma")
    if any(not math.isfinite(s) or s < 0 for s in vals):
        raise ValueError(f"sigma must be finite and >= 0, got {sigma!r}")
    return vals


def gaussian_resample(x, size, sigma, align_corners=False, truncate=4.0, padding='border'):
    """trx_gaussian_resample of x [B, C, *sp] (fp32, GPU) to [B, C, *size]: per axis a Gaussian of `sigma` voxels of x (a scalar or one per spatial
    axis; radius int(truncate sigma + 0.5), scipy.ndimage.gaussian_filter's), then linear interpolation at F.interpolate's positions where the size
    changes.  padding 'border' (indices clamped, scipy's 'nearest') or 'zeros' (scipy's 'constant').  Not differentiable."""
    _require_gpu(x, "x")
    nd = x.dim() - 2
    if nd not in (2, 3):
        raise ValueError(f"expected [B,C,H,W] or [B,C,D,H,W], got {tuple(x.shape)}")
    size = tuple(int(s) for s in size)
    if len(size) != nd:
        raise ValueError(f"size {size} does not match the {nd} spatial dims of {tuple(x.shape)}")
    if padding not in PADDING:
        raise ValueError(f"padding must be 'border' or 'zeros', got {padding!r}")
    truncate = float(truncate)
    if not math.isfinite(truncate) or truncate <= 0:
        raise ValueError(f"truncate must be finite and > 0, got {truncate!r}")
    sig = (ctypes.c_float * nd)(*_sigmas(sigma, nd))
    lib = _lib.load()
    x = x.contiguous()
    B, C = x.shape[0], x.shape[1]
    D, H, W = ((1,) + tuple(x.shape[2:])) if nd == 2 else tuple(x.shape[2:])
    Do, Ho, Wo = ((1,) + size) if nd == 2 else size
    out = torch.empty((B, C) + size, dtype=torch.float32, device=x.device)
    args = (nd, B * C, D, H, W, Do, Ho, Wo)
    ws_bytes = lib.trx_gaussian_workspace_bytes(*args)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_gaussian_workspace_bytes rejected {tuple(x.shape)} -> {size}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.trx_gaussian_resample(_lib.ptr(x), _lib.ptr(out), *args, sig, truncate, int(bool(align_corners)), PADDING[padding], _lib.ptr(ws),
                                       ws_bytes, _lib.current_stream(x.device))
    _lib.check(rc, "trx_gaussian_resample")
    return out


class _SmoothZeros(torch.autograd.Function):
    """The same-size operator with zero padding is symmetric (tap t of output i is tap 2R - t of output i - R + t, and g is even): its adjoint
    is the same call."""

    @staticmethod
    def forward(ctx, x, sigma, truncate):
        ctx.sigma, ctx.truncate = sigma, truncate
        return gaussian_resample(x.detach(), x.shape[2:], sigma, False, truncate, 'zeros')

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        return gaussian_resample(grad, grad.shape[2:], ctx.sigma, False, ctx.truncate, 'zeros'), None, None


def gaussian_smooth(x, sigma, voxel=None, truncate=4.0, padding='border'):
    """x [B, C, *sp] (fp32, GPU) smoothed by a Gaussian, same size.  sigma: a scalar or one value per spatial axis, in voxels - or, with
    voxel=(dz, dy, dx) / (dy, dx) (the voxel sizes in mm), in millimetres: each axis gets sigma / voxel.  padding='zeros' is differentiable (the
    operator is its own adjoint); with padding='border' a tensor that requires grad raises ValueError."""
    nd = x.dim() - 2
    sig = _sigmas(sigma, nd)
    if voxel is not None:
        vox = _per_axis(voxel, nd, "voxel")
        if any(not math.isfinite(v) or v <= 0 for v in vox):
            raise ValueError(f"voxel sizes must be finite and > 0, got {voxel!r}")
        sig = [s / v for s, v in zip(sig, vox)]
    if padding == 'zeros':
        return _SmoothZeros.apply(x, tuple(sig), float(truncate))
    if x.requires_grad:
        raise ValueError("gaussian_smooth with padding='border' is not differentiable (the clamped boundary is not symmetric): use padding='zeros' or detach x")
    return gaussian_resample(x, x.shape[2:], sig, False, truncate, padding)


def _factors(shrink, nd, levels, name):
    """A schedule's shrink factors as `levels` tuples of nd ints >= 1 (nd None: of any one length; a bare int stands for every axis), the finest all
    ones; ValueError otherwise."""
    if not isinstance(shrink, (list, tuple)) or len(shrink) != levels:
        raise ValueError(f"{name} needs {levels} entries (one per level, coarsest first), got {shrink!r}")
    out = []
    for f in shrink:
        f = tuple(f) if isinstance(f, (list, tuple)) else (f,) * (nd or 1)
        if not f or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in f) or (nd is not None and len(f) != nd):
            raise ValueError(f"{name}: a level's factors are ints >= 1, one per spatial axis, got {f!r}")
        out.append(f)
    if any(v != 1 for v in out[-1]):
        raise ValueError(f"{name}: the finest level's factors must all be 1, got {out[-1]!r}")
    return out


def _level_sigmas(sigma, shrink, nd, levels, name):
    """A schedule's sigmas (voxels of the full image): None -> f / 2 where f > 1, else 0 (elastix's default).  nd None (the number of axes is not
    known yet): a level's sigmas are checked against the length of its factors, unless those were a bare int - then any length stands until optim."""
    if sigma is None:
        return [tuple(f / 2 if f > 1 else 0.0 for f in fs) for fs in shrink]
    if not isinstance(sigma, (list, tuple)) or len(sigma) != levels:
        raise ValueError(f"{name} needs {levels} entries (one per level, coarsest first), got {sigma!r}")
    out = []
    for k, s in enumerate(sigma):
        n = nd if nd is not None else len(shrink[k])
        if nd is None and n == 1 and isinstance(s, (list, tuple)):
            n = len(s)
        out.append(tuple(_sigmas(list(s) if isinstance(s, (list, tuple)) else s, n)))
    return out


def schedule_shapes(spatial, shrink):
    """Level shapes of a schedule: ceil(S_a / f_a) per axis."""
    return [tuple(-(-int(s) // int(f)) for s, f in zip(spatial, fs)) for fs in shrink]


def pyramid_schedule(spatial, levels, voxel=None):
    """(shrink, sigma) of a `levels`-level pyramid of an image of shape `spatial`, each `levels` tuples of nd values, coarsest first (host only).
    Level k shrinks by t = 2^(levels - 1 - k) along the axis with the smallest voxel; along axis a by f_a = max(1, floor(t v_min / v_a + 1e-6)),
    so that the level's voxels come out as isotropic as whole factors allow (f_a = t without `voxel`); f_a is lowered while ceil(S_a / f_a)
    would fall below MIN_SIZE.  sigma_a = f_a / 2 voxels where f_a > 1, else 0.  A level has shape ceil(S_a / f_a).  ValueError if two
    neighbouring levels have the same shape."""
    spatial = tuple(int(s) for s in spatial)
    levels = int(levels)
    nd = len(spatial)
    if levels < 1:
        raise ValueError(f"levels must be >= 1, got {levels}")
    if voxel is not None:
        voxel = _per_axis(voxel, nd, "voxel")
        if any(not math.isfinite(v) or v <= 0 for v in voxel):
            raise ValueError(f"voxel sizes must be finite and > 0, got {voxel!r}")
    def factors(L):
        out = []
        for k in range(L):
            t = 2 ** (L - 1 - k)
            fs = []
            for a, S in enumerate(spatial):
                f = t if voxel is None else max(1, math.floor(t * min(voxel) / voxel[a] + 1e-6))
                while f > 1 and math.ceil(S / f) < MIN_SIZE:
                    f -= 1
                fs.append(f)
            out.append(tuple(fs))
        return out

    def stalls(fs):      # the shape that two neighbouring levels share, or None
        shapes = schedule_shapes(spatial, fs)
        return next((shapes[k] for k in range(len(fs) - 1, 0, -1) if shapes[k - 1] == shapes[k]), None)

    shrink = factors(levels)
    stuck = stalls(shrink)
    if stuck is not None:
        works = next(L for L in range(levels - 1, 0, -1) if stalls(factors(L)) is None)
        raise ValueError(f"levels={levels}: no axis of {stuck} can be halved without going below {MIN_SIZE} voxels; "
                         f"the largest levels that works for {spatial} is {works}")
    return shrink, _level_sigmas(None, shrink, nd, levels, "sigma")


def scheduled_pyramid(x, levels, align_corners, shrink, sigma):
    """pyramid()'s levels under a schedule: level k = gaussian_resample of the full-resolution x to ceil(S / f_k) with sigma[k] voxels of x, border
    padding; a level whose factors are all 1 and whose sigmas are all 0 is x itself."""
    nd = x.dim() - 2
    shrink = _factors(shrink, nd, int(levels), "shrink")
    sigma = _level_sigmas(sigma, shrink, nd, int(levels), "sigma")
    out = []
    for fs, sg, shape in zip(shrink, sigma, schedule_shapes(x.shape[2:], shrink)):
        same = all(f == 1 for f in fs) and all(s == 0 for s in sg)
        out.append(x if same else gaussian_resample(x, shape, sg, align_corners))
    return out
