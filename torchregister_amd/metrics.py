"""Scoring a registration on its labels: the exact Euclidean distance transform in millimetres (trx_distance_transform), what is
built on it - signed distance maps, masks grown or shrunk by a margin, Hausdorff / percentile / average symmetric surface distances - and label overlap
(Dice; trx_label_overlap).  Every function takes GPU tensors; shape and value errors are ValueErrors raised before anything touches a device.  Nothing here
is differentiable."""
import collections
import ctypes
import math

import torch

from . import _lib
from ._engine import _dhw


def _on_gpu(t, name):
    if not t.is_cuda:
        raise _lib.TrxError(f"{name} is on {t.device}: torchregister_amd runs only on an AMD GPU through its HIP library (no CPU fallback). "
                            f"Move the tensors to 'cuda'.")


def _mask_shape(mask, name="mask"):
    """A binary mask [B,1,*spatial] or [B,*spatial], any numeric dtype -> (B, spatial); shapes only."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"{name} must be a tensor [B,1,*spatial] or [B,*spatial], got {type(mask).__name__}")
    shape = tuple(mask.shape)
    if len(shape) in (4, 5) and shape[1] == 1:
        sp = shape[2:]
    elif len(shape) in (3, 4):
        sp = shape[1:]
    else:
        raise ValueError(f"{name} must be [B,1,*spatial] or [B,*spatial] with 2 or 3 spatial axes, got {shape}")
    if shape[0] < 1 or min(sp) < 1:
        raise ValueError(f"{name} {shape} has an empty axis")
    if max(sp) > 16384:
        raise ValueError(f"{name} {shape}: at most 16384 voxels per axis")
    return shape[0], tuple(sp)


def _mask_bytes(mask, name="mask"):
    """-> contiguous uint8 [B,*spatial] of 0 / 1 on the mask's device (non-zero = set), after the shape and the device checks."""
    B, sp = _mask_shape(mask, name)
    _on_gpu(mask, name)
    return (mask.detach().reshape((B,) + sp) != 0).to(torch.uint8).contiguous()


def _voxel(voxel, nd):
    """voxel=None or nd finite sizes > 0 in the tensor's axis order -> a ctypes float array or None."""
    if voxel is None:
        return None
    try:
        v = [float(x) for x in voxel]
    except (TypeError, ValueError):
        raise ValueError(f"voxel must be {nd} sizes in the tensor's axis order, got {voxel!r}") from None
    if len(v) != nd or not all(math.isfinite(x) and x > 0 for x in v):
        raise ValueError(f"voxel must be {nd} finite sizes > 0 in the tensor's axis order, got {voxel!r}")
    return (ctypes.c_float * nd)(*v)


def _radius(radius):
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise ValueError(f"radius must be a finite number >= 0, got {radius!r}") from None
    if isinstance(radius, bool) or not math.isfinite(r) or r < 0:
        raise ValueError(f"radius must be a finite number >= 0, got {radius!r}")
    return r


def _dist2(m, sp, voxel_c, want_indices):
    """trx_distance_transform on uint8 [B,*sp] -> (dist2 [B,1,*sp] fp32, nearest [B,nd,*sp] int32 or None)."""
    lib = _lib.load()
    B, nd = m.shape[0], len(sp)
    geom = (nd, B) + _dhw(sp)
    nbytes = lib.trx_distance_workspace_bytes(*geom)
    if nbytes == 0:
        raise _lib.TrxError(f"trx_distance_workspace_bytes rejected {tuple(m.shape)}")
    d2 = torch.empty((B, 1) + sp, dtype=torch.float32, device=m.device)
    idx = torch.empty((B, nd) + sp, dtype=torch.int32, device=m.device) if want_indices else None
    ws = torch.empty(nbytes, dtype=torch.uint8, device=m.device)
    with torch.cuda.device(m.device):
        rc = lib.trx_distance_transform(_lib.ptr(m), *geom, voxel_c, _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(ws), nbytes, _lib.current_stream(m.device))
    _lib.check(rc, "trx_distance_transform")
    return d2, idx


def distance_transform(mask, voxel=None, squared=False, return_indices=False):
    """The exact Euclidean distance [B,1,*spatial] fp32 from every voxel centre to the centre of the nearest NON-ZERO voxel of `mask` ([B,1,*spatial] or
    [B,*spatial], any numeric dtype, on the GPU), 0 on the mask itself, +inf for a pair whose mask is empty.  voxel: the voxel sizes in the tensor's
    axis order, (dz, dy, dx) or (dy, dx), for a distance in millimetres; None: in voxels, computed in integers (the squared distance is exact below
    2^24).  squared=True returns the squared distance the kernel computes (trx_distance_transform); otherwise its torch.sqrt.  return_indices=True:
    also the index [B,nd,*spatial] int32 of a nearest non-zero voxel, channel a along spatial axis a (-1 for an empty pair); of several equidistant
    ones always the same.  scipy.ndimage.distance_transform_edt(m, sampling=voxel), the distance to the nearest ZERO voxel, is
    tr.distance_transform(m == 0, voxel).  No host sync."""
    B, sp = _mask_shape(mask)
    vc = _voxel(voxel, len(sp))
    d2, idx = _dist2(_mask_bytes(mask), sp, vc, return_indices)
    d = d2 if squared else torch.sqrt(d2)
    return (d, idx) if return_indices else d


def signed_distance(mask, voxel=None):
    """distance_transform(mask) - distance_transform(mask == 0) [B,1,*spatial] fp32: >= one voxel size outside the mask, <= minus one voxel size inside.
    Two segmentations can be registered through their signed distance maps with the fused MSE / NCC loops as they are.  A pair whose mask is empty or
    full has no such map: ValueError (this check reads one flag per pair back: a host sync)."""
    B, sp = _mask_shape(mask)
    vc = _voxel(voxel, len(sp))
    _check_not_constant(mask.detach().reshape(B, -1) != 0)      # the argument alone decides: also on CPU tensors, before the device check
    m = _mask_bytes(mask)
    outside, _ = _dist2(m, sp, vc, False)
    inside, _ = _dist2(1 - m, sp, vc, False)
    return torch.sqrt(outside) - torch.sqrt(inside)


def _check_not_constant(flat):
    any_, all_ = flat.any(dim=1).cpu(), flat.all(dim=1).cpu()
    for b in range(flat.shape[0]):
        if not bool(any_[b]) or bool(all_[b]):
            raise ValueError(f"signed_distance: the mask of pair {b} is {'full' if bool(all_[b]) else 'empty'}: it has no boundary to measure from")


def dilate_mask(mask, radius, voxel=None):
    """The mask grown by `radius` (mm, or voxels without `voxel`; finite, >= 0): distance_transform(mask, voxel) <= radius as uint8 [B,1,*spatial], ready
    for mask= / moving_mask=."""
    B, sp = _mask_shape(mask)
    vc, r = _voxel(voxel, len(sp)), _radius(radius)
    d2, _ = _dist2(_mask_bytes(mask), sp, vc, False)
    return (torch.sqrt(d2) <= r).to(torch.uint8)


def erode_mask(mask, radius, voxel=None):
    """The mask shrunk by `radius`: distance_transform(mask == 0, voxel) > radius as uint8 [B,1,*spatial].  A full mask stays full (nothing to measure from)."""
    B, sp = _mask_shape(mask)
    vc, r = _voxel(voxel, len(sp)), _radius(radius)
    d2, _ = _dist2(1 - _mask_bytes(mask), sp, vc, False)
    return (torch.sqrt(d2) > r).to(torch.uint8)


def mask_surface(mask):
    """The surface voxels of a binary mask, uint8 [B,1,*spatial]: set, with at least one of the 2 nd face neighbours not set or outside the volume -
    mask & ~scipy.ndimage.binary_erosion(mask, border_value=0), MedPy's surface (trx_mask_surface)."""
    B, sp = _mask_shape(mask)
    m = _mask_bytes(mask)
    out = torch.empty((B, 1) + sp, dtype=torch.uint8, device=m.device)
    with torch.cuda.device(m.device):
        rc = _lib.load().trx_mask_surface(_lib.ptr(m), len(sp), B, *_dhw(sp), _lib.ptr(out), _lib.current_stream(m.device))
    _lib.check(rc, "trx_mask_surface")
    return out


def _label_map(t, name):
    B, sp = _mask_shape(t, name)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer label map, got {t.dtype}")
    return B, sp


def label_overlap(a, b, labels):
    """(dice [B,L] fp64, counts [B,L,3] int64) of two integer label maps [B,1,*spatial] or [B,*spatial] on the GPU for the labels 0 .. L - 1
    (L = labels, 1 .. 4096): counts[b, l] = |a = l|, |b = l|, |a = l and b = l| (trx_label_overlap), dice = 2 |a and b| / (|a| + |b|), NaN where a
    label is absent from both.  A value outside [0, L) counts nowhere.  uint8 and int32 maps go to the kernel as they are, other integer dtypes are cast
    to int32; a floating dtype is a ValueError.  No host sync."""
    (B, sp), (Bb, spb) = _label_map(a, "a"), _label_map(b, "b")
    if (B, sp) != (Bb, spb):
        raise ValueError(f"label maps of different shapes: {tuple(a.shape)} and {tuple(b.shape)}")
    if isinstance(labels, bool) or not isinstance(labels, int) or not 1 <= labels <= 4096:
        raise ValueError(f"labels must be an int in 1 .. 4096, got {labels!r}")
    _on_gpu(a, "a")
    _on_gpu(b, "b")
    dt = torch.uint8 if a.dtype == torch.uint8 and b.dtype == torch.uint8 else torch.int32
    a_, b_ = (t.detach().reshape((B,) + sp).to(dt).contiguous() for t in (a, b))
    counts = torch.empty((B, labels, 3), dtype=torch.int64, device=a_.device)
    with torch.cuda.device(a_.device):
        rc = _lib.load().trx_label_overlap(_lib.ptr(a_), _lib.ptr(b_), 1 if dt == torch.uint8 else 4, len(sp), B, *_dhw(sp), labels, _lib.ptr(counts),
                                           _lib.current_stream(a_.device))
    _lib.check(rc, "trx_label_overlap")
    c = counts.double()
    return 2.0 * c[..., 2] / (c[..., 0] + c[..., 1]), counts


SurfaceDistances = collections.namedtuple("SurfaceDistances", "hausdorff hd_percentile assd n_a n_b")


def surface_distances(a, b, voxel=None, percentile=95.0):
    """Surface distances of two binary masks per pair, SurfaceDistances(hausdorff, hd_percentile, assd, n_a, n_b): fp64 [B] (n_a, n_b: int64 [B], the
    surface voxel counts), on the masks' device.  d_ab = the distance transform of b's surface (mask_surface) read at a's surface voxels, d_ba the other
    way round, in mm with `voxel`; hausdorff = max(max d_ab, max d_ba); hd_percentile = numpy's linear-interpolation percentile of the concatenation of
    d_ab and d_ba (MedPy's hd95 at 95); assd = (mean d_ab + mean d_ba) / 2.  A pair in which either mask is empty gives NaN.  The selection and the
    percentile are torch on the compacted surface values (a sort): this function synchronises with the host once per pair."""
    (B, sp), (Bb, spb) = _mask_shape(a, "a"), _mask_shape(b, "b")
    if (B, sp) != (Bb, spb):
        raise ValueError(f"masks of different shapes: {tuple(a.shape)} and {tuple(b.shape)}")
    vc = _voxel(voxel, len(sp))
    try:
        q = float(percentile)
    except (TypeError, ValueError):
        raise ValueError(f"percentile must be a number in 0 .. 100, got {percentile!r}") from None
    if not 0.0 <= q <= 100.0:
        raise ValueError(f"percentile must be a number in 0 .. 100, got {percentile!r}")
    sa, sb = mask_surface(a), mask_surface(b)
    da, _ = _dist2(sa.reshape((B,) + sp), sp, vc, False)      # distance to a's surface
    db, _ = _dist2(sb.reshape((B,) + sp), sp, vc, False)
    nan = float("nan")
    rows = []
    for p in range(B):
        d_ab, d_ba = torch.sqrt(db[p][sa[p] != 0]).double(), torch.sqrt(da[p][sb[p] != 0]).double()
        na, nb = d_ab.numel(), d_ba.numel()      # the compaction's sizes: the host sync
        if na == 0 or nb == 0:
            rows.append((nan, nan, nan, na, nb))
            continue
        both = torch.sort(torch.cat([d_ab, d_ba])).values
        pos = q / 100.0 * (both.numel() - 1)
        lo = int(math.floor(pos))
        hi = min(lo + 1, both.numel() - 1)
        pct = both[lo] + (both[hi] - both[lo]) * (pos - lo)
        rows.append((torch.maximum(d_ab.max(), d_ba.max()), pct, 0.5 * (d_ab.mean() + d_ba.mean()), na, nb))
    dev = sa.device
    col = lambda k, dt: torch.stack([torch.as_tensor(r[k], dtype=dt, device=dev) for r in rows])  # noqa: E731
    return SurfaceDistances(col(0, torch.float64), col(1, torch.float64), col(2, torch.float64), col(3, torch.int64), col(4, torch.int64))
