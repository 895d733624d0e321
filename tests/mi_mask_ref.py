"""The region-of-interest mask of the mutual-information entry points (trx_mi_cfg.mask, include/trx.h), restated without any new maths: mutual
information depends on nothing but the multiset of (target, warped) value pairs, so for pair b the voxels inside the mask are selected -
t[M_b], w[M_b] - and handed to tests/mi_ref.py as an image of N_m voxels.  Boolean indexing is differentiable: torch autograd gives d loss /
d warped, zero outside the mask.  An empty mask has loss 0 and gradient 0 by definition.  The affine form puts oracle/compose.py::affine_warp in
front (tests/affine_mi_ref.py's phantoms, starts and loop configurations), the flow forms oracle/compose.py::flow_warp (+ tests/bspline_ref.py,
tests/bspline_bending_ref.py).  Nothing here touches the GPU."""
import functools
import math

import numpy as np
import torch

import affine_mi_ref as aref
import mi_ref

CHUNK = 16384      # voxels per block of the histogram and gradient passes (csrc/mi_dev.h: kMiChunk)


# ---------------------------------------------------------------------------------------------------------------------------------------
# masks [1,1,*shape] bool
# ---------------------------------------------------------------------------------------------------------------------------------------
def ellipsoid(shape, radius=0.7, centre=None):
    """Voxels whose centre, in the normalised coordinates (2i + 1) / S - 1 of every axis, lies within `radius` of `centre` (default: the middle):
    3 249 of 17 917 voxels at 19x23x41, 6 387 of 16 637 at 131x127, 32 of 210 at 5x6x7."""
    centre = (0.0,) * len(shape) if centre is None else centre
    d = torch.zeros(shape, dtype=torch.float64)
    for ax, (s, c) in enumerate(zip(shape, centre)):
        x = ((2.0 * torch.arange(s, dtype=torch.float64) + 1.0) / s - 1.0 - c) / radius
        d = d + (x * x).reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return (d <= 1.0)[None, None]


def first_chunk_empty(shape):
    """Zero for every flat index below CHUNK: the first block of a pair has nothing to add (and, in pass 2, an all-zero partial row to write)."""
    return (torch.arange(math.prod(shape)) >= CHUNK).reshape((1, 1) + tuple(shape))


def checkerboard(shape):
    """(sum of the indices) even: neighbouring lanes diverge."""
    s = torch.zeros(shape, dtype=torch.long)
    for ax, n in enumerate(shape):
        s = s + torch.arange(n).reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return (s % 2 == 0)[None, None]


def single_voxel(shape):
    m = torch.zeros(math.prod(shape), dtype=torch.bool)
    m[(2 * math.prod(shape)) // 3] = True
    return m.reshape((1, 1) + tuple(shape))


def ones(shape):
    return torch.ones((1, 1) + tuple(shape), dtype=torch.bool)


def zeros(shape):
    return torch.zeros((1, 1) + tuple(shape), dtype=torch.bool)


def loop_mask(shape):
    """The mask of the loop tests: the ellipsoid of radius 1.1, which cuts the corners off (1 808 of 2 688 voxels at 12x14x16, 600 of 672 at 24x28).
    The gradient scales with 1 / N_m, and the rates of affine_mi_ref.LOOPS are as high as the unmasked objective allows: under the radius 0.7 .. 1.0
    ellipsoids the SGD rows overshoot (the fp64 loss rises in between), under this one every configuration descends in every iteration."""
    return ellipsoid(shape, 1.1)


MASKS = {"ellipsoid": ellipsoid, "first-chunk-empty": first_chunk_empty, "checkerboard": checkerboard, "single-voxel": single_voxel, "ones": ones,
         "zeros": zeros}


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def select(x, mask, b):
    """The voxels of pair b inside its mask as a [1, N_m] image."""
    return x[b].reshape(-1)[mask[b].reshape(-1) != 0][None]


def joint(target, warped, mask, bins=32, rng=None, dtype=torch.float64):
    """P [B][K][K] over the selected voxels (zeros for an empty mask)."""
    out = []
    for b in range(target.shape[0]):
        t, w = select(target, mask, b), select(warped, mask, b)
        out.append(mi_ref.joint(t, w, bins, rng[b:b + 1], dtype)[0] if t.shape[1] else torch.zeros(bins, bins, dtype=dtype))
    return torch.stack(out)


def loss(target, warped, mask, bins=32, alpha=1.0, normalized=False, rng=None, dtype=torch.float64):
    """[B] losses: mi_ref.loss of the selected voxels; 0 (attached to `warped`, so that autograd returns zeros) for an empty mask."""
    out = []
    for b in range(target.shape[0]):
        t, w = select(target, mask, b), select(warped, mask, b)
        out.append(mi_ref.loss(t, w, bins, alpha, normalized, rng[b:b + 1], dtype)[0] if t.shape[1] else (warped[b].sum() * 0.0).to(dtype))
    return torch.stack(out)


def loss_grad(target, warped, mask, rng, bins=32, alpha=1.0, normalized=False, dtype=torch.float64):
    """(loss [B], d loss / d warped like warped - zero outside the mask) as fp64 tensors; the inputs stay fp32, so the bins are the kernel's."""
    w = warped.clone().requires_grad_()
    ls = loss(target, w, mask, bins, alpha, normalized, rng, dtype)
    (g,) = torch.autograd.grad(ls.sum(), w)
    return ls.detach().double(), g.double()


def weighted_joint(target, warped, mask, bins, rng, dtype=torch.float64):
    """The same table another way: every voxel's weights times its 0 / 1 mask value into the K^2 cells, divided by N_m."""
    B = target.shape[0]
    t, w = target.reshape(B, -1), warped.reshape(B, -1)
    a, c, u, _ = mi_ref.coords(t, w, bins, rng)
    wt = mi_ref.weights((u - c.to(u.dtype)).to(dtype)) * mask.reshape(B, -1, 1).to(dtype)
    cell = (a * bins + c - 1)[:, :, None] + torch.arange(4) + (torch.arange(B) * bins * bins)[:, None, None]
    P = torch.zeros(B * bins * bins, dtype=dtype).index_add(0, cell.reshape(-1), wt.reshape(-1)).reshape(B, bins, bins)
    return P / mask.reshape(B, -1).sum(1).to(dtype)[:, None, None]


def fit_range(target, moving, mask):
    """mi_ref.fit_range with the target's min / max taken inside the mask (a pair with an empty mask: over the whole target)."""
    rng = mi_ref.fit_range(target, moving)
    for b in range(target.shape[0]):
        t = select(target, mask, b)
        if t.shape[1]:
            rng[b, 0], rng[b, 1] = t.min(), t.max()
    return rng


# ---------------------------------------------------------------------------------------------------------------------------------------
# affine_warp in front
# ---------------------------------------------------------------------------------------------------------------------------------------
def evaluate(mov, tgt, theta, rng, mask, bins=32, alpha=1.0, normalized=False, dtype=torch.float64):
    """affine_mi_ref.evaluate on the selected voxels: (loss [B], dtheta [B,nd,nd+1], P [B,K,K]) as fp64 tensors."""
    from oracle import compose
    th = theta.detach().to(dtype).clone().requires_grad_()
    warped = compose.affine_warp(th, mov.to(dtype))
    ls = loss(tgt, warped, mask, bins, alpha, normalized, rng, dtype)
    (g,) = torch.autograd.grad(ls.sum(), th)
    return ls.detach().double(), g.double(), joint(tgt, warped.detach(), mask, bins, rng, dtype).double()


def loop(mov, tgt, rng, mask, mode, optimizer, lr, iters, start, mi, dtype):
    """affine_mi_ref.loop with the selection in front of the criterion: (losses [iters], final parameter)."""
    from oracle import compose
    nd = mov.dim() - 2
    mov = mov.to(dtype)
    p = start.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        theta = compose.pose_to_theta(p) if mode == "rigid" else p.reshape(1, nd, nd + 1)
        e = loss(tgt, compose.affine_warp(theta, mov), mask, rng=rng, dtype=dtype, **mi).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy().copy()


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    """(r64, r32) of one affine_mi_ref.LOOPS configuration under loop_mask, the ranges fitted inside it - computed once per process."""
    shape, mode, optimizer, lr, normalized = aref.LOOPS[name]
    mov, tgt = aref.pair(shape)
    mask = loop_mask(shape)
    rng = fit_range(tgt, mov, mask)
    mi = dict(bins=32, alpha=1.0, normalized=normalized)
    return tuple(loop(mov, tgt, rng, mask, mode, optimizer, lr, aref.ITERS, aref.start_of(shape, mode), mi, dt) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# flow_warp in front: the direct flow (spacing None) and the control lattice
# ---------------------------------------------------------------------------------------------------------------------------------------
def flow_loop(mov, tgt, rng, mask, iters, optimizer, lr, dtype, mi, spacing=None, param0=None, lam=0.0):
    """test_gpu_mi.py's loop arbiter with the selection in front of the criterion: (losses [iters], final parameter)."""
    import bspline_bending_ref as bref
    import bspline_ref
    from oracle import compose
    sp = tuple(mov.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    p = param0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        flow = p if spacing is None else bspline_ref.expand(p, sp, spacing, base=None, dtype=dtype)
        e = loss(tgt, compose.flow_warp(mov, flow), mask, rng=rng, dtype=dtype, **mi).sum()
        if lam:
            e = e + lam * bref.energy_squares(p, sp, spacing, dtype=dtype).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy()


# id -> (shape, spacing (None: direct flow), optimiser, lr, bending weight); rates and starts of tests/test_gpu_mi.py's loops
FLOW_LOOPS = {
    "bspline-3d-bending": ((12, 14, 16), 4, "adam", 0.1, 50.0),
    "bspline-2d-bending": ((24, 28), 5, "adam", 0.1, 50.0),
    "direct-flow": ((12, 14, 16), None, "adam", 0.05, 0.0),
}
FLOW_ITERS = 10


def multimodal(shape):
    """The pair of tests/test_mi_host.py and tests/test_gpu_mi.py: a blob phantom; the phantom warped by a small flow and sent through 4x(1 - x)."""
    import phantoms as ph
    from oracle import compose
    tgt = ph.blobs(shape, 3)
    w = compose.flow_warp(tgt, ph.flow_field(shape, amp=1.2, f=0.013).expand(1, -1, *shape))
    return (4.0 * w * (1.0 - w)).float(), tgt


@functools.lru_cache(maxsize=None)
def flow_loop_pair(name):
    """(mov, tgt, mask, start, r64, r32) of one FLOW_LOOPS configuration under loop_mask, the ranges fitted inside it."""
    import bspline_ref
    import phantoms as ph
    shape, spacing, optimizer, lr, lam = FLOW_LOOPS[name]
    mov, tgt = multimodal(shape)
    mask = loop_mask(shape)
    rng = fit_range(tgt, mov, mask)
    if spacing is None:
        p0 = 0.3 * ph.flow_field(shape, 1.0, 0.05) + 0.17
    else:
        g = torch.Generator().manual_seed(7)
        p0 = (torch.rand((1, len(shape)) + bspline_ref.grid(shape, spacing), generator=g) - 0.5) * 0.4
    kw = dict(mi=dict(bins=32, alpha=1.0, normalized=False), spacing=spacing, param0=p0, lam=lam)
    r64, r32 = (flow_loop(mov, tgt, rng, mask, FLOW_ITERS, optimizer, lr, dt, **kw) for dt in (torch.float64, torch.float32))
    return mov, tgt, mask, p0, r64, r32


# ---------------------------------------------------------------------------------------------------------------------------------------
# what the mask is for: a bright block in the target that the moving image lacks
# ---------------------------------------------------------------------------------------------------------------------------------------
OCC_SHAPE = (24, 28, 32)
OCC_BLOCK = (slice(0, 10), slice(0, 12), slice(0, 14))      # one corner region of the target, 1 680 of 21 504 voxels
OCC_VALUE = 1.5                                             # the phantom stays below 1.2
OCC_LR, OCC_ITERS = 0.01, 120                               # rigid, Adam, from affine_mi_ref.pose0
# The pose the fp64 arbiter reaches on the clean pair (no block, no mask) after 300 iterations of the same optimiser: the pose error is measured
# against it (max |p - OCC_TRUTH| over the six pose parameters).  tests/test_mi_mask_host.py asserts that the arbiter reproduces it.
OCC_TRUTH = (-0.00457271, -0.10267978, -0.00462061, -0.23151682, 0.12153695, -0.07367223)
OCC_MI = dict(bins=32, alpha=1.0, normalized=False)


def occluded_pair():
    """(moving, target with the block, mask excluding the block): affine_mi_ref.pair with OCC_VALUE pasted over OCC_BLOCK of the target."""
    mov, tgt = aref.pair(OCC_SHAPE)
    tgt = tgt.clone()
    mask = torch.ones_like(tgt, dtype=torch.bool)
    tgt[(0, 0) + OCC_BLOCK] = OCC_VALUE
    mask[(0, 0) + OCC_BLOCK] = False
    return mov, tgt, mask


def occluder_clean_pose():
    mov, tgt = aref.pair(OCC_SHAPE)
    return aref.loop(mov, tgt, mi_ref.fit_range(tgt, mov), "rigid", "adam", OCC_LR, 300, aref.pose0(3), OCC_MI, torch.float64)[1]


def pose_error(pose):
    """max |pose - OCC_TRUTH| of a pose [6] (array)."""
    return float(np.max(np.abs(np.asarray(pose, dtype=np.float64).reshape(6) - np.asarray(OCC_TRUTH))))


@functools.lru_cache(maxsize=None)
def occluder_errors(dtype=torch.float64):
    """(masked, unmasked) pose errors of the arbiter after OCC_ITERS iterations on the occluded pair, with and without the mask."""
    mov, tgt, mask = occluded_pair()
    masked = loop(mov, tgt, fit_range(tgt, mov, mask), mask, "rigid", "adam", OCC_LR, OCC_ITERS, aref.pose0(3), OCC_MI, dtype)[1]
    unmasked = aref.loop(mov, tgt, mi_ref.fit_range(tgt, mov), "rigid", "adam", OCC_LR, OCC_ITERS, aref.pose0(3), OCC_MI, dtype)[1]
    return pose_error(masked), pose_error(unmasked)
