"""The definition of the nearest-neighbour and cubic B-spline resampling (trx_spline_coefficients, trx_transform_resample) in
torch, on the CPU, in fp64 - or in fp32 through `dtype`, the yardstick of what the number format costs.

Coefficients: those of the interpolating cubic B-spline with whole-sample mirror boundaries (index i outside 0 .. n-1 reflects about 0 and n-1, period
2 (n-1)), per axis of n > 1 voxels by the recursive filter with z = sqrt(3) - 2:
  c+[0] = (s[0] + z^(n-1) s[n-1] + sum_{k=1..n-2} (z^k + z^(2n-2-k)) s[k]) / (1 - z^(2n-2)),   c+[k] = s[k] + z c+[k-1],
  c-[n-1] = z / (z^2 - 1) (c+[n-1] + z c+[n-2]),   c-[k] = z (c-[k+1] - c+[k]),   c = 6 c-;      an axis of one voxel is left alone.
Cubic sample at voxel position p: per axis i0 = floor(p), r = p - i0, taps i0 - 1 .. i0 + 2 mirrored, weights ((1-r)^3, 3r^3 - 6r^2 + 4,
-3r^3 + 3r^2 + 3r + 1, r^3) / 6, the tensor-product sum; 0 where p_a < -0.5 or p_a > S_a - 0.5 on some axis.  Nearest sample: rint (half to even)
per axis, 0 where the rounded index lies outside.  Positions: theta None: p = x + flow(x) on x's own lattice; else the composed warp's closed form
of tests/affine_flow_ref.py (a missing flow is zero).  Nothing here touches the GPU; tests/test_spline_host.py asserts the conditions the GPU tests
rely on.  Not a test."""
import functools
import itertools
import math

import torch

import affine_flow_ref as fr
import affine_mi_grids_ref as gref
import phantoms as ph

Z = math.sqrt(3.0) - 2.0


def mirror(i, n):
    """Whole-sample mirror of a long tensor of indices into 0 .. n-1."""
    if n == 1:
        return torch.zeros_like(i)
    p = 2 * (n - 1)
    i = torch.remainder(i, p)
    return torch.where(i >= n, p - i, i)


def coefficients(x, dtype=torch.float64):
    """x [B,C,*spatial] -> the coefficients, the same shape, every operation in `dtype`."""
    x = x.to(dtype)
    for ax in range(2, x.dim()):
        n = x.shape[ax]
        if n == 1:
            continue
        s = x.movedim(ax, 0)
        cp = [None] * n
        acc = s[0] + Z ** (n - 1) * s[n - 1]
        for k in range(1, n - 1):
            acc = acc + (Z ** k + Z ** (2 * n - 2 - k)) * s[k]
        cp[0] = acc / (1.0 - Z ** (2 * n - 2))
        for k in range(1, n):
            cp[k] = s[k] + Z * cp[k - 1]
        cm = [None] * n
        cm[n - 1] = Z / (Z * Z - 1.0) * (cp[n - 1] + Z * cp[n - 2])
        for k in range(n - 2, -1, -1):
            cm[k] = Z * (cm[k + 1] - cp[k])
        x = (6.0 * torch.stack(cm)).movedim(0, ax)
    return x


def coefficients_fir(x, reach=16, dtype=torch.float64):
    """The form the kernels evaluate: c[k] = sum_{|j| <= reach} sqrt(3) z^|j| s[mirror(k - j)] per axis."""
    x = x.to(dtype)
    j = torch.arange(-reach, reach + 1)
    h = (math.sqrt(3.0) * torch.tensor(Z, dtype=torch.float64) ** j.abs()).to(dtype)
    for ax in range(2, x.dim()):
        n = x.shape[ax]
        if n == 1:
            continue
        idx = mirror(torch.arange(n)[:, None] - j[None, :], n)                 # [n, 2 reach + 1]
        x = (x.movedim(ax, -1)[..., idx] * h).sum(-1).movedim(-1, ax)
    return x


def positions(x_shape, theta=None, flow=None, scale=None, size=None, dtype=torch.float64):
    """The sample positions [B, *S_t, nd] (x, y(, z) last) in voxels of the sampled image of spatial shape x_shape, every operation in `dtype`."""
    nd = len(x_shape)
    if theta is None:
        idx = torch.meshgrid(*[torch.arange(s, dtype=dtype) for s in flow.shape[2:]], indexing="ij")
        return torch.stack([idx[c] + flow[:, c].to(dtype) for c in range(nd)][::-1], dim=-1)
    if flow is None:
        flow = torch.zeros((theta.shape[0], nd) + tuple(x_shape if size is None else size))
    m = fr.composed_grid(fr.effective(theta.to(dtype), scale), flow.to(dtype))
    return ((m + 1.0) * torch.tensor(tuple(x_shape)[::-1], dtype=dtype) - 1.0) / 2.0


def weights(r):
    return torch.stack([(1 - r) ** 3, 3 * r ** 3 - 6 * r ** 2 + 4, -3 * r ** 3 + 3 * r ** 2 + 3 * r + 1, r ** 3], -1) / 6


def outside(pos, x_shape):
    """[B, *S_t] bool: the position leaves the field of view, p_a < -0.5 or p_a > S_a - 0.5 on some axis."""
    S = torch.tensor(tuple(x_shape)[::-1], dtype=pos.dtype)
    return ((pos < -0.5) | (pos > S - 0.5)).any(-1)


def _gather(x, lin):
    B, C = x.shape[:2]
    return torch.gather(x.reshape(B, C, -1), 2, lin.reshape(B, 1, -1).expand(-1, C, -1)).reshape((B, C) + tuple(lin.shape[1:]))


def sample_cubic(coef, pos, dtype=torch.float64):
    """coef [B,C,*S_m], pos [B,*S_t,nd] -> [B,C,*S_t] in `dtype`."""
    coef, pos = coef.to(dtype), pos.to(dtype)
    Sm = tuple(coef.shape[2:])
    nd = len(Sm)
    i0 = torch.floor(pos)
    w = weights(pos - i0)                                                       # [B,*S_t,nd,4]
    i0 = i0.long()
    out = torch.zeros((coef.shape[0], coef.shape[1]) + tuple(pos.shape[1:-1]), dtype=dtype)
    for off in itertools.product(range(4), repeat=nd):                          # offsets along x, y(, z)
        ww = torch.ones(pos.shape[:-1], dtype=dtype)
        lin = torch.zeros(pos.shape[:-1], dtype=torch.long)
        for r in reversed(range(nd)):                                           # z, y, x: the tensor's axis nd - 1 - r
            S = Sm[nd - 1 - r]
            lin = lin * S + mirror(i0[..., r] - 1 + off[r], S)
            ww = ww * w[..., r, off[r]]
        out = out + ww[:, None] * _gather(coef, lin)
    return torch.where(outside(pos, Sm)[:, None], torch.zeros_like(out), out)


def sample_nearest(x, pos):
    """x [B,C,*S_m], pos [B,*S_t,nd] -> [B,C,*S_t]: x at rint(pos) (half to even), 0 where a rounded index lies outside."""
    Sm = tuple(x.shape[2:])
    nd = len(Sm)
    r = torch.round(pos).long()
    ok = torch.ones(pos.shape[:-1], dtype=torch.bool)
    lin = torch.zeros(pos.shape[:-1], dtype=torch.long)
    for a in reversed(range(nd)):
        S = Sm[nd - 1 - a]
        ok &= (r[..., a] >= 0) & (r[..., a] < S)
        lin = lin * S + r[..., a].clamp(0, S - 1)
    return _gather(x, lin) * ok[:, None].to(x.dtype)


def kept(pos, x_shape, nearest=False, eps=1e-4):
    """[B, *S_t] bool: the voxels of the comparisons - the fp64 position is farther than eps from every face of the field of view (fp32 may land on
    the other side) and, for nearest, from every rounding tie (p - 0.5 an integer: a face is one of them)."""
    S = torch.tensor(tuple(x_shape)[::-1], dtype=pos.dtype)
    if nearest:
        h = pos - 0.5
        return ((h - torch.round(h)).abs() > eps).all(-1)
    return (((pos + 0.5).abs() > eps) & ((pos - (S - 0.5)).abs() > eps)).all(-1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the coefficient cases: B = 2, C = 2 (N = 4 volumes) of white noise in [0, 1) - the hardest input of the filter, |c| up to 6.4 x the range
# ---------------------------------------------------------------------------------------------------------------------------------------
COEF_SHAPES = {
    "2x3x33": (2, 3, 33),        # axes shorter than the filter's reach, W below a wave
    "7x9x11": (7, 9, 11),        # odd
    "5x13": (5, 13),             # 2-D
    "6x8": (6, 8),
    "12x14x70": (12, 14, 70),    # more than one tile per line, more than one block per volume, W no multiple of a tile
    "1x6x8": (1, 6, 8),          # an axis of one voxel inside a 3-D call
    "40x41x6": (40, 41, 6),      # y and z long enough for runs that reach no end of their line (the unmirrored loads), next to runs that do
}


@functools.lru_cache(maxsize=None)
def volume(shape, seed=3):
    """[2,2,*shape] fp32, uniform in [0, 1)."""
    return torch.rand((2, 2) + tuple(shape), generator=torch.Generator().manual_seed(seed + sum(shape)))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the resample cases, one per position chain: B = 2 with a map per pair, 2 channels.  Each transform is chosen so that between 5 % and 50 % of
# the target voxels sample outside the field of view and at most 1 % lie within 1e-4 of a face or a rounding tie (tests/test_spline_host.py).
# name -> (target shape, moving shape, has theta, flow amplitude in voxels or None, world scale, zoom of the map, seed)
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = {
    "flow": ((7, 9, 11), (7, 9, 11), False, 1.6, False, 1.0, 1),
    "flow-2x3x33": ((2, 3, 33), (2, 3, 33), False, 0.6, False, 1.0, 2),
    "flow-1x6x8": ((1, 6, 8), (1, 6, 8), False, 0.52, False, 1.0, 3),
    "theta": ((12, 14, 70), (12, 14, 70), True, None, False, 1.0, 4),
    "grids-world": ((10, 12, 14), (20, 18, 16), True, None, True, 1.0, 5),
    "composed": ((9, 11, 13), (12, 7, 15), True, 1.2, False, 0.9, 6),
    "2d": ((6, 8), (5, 13), True, 0.8, False, 0.9, 7),
    "2d-flow": ((5, 13), (5, 13), False, 1.0, False, 1.0, 8),
}


def case_scale(name):
    """The scale [nd,nd+1] fp64 of a case, or None where theta is the effective one."""
    tshape, mshape, _, _, world, _, _ = CASES[name]
    if not world:
        return None
    return gref.scale_of(mshape, tshape, *((gref.VOXEL_M3, gref.VOXEL_T3) if len(tshape) == 3 else (gref.VOXEL_M2, gref.VOXEL_T2)))


@functools.lru_cache(maxsize=None)
def case(name):
    """(x [2,2,*S_m] fp32, theta [2,nd,nd+1] fp32 or None - the UNSCALED theta -, flow [2,nd,*S_t] fp32 or None) of a CASES row."""
    tshape, mshape, has_theta, amp, _, zoom, seed = CASES[name]
    nd = len(tshape)
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.cat([ph.blobs(mshape, 10 * seed + 2 * b + c) for c in range(2)], dim=1) for b in range(2)]) + 0.3 * torch.rand((2, 2) + mshape, generator=g)
    theta = None
    if has_theta:
        base = torch.tensor(ph.THETA_ROT3 if nd == 3 else ph.THETA_STAR2, dtype=torch.float64)
        scale = case_scale(name)
        rows = []
        for b in range(2):
            te = base.clone()
            te[:, :nd] = te[:, :nd] * (zoom + 0.08 * b) + 0.06 * (torch.rand(nd, nd, generator=g, dtype=torch.float64) - 0.5)
            te[:, nd] = 0.12 * (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) + (0.06 if b else -0.06)
            rows.append(te if scale is None else te / scale)
        theta = torch.stack(rows).float()
    flow = None
    if amp is not None:
        lin = [torch.linspace(-1, 1, s, dtype=torch.float64) if s > 1 else torch.zeros(1, dtype=torch.float64) for s in tshape]
        axes = torch.meshgrid(*lin, indexing="ij")
        flow = torch.stack([torch.stack([amp * (1.0 + 0.25 * b) * torch.sin((1.3 + 0.4 * c) * axes[(c + 1) % nd] + 2.0 * axes[(c + 2) % nd] * (nd == 3) + 0.3 * c + b)
                                         for c in range(nd)]) for b in range(2)])
        flow = (flow + 0.13 * (torch.rand(flow.shape, generator=g, dtype=torch.float64) - 0.5)).float()
    return x.float(), theta, flow


def case_positions(name, dtype=torch.float64):
    x, theta, flow = case(name)
    return positions(x.shape[2:], theta, flow, case_scale(name), size=CASES[name][0], dtype=dtype)


def labels(shape, seed=11):
    """[2,2,*shape] fp32: an integer label map of values 0 .. 7."""
    return torch.randint(0, 8, (2, 2) + tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# what it is for: an analytic 24 x 28 x 32 volume (frequencies 0.15 .. 0.4 rad / voxel) resampled through a 0.3 rad rotation about x plus a sub-voxel
# shift, against the analytic value on the interior voxels
# ---------------------------------------------------------------------------------------------------------------------------------------
ANALYTIC_SHAPE = (24, 28, 32)
ANALYTIC_ANGLE, ANALYTIC_SHIFT = 0.3, (0.37, -0.21, 0.45)          # radians; voxels along z, y, x


def analytic_fn(z, y, x):
    return torch.sin(0.35 * x + 0.2 * y) * torch.cos(0.3 * y - 0.25 * z) + 0.5 * torch.sin(0.4 * z + 0.15 * x)


@functools.lru_cache(maxsize=None)
def analytic():
    """(image [1,1,*S] fp32, flow [1,3,*S] fp32, analytic value at x + flow(x) [*S] fp64 - at the fp32 flow's own positions -, interior [*S] bool:
    positions 2 .. S - 3 on every axis)."""
    S = ANALYTIC_SHAPE
    g = torch.stack(torch.meshgrid(*[torch.arange(n, dtype=torch.float64) for n in S], indexing="ij"))
    c = (torch.tensor(S, dtype=torch.float64) - 1) / 2
    a = ANALYTIC_ANGLE
    R = torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]], dtype=torch.float64)
    p = (R @ (g.reshape(3, -1) - c[:, None]) + c[:, None] + torch.tensor(ANALYTIC_SHIFT, dtype=torch.float64)[:, None]).reshape(3, *S)
    flow = (p - g).float()[None]
    p = g + flow[0].double()                                          # where the fp32 flow actually points
    interior = torch.stack([(p[k] >= 2) & (p[k] <= S[k] - 3) for k in range(3)]).all(0)
    return analytic_fn(*g).float()[None, None], flow, analytic_fn(*p), interior


def rms(d, keep):
    return d[keep].pow(2).mean().sqrt().item()
