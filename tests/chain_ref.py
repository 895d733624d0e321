"""CPU restatement of csrc/chain.hip (include/trx.h: trx_transform_points, trx_affine_then_flow_resample) in torch, in a dtype of
the caller's choice, and the cases of tests/test_chain_host.py and tests/test_gpu_chain.py.

Points [B,P,nd] and flows [B,nd,*S] are in voxels, component a along spatial axis a (z, y, x / y, x); theta [B,nd,nd+1] is an effective theta between
normalised cubes, rows and columns x, y(, z).  norm_a(p)_c = (2 p_c + 1) / S_a,c - 1, unnorm_b(m)_r = ((m_r + 1) S_b,r - 1) / 2.  S(f, p): Sb (border)
is tests/flowops_ref.py::sample_border's rule at a free position, S0 (zeros) tests/svf_ref.py::sample's (tests/test_chain_host.py holds this file's
sampler against both).
  chain 0 (flow on S_a):  p' = p + S(flow, p);  out = unnorm_b(theta (norm_a(p'), 1));  theta None: out = p'
  chain 1 (flow on S_b):  q = unnorm_b(theta (norm_a(p), 1)), theta None: q = p;  out = q + S(flow, q), flow None: out = q
A non-finite point gives NaN in every component.  The image operator: chain 1's positions of the output lattice's voxels fed to
spline_ref.sample_nearest / sample_cubic and, for order 1, to F.grid_sample(bilinear, zeros, align_corners=False) on the positions normalised with
the source sizes; a NaN position is sent to -2 first (every corner outside: 0), which is what the kernel's clamp into [-2, S + 1] does.  Not a test."""
import functools
import itertools

import torch
import torch.nn.functional as F

import phantoms as ph
import spline_ref as sr
import svf_ref


def sample_at(f, p, padding="border"):
    """S(f, p): f [B,C,*S], p [B,P,nd] (tensor axis order) in f's dtype -> [B,P,C].  The weight of a corner is (y-factor * x-factor) * z-factor and the
    corners are added z, y, x with x fastest, as in the kernels."""
    assert padding in ("border", "zeros")
    B, C = f.shape[:2]
    S = tuple(f.shape[2:])
    nd = len(S)
    idx, fac, oks = [], [], []
    for a, n in enumerate(S):
        pa = p[..., a]
        if padding == "border":
            pc = torch.where(torch.isnan(pa), torch.zeros_like(pa), pa).clamp(0, n - 1)
            i0 = torch.floor(pc).clamp(max=max(n - 2, 0))
            t = pc - i0
            i0 = i0.long()
            idx.append((i0, (i0 + 1).clamp(max=n - 1)))
            oks.append((torch.ones_like(i0, dtype=torch.bool),) * 2)
        else:
            near = (pa > -2) & (pa < n + 1)
            pc = torch.where(near, pa, torch.full_like(pa, -2.0))
            fl = torch.floor(pc)
            t = pc - fl
            i0 = fl.long()
            idx.append((i0.clamp(0, n - 1), (i0 + 1).clamp(0, n - 1)))
            oks.append(((i0 >= 0) & (i0 < n), (i0 + 1 >= 0) & (i0 + 1 < n)))
        fac.append((1 - t, t))
    flat = f.reshape(B, C, -1)
    acc = torch.zeros((B, C, p.shape[1]), dtype=f.dtype)
    for kappa in itertools.product((0, 1), repeat=nd):
        lin = torch.zeros_like(idx[0][0])
        ok = torch.ones_like(lin, dtype=torch.bool)
        for a, k in enumerate(kappa):
            lin = lin * S[a] + idx[a][k]
            ok &= oks[a][k]
        w = fac[nd - 2][kappa[nd - 2]] * fac[nd - 1][kappa[nd - 1]]
        if nd == 3:
            w = w * fac[0][kappa[0]]
        v = torch.gather(flat, 2, lin[:, None].expand(-1, C, -1)) * ok[:, None].to(f.dtype)
        acc = acc + w[:, None] * v
    return acc.transpose(1, 2)


def affine_points(theta, p, Sa, Sb):
    """unnorm_b(theta (norm_a(p), 1)) for p [B,P,nd] in tensor axis order -> the same order."""
    nd = p.shape[-1]
    n = [(2.0 * p[..., c] + 1.0) / Sa[c] - 1.0 for c in range(nd)]
    hom = torch.stack(n[::-1] + [torch.ones_like(n[0])], dim=-1)                               # (n_x, n_y(, n_z), 1)
    m = torch.einsum("bpk,brk->bpr", hom, theta.to(p.dtype).expand(p.shape[0], nd, nd + 1))    # x, y(, z)
    return torch.stack([((m[..., nd - 1 - c] + 1.0) * Sb[c] - 1.0) / 2.0 for c in range(nd)], dim=-1)


def chain(points, theta, flow, from_shape, to_shape, which, padding="border", dtype=torch.float64):
    """The image of points [B,P,nd] under chain `which` (0 / 1) from lattice from_shape to lattice to_shape, every operation in `dtype`."""
    p = points.to(dtype)
    bad = ~torch.isfinite(p).all(-1, keepdim=True)
    p = torch.where(bad, torch.zeros_like(p), p)
    th = None if theta is None else theta.to(dtype)
    fl = None if flow is None else flow.to(dtype).expand(p.shape[0], *flow.shape[1:])
    if which == 0:
        if fl is not None:
            p = p + sample_at(fl, p, padding)
        if th is not None:
            p = affine_points(th, p, from_shape, to_shape)
    else:
        if th is not None:
            p = affine_points(th, p, from_shape, to_shape)
        if fl is not None:
            p = p + sample_at(fl, p, padding)
    return torch.where(bad, torch.full_like(p, float("nan")), p)


def lattice_points(shape, B=1, dtype=torch.float64):
    """[B, prod(shape), nd]: the voxel indices of a lattice in memory order."""
    g = svf_ref.identity(shape, dtype)[0].reshape(len(shape), -1).T
    return g[None].expand(B, -1, -1).contiguous()


def image_positions(theta, flow, out_shape, src_shape, padding="border", dtype=torch.float64):
    """[B, *out_shape, nd] (x, y(, z) last, spline_ref's order): chain 1's position of every output voxel in the source lattice."""
    B = (theta if theta is not None else flow).shape[0]
    pos = chain(lattice_points(out_shape, B, dtype), theta, flow, out_shape, src_shape, 1, padding, dtype)
    return pos.flip(-1).reshape((B,) + tuple(out_shape) + (len(out_shape),))


def resample(x, theta, flow, out_shape, order, padding="border", dtype=torch.float64):
    """[B,C,*out_shape]: x [B,C,*src_shape] sampled at image_positions by order 0, 1 or 3 (3: the fp64 / fp32 coefficients are made here)."""
    src_shape = tuple(x.shape[2:])
    pos = image_positions(theta, flow, out_shape, src_shape, padding, dtype)
    if order == 0:
        return sr.sample_nearest(x.to(dtype), pos)
    if order == 3:
        return sr.sample_cubic(sr.coefficients(x, dtype), pos, dtype)
    pos = torch.where(torch.isnan(pos), torch.full_like(pos, -2.0), pos)
    S = torch.tensor(src_shape[::-1], dtype=dtype)
    return F.grid_sample(x.to(dtype), (2.0 * pos + 1.0) / S - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False)


def check_image(got, r64, r32, pos, src_shape, order, value_range, figures=None):
    """What an image through the chain is held to, shared by tests/test_gpu_chain.py (the fixed cases) and tests/fuzz_ops.py (the random ones):
    (messages of what does not hold, the number of kept voxels outside the field of view).  got [B,C,*out] fp32 on the CPU against the restatement's
    r64 / r32 at the fp64 positions pos [B,*out,nd].  Orders 1 and 3: within max(1e-5 x value_range, twice the restatement's own fp32 - fp64 gap) on the
    kept voxels (spline_ref.kept); order 0: no kept voxel differs; voxels outside the field of view (orders 0, 3: beyond half a voxel; order 1: beyond a
    whole voxel, where the last corner has left) are exactly 0.  figures: a dict that receives image_err, image_bar, image_fp32_gap."""
    msgs = []
    keep1 = sr.kept(pos, src_shape, nearest=order == 0)
    keep = keep1[:, None].expand_as(got)
    if order == 0:
        bad = int((got[keep].double() != r64[keep]).sum())
        if figures is not None:
            figures.update(nearest_unequal=bad)
        if bad:
            msgs.append(f"image order 0: {bad} kept voxels differ")
        outside = sr.outside(pos, src_shape)
    else:
        some = bool(keep1.any())
        gap = (r32.double() - r64)[keep].abs().max().item() if some else 0.0
        err, limit = (got.double() - r64)[keep].abs().max().item() if some else 0.0, max(1e-5 * value_range, 2.0 * gap) if some else 0.0
        if figures is not None:
            figures.update(image_err=err, image_bar=limit, image_fp32_gap=gap)
        if not err <= limit:
            msgs.append(f"image order {order}: err {err:.3e} bar {limit:.3e}")
        S = torch.tensor(tuple(src_shape)[::-1], dtype=torch.float64)
        outside = sr.outside(pos, src_shape) if order == 3 else ((pos < -1.0 - 1e-4) | (pos > S + 1e-4)).any(-1)
    outside = (outside & keep1)[:, None].expand_as(got)
    if bool(got[outside].any()):
        msgs.append(f"image order {order}: {int((got[outside] != 0).sum())} voxels outside the field of view are not 0")
    return msgs, int(outside.sum())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: B = 2 with a theta per pair, 2 channels.  name -> (output lattice S_a, source lattice S_b, has theta, flow amplitude in voxels or
# None, seed).  The flow lives on S_b.  tests/test_chain_host.py asserts that spline_ref.kept removes at most 1 % of the voxels of every case.
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = {
    "9x11x13": ((9, 11, 13), (12, 10, 7), True, 1.2, 1),          # odd sizes, W below one wave, unequal lattices
    "20x18x16": ((20, 18, 16), (10, 12, 14), True, 1.0, 2),       # more than one block per pair
    "2d": ((17, 19), (14, 23), True, 1.0, 3),
    "1x12x20": ((1, 12, 20), (1, 9, 15), True, 0.8, 4),           # an axis of one voxel
    "flow-only": ((7, 9, 11), (7, 9, 11), False, 1.4, 5),         # theta None: equal lattices
    "theta-only": ((9, 11, 13), (12, 10, 7), True, None, 6),      # flow None
}


def smooth_flow(shape, amp, g, B=2):
    """[B,nd,*shape] fp32: waves of amplitude amp with a jitter of 0.13 voxel (off the voxel lattice); channel 0 of a lattice one voxel deep is zero."""
    nd = len(shape)
    lin = [torch.linspace(-1, 1, s, dtype=torch.float64) if s > 1 else torch.zeros(1, dtype=torch.float64) for s in shape]
    axes = torch.meshgrid(*lin, indexing="ij")
    flow = torch.stack([torch.stack([amp * (1.0 + 0.25 * b) * torch.sin((1.3 + 0.4 * c) * axes[(c + 1) % nd] + 2.0 * axes[(c + 2) % nd] * (nd == 3) + 0.3 * c + b)
                                     for c in range(nd)]) for b in range(B)])
    flow = flow + 0.13 * (torch.rand(flow.shape, generator=g, dtype=torch.float64) - 0.5)
    for c, s in enumerate(shape):
        if s == 1:
            flow[:, c] = 0.0
    return flow.float()


def thetas(nd, g, flat=False, B=2):
    """[B,nd,nd+1] fp32: rotation-like maps with generic entries, a zoom and a shift per pair, so that part of the output leaves the source's field of
    view.  flat: the z row and column are those of the identity (a lattice one voxel deep)."""
    base = torch.tensor(ph.THETA_ROT3 if nd == 3 else ph.THETA_STAR2, dtype=torch.float64)
    rows = []
    for b in range(B):
        te = base.clone()
        te[:, :nd] = te[:, :nd] * (0.95 + 0.08 * b) + 0.06 * (torch.rand(nd, nd, generator=g, dtype=torch.float64) - 0.5)
        te[:, nd] = 0.12 * (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) + (0.06 if b else -0.06)
        if flat:
            te[2] = torch.tensor([0.0, 0.0, 1.0, 0.0], dtype=torch.float64)
            te[:2, 2] = 0.0
        rows.append(te)
    return torch.stack(rows).float()


@functools.lru_cache(maxsize=None)
def case(name):
    """(x [2,2,*S_b] fp32, theta [2,nd,nd+1] fp32 or None, flow [2,nd,*S_b] fp32 or None) of a CASES row."""
    out_shape, src_shape, has_theta, amp, seed = CASES[name]
    nd = len(out_shape)
    g = torch.Generator().manual_seed(40 + seed)
    x = torch.cat([torch.cat([ph.blobs(src_shape, 10 * seed + 2 * b + c) for c in range(2)], dim=1) for b in range(2)]) + 0.3 * torch.rand((2, 2) + src_shape, generator=g)
    theta = thetas(nd, g, flat=out_shape[0] == 1 and nd == 3) if has_theta else None
    flow = None if amp is None else smooth_flow(src_shape, amp, g)
    return x.float(), theta, flow


@functools.lru_cache(maxsize=None)
def reference(name, order, padding="border"):
    """(fp64, fp32) restatement of a case's image, computed once and shared (never modified)."""
    x, theta, flow = case(name)
    return tuple(resample(x, theta, flow, CASES[name][0], order, padding, dt) for dt in (torch.float64, torch.float32))


def labels(shape, seed=11):
    """[2,2,*shape] fp32: an integer label map of values 1 .. 7 (0 is what the padding gives)."""
    return torch.randint(1, 8, (2, 2) + tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


POINT_COUNTS = (1, 63, 65, 1000)


def points_for(shape, P, seed, B=2, nan_at=None):
    """[B,P,nd] fp32: uniform from 4 voxels outside the lattice to 4 voxels outside; the first points of a large enough set lie on faces and corners,
    and point nan_at of pair 0 (if given and P > nan_at) has a NaN component."""
    nd = len(shape)
    g = torch.Generator().manual_seed(seed)
    S = torch.tensor(shape, dtype=torch.float32)
    p = torch.rand((B, P, nd), generator=g) * (S + 7.0) - 4.0
    if P >= 8:
        p[:, 0] = 0.0
        p[:, 1] = S - 1.0
        p[:, 2] = -0.5
        p[:, 3] = S - 0.5
        p[:, 4, 0] = 0.0
        p[:, 5, nd - 1] = S[nd - 1] - 1.0
    if nan_at is not None and P > nan_at:
        p[0, nan_at, nd - 1] = float("nan")
    return p
