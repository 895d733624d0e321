"""CPU restatement of the stationary-velocity-field operators of csrc/svf.hip (include/trx.h: trx_svf_exp, trx_svf_exp_backward) in torch, any
dtype: a voxel-space sampler of its own (so that an axis of one voxel is defined), exp by scaling and squaring - differentiable, so torch
autograd through it is one form of the adjoint -, the adjoint written out (the splat as an index_add_), a central-difference Jacobian
determinant, and the fields the tests use."""
import itertools
import math

import numpy as np
import torch


def identity(spatial, dtype=torch.float64):
    """[1, nd, *spatial]: channel a holds the voxel index along axis a."""
    return torch.stack(torch.meshgrid(*[torch.arange(s, dtype=dtype) for s in spatial], indexing="ij"))[None]


def _corners(u):
    """For p = x + u(x) (ONE add in u's dtype): per corner kappa (a tuple of 0 / 1 per axis) the flat index of i0 + kappa clamped into the
    volume [B, n], whether it lies inside [B, n], and the per-axis factors (1 - t or t) [B, nd, n] with their derivatives (-1 or +1)."""
    B, nd = u.shape[:2]
    spatial = u.shape[2:]
    p = (identity(spatial, u.dtype) + u).reshape(B, nd, -1)
    i0 = torch.floor(p)
    t = p - i0
    i0 = i0.detach().clamp(-4, max(spatial) + 4).long()
    out = []
    for kappa in itertools.product((0, 1), repeat=nd):
        lin = torch.zeros_like(i0[:, 0])
        ok = torch.ones_like(i0[:, 0], dtype=torch.bool)
        fac = []
        for a, k in enumerate(kappa):
            idx = i0[:, a] + k
            ok &= (idx >= 0) & (idx < spatial[a])
            lin = lin * spatial[a] + idx.clamp(0, spatial[a] - 1)
            fac.append(t[:, a] if k else 1 - t[:, a])
        out.append((kappa, lin, ok, fac))
    return out


def sample(f, u):
    """S(f, x + u(x)) for every voxel x: bi / trilinear, corners outside the volume contribute zero.  f, u: [B, nd, *spatial]."""
    B, nd = u.shape[:2]
    flat = f.reshape(B, f.shape[1], -1)
    acc = torch.zeros_like(flat)
    for _, lin, ok, fac in _corners(u):
        w = math.prod(fac[1:], start=fac[0]) * ok.to(u.dtype)
        acc = acc + w[:, None] * torch.gather(flat, 2, lin[:, None].expand(-1, flat.shape[1], -1))
    return acc.reshape(f.shape)


def levels(v, squarings, inverse=False):
    """[u_0, ..., u_K]: u_0 = +-2^-K v, u_{k+1} = u_k + S(u_k, x + u_k)."""
    us = [v * ((-1.0 if inverse else 1.0) / 2 ** squarings)]
    for _ in range(squarings):
        us.append(us[-1] + sample(us[-1], us[-1]))
    return us


def exp(v, squarings, inverse=False, dtype=torch.float64):
    """flow = u_K.  Differentiable: autograd through it is the adjoint's first form."""
    return levels(v.to(dtype), squarings, inverse)[-1]


def square_backward(u, g):
    """The adjoint of u -> u + S(u, x + u) at u, applied to g, written out: g + the splat of g + the derivative of the sample with respect
    to its position over the in-bounds corners."""
    B, nd = u.shape[:2]
    uf, gf = u.reshape(B, nd, -1), g.reshape(B, nd, -1)
    splat = torch.zeros_like(gf)
    dpos = torch.zeros_like(gf)
    for kappa, lin, ok, fac in _corners(u):
        okf = ok.to(u.dtype)
        w = math.prod(fac[1:], start=fac[0]) * okf
        for b in range(B):
            splat[b].index_add_(1, lin[b], w[b][None] * gf[b])
        s = (gf * torch.gather(uf, 2, lin[:, None].expand(-1, nd, -1))).sum(1) * okf          # sum_a g_a(y) u_a(corner)
        for c in range(nd):
            dw = math.prod([fac[a] for a in range(nd) if a != c], start=torch.ones_like(s)) * (1.0 if kappa[c] else -1.0)
            dpos[:, c] += dw * s
    return (gf + splat + dpos).reshape(u.shape)


def exp_backward(v, dflow, squarings, inverse=False, dtype=torch.float64):
    """dL/dv for flow = exp(v): the explicit adjoint, level by level."""
    with torch.no_grad():
        us = levels(v.to(dtype), squarings, inverse)
        g = dflow.to(dtype)
        for k in range(squarings - 1, -1, -1):
            g = square_backward(us[k], g)
        return g * ((-1.0 if inverse else 1.0) / 2 ** squarings)


def exp_backward_autograd(v, dflow, squarings, inverse=False, dtype=torch.float64):
    """The same through torch autograd."""
    v = v.to(dtype).clone().requires_grad_()
    (exp(v, squarings, inverse, dtype) * dflow.to(dtype)).sum().backward()
    return v.grad


def jacobian_det(flow):
    """det d(id + flow)/dx by central differences on the interior (every axis loses its first and last voxel): [B, *(spatial - 2)]."""
    nd = flow.shape[1]
    J = torch.zeros(flow.shape[:1] + tuple(s - 2 for s in flow.shape[2:]) + (nd, nd), dtype=flow.dtype)
    for j in range(nd):
        hi = tuple(slice(2, None) if a == j else slice(1, -1) for a in range(nd))
        lo = tuple(slice(None, -2) if a == j else slice(1, -1) for a in range(nd))
        for i in range(nd):
            J[..., i, j] = 0.5 * (flow[(slice(None), i) + hi] - flow[(slice(None), i) + lo]) + (1.0 if i == j else 0.0)
    return torch.linalg.det(J)


def share_outside(flow):
    """Fraction of voxels x whose x + flow(x) lies outside [0, S - 1] on some axis."""
    spatial = flow.shape[2:]
    p = identity(spatial, flow.dtype) + flow
    out = torch.zeros_like(p[:, 0], dtype=torch.bool)
    for a, s in enumerate(spatial):
        out |= (p[:, a] < 0) | (p[:, a] > s - 1)
    return out.double().mean().item()


def smooth_field(B, spatial, amplitude, seed, noise=0.05):
    """fp32 [B, nd, *spatial]: per channel four low-frequency cosines with random phases, scaled so that their amplitudes sum to `amplitude`,
    plus uniform noise in [-noise, noise].  (Pure noise is no test field: each squaring amplifies rounding by the field's Lipschitz constant.)"""
    rng = np.random.RandomState(seed)
    nd = len(spatial)
    ax = np.meshgrid(*[np.arange(s, dtype=np.float64) / max(s - 1, 1) for s in spatial], indexing="ij")
    out = np.zeros((B, nd) + tuple(spatial))
    for b in range(B):
        for c in range(nd):
            amps = rng.uniform(0.5, 1.0, 4)
            for j in range(4):
                freq, phase = rng.choice([0.0, 0.5, 1.0, 1.5], nd), rng.uniform(0, 2 * np.pi)
                out[b, c] += amps[j] / amps.sum() * amplitude * np.cos(2 * np.pi * sum(f * x for f, x in zip(freq, ax)) + phase)
    out += rng.uniform(-noise, noise, out.shape)
    return torch.from_numpy(out).float()


def fold_field(spatial):
    """fp64 [1, nd, *spatial], closed form: env = prod_a sin^2(pi x_a / (S_a - 1)); last channel -2.5 (S - 1) / (2 pi) sin(2 pi x / (S - 1)) env
    along the last axis, first channel 0.5 env, the others zero.  id + v folds; exp(v) does not."""
    nd = len(spatial)
    ax = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) / (s - 1) for s in spatial], indexing="ij")
    env = math.prod([torch.sin(math.pi * x) ** 2 for x in ax][1:], start=torch.sin(math.pi * ax[0]) ** 2)
    v = torch.zeros((1, nd) + tuple(spatial), dtype=torch.float64)
    S = spatial[-1]
    v[0, nd - 1] = -2.5 * (S - 1) / (2 * math.pi) * torch.sin(2 * math.pi * ax[-1]) * env
    v[0, 0] = v[0, 0] + 0.5 * env
    return v


# (B, spatial, squarings, amplitude) of the operator tests; the last but one is checked for the operators only (an axis of one voxel)
CASES = [(1, (13, 18, 23), 6, 3.0), (2, (9, 10, 11), 4, 6.0), (1, (19, 26), 6, 4.0), (3, (8, 8, 8), 1, 1.5), (1, (6, 7, 8), 10, 2.0), (1, (5, 6, 7), 0, 1.0),
         (1, (1, 12, 20), 3, 2.0), (1, (9, 10, 11), 12, 1.0)]

SEEDS = {(c, inv): 1 for c in range(len(CASES)) for inv in (False, True)}
SEEDS.update({(7, False): 2, (7, True): 5})
# share of voxels that exp(v) maps outside the volume, at least (asserted on the CPU for both signs): the out-of-bounds corners are exercised
MIN_OUTSIDE = {0: 0.15, 1: 0.35, 4: 0.31}


def case_inputs(case, inverse, seed=None):
    """(velocity, dflow) of a case, fp32: dflow is a smooth field plus noise 0.5.  The seed is the first for which the adjoint in fp32 and in
    fp64 agree everywhere to 1e-5 max|dvel| (SEEDS; tests/test_svf_host.py asserts that): the gradient of a trilinear sample jumps where a
    sampling position crosses a lattice plane, so at other seeds single elements can differ by far more between ANY two precisions."""
    B, spatial, K, amp = CASES[case]
    seed = SEEDS[(case, bool(inverse))] if seed is None else seed
    return smooth_field(B, spatial, amp, 100 * case + seed), smooth_field(B, spatial, 1.0, 5000 + 100 * case + seed, noise=0.5)


_DIRECTIONS = {}


def directions(case, inverse, n=8, eps=1e-4, amplitude=0.01, candidates=32):
    """n smooth directions d for the directional identity <dvel, d> = <dflow, (exp(v + eps d) - exp(v - eps d)) / (2 eps)> of a case, each
    with the right-hand side in fp64: [(d, rhs)].  exp is piecewise smooth - a sampling position that crosses a lattice plane between
    v - eps d and v + eps d puts a kink inside the difference quotient, and the quotient is then wrong by far more than its O(eps^2) - so
    the directions are small (max |eps d| = 1e-6) and a candidate (seeds 9000, 9001, ...) is kept only if the restatement's own fp64
    adjoint, which equals autograd to 1e-14, meets the identity to 1e-6 relative: the quotient is then clean."""
    key = (case, bool(inverse), n, eps, amplitude)
    if key not in _DIRECTIONS:
        v, g = case_inputs(case, inverse)
        _DIRECTIONS[key] = directions_for(v, g, CASES[case][2], inverse, n, eps, amplitude, candidates)
    return _DIRECTIONS[key]


def directions_for(v, g, K, inverse, n=8, eps=1e-4, amplitude=0.01, candidates=32, b64=None):
    """directions() for any velocity v and dflow g: the first n of the candidates (seeds 9000, 9001, ...) that the fp64 adjoint b64 (made here when it
    is not given) meets the identity on to 1e-6 relative."""
    B, spatial = v.shape[0], tuple(v.shape[2:])
    v64, g64 = v.double(), g.double()
    b64 = exp_backward(v, g, K, inverse) if b64 is None else b64
    kept = []
    for j in range(candidates):
        d = amplitude * smooth_field(B, spatial, 1.0, 9000 + j, noise=0.0).double()
        rhs = (g64 * (exp(v64 + eps * d, K, inverse) - exp(v64 - eps * d, K, inverse)) / (2 * eps)).sum().item()
        lhs = (b64 * d).sum().item()
        if abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)):
            kept.append((d, rhs))
        if len(kept) == n:
            break
    return kept
