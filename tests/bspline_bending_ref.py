"""Restatement of the bending energy of the cubic B-spline free-form deformation (include/trx.h: trx_bspline_bending), written from its
definition on top of tests/bspline_ref.py: dense per-axis derivative matrices M_a^(k) [S_a][G_a], on the CPU, in fp64 (or fp32).  Not a test.

  squares form: E_b = (1/N) sum_c sum_{k: sum k = 2} mult_k sum_voxels (ctrl_{b,c} x_z M_z^(kz) x_y M_y^(ky) x_x M_x^(kx))^2   (differentiable)
  Gram form:    g = dE_b/dctrl_{b,c} = (2/N) sum_k mult_k (R_z^(kz) (x) R_y^(ky) (x) R_x^(kx)) ctrl_{b,c},  R_a^(k) = M_a^(k)^T M_a^(k),
                E_b = 1/2 sum_c <ctrl_{b,c}, g>
mult_k = 2! / (kz! ky! kx!): 1 for zz, yy, xx and 2 for zy, zx, yx (2-D: yy, xx and 2 yx).
"""
import itertools
import math

import torch

import bspline_ref as ref


def deriv_matrix(S, d, k, dtype=torch.float64):
    """M^(k) [S][G]: the k-th derivative with respect to the voxel coordinate; weights formed in fp64 and rounded once to `dtype`."""
    if k == 0:
        return ref.axis_matrix(S, d, dtype)
    G = (S - 1) // d + 4
    M = torch.zeros(S, G, dtype=torch.float64)
    for x in range(S):
        i0, t = x // d, (x % d) / d
        if k == 1:
            w = [-(1 - t) ** 2 / 2, (3 * t ** 2 - 4 * t) / 2, (-3 * t ** 2 + 2 * t + 1) / 2, t ** 2 / 2]
        else:
            w = [1 - t, 3 * t - 2, 1 - 3 * t, t]
        for l in range(4):
            M[x, i0 + l] = w[l] / d ** k
    return M.to(dtype)


def terms(nd):
    """[(k per axis, multiplicity)] of the second derivatives."""
    return [(k, math.factorial(2) // math.prod(math.factorial(v) for v in k)) for k in itertools.product(range(3), repeat=nd) if sum(k) == 2]


def energy_squares(ctrl, spatial, spacing, dtype=torch.float64):
    """E [B] from the definition; differentiable (torch autograd)."""
    nd = len(spatial)
    sp = ref.per_axis(spacing, nd)
    assert tuple(ctrl.shape[2:]) == ref.grid(spatial, sp), (tuple(ctrl.shape), ref.grid(spatial, sp))
    c = ctrl.to(dtype)
    mats = [[deriv_matrix(S, d, k, dtype) for k in range(3)] for S, d in zip(spatial, sp)]
    e = 0.0
    for k, mult in terms(nd):
        dd = ref._contract(c, [mats[a][k[a]] for a in range(nd)])
        e = e + mult * (dd * dd).flatten(1).sum(dim=1)
    return e / math.prod(spatial)


def gram_matrix(S, d, k, dtype=torch.float64):
    """R^(k) = M^(k)^T M^(k) [G][G]: the weights in `dtype`, the products summed in fp64, the result stored in `dtype`."""
    M = deriv_matrix(S, d, k, dtype).double()
    return (M.t() @ M).to(dtype)


def energy_gram(ctrl, spatial, spacing, dtype=torch.float64):
    """(E [B], dE/dctrl [B, nd, *grid]) in the Gram form, all arithmetic in `dtype`."""
    nd = len(spatial)
    sp = ref.per_axis(spacing, nd)
    assert tuple(ctrl.shape[2:]) == ref.grid(spatial, sp), (tuple(ctrl.shape), ref.grid(spatial, sp))
    c = ctrl.to(dtype)
    grams = [[gram_matrix(S, d, k, dtype) for k in range(3)] for S, d in zip(spatial, sp)]
    g = torch.zeros_like(c)
    for k, mult in terms(nd):
        g = g + mult * ref._contract(c, [grams[a][k[a]] for a in range(nd)])
    g = g * (2.0 / math.prod(spatial))
    return 0.5 * (c * g).flatten(1).sum(dim=1), g
