"""Restatement of the cubic B-spline free-form deformation of include/trx.h (trx_bspline_*), written from its definition: per-axis dense
matrices M_a [S_a][G_a] and tensor contractions with them, on the CPU, in fp64 (or fp32 on request).  Not a test.

Per axis of S voxels with spacing d: G = (S - 1) // d + 4 control points, point i at voxel (i - 1) d; at voxel x, i0 = x // d,
t = (x % d) / d, and row x of M holds B0(t), B1(t), B2(t), B3(t) in columns i0 .. i0 + 3.
  expand: flow_c = base_c + ctrl_c x_z M_z x_y M_y x_x M_x        reduce: dctrl_c = dflow_c x_z M_z^T x_y M_y^T x_x M_x^T
"""
import torch


def grid(spatial, spacing):
    return tuple((int(s) - 1) // int(d) + 4 for s, d in zip(spatial, per_axis(spacing, len(spatial))))


def per_axis(spacing, nd):
    return (int(spacing),) * nd if isinstance(spacing, int) else tuple(int(d) for d in spacing)


def axis_matrix(S, d, dtype=torch.float64):
    """M [S][G]: the weights are formed in fp64 and rounded once to `dtype`."""
    G = (S - 1) // d + 4
    M = torch.zeros(S, G, dtype=torch.float64)
    for x in range(S):
        i0, t = x // d, (x % d) / d
        M[x, i0 + 0] = (1 - t) ** 3 / 6
        M[x, i0 + 1] = (3 * t ** 3 - 6 * t ** 2 + 4) / 6
        M[x, i0 + 2] = (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6
        M[x, i0 + 3] = t ** 3 / 6
    return M.to(dtype)


def _contract(x, mats):
    """x [B, C, *n] times one matrix [m_a][n_a] per spatial axis -> [B, C, *m]."""
    for a, M in enumerate(mats):
        x = torch.movedim(torch.tensordot(x, M, dims=([2 + a], [1])), -1, 2 + a)
    return x


def expand(ctrl, spatial, spacing, base=None, dtype=torch.float64):
    """ctrl [B, nd, *grid] -> flow [B, nd, *spatial] (+ base); differentiable (torch autograd)."""
    nd = len(spatial)
    sp = per_axis(spacing, nd)
    assert tuple(ctrl.shape[2:]) == grid(spatial, sp), (tuple(ctrl.shape), grid(spatial, sp))
    flow = _contract(ctrl.to(dtype), [axis_matrix(S, d, dtype) for S, d in zip(spatial, sp)])
    return flow if base is None else flow + base.to(dtype)


def reduce(dflow, spacing, dtype=torch.float64):
    """dflow [B, nd, *spatial] -> dctrl [B, nd, *grid]: the transposes of expand's matrices."""
    spatial = tuple(dflow.shape[2:])
    sp = per_axis(spacing, len(spatial))
    return _contract(dflow.to(dtype), [axis_matrix(S, d, dtype).t() for S, d in zip(spatial, sp)])
