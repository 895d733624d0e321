"""The fp64 restatement of the principal-axes / pose-search initialiser: raw and central second moments by plain torch sums, the
candidate construction, the Euler grid, the scoring through tests/affine_mi_world_ref.py::evaluate (tests/mi_overlap_ref.py::evaluate under a moving mask)
and the refinement through affine_mi_world_ref.loop.  Plus the pair of the GPU tests: the rehearsal scene of the issue - phantoms.blobs((32,32,32), 3, 8)
as a function of the target's lattice - seen through a second, oblique and flipped header after a rigid world motion of 130 degrees and a non-monotone
intensity map.  Nothing here touches the GPU or the package's own functions.  Not a test."""
import functools
import itertools
import math

import numpy as np
import torch

import affine_mi_world_ref as wref
import mi_mask_ref as mref
import mi_overlap_ref as oref
import mi_ref


# ---------------------------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------------------------
def _index_columns(shape):
    """[nvox, ncol - 1] fp64: per voxel x, y(, z) and the products xx, xy, yy(, xz, yz, zz) - the kernel's column order - x the index along the LAST axis."""
    nd = len(shape)
    idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij"), dim=-1).reshape(-1, nd).flip(1)
    cols = [idx[:, a] for a in range(nd)]
    for j in range(nd):
        for i in range(j + 1):
            cols.append(idx[:, i] * idx[:, j])
    return torch.stack(cols, dim=1)


def raw_moments(x, mask=None, offset=None):
    """(sums [B, ncol], sums of |term| [B, ncol]) fp64 of x [B,1,*shape]: trx_image_moments2's definition by plain sums.  offset [B] (None = 0)."""
    B, shape = x.shape[0], tuple(x.shape[2:])
    cols = torch.cat([torch.ones(math.prod(shape), 1, dtype=torch.float64), _index_columns(shape)], dim=1)
    v = x.double().reshape(B, -1)
    w = v if offset is None else v - offset.double().reshape(B, 1)
    if mask is not None:
        w = torch.where(mask.reshape(B, -1) != 0, w, torch.zeros_like(w))
    terms = w[:, :, None] * cols[None]
    return terms.sum(1), terms.abs().sum(1)


def check_raw_moments(got, first_order, want, mag, nvox, worst=None):
    """What trx_image_moments2's rows are held to, shared by tests/test_gpu_world_search.py (the fixed shapes) and tests/fuzz_ops.py (the random ones): the
    messages of what does not hold.  got [B, ncol] fp64 against raw_moments' (want, mag): finite, and per column within nvox 2^-52 sum |term| - the
    worst-case error of an fp64 sum of nvox terms in any order; first_order [B, 1 + nd], trx_image_moments' rows of the same input: got's first columns,
    bit for bit.  worst: a dict whose 'raw sums' receives the largest error / bar."""
    msgs = []
    err, limit = (got - want).abs(), nvox * 2.0 ** -52 * mag
    ok = err <= limit
    if worst is not None:
        ratio = torch.where(err == 0, torch.zeros_like(err), err / limit).max().item()
        worst["raw sums"] = max(worst.get("raw sums", 0.0), ratio)
    if not bool(torch.isfinite(got).all()):
        msgs.append("a raw sum is not finite")
    if not bool(ok.all()):
        b, c = (int(v) for v in torch.nonzero(~ok)[0])
        msgs.append(f"raw sums: volume {b} column {c} err {err[b, c]:.3e} bar {limit[b, c]:.3e}")
    if not torch.equal(got[:, :first_order.shape[1]], first_order):
        msgs.append("the order-1 columns are not trx_image_moments' bits")
    return msgs


def min_offset(x, mask=None):
    """[B] fp32: the minimum over the counted voxels, the offset image_covariance hands to the kernel."""
    B = x.shape[0]
    v = x.float().reshape(B, -1)
    if mask is not None:
        v = torch.where(mask.reshape(B, -1) != 0, v, torch.full_like(v, float("inf")))
    return v.amin(1)


def covariance(x, mask=None):
    """(mass [B], centre [B,nd], cov [B,nd,nd]) fp64 in the TENSOR's axis order, weights v - min over the counted voxels: central sums, formed directly."""
    B, shape = x.shape[0], tuple(x.shape[2:])
    nd = len(shape)
    idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij"), dim=-1).reshape(-1, nd)
    w = x.double().reshape(B, -1) - min_offset(x, mask).double()[:, None]
    if mask is not None:
        w = torch.where(mask.reshape(B, -1) != 0, w, torch.zeros_like(w))
    mass = w.sum(1)
    c = (w[:, :, None] * idx[None]).sum(1) / mass[:, None]
    d = idx[None] - c[:, None, :]
    cov = (w[:, :, None, None] * d[:, :, :, None] * d[:, :, None, :]).sum(1) / mass[:, None, None]
    return mass, c, cov


def world_moments(x, A, mask=None):
    """(centre [nd], cov [nd,nd]) of x [1,1,*shape] in world mm under the header A."""
    nd = x.dim() - 2
    _, c, C = covariance(x, mask)
    lin = A[:nd, :nd]
    return lin @ c[0] + A[:nd, nd], lin @ C[0] @ lin.T


# ---------------------------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------------------------
def axes(C):
    """(eigenvalues ascending, eigenvectors in columns) by numpy, every eigenvector's sign such that its first entry of largest magnitude is positive."""
    w, V = np.linalg.eigh(C.numpy())
    for k in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, k])), k] < 0:
            V[:, k] = -V[:, k]
    return torch.from_numpy(w), torch.from_numpy(V)


def about(R, ct, cm):
    """[nd+1,nd+1]: p_m = R (p_t - c_t) + c_m."""
    nd = R.shape[0]
    T = torch.eye(nd + 1, dtype=torch.float64)
    T[:nd, :nd], T[:nd, nd] = R, cm - R @ ct
    return T


def candidates(Cm, cm, Ct, ct):
    """[K,nd+1,nd+1]: the documented order - sign diagonals as itertools.product((1, -1), repeat=nd), those with det R = -1 left out."""
    nd = Cm.shape[0]
    Vm, Vt = axes(Cm)[1], axes(Ct)[1]
    out = []
    for s in itertools.product((1.0, -1.0), repeat=nd):
        R = Vm @ torch.diag(torch.tensor(s, dtype=torch.float64)) @ Vt.T
        if torch.linalg.det(R) > 0:
            out.append(about(R, ct, cm))
    return torch.stack(out)


def euler_grid(nd, step):
    """[C,nd,nd]: the identity, then Rz(g) Ry(b) Rx(a) over a, b, g (a slowest) without the identity; 2-D: the angle alone."""
    full, half = np.arange(-180.0, 180.0, step), np.arange(-90.0, 90.0 + step / 2, step)
    if nd == 2:
        rest = [wref.rot2(math.radians(g)) for g in full if g != 0.0]
    else:
        rest = [wref.rotation(math.radians(a), math.radians(b), math.radians(g)) for a in full for b in half for g in full if (a, b, g) != (0.0, 0.0, 0.0)]
    return torch.stack([torch.eye(nd, dtype=torch.float64)] + rest)


def angle_between(Ra, Rb):
    """Rotation distance in degrees between two rotation matrices (any nd)."""
    nd = Ra.shape[0]
    t = float(torch.trace(Ra.T @ Rb))
    c = (t - 1.0) / 2.0 if nd == 3 else t / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))


# ---------------------------------------------------------------------------------------------------------------------------------------
# scoring, refinement, choice
# ---------------------------------------------------------------------------------------------------------------------------------------
def identity_theta(nd, dtype=torch.float64):
    return torch.eye(nd, nd + 1, dtype=dtype)[None]


def fit_range(tgt, mov, mask=None, mmask=None):
    if mmask is not None:
        return oref.fit_range(tgt, mov, mask, mmask)
    return mi_ref.fit_range(tgt, mov) if mask is None else mref.fit_range(tgt, mov, mask)


def score(mov, tgt, rec, rng, mask=None, mmask=None, dtype=torch.float64, bins=32):
    """The loss at theta = identity under one record [1,32]; with a moving mask the overlap rule of mi_overlap_ref at the effective theta."""
    nd = mov.dim() - 2
    if mmask is None:
        return wref.evaluate(mov, tgt, identity_theta(nd), rec, rng, bins, 1.0, False, dtype, mask)[0][0].item()
    te = wref.theta_eff(identity_theta(nd), rec)
    return oref.evaluate(mov, tgt, te, wref.ONES(nd), rng, mask, mmask, bins, 1.0, False, dtype)[0][0].item()


def score_is_border_stable(mov, tgt, rec, mask, mmask):
    nd = mov.dim() - 2
    te = wref.theta_eff(identity_theta(nd), rec)
    i = oref.affine_coords(te, wref.ONES(nd), mov.shape[2:], tgt.shape[2:])
    return oref.border_stable(i, mov.shape[2:], mask, mmask)


def records(mshape, tshape, Am, At, T0s, c):
    return [wref.record(mshape, tshape, Am, At, T0, c) for T0 in T0s]


def refine(mov, tgt, rec, rng, iters, lr=0.01, dtype=torch.float64, mask=None):
    """(best loss, pose at the best loss) of the rigid Adam loop from pose 0 under one record: the loss of iteration i is taken at the pose before its step."""
    nd = mov.dim() - 2
    p = torch.zeros(6 if nd == 3 else 3, dtype=dtype, requires_grad=True)
    opt = torch.optim.Adam([p], lr)
    best, best_p = float("inf"), None
    import affine_mi_grids_ref as gref
    for _ in range(iters):
        opt.zero_grad()
        theta = gref.pose_to_theta(p)
        warped = gref.warp(wref.theta_eff(theta.reshape(1, nd, nd + 1), rec), wref.ONES(nd), mov, tgt.shape[2:])
        e = (mi_ref.loss(tgt, warped, rng=rng, dtype=dtype, bins=32, alpha=1.0, normalized=False) if mask is None else
             mref.loss(tgt, warped, mask, rng=rng, dtype=dtype, bins=32, alpha=1.0, normalized=False)).sum()
        if e.item() < best:
            best, best_p = e.item(), p.detach().clone()
        e.backward()
        opt.step()
    return best, best_p


def search(mov, tgt, Am, At, T0s, c, keep, iters, dtype=torch.float64, mask=None):
    """The restated world_search over given candidates: (scores [K], kept, refined [keep], chosen, T of the chosen one [nd+1,nd+1])."""
    mshape, tshape = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    rng = fit_range(tgt, mov, mask)
    recs = records(mshape, tshape, Am, At, T0s, c)
    scores = torch.tensor([score(mov, tgt, r, rng, mask, None, dtype) for r in recs])
    kept = torch.sort(scores, stable=True).indices[:keep]
    if iters == 0:
        return scores, kept, scores[kept], int(kept[0]), T0s[int(kept[0])]
    runs = [refine(mov, tgt, recs[int(k)], rng, iters, 0.01, dtype, mask) for k in kept]
    refined = torch.tensor([r[0] for r in runs])
    j = int(torch.sort(refined, stable=True).indices[0])
    import affine_mi_grids_ref as gref
    k = int(kept[j])
    theta = gref.pose_to_theta(runs[j][1].double())[0]
    T = wref.world_matrix(theta, wref.geometry(mshape, tshape, Am, At, T0s[k], c))
    return scores, kept, refined, k, T


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pair of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------------
def axis_angle(axis, deg):
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    K = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    t = math.radians(deg)
    return torch.eye(3, dtype=torch.float64) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def scene(u, seed=3, nblob=8):
    """phantoms.blobs as a function: u [..., d] positions in the cube [-1, 1]^d in the TENSOR's axis order -> the sum of the same Gaussians (same draws)."""
    g = torch.Generator().manual_seed(int(seed))
    d = u.shape[-1]
    img = torch.zeros(u.shape[:-1], dtype=torch.float64)
    for _ in range(nblob):
        c = torch.rand(d, generator=g) - 0.5
        sig = 0.05 + 0.2 * torch.rand(1, generator=g)
        a = torch.rand(1, generator=g)
        r2 = sum((u[..., k] - float(c[k])) ** 2 for k in range(d))
        img += float(a) * torch.exp(-r2 / (2 * float(sig) ** 2))
    return img


def lattice_points(shape, A):
    nd = len(shape)
    idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij"), dim=-1)
    return idx @ A[:nd, :nd].T + A[:nd, nd]


def modality(s):
    """The non-monotone intensity map of the rehearsal: 4 s (1 - s) + 0.3 s on s clamped to [0, 1]."""
    s = s.clamp(0.0, 1.0)
    return 4.0 * s * (1.0 - s) + 0.3 * s


TSHAPE3, MSHAPE3 = (32, 32, 32), (24, 28, 32)
TVOXEL3, MVOXEL3 = (1.0, 1.0, 1.0), (1.7, 1.4, 1.2)
TRUE_AXIS, TRUE_DEG, TRUE_SHIFT = (0.3, -0.5, 0.8), 130.0, (1.6, -1.0, 0.6)        # mm: 0.10, -0.06, 0.04 of the target's 16 mm half extent
TSHAPE2, MSHAPE2 = (40, 48), (44, 40)
TVOXEL2, MVOXEL2 = (1.0, 1.0), (1.2, 1.1)
TRUE_DEG2, TRUE_SHIFT2 = 150.0, (1.5, -1.0)


@functools.lru_cache(maxsize=None)
def pair3():
    """(moving [1,1,24,28,32], target [1,1,32,32,32], A_m, A_t, T_true): the target is the scene on its own lattice - 1 mm voxels under
    affine_mi_world_ref.world_headers()'s target header (slightly rotated, centred on WORLD_T_CENTRE); T_true turns by 130 degrees about (0.3, -0.5, 0.8)
    through the target's centre and shifts; the moving lattice lies under world_headers()'s oblique header with tensor axis 1 flipped, centred
    WORLD_M_OFFSET off the image of the target's centre, and moving(q) = modality(scene(T_true^-1 q))."""
    At = wref.header(TSHAPE3, TVOXEL3, wref.rotation(-0.05, 0.04, 0.1), centre=wref.WORLD_T_CENTRE)
    c = torch.tensor(wref.WORLD_T_CENTRE, dtype=torch.float64)
    R = axis_angle(TRUE_AXIS, TRUE_DEG)
    T = wref.translation(c + torch.tensor(TRUE_SHIFT, dtype=torch.float64)) @ _homog(R) @ wref.translation(-c)
    cm = (T @ torch.cat([c, torch.ones(1, dtype=torch.float64)]))[:3] + torch.tensor(wref.WORLD_M_OFFSET, dtype=torch.float64)
    Am = wref.header(MSHAPE3, MVOXEL3, wref.rotation(*wref.OBLIQUE), flip=1, centre=cm)
    return _images(TSHAPE3, MSHAPE3, Am, At, T) + (Am, At, T)


@functools.lru_cache(maxsize=None)
def pair2():
    """The 2-D pair: the scene (seed 3, 8 blobs, 2-D) on 40 x 48, turned by 150 degrees about the target's centre onto a flipped, oblique 44 x 40 lattice."""
    At = wref.header(TSHAPE2, TVOXEL2, wref.rot2(-0.06), centre=(20.5, -14.0))
    c = torch.tensor((20.5, -14.0), dtype=torch.float64)
    T = wref.translation(c + torch.tensor(TRUE_SHIFT2, dtype=torch.float64)) @ _homog(wref.rot2(math.radians(TRUE_DEG2))) @ wref.translation(-c)
    cm = (T @ torch.cat([c, torch.ones(1, dtype=torch.float64)]))[:2] + torch.tensor((0.5, -0.75), dtype=torch.float64)
    Am = wref.header(MSHAPE2, MVOXEL2, wref.rot2(0.3), flip=1, centre=cm)
    return _images(TSHAPE2, MSHAPE2, Am, At, T) + (Am, At, T)


def _homog(R):
    nd = R.shape[0]
    H = torch.eye(nd + 1, dtype=torch.float64)
    H[:nd, :nd] = R
    return H


def _images(tshape, mshape, Am, At, T):
    nd = len(tshape)
    size = torch.tensor([s - 1.0 for s in tshape], dtype=torch.float64)

    def in_cube(p):       # world -> the target's voxel index (tensor order) -> blobs' cube, linspace(-1, 1, S) along every axis
        Ai = torch.linalg.inv(At)
        return 2.0 * (p @ Ai[:nd, :nd].T + Ai[:nd, nd]) / size - 1.0
    tgt = scene(in_cube(lattice_points(tshape, At)))
    Ti = torch.linalg.inv(T)
    mov = modality(scene(in_cube(lattice_points(mshape, Am) @ Ti[:nd, :nd].T + Ti[:nd, nd])))
    return mov.float()[None, None], tgt.float()[None, None]


def rotation_error(T, T_true):
    """Degrees between the rotation parts of two rigid world transforms."""
    nd = T.shape[0] - 1
    return angle_between(T[:nd, :nd].double(), T_true[:nd, :nd].double())
