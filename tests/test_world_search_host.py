"""CPU checks of the principal-axes / pose-search initialiser: the restatement tests/world_search_ref.py against numpy and a
closed form, the package's host functions (principal_axes_candidates, rotation_grid, covariance_from_sums) against the restatement, the C ABI's refusals
of trx_image_moments2 without a GPU, the Python refusals, and the conditions the GPU tests rely on (rehearsed here in the fp64 arbiter)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import affine_mi_world_ref as wref
import torchregister_amd as tr
import world_search_ref as sref
from torchregister_amd import _engine as eng


# 1. moments ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all-voxels", "masked"])
@pytest.mark.parametrize("shape", [(5, 6, 7), (9, 11)], ids=str)
def test_restatement_moments_equal_numpy(shape, masked):
    """raw_moments / covariance of the restatement against numpy (np.average and np.cov with weights), and covariance_from_sums - the package's way from
    the kernel's rows to the central moments - against the central sums formed directly."""
    nd = len(shape)
    g = torch.Generator().manual_seed(11)
    x = torch.rand(2, 1, *shape, generator=g) + 0.25
    mask = (torch.rand(2, 1, *shape, generator=g) > 0.3).to(torch.uint8) if masked else None
    off = sref.min_offset(x, mask)
    sums, _ = sref.raw_moments(x, mask, off)
    mass, c, cov = sref.covariance(x, mask)
    assert tuple(sums.shape) == (2, 1 + nd + nd * (nd + 1) // 2)
    idx = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1).reshape(-1, nd)
    for b in range(2):
        w = x[b, 0].double().numpy().reshape(-1) - float(off[b])
        if masked:
            w = w * (mask[b, 0].numpy().reshape(-1) != 0)
        assert abs(sums[b, 0].item() - w.sum()) <= 1e-12 * w.sum() and abs(mass[b].item() - w.sum()) <= 1e-12 * w.sum()
        cn = np.average(idx, axis=0, weights=w)
        Cn = np.cov(idx.T, aweights=w, ddof=0)
        assert np.abs(c[b].numpy() - cn).max() <= 1e-12 and np.abs(cov[b].numpy() - Cn).max() <= 1e-11
        # the rows are in x, y(, z) order = the tensor's axes reversed
        assert np.abs(sums[b, 1:1 + nd].numpy() - (w[:, None] * idx[:, ::-1]).sum(0)).max() <= 1e-10 * np.abs(sums[b, 1:1 + nd].numpy()).max()
        assert abs(sums[b, 1 + nd].item() - (w * idx[:, -1] ** 2).sum()) <= 1e-10 * sums[b, 1 + nd].item()                   # xx
        assert abs(sums[b, 2 + nd].item() - (w * idx[:, -1] * idx[:, -2]).sum()) <= 1e-10 * sums[b, 2 + nd].item()        # xy
    m2, c2, cov2 = eng.covariance_from_sums(sums, nd)
    assert (m2 - mass).abs().max().item() <= 1e-12 * mass.max().item()
    assert (c2 - c).abs().max().item() <= 1e-11 and (cov2 - cov).abs().max().item() <= 1e-10
    with pytest.raises(ValueError):
        eng.covariance_from_sums(torch.zeros_like(sums), nd)


def test_covariance_of_an_anisotropic_gaussian_under_an_oblique_header():
    """A Gaussian exp(-(p - mu)^T S^-1 (p - mu) / 2) with S = Q diag(2^2, 3^2, 4.5^2) Q^T mm^2 sampled at the voxel centres of a 44 x 48 x 52 lattice
    @ 1.2 x 1.0 x 0.9 mm under an oblique, flipped header.  World covariance A C A^T and world centre of the restatement against S and mu.  The bar is
    derived, three terms: (a) point sampling at spacing h aliases a Gaussian of width s by at most 2 (1 + (2 pi s / h)^2) exp(-2 pi^2 s^2 / h^2) relative
    per axis (Poisson summation; taken at the smallest s and the largest h, times nd); (b) the weights are v - min, a pedestal d = min v over N voxels at
    most r^2 from the centre: |dC| <= 2 d N r^2 / mass; (c) the lattice cuts the tails beyond Mahalanobis radius k, k^2 = -2 ln(largest value on the
    lattice's boundary): at most (k^2 + nd + 2)^2 exp(-k^2 / 2) s_max^2."""
    shape, voxel = (44, 48, 52), (1.2, 1.0, 0.9)
    A = wref.header(shape, voxel, wref.rotation(*wref.OBLIQUE), flip=1, centre=(12.0, -7.0, 4.0))
    Q = wref.rotation(0.7, -0.4, 1.1)
    sig = torch.tensor([2.0, 3.0, 4.5], dtype=torch.float64)
    S = Q @ torch.diag(sig ** 2) @ Q.T
    mu = torch.tensor([12.4, -6.7, 3.8], dtype=torch.float64)
    d = sref.lattice_points(shape, A) - mu
    img = torch.exp(-0.5 * torch.einsum("...i,ij,...j->...", d, torch.linalg.inv(S), d))
    c, C = sref.world_moments(img[None, None], A)
    N, nd = math.prod(shape), 3
    inner = torch.zeros(shape, dtype=torch.bool)
    inner[1:-1, 1:-1, 1:-1] = True
    k2 = -2.0 * math.log(img[~inner].max().item())
    a = 2.0 * (1.0 + (2.0 * math.pi * 2.0 / 1.2) ** 2) * math.exp(-2.0 * math.pi ** 2 * 2.0 ** 2 / 1.2 ** 2) * nd * S.abs().max().item()
    b = 2.0 * img.min().item() * N * d.pow(2).sum(-1).max().item() / img.sum().item()
    t = (k2 + nd + 2.0) ** 2 * math.exp(-k2 / 2.0) * sig.max().item() ** 2
    err, cerr = (C - S).abs().max().item(), (c - mu).abs().max().item()
    print(f"covariance err {err:.3e} mm^2, centre err {cerr:.3e} mm; bar {a + b + t:.3e} = aliasing {a:.1e} + pedestal {b:.1e} + tails {t:.1e} (k^2 = {k2:.1f})")
    assert err <= a + b + t and cerr <= math.sqrt(a + b + t)
    w = sref.axes(C)[0]
    assert (w - sig ** 2).abs().max().item() <= 2.0 * (a + b + t)


# 2. candidates -----------------------------------------------------------------------------------------------------------------------------
def _spd(nd, seed):
    g = torch.Generator().manual_seed(seed)
    M = torch.randn(nd, nd, generator=g, dtype=torch.float64)
    return M @ M.T + torch.diag(torch.arange(1, nd + 1, dtype=torch.float64))


@pytest.mark.parametrize("nd", [2, 3])
def test_candidates_are_proper_rotations_about_the_centres_in_the_documented_order(nd):
    """K = 4 / 2, R^T R = I and det R = +1 to 1e-12, T0_k takes c_t to c_m, V_m^T R_k V_t is the k-th sign diagonal of the documented order, and the package
    agrees with the restatement.  T0_k c_t = c_m: the matrix carries t = c_m - R c_t, so T0_k c_t = R c_t + (c_m - R c_t) in floating point - two roundings
    of magnitude |R c_t| + |c_m| at most, not zero: the bar is 4 x 2^-53 (|R| |c_t| + |c_m|) per entry, the fp64 bound of that expression."""
    Cm, Ct = torch.stack([_spd(nd, 1), _spd(nd, 2)]), torch.stack([_spd(nd, 3), _spd(nd, 4)])
    g = torch.Generator().manual_seed(5)
    cm, ct = 30.0 * torch.randn(2, nd, generator=g, dtype=torch.float64), 30.0 * torch.randn(2, nd, generator=g, dtype=torch.float64)
    T0 = tr.principal_axes_candidates(Cm, cm, Ct, ct)
    K = 4 if nd == 3 else 2
    assert tuple(T0.shape) == (2, K, nd + 1, nd + 1) and T0.dtype == torch.float64
    signs = [s for s in __import__("itertools").product((1.0, -1.0), repeat=nd)]
    for b in range(2):
        want = sref.candidates(Cm[b], cm[b], Ct[b], ct[b])
        assert (T0[b] - want).abs().max().item() <= 1e-12 * 30.0
        Vm, Vt = sref.axes(Cm[b])[1], sref.axes(Ct[b])[1]
        proper = [s for s in signs if np.prod(s) * float(torch.linalg.det(Vm) * torch.linalg.det(Vt)) > 0]
        assert len(proper) == K
        for k in range(K):
            R = T0[b, k, :nd, :nd]
            assert (R.T @ R - torch.eye(nd, dtype=torch.float64)).abs().max().item() <= 1e-12 and abs(float(torch.linalg.det(R)) - 1.0) <= 1e-12
            assert T0[b, k, nd].tolist() == [0.0] * nd + [1.0]
            got = R @ ct[b] + T0[b, k, :nd, nd]
            bar = 4.0 * 2.0 ** -53 * (R.abs() @ ct[b].abs() + cm[b].abs())
            assert bool(((got - cm[b]).abs() <= bar).all()), (got - cm[b], bar)
            assert (Vm.T @ R @ Vt - torch.diag(torch.tensor(proper[k], dtype=torch.float64))).abs().max().item() <= 1e-12
    with pytest.raises(ValueError):
        tr.principal_axes_candidates(Cm, cm, Ct[:, :1], ct)


def test_a_relayout_under_a_rotated_header_is_among_the_candidates():
    """A target and the same physical image in another memory layout (affine_mi_world_ref.relayout: an axis flipped, two swapped) whose header is then
    turned by Q about the world origin: the moving image is the target's content rotated by Q, the moments (restated) are exact images of each other,
    and one of the four candidates is p_m = Q p_t to 1e-9."""
    import phantoms as ph
    shape = (12, 14, 16)
    tgt = ph.blobs(shape, 3, nblob=8)
    At = wref.header(shape, (1.5, 1.0, 1.2), wref.rotation(-0.05, 0.04, 0.1), centre=(3.0, -2.0, 1.0))
    Q = sref._homog(sref.axis_angle((0.3, -0.5, 0.8), 130.0))
    mov, Ar = wref.relayout(tgt, At)
    Am = Q @ Ar
    (cm, Cm), (ct, Ct) = sref.world_moments(mov, Am), sref.world_moments(tgt, At)
    w = sref.axes(Ct)[0]
    assert float((w[1:] - w[:-1]).min()) > 1e-3 * float(w.max())          # distinct eigenvalues: the axes are defined
    T0 = tr.principal_axes_candidates(Cm[None], cm[None], Ct[None], ct[None])[0]
    errs = [(T - Q).abs().max().item() for T in T0]
    print("max |T0_k - Q|:", ["%.2e" % e for e in errs])
    assert min(errs) <= 1e-9 and sorted(errs)[1] > 0.1


# 3. the grid ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd,step", [(3, 45), (3, 90), (3, 30), (2, 45), (2, 15)])
def test_rotation_grid(nd, step):
    G = tr.rotation_grid(nd, step)
    n = 360 // step
    assert G.shape[0] == (n * n * (180 // step + 1) if nd == 3 else n) and tuple(G.shape[1:]) == (nd, nd) and G.dtype == torch.float64
    assert torch.equal(G[0], torch.eye(nd, dtype=torch.float64))
    assert (G.transpose(1, 2) @ G - torch.eye(nd, dtype=torch.float64)).abs().max().item() <= 1e-12
    assert (torch.linalg.det(G) - 1.0).abs().max().item() <= 1e-12
    assert (G - sref.euler_grid(nd, float(step))).abs().max().item() <= 1e-12


def test_rotation_grid_refuses_a_step_that_does_not_divide_90():
    for nd, step in ((3, 40), (3, 0), (3, -45), (2, 50), (3, 180), (4, 45), (1, 45), (3, float("nan"))):
        with pytest.raises(ValueError):
            tr.rotation_grid(nd, step)


# 4. the C ABI without a GPU --------------------------------------------------------------------------------------------------------------------
def test_image_moments2_refusals_without_a_gpu():
    """trx_image_moments2 and its workspace query reject bad arguments before any HIP call, as trx_image_moments does."""
    from torchregister_amd import _lib
    lib = _lib.load()
    assert "trx_image_moments2" in _lib.SIGNATURES and "trx_image_moments2_workspace_bytes" in _lib.SIGNATURES
    P = ctypes.c_void_p
    q = lib.trx_image_moments2_workspace_bytes
    for bad in ((1, 1, 1, 8, 8), (4, 1, 8, 8, 8), (2, 1, 2, 8, 8), (3, 1, 0, 8, 8), (3, 1, 8, 0, 8), (3, 1, 8, 8, 0), (3, 0, 8, 8, 8), (3, 65536, 8, 8, 8),
                (3, 1, 2048, 1024, 1024)):
        assert q(*bad) == 0, bad
    assert q(3, 1, 5, 6, 7) == 10 * 8 and q(3, 2, 26, 26, 25) == 2 * 2 * 10 * 8 and q(2, 3, 1, 130, 127) == 3 * 2 * 10 * 8
    assert q(3, 65535, 2, 2, 2) == 65535 * 10 * 8
    n = q(3, 1, 8, 8, 8)
    f = lambda x, o, w, nd, N, d, h, ww, k: lib.trx_image_moments2(x, None, None, nd, N, d, h, ww, o, w, k, None)  # noqa: E731
    assert f(None, P(16), P(16), 3, 1, 8, 8, 8, n) == -1 and f(P(16), None, P(16), 3, 1, 8, 8, 8, n) == -1 and f(P(16), P(16), None, 3, 1, 8, 8, 8, n) == -1
    assert f(P(16), P(16), P(16), 1, 1, 1, 8, 8, n) == -2 and f(P(16), P(16), P(16), 4, 1, 8, 8, 8, n) == -2 and f(P(16), P(16), P(16), 2, 1, 2, 8, 8, n) == -2
    for d, h, w in ((0, 8, 8), (8, 0, 8), (8, 8, 0)):
        assert f(P(16), P(16), P(16), 3, 1, d, h, w, n) == -1
    assert f(P(16), P(16), P(16), 3, 0, 8, 8, 8, n) == -1 and f(P(16), P(16), P(16), 3, 65536, 8, 8, 8, 1 << 40) == -1
    assert f(P(16), P(16), P(16), 3, 1, 8, 8, 8, n - 1) == -3
    assert f(P(16), P(16), P(16), 3, 2, 8, 8, 8, n) == -3          # two volumes need twice the rows


# 5. Python refusals ---------------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    ts, ms = (5, 6, 7), (9, 7, 6)
    Am, At = wref.oblique_pair(ts, ms)
    mov, tgt = torch.zeros(1, 1, *ms), torch.zeros(1, 1, *ts)
    mi = lambda mode="rigid", loop=True: tr.Register(mode, criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=loop)  # noqa: E731
    assert eng.WORLD_INITS == (None, "centers", "moments", "principal_axes", "search")
    # 'principal' stays an unknown string; the new strings need the headers; world_search= needs one of the new strings and known keys
    for kw in (dict(moving_affine=Am, target_affine=At, world_init="principal"), dict(world_init="principal_axes"), dict(world_init="search"),
               dict(moving_affine=Am, world_init="search"), dict(moving_affine=Am, target_affine=At, world_init="moments", world_search=dict(step=45)),
               dict(moving_affine=Am, target_affine=At, world_search=dict(step=45)), dict(world_search=dict(step=45)),
               dict(moving_affine=Am, target_affine=At, world_init="search", world_search=dict(stride=45)),
               dict(moving_affine=Am, target_affine=At, world_init="search", world_search=45)):
        with pytest.raises(ValueError):
            mi().optim(mov, tgt, lr=0.01, max_epochs=1, **kw)
        with pytest.raises(ValueError):
            tr.AffineMISolver(mov, tgt, mode="rigid", **kw)
        with pytest.raises(ValueError):
            tr.rigid_register(mov, tgt, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, device_loop=True, debug=False, **kw)
    # the support rule is WORLD_SUPPORT's
    for init in ("principal_axes", "search"):
        ok = dict(moving_affine=Am, target_affine=At, world_init=init)
        for reg in (mi(loop=False), tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline"), tr.Register("affine"), tr.Register("flow")):
            with pytest.raises(ValueError, match="world"):
                reg.optim(mov, tgt, lr=0.01, max_epochs=1, **ok)
        with pytest.raises(ValueError, match="world"):
            tr.affine_register(mov, tgt, criterions=[tr.NCCLoss()], weights=[1.0], grad_edges=False, debug=False, **ok)
    with pytest.raises(ValueError):
        tr.world_geometry(ms, ts, Am, At, init="principal_axes")        # needs the images: world_setup / optim
    for name in ("WorldSearch", "image_covariance", "principal_axes_candidates", "rotation_grid", "world_search"):
        assert hasattr(tr, name)


# 6. what the GPU tests rely on, rehearsed in the arbiter ---------------------------------------------------------------------------------------
def test_rehearsal_of_the_gpu_pair():
    """The 3-D pair of tests/test_gpu_world_search.py in fp64: one principal-axes candidate lies within 5 degrees of the truth and the others beyond 170; its
    score is the lowest by a wide margin; after 20 iterations of refinement the best and second-best losses differ by more than 100 x the arbiter's own
    fp32-fp64 gap (the condition of the choice test); 60 iterations of the rigid loop from the refined start end within 0.2 degrees of the truth, while the
    same loop from the centre-of-mass alignment ('moments') stays beyond 90 degrees.  Measured here: candidates 179.6 / 179.6 / 177.6 / 2.5 degrees, scores
    0.422 / 0.518 / 0.513 / 0.181 (truth 0.132), refined 0.1325 against 0.3756 with a gap of 1.1e-6, the main run ends 0.073 degrees from the truth, the
    'moments' run 118.9 degrees."""
    import affine_mi_grids_ref as gref
    mov, tgt, Am, At, T = sref.pair3()
    ms, ts = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    (cm, Cm), (ct, Ct) = sref.world_moments(mov, Am), sref.world_moments(tgt, At)
    T0s = sref.candidates(Cm, cm, Ct, ct)
    angles = sorted(sref.rotation_error(T0, T) for T0 in T0s)
    assert angles[0] <= 5.0 and angles[1] >= 170.0
    r64, r32 = (sref.search(mov, tgt, Am, At, T0s, ct, 4, 20, dt) for dt in (torch.float64, torch.float32))
    s = torch.sort(r64[2]).values
    gap = (r64[2] - r32[2]).abs().max().item()
    print(f"scores {r64[0].tolist()}, refined {r64[2].tolist()}, margin {(s[1] - s[0]).item():.4f} against 100 x gap {100 * gap:.2e}")
    assert r64[3] == r32[3] == int(torch.argmin(r64[0])) and sref.rotation_error(T0s[r64[3]], T) <= 5.0
    assert (s[1] - s[0]).item() > 100.0 * gap
    rng = sref.fit_range(tgt, mov)
    ends = {}
    for name, T0 in (("principal_axes", r64[4]), ("moments", wref.translation(cm - ct))):
        _, pose = sref.refine(mov, tgt, wref.record(ms, ts, Am, At, T0, ct), rng, 60)
        ends[name] = sref.rotation_error(wref.world_matrix(gref.pose_to_theta(pose.double())[0], wref.geometry(ms, ts, Am, At, T0, ct)), T)
    print("rotation distance to the truth after 60 iterations:", ends)
    assert ends["principal_axes"] <= 0.2 and ends["moments"] > 90.0
