"""Host checks (no GPU) of world-geometry registration: the package's world_geometry / converters / world_setup against the
restatement tests/affine_mi_world_ref.py and against hand arithmetic, the refusals, and the rehearsal in the fp64 arbiter of what the GPU tests of
tests/test_gpu_affine_mi_world.py rely on."""
import math

import numpy as np
import pytest
import torch

import affine_mi_grids_ref as gref
import affine_mi_world_ref as wref

import torchregister_amd as tr
from torchregister_amd import _engine as eng


# 1 ---------------------------------------------------------------------------------------------------------------------------------------
ALIGNED = [((20, 18, 16), (1.2, 0.9, 0.8), (10, 12, 14), (3.0, 1.0, 1.0)), ((21, 15), (0.9, 1.3), (13, 17), (2.0, 1.0))]


@pytest.mark.parametrize("ms,mv,ts,tv", ALIGNED, ids=["3d", "2d"])
def test_aligned_headers_are_the_voxel_size_scale(ms, mv, ts, tv):
    """Diagonal headers, centres at 0, T0 = I: theta_eff = theta (.) grid_scale within 1e-12 and l = the half extents."""
    nd = len(ts)
    geo = tr.world_geometry(ms, ts, wref.header(ms, mv), wref.header(ts, tv))
    rec, c = geo
    assert tuple(rec.shape) == (1, 32) and rec.dtype == torch.float64 and c.abs().max().item() <= 1e-12
    assert torch.allclose(geo.extent[0], eng._half_extents(ms, mv, "moving_voxel"), rtol=0, atol=1e-12)
    g = torch.Generator().manual_seed(3)
    theta = torch.randn(4, nd, nd + 1, generator=g, dtype=torch.float64)
    te = wref.theta_eff(theta, rec.expand(4, 32))
    want = theta * tr.grid_scale(ms, ts, mv, tv)
    err = (te - want).abs().max().item()
    print(f"{ts} from {ms}: |theta_eff - theta * scale| {err:.1e}")
    assert err <= 1e-12
    # the host restatement of the device function rounds the same numbers to fp32
    assert (eng.world_theta_host(theta.float(), rec.expand(4, 32), nd).double() - theta.float().double() * tr.grid_scale(ms, ts, mv, tv)).abs().max().item() <= 3e-7
    # the record is the restatement's
    assert torch.allclose(rec, wref.record(ms, ts, wref.header(ms, mv), wref.header(ts, tv)), rtol=0, atol=1e-12)


# 2 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tshape,mshape", [((19, 23, 41), (24, 20, 30)), ((13, 17), (21, 15))], ids=["3d", "2d"])
def test_chain_rule_against_finite_differences(tshape, mshape):
    """sum(g (.) theta_eff(theta)) is linear in theta: central differences against the chain rule (the package's and the restatement's), 1e-8.  Oblique
    headers (0.3 / -0.2 / 0.15 rad, one flipped axis, origins tens of mm apart), 'centers' as T0."""
    nd = len(tshape)
    Am, At = wref.oblique_pair(tshape, mshape)
    assert (Am[:nd, nd] - At[:nd, nd]).abs().max().item() > 10.0
    geo = tr.world_geometry(mshape, tshape, Am, At, init="centers")
    gen = torch.Generator().manual_seed(7)
    g, theta = torch.randn(1, nd, nd + 1, generator=gen, dtype=torch.float64), torch.randn(1, nd, nd + 1, generator=gen, dtype=torch.float64)
    f = lambda th: (g * wref.theta_eff(th, geo.record)).sum().item()  # noqa: E731
    fd = torch.zeros_like(theta)
    h = 1e-3
    for r in range(nd):
        for c in range(nd + 1):
            d = torch.zeros_like(theta)
            d[0, r, c] = h
            fd[0, r, c] = (f(theta + d) - f(theta - d)) / (2 * h)
    for name, got in (("package", eng.world_chain_host(g, geo.record, nd)), ("restatement", wref.chain(g, geo.record))):
        err = (got - fd).abs().max().item() / fd.abs().max().item()
        print(f"{nd}-D {name}: chain rule against finite differences {err:.1e} relative")
        assert err <= 1e-8


# 3 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tshape,mshape", [((40, 40, 40), (25, 33, 52)), ((24, 28), (30, 22))], ids=["3d", "2d"])
def test_the_record_does_not_depend_on_the_level(tshape, mshape):
    nd = len(tshape)
    Am, At = wref.oblique_pair(tshape, mshape)
    full = tr.world_geometry(mshape, tshape, Am, At, init="centers")
    tl, ml = tr.pyramid_shapes(tshape, 2)[0], tr.pyramid_shapes(mshape, 2)[0]
    assert tl != tuple(tshape)
    lvl = tr.world_geometry(ml, tl, eng.level_affine(Am, mshape, ml), eng.level_affine(At, tshape, tl), init=full.init, center=full.center)
    scale = full.record.abs().max().item()
    err = (lvl.record - full.record).abs().max().item()
    print(f"{nd}-D: level record against the full-resolution one {err:.1e} (entries up to {scale:.1f})")
    assert err <= 1e-12 * max(1.0, scale)
    # ... also when the level works out its own centre and 'centers' translation: the geometric centre is the field of view's
    own = tr.world_geometry(ml, tl, eng.level_affine(Am, mshape, ml), eng.level_affine(At, tshape, tl), init="centers")
    assert (own.record - full.record).abs().max().item() <= 1e-11 * max(1.0, scale)


# 4 ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tshape,mshape", [((19, 23, 41), (24, 20, 30)), ((13, 17), (21, 15))], ids=["3d", "2d"])
def test_converters_are_inverse_and_match_the_record(tshape, mshape):
    nd = len(tshape)
    Am, At = wref.oblique_pair(tshape, mshape)
    T = torch.eye(nd + 1, dtype=torch.float64)
    T[:nd, :nd] = wref.rotation(0.1, 0.05, -0.07)[:nd, :nd] if nd == 3 else wref.rot2(0.1)
    T[:nd, nd] = torch.tensor([3.0, -2.0, 1.0][:nd], dtype=torch.float64)
    theta = tr.theta_from_world(T, Am, At, mshape, tshape)
    back = tr.world_from_theta(theta, Am, At, mshape, tshape)
    assert tuple(theta.shape) == (1, nd, nd + 1) and (back[0] - T).abs().max().item() <= 1e-12 * T.abs().max().item()
    assert (tr.theta_from_world(back, Am, At, mshape, tshape) - theta).abs().max().item() <= 1e-12
    # the loop's theta_eff at Theta = I with T0 = T is the converter's theta, and world_matrix of it is T
    geo = tr.world_geometry(mshape, tshape, Am, At, init=T)
    ident = torch.eye(nd, nd + 1, dtype=torch.float64)[None]
    assert (wref.theta_eff(ident, geo.record) - theta).abs().max().item() <= 1e-12
    assert (geo.matrix(ident)[0] - T).abs().max().item() <= 1e-12
    # ... and for a general theta: world_from_theta(theta_eff) = T0 Tr(c) Theta Tr(-c)
    th = ident + 0.1 * torch.randn(1, nd, nd + 1, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    M = tr.world_from_theta(wref.theta_eff(th, geo.record), Am, At, mshape, tshape)
    assert (M - geo.matrix(th)).abs().max().item() <= 1e-11
    assert (geo.matrix(th)[0] - wref.world_matrix(th[0], wref.geometry(mshape, tshape, Am, At, T))).abs().max().item() <= 1e-12


# 5 ---------------------------------------------------------------------------------------------------------------------------------------
def _numpy_moments(x, mask=None):
    """image_moments restated on the CPU (the kernel is checked against numpy on the GPU): (mass [B], centre [B,nd] in the tensor's axis order)."""
    out_m, out_c = [], []
    for b in range(x.shape[0]):
        v = x[b, 0].double()
        m = torch.ones_like(v, dtype=torch.bool) if mask is None else (mask[b].reshape(v.shape) != 0)
        w = torch.where(m, v - v[m].min(), torch.zeros_like(v))
        idx = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in v.shape], indexing="ij"), dim=-1)
        out_m.append(w.sum())
        out_c.append((w[..., None] * idx).reshape(-1, v.dim()).sum(0) / w.sum())
    return torch.stack(out_m), torch.stack(out_c)


def test_world_init_modes_on_two_blobs(monkeypatch):
    """T0 of 'centers' and 'moments' against hand arithmetic.  A symmetric blob of sigma 4 mm at a known world position has its centre of mass there
    (to the truncation by the lattice, < 0.05 mm here), so 'moments' must give the translation between the two blob positions and c the target's."""
    monkeypatch.setattr(eng, "image_moments", _numpy_moments)
    ts, ms = (24, 26, 28), (30, 24, 22)
    At = wref.header(ts, (1.5, 1.0, 1.0), wref.rotation(-0.05, 0.04, 0.1), centre=(10.0, -5.0, 3.0))
    Am = wref.header(ms, (1.0, 1.2, 1.1), wref.rotation(*wref.OBLIQUE), flip=1, centre=(-30.0, 22.0, 8.0))
    pt, pm = (11.0, -4.0, 2.0), (-31.0, 23.5, 9.0)
    far = lambda p: tuple(v + 200.0 for v in p)  # noqa: E731  (the second blob of two_blobs, out of sight: one blob)
    tgt, mov = wref.two_blobs(ts, At, (pt, far(pt)), sigma=(4.0, 4.0)), wref.two_blobs(ms, Am, (pm, far(pm)), sigma=(4.0, 4.0))
    geo = eng.world_setup(mov, tgt, Am, At, "moments")
    want = torch.tensor(pm, dtype=torch.float64) - torch.tensor(pt, dtype=torch.float64)
    print("moments T0 translation", geo.init[0, :3, 3].tolist(), "want", want.tolist(), "c", geo.center[0].tolist())
    assert (geo.init[0, :3, 3] - want).abs().max().item() <= 0.1 and (geo.center[0] - torch.tensor(pt, dtype=torch.float64)).abs().max().item() <= 0.05
    assert torch.equal(geo.init[0, :3, :3], torch.eye(3, dtype=torch.float64)) and geo.init[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    # exactly the restatement's centres of mass (two real blobs, and a mask that keeps one of them)
    tgt2 = wref.two_blobs(ts, At, ((4.0, -9.0, 1.0), (16.0, 0.0, 6.0)))
    mask = torch.zeros(1, 1, *ts, dtype=torch.uint8)
    mask[..., :14] = 1
    for m in (None, mask):
        geo = eng.world_setup(mov, tgt2, Am, At, "moments", mask=m)
        ct, cm = wref.centre_of_mass_world(tgt2, At, m), wref.centre_of_mass_world(mov, Am)
        assert (geo.center[0] - ct).abs().max().item() <= 1e-10 and (geo.init[0, :3, 3] - (cm - ct)).abs().max().item() <= 1e-10
    # 'centers': by hand, the lattice centres are the `centre` the headers were built with
    geo = eng.world_setup(mov, tgt, Am, At, "centers")
    assert (geo.init[0, :3, 3] - torch.tensor([-40.0, 27.0, 5.0], dtype=torch.float64)).abs().max().item() <= 1e-12
    assert (geo.center[0] - torch.tensor([10.0, -5.0, 3.0], dtype=torch.float64)).abs().max().item() <= 1e-12
    # None: trust the headers; a matrix: taken as it is, per pair
    geo = eng.world_setup(mov, tgt, Am, At, None)
    assert torch.equal(geo.init[0], torch.eye(4, dtype=torch.float64)) and (geo.center[0] - torch.tensor([10.0, -5.0, 3.0], dtype=torch.float64)).abs().max().item() <= 1e-12
    T = wref.translation((1.0, 2.0, 3.0))
    geo = eng.world_setup(mov.repeat(2, 1, 1, 1, 1), tgt.repeat(2, 1, 1, 1, 1), Am, torch.stack([At, At]), torch.stack([T, torch.eye(4, dtype=torch.float64)]))
    assert geo.B == 2 and torch.equal(geo.init[0], T) and torch.equal(geo.init[1], torch.eye(4, dtype=torch.float64)) and tuple(geo.record.shape) == (2, 32)


# 6 ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals(device="cpu"):
    """Every ValueError of the feature; none of them needs a device (run again next to one by the GPU tests)."""
    ts, ms = (5, 6, 7), (9, 7, 6)
    Am, At = wref.oblique_pair(ts, ms)
    bad = lambda f: (lambda A: (f(A), A)[1])(Am.clone())  # noqa: E731
    nan = bad(lambda A: A.__setitem__((0, 1), float("nan")))
    inf = bad(lambda A: A.__setitem__((1, 3), float("inf")))
    row = bad(lambda A: A.__setitem__((3, 0), 1e-3))
    row2 = bad(lambda A: A.__setitem__((3, 3), 2.0))
    sing = bad(lambda A: A.__setitem__((slice(0, 3), 0), A[:3, 1] * (1.0 + 1e-10)))
    for A in (nan, inf, row, row2, sing, torch.eye(3, dtype=torch.float64), torch.zeros(2, 3, 4, 4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            tr.world_geometry(ms, ts, A, At)
        with pytest.raises(ValueError):
            tr.world_geometry(ms, ts, Am, A)
        with pytest.raises(ValueError):
            tr.theta_from_world(torch.eye(4), A, At, ms, ts)
        with pytest.raises(ValueError):
            tr.world_from_theta(torch.eye(3, 4), Am, A, ms, ts)
    for kw in (dict(moving_affine=Am, target_affine=None), dict(moving_affine=None, target_affine=At)):
        with pytest.raises(ValueError):
            tr.world_geometry(ms, ts, **kw)
    with pytest.raises(ValueError):
        tr.world_geometry(ms, ts, Am, At, init="moments")        # needs the images: world_setup / optim
    with pytest.raises(ValueError):
        tr.world_geometry(ms, ts, Am, At, init=nan)
    with pytest.raises(ValueError):
        tr.world_geometry(ms, ts, Am, At, center=torch.tensor([0.0, float("nan"), 0.0]))
    with pytest.raises(ValueError):
        tr.world_geometry(ms, (5, 6), Am, At)
    with pytest.raises(ValueError):
        tr.world_geometry(ms, ts, torch.stack([Am] * 2), torch.stack([At] * 3))
    mov, tgt = torch.zeros(1, 1, *ms, device=device), torch.zeros(1, 1, *ts, device=device)
    mi = lambda mode="rigid", loop=True: tr.Register(mode, criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=loop)  # noqa: E731
    # one affine without the other; affines together with voxel sizes; an unknown world_init; world_init without headers
    for kw in (dict(moving_affine=Am), dict(target_affine=At), dict(moving_affine=Am, target_affine=At, moving_voxel=(1, 1, 1), target_voxel=(1, 1, 1)),
               dict(moving_affine=Am, target_affine=At, world_init="principal"), dict(world_init="centers"), dict(moving_affine=nan, target_affine=At),
               dict(moving_affine=Am, target_affine=At, world_init=row)):
        with pytest.raises(ValueError):
            mi().optim(mov, tgt, lr=0.01, max_epochs=1, **kw)
        with pytest.raises(ValueError):
            tr.AffineMISolver(mov, tgt, mode="rigid", **kw)
        with pytest.raises(ValueError):
            tr.rigid_register(mov, tgt, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, device_loop=True, debug=False, **kw)
    # the support rule: GRIDS_SUPPORT's - anywhere but mode 'rigid' / 'affine' with device_loop=True
    ok = dict(moving_affine=Am, target_affine=At)
    for reg in (mi(loop=False), tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline"), tr.Register("affine"),
                tr.Register("flow")):
        with pytest.raises(ValueError, match="world"):
            reg.optim(mov, tgt, lr=0.01, max_epochs=1, **ok)
    with pytest.raises(ValueError, match="world"):
        tr.affine_register(mov, tgt, criterions=[tr.NCCLoss()], weights=[1.0], grad_edges=False, debug=False, **ok)
    with pytest.raises(ValueError):
        tr.affine_mi_loss_grad(mov, tgt, torch.zeros(1, 3, 4), torch.zeros(1, 4), scale=torch.ones(3, 4), world=torch.zeros(1, 32))


def test_refusals():
    check_refusals()


# 7 ---------------------------------------------------------------------------------------------------------------------------------------
def test_rehearsal_of_what_it_is_for():
    """GPU test 7 in the arbiter (fp64): the world phantom of affine_mi_grids_ref on 10x30x30 @ 3x1x1 mm (header rotated by -0.05 / 0.04 / 0.1 rad, centre
    (2, -3, 1.5) mm) and on 26x22x18 @ 1.2x1.4x1.7 mm under an oblique header (0.3 / -0.2 / 0.15 rad, tensor axis 1 flipped, centre 1 / -2 / 1.5 mm off the
    image of the target's centre), true transform Tr(c) Theta(WORLD_POSE) Tr(-c).  The proposed phantom and header satisfy the condition as they are, no other
    header had to be chosen: rigid, Adam 0.01, 32 bins, zero start, 120 iterations end 5.8e-3 from the true pose with the headers and 1.39 from it
    with the voxel sizes alone (the flipped axis and the 0.3 rad are out of that run's reach)."""
    _, pose_h, err_h, best_h = wref.world_run(True)
    _, pose_v, err_v, best_v = wref.world_run(False)
    print(f"max |pose - true|: headers {err_h:.4f} (best loss {best_h:.4f}), voxel sizes only {err_v:.4f} (best loss {best_v:.4f})")
    assert err_h <= 0.5 * err_v and err_h <= 0.02 and best_h < best_v
    # the origins of the two headers lie tens of mm apart, and the header is what the package's geometry sees
    Am, At, T = wref.world_headers()
    assert (Am[:3, 3] - At[:3, 3]).abs().max().item() > 10.0
    (ts, _), (ms, _) = gref.WORLD_TARGET, gref.WORLD_MOVING
    geo = tr.world_geometry(ms, ts, Am, At)
    assert torch.allclose(geo.record, wref.record(ms, ts, Am, At), rtol=0, atol=1e-11)
    th = gref.pose_to_theta(torch.tensor(wref.WORLD_POSE, dtype=torch.float64))
    assert (geo.matrix(th)[0] - T).abs().max().item() <= 1e-10


@pytest.mark.parametrize("name", list(wref.LOOPS))
def test_loop_table_meets_its_conditions(name):
    """What _loop_bars' floors rely on: the fp64 loss falls in every iteration, and the arbiter's two precisions stay within 1e-5 (loss) and 2e-5
    (parameters)."""
    r64, r32 = wref.loop_pair(name)
    lgap, pgap = np.max(np.abs(r64[0] - r32[0])), np.max(np.abs(r64[1] - r32[1]))
    print(f"{name}: {r64[0][0]:.5f} -> {r64[0][-1]:.5f}, fp32-fp64 loss {lgap:.1e} parameters {pgap:.1e}")
    assert np.all(np.diff(r64[0]) < 0) and lgap <= 1e-5 and pgap <= 2e-5
    # the start samples where the grids loops do: theta_eff(I) = I under this T0
    nd = len(wref.LOOPS[name][0])
    rec = wref.loop_setup(name)[2]
    assert (wref.theta_eff(torch.eye(nd, nd + 1, dtype=torch.float64)[None], rec)[0] - torch.eye(nd, nd + 1, dtype=torch.float64)).abs().max().item() <= 1e-12


def test_reach_pair_is_beyond_the_rigid_cap():
    """The pair of the GPU reach test: contents 40 mm apart, beyond 0.25 l of the moving lattice on the axes the offset uses, and the centres of mass
    show it."""
    mov, tgt, Am, At = wref.reach_pair()
    shift = torch.tensor(wref.REACH_SHIFT, dtype=torch.float64)
    geo = tr.world_geometry(wref.REACH_MSHAPE, wref.REACH_TSHAPE, Am, At)
    assert math.isclose(float(shift.norm()), 40.0, rel_tol=1e-12)
    assert bool((shift.abs()[:2] > 0.25 * geo.extent[0][:2]).all())
    d = wref.centre_of_mass_world(mov, Am) - wref.centre_of_mass_world(tgt, At)
    print("centres of mass apart by", d.tolist(), "0.25 l =", (0.25 * geo.extent[0]).tolist())
    assert (d - shift).abs().max().item() <= 1.0 and bool((d.abs()[:2] > 0.25 * geo.extent[0][:2]).all())


def test_layout_change_is_the_same_physical_image():
    """relayout: voxel j of the new tensor lies where voxel M j of the old one did."""
    x = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(1, 1, 2, 3, 4)
    A = wref.oblique_pair((2, 3, 4), (2, 3, 4))[0]
    y, Ay = wref.relayout(x, A)
    assert y.shape == (1, 1, 2, 4, 3)
    for j in ((0, 0, 0), (1, 3, 2), (0, 2, 1)):
        p = Ay @ torch.tensor(j + (1,), dtype=torch.float64)
        i = torch.linalg.solve(A, p)[:3].round().long().tolist()
        assert y[0, 0][j].item() == x[0, 0][tuple(i)].item()
