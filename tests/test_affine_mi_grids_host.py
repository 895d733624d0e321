"""Host-side checks of the cross-lattice rigid / affine mutual-information path: grid_scale and the geometry it stands
for, the refusals of the three *_grids entry points (each before any HIP call, so no GPU is needed), the dispatch of moving_voxel= / target_voxel= and
of differing shapes, and the conditions the GPU tests (tests/test_gpu_affine_mi_grids.py) rely on in their arbiter (tests/affine_mi_grids_ref.py):
every loop configuration descends with its two precisions together, and the registration the feature is for gains from the world scale."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import mi_ref

OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5


# ---------------------------------------------------------------------------------------------------------------------------------------
# grid_scale and what it means
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_grid_scale_values_and_refusals():
    import torchregister_amd as tr
    import TorchRegister
    assert TorchRegister.grid_scale is tr.grid_scale and tr.grid_scale is tr._engine.grid_scale
    s = tr.grid_scale((9, 7, 6), (5, 6, 7))
    assert s.shape == (3, 4) and s.dtype == torch.float64 and not s.is_cuda and bool((s == 1).all())
    assert bool((tr.grid_scale((21, 15), (13, 17)) == 1).all()) and tr.grid_scale((21, 15), (13, 17)).shape == (2, 3)
    # rows / columns in theta's order (x, y, z) = the tensor's axes reversed: scale[r][c] = e_target[c] / e_moving[r], translation column 1
    s = tr.grid_scale((20, 18, 16), (10, 12, 14), (1.2, 0.9, 0.8), (3.0, 1.0, 1.0))
    e_m, e_t = [16 * 0.8 / 2, 18 * 0.9 / 2, 20 * 1.2 / 2], [14 * 1.0 / 2, 12 * 1.0 / 2, 10 * 3.0 / 2]
    for r, c in itertools.product(range(3), range(3)):
        assert s[r, c].item() == pytest.approx(e_t[c] / e_m[r], rel=1e-15)
    assert s[:, 3].tolist() == [1.0, 1.0, 1.0]
    assert torch.equal(s, gref.scale_of((20, 18, 16), (10, 12, 14), (1.2, 0.9, 0.8), (3.0, 1.0, 1.0)))
    s2 = tr.grid_scale((30, 22), (24, 28), (0.9, 1.3), (2.0, 1.0))
    assert s2[0, 1].item() == pytest.approx((24 * 2.0) / (22 * 1.3)) and s2[:, 2].tolist() == [1.0, 1.0]
    # equal lattices and equal voxels: ones on the diagonal (theta's diagonal keeps its meaning), ratios of extents off it - ones only for a cube
    assert bool((tr.grid_scale((8, 8, 8), (8, 8, 8), (2.0, 2.0, 2.0), (2.0, 2.0, 2.0)) == 1).all())
    s = tr.grid_scale((8, 9, 10), (8, 9, 10), (3.0, 1.0, 1.0), (3.0, 1.0, 1.0))
    assert s.diagonal().tolist() == [1.0, 1.0, 1.0] and s[0, 2].item() == pytest.approx(24.0 / 10.0) and s[2, 0].item() == pytest.approx(10.0 / 24.0)
    for kw in (dict(moving_voxel=(1, 1, 1)), dict(target_voxel=(1, 1, 1))):
        with pytest.raises(ValueError, match="both"):
            tr.grid_scale((8, 8, 8), (8, 8, 8), **kw)
    for bad in ((0.0, 1, 1), (-1.0, 1, 1), (float("nan"), 1, 1), (float("inf"), 1, 1), (1, 1)):
        with pytest.raises(ValueError):
            tr.grid_scale((8, 8, 8), (8, 8, 8), bad, (1, 1, 1))
        with pytest.raises(ValueError):
            tr.grid_scale((8, 8, 8), (8, 8, 8), (1, 1, 1), bad)
    with pytest.raises(ValueError):
        tr.grid_scale((8, 8), (8, 8, 8))
    with pytest.raises(ValueError):
        tr.grid_scale((8, 0, 8), (8, 8, 8))


def _moving_mm(theta_eff, tshape, tvoxel, mshape, mvoxel):
    """Where affine_grid + grid_sample send the target's voxel centres, in millimetres of the moving volume: [N, 3] (x, y, z), fp64.  The normalised
    coordinate of a voxel centre is its world coordinate over the half extent, on both lattices (align_corners=False)."""
    e_t, e_m = gref.half_extents(tshape, tvoxel), gref.half_extents(mshape, mvoxel)
    xt = gref.voxel_centres_mm(tshape, tvoxel).reshape(-1, 3)
    xn = torch.cat([xt / e_t, torch.ones(len(xt), 1, dtype=torch.float64)], dim=1)
    return xt, (xn @ theta_eff.T) * e_m


def test_theta_times_scale_is_rigid_in_millimetres():
    """Theta(pose) under the world scale preserves every distance between target voxel centres to 1e-12 mm on 10x12x14 @ 3x1x1 mm against
    20x18x16 @ 1.2x0.9x0.8 mm; the plain theta (scale 1: the normalised cubes coincide) changes distances by more than 10 %."""
    import torchregister_amd as tr
    tshape, tvoxel, mshape, mvoxel = (10, 12, 14), (3.0, 1.0, 1.0), (20, 18, 16), (1.2, 0.9, 0.8)
    theta = gref.pose_to_theta(torch.tensor([0.2, -0.15, 0.1, 0.3, -0.2, 0.1], dtype=torch.float64))[0]
    idx = torch.arange(0, 10 * 12 * 14, 7)

    def change(scale):
        xt, xm = _moving_mm(theta * scale, tshape, tvoxel, mshape, mvoxel)
        i, j = torch.triu_indices(len(idx), len(idx), offset=1)
        dt, dm = (xt[idx][i] - xt[idx][j]).norm(dim=1), (xm[idx][i] - xm[idx][j]).norm(dim=1)      # every pair of distinct points
        return (dm - dt).abs().max().item(), ((dm - dt).abs() / dt).max().item()

    abs_world, _ = change(tr.grid_scale(mshape, tshape, mvoxel, tvoxel))
    _, rel_plain = change(tr.grid_scale(mshape, tshape))
    print(f"distances: world scale changes them by {abs_world:.1e} mm at most, scale 1 by {100 * rel_plain:.1f} %")
    assert abs_world <= 1e-12 and rel_plain > 0.10
    # and the world map is the one world_matrix documents: moving_mm = theta[:, :3] target_mm + e_moving * theta[:, 3]
    xt, xm = _moving_mm(theta * tr.grid_scale(mshape, tshape, mvoxel, tvoxel), tshape, tvoxel, mshape, mvoxel)
    want = xt @ theta[:, :3].T + gref.half_extents(mshape, mvoxel) * theta[:, 3]
    assert (xm - want).abs().max().item() <= 1e-12


def test_gradient_of_the_unscaled_theta_is_the_scaled_gradient():
    """dL/dtheta = dL/dtheta_eff * scale, by autograd on both sides: the chain rule the reduction behind pass 2 applies."""
    tshape, mshape = (5, 6, 7), (9, 7, 6)
    mov, tgt = gref.pair(tshape, mshape)
    rng = mi_ref.fit_range(tgt, mov)
    scale = gref.kernel_scale(gref.scale_of(mshape, tshape, gref.VOXEL_M3, gref.VOXEL_T3))
    th = aref.theta0(3)[None].double()
    _, g, _ = gref.evaluate(mov, tgt, th, scale, rng)
    _, g_eff, _ = gref.evaluate(mov, tgt, th * scale, torch.ones(3, 4, dtype=torch.float64), rng)
    assert g.abs().max().item() > 0 and torch.allclose(g, g_eff * scale, rtol=1e-12, atol=1e-15)
    # ... and against central differences of the arbiter's own loss
    h = 1e-6
    for i, j in ((0, 0), (1, 3), (2, 1)):
        d = torch.zeros(1, 3, 4, dtype=torch.float64)
        d[0, i, j] = h
        fd = (gref.evaluate(mov, tgt, th + d, scale, rng)[0] - gref.evaluate(mov, tgt, th - d, scale, rng)[0]).item() / (2 * h)
        assert abs(fd - g[0, i, j].item()) <= 1e-5 * g.abs().max().item(), (i, j, fd, g[0, i, j].item())


@pytest.mark.parametrize("name", list(gref.LOOPS))
def test_arbiter_descends_and_its_precisions_stay_together(name):
    """The conditions tests/test_affine_mi_host.py asserts for the one-lattice table, for every cross-lattice row: the fp64 loss falls in every
    one of the 10 iterations and the fp32 run stays within 1e-5 (loss curve) and 2e-5 (final parameter) of it."""
    (l64, p64), (l32, p32) = gref.loop_pair(name)
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    print(f"{name}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, lgap {lgap:.1e}, pgap {pgap:.1e}")
    assert len(l64) == gref.ITERS and np.all(np.isfinite(l64)) and np.all(np.diff(l64) < 0), l64
    assert lgap <= 1e-5 and pgap <= 2e-5, (lgap, pgap)


def test_what_it_is_for_in_the_arbiter():
    """A phantom defined in millimetres on 10x30x30 @ 3x1x1 mm (target) and, moved rigidly and sent through 4w(1 - w), on 26x22x18 @ 1.2x1.4x1.7 mm
    (moving): rigid, Adam 0.01, 32 bins, zero start, 120 iterations in fp64.  Under the world scale Theta(pose) can be the motion, under scale 1 it
    cannot: the pose error with the world scale is at most half the other."""
    _, _, err_w, best_w = gref.world_run(True)
    _, _, err_1, best_1 = gref.world_run(False)
    print(f"max |pose - true|: world scale {err_w:.4f} (best loss {best_w:.4f}), scale 1 {err_1:.4f} (best loss {best_1:.4f})")
    assert err_w <= 0.5 * err_1 and best_w < best_1


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------------------------
def _vol(_lib, ndim=3, B=2, dhw=(12, 14, 16), ptr=True):
    v = _lib.Volumes()
    v.ndim, v.B, (v.D, v.H, v.W) = ndim, B, dhw
    v.moving = v.target = 4096 if ptr else None          # never dereferenced: every call below is refused first
    v.moving_stride = v.target_stride = dhw[0] * dhw[1] * dhw[2]
    return v


def _grid(_lib, dhw=(15, 13, 18), scale=None, ndim=3, **entries):
    g = _lib.MovingGrid()
    g.D, g.H, g.W = dhw
    for k in range(12):
        g.scale[k] = 1.0 if scale is None else scale
    for k, v in entries.items():
        g.scale[int(k[1:])] = v
    return g


def _cfg(_lib, bins=32, alpha=1.0, rng=4096):
    c = _lib.MICfg()
    c.bins, c.alpha, c.normalized, c.range = bins, alpha, 0, rng
    return c


def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    vol = _vol(_lib)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), 32)
    inf, nan = float("inf"), float("nan")
    # (grid, expected) - shared by the three entry points
    grids = [(None, ARG), (_grid(_lib, (0, 13, 18)), ARG), (_grid(_lib, (15, -1, 18)), ARG), (_grid(_lib, (15, 13, 0)), ARG),
             (_grid(_lib, (2048, 1024, 1024)), ARG), (_grid(_lib, s0=nan), ARG), (_grid(_lib, s5=inf), ARG), (_grid(_lib, s3=nan), ARG),
             (_grid(_lib, s11=-inf), ARG), (_grid(_lib, s0=0.0), ARG), (_grid(_lib, s6=-1.0), ARG), (_grid(_lib, s10=0.0), ARG)]
    ok_grids = [_grid(_lib), _grid(_lib, s3=0.0, s7=-2.0, s11=0.0), _grid(_lib, (1, 1, 1))]      # the translation column may be anything finite

    def grad(v=vol, g=_grid(_lib), c=_cfg(_lib), theta=4096, loss=4096, ws=4096, nbytes=n):
        return lib.trx_affine_mi_loss_grad_grids(ref(v), ref(g), ref(c), P(theta) if theta else None, P(loss) if loss else None, P(4096), P(ws) if ws else None,
                                                 nbytes, None)

    opt = _lib.OptCfg(_lib.OPT_ADAM, 0.01, 0.9, 0.999, 1e-8)

    def state(**kw):
        st = _lib.AffineState()
        st.mode = _lib.PARAM_AFFINE
        for f in ("param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "losses", "step"):
            setattr(st, f, 4096)
        st.losses_capacity = 5
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def run(v=vol, g=_grid(_lib), c=_cfg(_lib), o=opt, st=state(), iters=1, ws=4096, nbytes=n):
        return lib.trx_affine_mi_run_grids(ref(v), ref(g), ref(c), ref(o), ref(st), iters, P(ws) if ws else None, nbytes, None)

    def warp(v=vol, g=_grid(_lib), theta=4096, channels=2, out=4096):
        return lib.trx_affine_warp_grids(ref(v), ref(g), P(theta) if theta else None, channels, P(out) if out else None, None)

    for g, want in grids:
        assert grad(g=g) == want and run(g=g) == want and warp(g=g) == want, (None if g is None else (g.D, g.H, g.W, list(g.scale)), want)
    # a good grid passes the grid check: the call gets as far as the next refusal (the workspace; for the warp: the null output)
    for g in ok_grids:
        assert grad(g=g, nbytes=n - 1) == WS and run(g=g, nbytes=n - 1) == WS and warp(g=g, out=None) == ARG
    # 2-D: the moving lattice is a plane too
    v2 = _vol(_lib, 2, 1, (1, 13, 17))
    n2 = lib.trx_affine_mi_workspace_bytes(ctypes.byref(v2), 32)
    assert grad(v=v2, g=_grid(_lib, (2, 21, 15)), nbytes=n2) == NDIM and run(v=v2, g=_grid(_lib, (2, 21, 15)), nbytes=n2) == NDIM
    assert warp(v=v2, g=_grid(_lib, (2, 21, 15))) == NDIM
    assert grad(v=v2, g=_grid(_lib, (1, 21, 15), s6=nan, s11=-1.0), nbytes=n2 - 1) == WS      # entries past ndim (ndim + 1) are not read
    # the refusals of the one-lattice entry points hold as they are
    assert grad(v=None) == ARG and grad(c=None) == ARG and grad(theta=None) == ARG and grad(loss=None) == ARG and grad(ws=None) == ARG
    assert grad(v=_vol(_lib, ptr=False)) == ARG and grad(c=_cfg(_lib, rng=None)) == ARG and grad(c=_cfg(_lib, bins=7)) == ARG
    assert grad(c=_cfg(_lib, alpha=nan)) == ARG and grad(v=_vol(_lib, B=0)) == ARG and grad(v=_vol(_lib, ndim=4)) == NDIM
    assert grad(nbytes=n - 1) == WS and grad(nbytes=0) == WS
    assert run(v=None) == ARG and run(c=None) == ARG and run(o=None) == ARG and run(st=None) == ARG and run(ws=None) == ARG and run(iters=-1) == ARG
    assert run(v=_vol(_lib, ndim=4)) == NDIM and run(nbytes=n - 1) == WS and run(iters=6) == CAP
    assert run(st=state(param=None)) == ARG and run(st=state(adam_m=None)) == ARG and run(st=state(mode=2)) == ARG
    assert run(o=_lib.OptCfg(7, 0.01, 0.9, 0.999, 1e-8)) == ARG
    assert run(iters=0) == OK                                     # nothing to enqueue: no HIP call either
    assert warp(v=None) == ARG and warp(theta=None) == ARG and warp(out=None) == ARG and warp(channels=0) == ARG
    assert warp(v=_vol(_lib, ndim=4)) == NDIM and warp(v=_vol(_lib, B=0)) == ARG
    # the workspace depends on the target lattice alone: the query takes no moving grid and is what the calls above were held to
    assert n == lib.trx_affine_mi_workspace_bytes(ctypes.byref(_vol(_lib)), 32) > 0


def test_entry_points_refuse_before_any_launch():
    check_refusals()


def check_dispatch(moving, target):
    """Differing shapes or voxel sizes anywhere but the fused mutual-information loop, and exactly one voxel size anywhere: ValueError - with CPU
    tensors the proof that nothing touched a device first (the GPU path itself refuses them with another exception type)."""
    import torch.nn as nn
    import torchregister_amd as tr
    mi = dict(criterion=[tr.MILoss()], weight=[1.0], optimizer="adam")
    vox = dict(moving_voxel=(1.2, 0.9, 0.8), target_voxel=(3.0, 1.0, 1.0))
    same = torch.zeros_like(target)
    for reg in (tr.Register("rigid", **mi), tr.Register("affine", **mi, device_loop=False), tr.Register("rigid", criterion=[nn.MSELoss()], weight=[1.0]),
                tr.Register("rigid", **mi, levels=2), tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="direct"),
                tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline", spacing=4, levels=2)):
        with pytest.raises(ValueError, match="lattice of its own"):
            reg.optim(moving, target, max_epochs=2)
        with pytest.raises(ValueError, match="lattice of its own"):
            reg.optim(same, target, max_epochs=2, **vox)
    for fn in (tr.affine_register, tr.rigid_register):
        with pytest.raises(ValueError, match="lattice of its own"):
            fn(moving, target, epochs=2, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False)
        with pytest.raises(ValueError, match="lattice of its own"):
            fn(same, target, epochs=2, criterions=[nn.MSELoss()], weights=[1.0], grad_edges=False, **vox)
    loop = tr.Register("rigid", **mi, device_loop=True)
    for kw in (dict(moving_voxel=(1.0, 1.0, 1.0)), dict(target_voxel=(1.0, 1.0, 1.0))):
        with pytest.raises(ValueError, match="both"):
            loop.optim(moving, target, max_epochs=2, **kw)
        with pytest.raises(ValueError, match="both"):
            tr.rigid_register(moving, target, epochs=2, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, device_loop=True, **kw)
    with pytest.raises(ValueError):
        loop.optim(moving, target, max_epochs=2, moving_voxel=(1.0, 0.0, 1.0), target_voxel=(1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="lattice of its own"):
        loop.optim(moving[0], target, max_epochs=2)                      # [1,H,W,?] against [1,1,D,H,W]: not the same number of dimensions
    assert loop.theta is None and loop.world_matrix is None and loop.target_shape is None


def test_dispatch_raises_before_any_device_work():
    check_dispatch(torch.zeros(1, 1, 9, 7, 6), torch.zeros(1, 1, 5, 6, 7))
