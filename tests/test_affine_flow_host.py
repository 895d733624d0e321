"""Host-side checks of the composed warp (a flow through an initial affine, sampled once): the definition in
tests/affine_flow_ref.py against the two warps it reduces to and its analytic backward against autograd, pyramid.level_theta against the chain it
folds, the refusals of the three entry points (each before any HIP call, so no GPU is needed), the validation of initial= with CPU tensors, the
conditions the GPU tests (tests/test_gpu_affine_flow.py) rely on, and what the feature is for."""
import ctypes

import numpy as np
import pytest
import torch

import affine_flow_ref as fr
import affine_mi_grids_ref as gref
import test_affine_mi_grids_host as ghost

OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.CASES))
def test_zero_flow_is_the_affine_warp_on_two_lattices(name):
    x, theta, flow, _ = fr.case(name, True)
    scale = fr.case_scale(name, True)
    got = fr.warp(x, theta, torch.zeros_like(flow), scale)
    want = gref.warp(theta.double(), gref.kernel_scale(scale), x, flow.shape[2:])
    assert (got - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(fr.CASES))
def test_identity_on_equal_lattices_is_the_flow_warp(name):
    from oracle import compose
    _, _, flow, _ = fr.case(name)
    nd = flow.shape[1]
    x = torch.rand((2, 2) + tuple(flow.shape[2:]), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = fr.warp(x, torch.eye(nd, nd + 1)[None].expand(2, -1, -1), flow)
    assert (got - compose.flow_warp(x, flow.double())).abs().max().item() <= 1e-12


@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("name", list(fr.CASES))
def test_analytic_backward_is_autograd(name, world):
    """The kernel's formula (a sampler written out corner by corner, times S_m / 2, theta_eff, 2 / S_t) against autograd through grid_sample, in
    fp64: equal to rounding away from the voxels where the derivative jumps, and the corner-by-corner sampler is grid_sample."""
    x, theta, flow, go = fr.case(name, world)
    scale = fr.case_scale(name, world)
    auto, formula = fr.backward(x, theta, flow, go, scale), fr.analytic_backward(x, theta, flow, go, scale)
    keep = fr.kept_voxels(theta, flow, x.shape[2:], scale)[:, None].expand_as(auto)
    assert auto.abs().max().item() > 0.05 and (auto - formula)[keep].abs().max().item() <= 1e-12
    val, _ = fr.sample_with_derivatives(x.double(), fr.sample_coords(theta, flow, x.shape[2:], scale))
    assert (val - fr.warp(x, theta, flow, scale)).abs().max().item() <= 1e-12


def test_autograd_matches_a_central_difference():
    x, theta, flow, go = fr.case("9x11x13")
    auto = fr.backward(x, theta, flow, go)
    keep = fr.kept_voxels(theta, flow, x.shape[2:])
    h, checked = 1e-6, 0
    for b, c, z, y, xx in ((0, 0, 4, 5, 6), (1, 1, 2, 7, 3), (0, 2, 6, 1, 11), (1, 2, 8, 10, 0), (0, 1, 0, 0, 12)):
        if not bool(keep[b, z, y, xx]):
            continue
        d = torch.zeros_like(flow, dtype=torch.float64)
        d[b, c, z, y, xx] = h
        fd = ((fr.warp(x, theta, flow.double() + d) - fr.warp(x, theta, flow.double() - d)) * go.double()).sum().item() / (2 * h)
        assert abs(fd - auto[b, c, z, y, xx].item()) <= 1e-7 * max(1.0, auto.abs().max().item()), (b, c, z, y, xx, fd, auto[b, c, z, y, xx].item())
        checked += 1
    assert checked >= 3


# ---------------------------------------------------------------------------------------------------------------------------------------
# level_theta
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [((10, 30, 30), (10, 15, 15), (26, 22, 18), (13, 11, 9)), ((33, 17, 9), (17, 9, 9), (20, 40, 31), (10, 20, 16)),
                                    ((17, 19), (9, 10), (14, 23), (14, 12)), ((12, 14, 16), (12, 14, 16), (15, 13, 18), (15, 13, 18))],
                         ids=["kept-z", "kept-x", "2d-kept-y", "finest"])
def test_level_theta_is_the_pointwise_chain(shapes):
    """level voxel -> full voxel -> normalised -> theta -> full moving voxel -> level moving voxel -> normalised, point by point, against the one
    matrix, for random thetas; an axis that keeps its size has a = 1; the finest level returns theta itself, bit for bit."""
    from torchregister_amd.pyramid import level_theta
    tf, tl, mf, ml = shapes
    nd = len(tf)
    g = torch.Generator().manual_seed(5)
    for _ in range(4):
        theta = torch.eye(nd, nd + 1, dtype=torch.float64) + 0.4 * (torch.rand(nd, nd + 1, generator=g, dtype=torch.float64) - 0.5)
        lvl = level_theta(theta[None], tf, tl, mf, ml)
        assert lvl.shape == (1, nd, nd + 1) and lvl.dtype == torch.float64
        pts = torch.rand(50, nd, generator=g, dtype=torch.float64) * (torch.tensor(tl, dtype=torch.float64) - 1.0)
        hom, want = fr.level_theta_pointwise(theta, tf, tl, mf, ml, pts)
        assert (hom @ lvl[0].T - want).abs().max().item() <= 1e-12
        if tf == tl and mf == ml:
            assert torch.equal(lvl[0], theta)
            assert torch.equal(level_theta(theta.float()[None], tf, tl, mf, ml)[0], theta.float())
    assert level_theta(torch.zeros(2, nd, nd + 1), tf, tl, mf, ml).dtype == torch.float32
    with pytest.raises(ValueError):
        level_theta(torch.zeros(1, nd + 1, nd), tf, tl, mf, ml)
    with pytest.raises(ValueError):
        level_theta(torch.zeros(1, nd, nd + 1), tf, tl[:-1], mf, ml)


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ptr = lambda p: P(p) if p else None  # noqa: E731
    _vol, _grid, _cfg = ghost._vol, ghost._grid, ghost._cfg
    vol = _vol(_lib, B=1)
    inf, nan = float("inf"), float("nan")
    grids = [(None, ARG), (_grid(_lib, (0, 13, 18)), ARG), (_grid(_lib, (15, -1, 18)), ARG), (_grid(_lib, (15, 13, 0)), ARG),
             (_grid(_lib, (2048, 1024, 1024)), ARG), (_grid(_lib, s0=nan), ARG), (_grid(_lib, s5=inf), ARG), (_grid(_lib, s3=nan), ARG),
             (_grid(_lib, s11=-inf), ARG), (_grid(_lib, s0=0.0), ARG), (_grid(_lib, s6=-1.0), ARG), (_grid(_lib, s10=0.0), ARG)]
    ok_grids = [_grid(_lib), _grid(_lib, s3=0.0, s7=-2.0, s11=0.0), _grid(_lib, (1, 1, 1))]

    def warp(v=vol, g=_grid(_lib), theta=4096, flow=4096, channels=2, out=4096):
        return lib.trx_affine_flow_warp(ref(v), ref(g), ptr(theta), ptr(flow), channels, ptr(out), None)

    def bwd(v=vol, g=_grid(_lib), theta=4096, flow=4096, channels=2, go=4096, dflow=4096):
        return lib.trx_affine_flow_warp_backward(ref(v), ref(g), ptr(theta), ptr(flow), channels, ptr(go), ptr(dflow), None)

    d3 = (ctypes.c_int * 3)(4, 4, 4)
    n = lib.trx_bspline_mi_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32)
    assert n > 0
    opt = _lib.OptCfg(_lib.OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)

    def state(**kw):
        st = _lib.BSplineState()
        for f in ("ctrl", "adam_m", "adam_v", "flow", "dflow", "losses", "step"):
            setattr(st, f, 4096)
        st.losses_capacity, st.bending_weight = 5, 0.0
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def run(v=vol, g=_grid(_lib), theta=4096, c=_cfg(_lib), o=opt, st=state(), sp=d3, iters=1, ws=4096, nbytes=n):
        return lib.trx_bspline_mi_run_grids(ref(v), ref(g), ptr(theta), ref(c), ref(o), ref(st), sp, iters, ptr(ws), nbytes, None)

    for g, want in grids:
        assert warp(g=g) == want and bwd(g=g) == want and run(g=g) == want, (None if g is None else (g.D, g.H, g.W, list(g.scale)), want)
    # a good grid passes the grid check: the call gets as far as the next refusal
    for g in ok_grids:
        assert warp(g=g, out=None) == ARG and bwd(g=g, dflow=None) == ARG and run(g=g, nbytes=n - 1) == WS
    # 2-D: the moving lattice is a plane too
    v2 = _vol(_lib, 2, 1, (1, 17, 19))
    assert warp(v=v2, g=_grid(_lib, (2, 14, 23))) == NDIM and bwd(v=v2, g=_grid(_lib, (2, 14, 23))) == NDIM
    n2 = lib.trx_bspline_mi_workspace_bytes(2, 1, 1, 17, 19, 1, 4, 4, 32)
    assert n2 > 0 and run(v=v2, g=_grid(_lib, (2, 14, 23)), nbytes=n2) == NDIM
    assert warp(v=v2, g=_grid(_lib, (1, 14, 23), s6=nan, s11=-1.0), out=None) == ARG      # entries past ndim (ndim + 1) are not read
    # what the plain counterparts refuse, theta and channels
    assert warp(v=None) == ARG and warp(theta=None) == ARG and warp(flow=None) == ARG and warp(out=None) == ARG and warp(channels=0) == ARG
    assert warp(v=_vol(_lib, ndim=4)) == NDIM and warp(v=_vol(_lib, B=0)) == ARG and warp(v=_vol(_lib, ptr=False)) == ARG
    assert warp(v=_vol(_lib, B=70000)) == ARG and warp(v=_vol(_lib, dhw=(2048, 1024, 1024))) == ARG and warp(v=_vol(_lib, 2, 1, (2, 17, 19))) == NDIM
    assert bwd(v=None) == ARG and bwd(theta=None) == ARG and bwd(flow=None) == ARG and bwd(go=None) == ARG and bwd(dflow=None) == ARG
    assert bwd(channels=-1) == ARG and bwd(v=_vol(_lib, ndim=1)) == NDIM and bwd(v=_vol(_lib, dhw=(12, 0, 16))) == ARG
    assert run(v=None) == ARG and run(theta=None) == ARG and run(c=None) == ARG and run(o=None) == ARG and run(st=None) == ARG and run(ws=None) == ARG
    assert run(sp=None) == ARG and run(iters=-1) == ARG and run(c=_cfg(_lib, rng=None)) == ARG and run(c=_cfg(_lib, bins=7)) == ARG
    assert run(c=_cfg(_lib, alpha=nan)) == ARG and run(v=_vol(_lib, ndim=4, B=1)) == NDIM and run(v=_vol(_lib, B=1, ptr=False)) == ARG
    assert run(st=state(ctrl=None)) == ARG and run(st=state(adam_m=None)) == ARG and run(st=state(bending_weight=-1.0)) == ARG
    assert run(st=state(bending_weight=nan)) == ARG and run(o=_lib.OptCfg(7, 0.1, 0.9, 0.999, 1e-8)) == ARG
    assert run(sp=(ctypes.c_int * 3)(0, 4, 4)) == ARG and run(nbytes=n - 1) == WS and run(nbytes=0) == WS and run(iters=6) == CAP
    assert run(iters=0) == OK                                     # nothing to enqueue: no HIP call either
    # the workspace is trx_bspline_mi_run's: it depends on the target lattice alone
    assert run(g=_grid(_lib, (40, 3, 7)), nbytes=n - 1) == WS and run(g=_grid(_lib, (40, 3, 7)), iters=0) == OK


def test_entry_points_refuse_before_any_launch():
    check_refusals()


def test_signatures_list_the_three_symbols():
    from torchregister_amd import _lib
    lib = _lib.load()
    for name in ("trx_affine_flow_warp", "trx_affine_flow_warp_backward", "trx_bspline_mi_run_grids"):
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert lib.trx_version() == 240


# ---------------------------------------------------------------------------------------------------------------------------------------
# initial=: validation before any device work
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_initial_dispatch(moving, target):
    """initial= anywhere but the B-spline mutual-information loop, or an initial that is not a theta / a finished rigid or affine Register of this
    target lattice: ValueError - with CPU tensors the proof that nothing touched a device first."""
    import torch.nn as nn
    import torchregister_amd as tr
    nd = target.dim() - 2
    theta = torch.eye(nd, nd + 1)[None]
    mi = dict(criterion=[tr.MILoss()], weight=[1.0], optimizer="adam")
    bad = [tr.Register("rigid", **mi, device_loop=True), tr.Register("affine", **mi), tr.Register("flow", **mi, flow_model="direct"),
           tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="bspline", spacing=4),
           tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="bspline", spacing=4, diffeomorphic=True),
           tr.Register("flow", criterion=[tr.MILoss(), nn.MSELoss()], weight=[1.0, 1.0], flow_model="bspline", spacing=4),
           tr.Register("flow", flow_model="bspline", spacing=4), tr.Register("flow", **mi, flow_model="unet")]
    for reg in bad:
        with pytest.raises(ValueError, match="initial="):
            reg.optim(moving, target, max_epochs=2, initial=theta)
        assert reg.theta is None and reg.initial is None
    good = dict(**mi, flow_model="bspline", spacing=4)
    for levels in (1, 2):
        reg = tr.Register("flow", **good, levels=levels)
        finished = tr.Register("rigid", **mi, device_loop=True)
        for initial in (torch.zeros(1, nd, nd), torch.zeros(3, nd, nd + 1), torch.zeros(nd + 1), "theta", finished, tr.Register("flow", **good)):
            with pytest.raises(ValueError, match="initial="):
                reg.optim(moving, target, max_epochs=2, initial=initial)          # wrong shapes, wrong types, a Register that has not run
        finished.theta, finished.target_shape = theta, tuple(s + 1 for s in target.shape[2:])
        with pytest.raises(ValueError, match="initial="):
            reg.optim(moving, target, max_epochs=2, initial=finished)             # ... or ran onto another lattice
        with pytest.raises(ValueError, match="initial="):
            reg.optim(moving, target, max_epochs=2, initial=theta, moving_voxel=(1.0,) * nd, target_voxel=(1.0,) * nd)
        # a valid request passes the validation and is refused by the device check (CPU tensors), not by a ValueError
        finished.target_shape = tuple(target.shape[2:])
        for initial in (theta, theta[0], finished):
            with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
                reg.optim(moving, target, max_epochs=2, initial=initial)
    fr_ = tr.flow_register(target.shape[2:], criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=4)
    with pytest.raises(ValueError, match="initial="):
        fr_.optimize(moving, target, initial=theta)
    with pytest.raises(ValueError, match="with `mi`"):
        tr.BSplineSolver(moving, target, 4, initial=theta)
    with pytest.raises(ValueError, match="without `squarings`"):
        tr.BSplineSolver(moving, target, 4, initial=theta, squarings=2)
    with pytest.raises(ValueError, match="initial_scale"):
        tr.BSplineSolver(moving, target, 4, mi=dict(bins=32), initial_scale=torch.ones(nd, nd + 1))


def test_initial_is_validated_before_any_device_work():
    import torchregister_amd as tr
    import TorchRegister
    assert TorchRegister.affine_flow_warp is tr.affine_flow_warp and tr.affine_flow_warp is tr._engine.affine_flow_warp
    assert tr.affine_flow_warp_backward is tr._engine.affine_flow_warp_backward
    check_initial_dispatch(torch.zeros(1, 1, 18, 14, 16), torch.zeros(1, 1, 10, 12, 16))      # (two pyramid levels exist for both lattices)
    check_initial_dispatch(torch.zeros(1, 1, 21, 15), torch.zeros(1, 1, 13, 17))


def test_without_initial_every_pinned_refusal_still_raises():
    ghost.check_dispatch(torch.zeros(1, 1, 9, 7, 6), torch.zeros(1, 1, 5, 6, 7))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the conditions the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("name", list(fr.CASES))
def test_cases_meet_their_conditions(name, world):
    """At most 0.5 % of a case's voxels lie within 1e-3 of an integer sample coordinate (they are left out of the backward comparisons), between 5 %
    and 50 % of each pair's samples leave the moving field of view, the two pairs have different maps, and the flow is off the voxel lattice."""
    x, theta, flow, go = fr.case(name, world)
    scale = fr.case_scale(name, world)
    tshape, mshape = fr.CASES[name][:2]
    assert x.shape == (2, 2) + mshape and flow.shape == (2, len(tshape)) + tshape and go.shape == (2, 2) + tshape and theta.dtype == torch.float32
    dropped = 1.0 - fr.kept_voxels(theta, flow, mshape, scale).double().mean().item()
    outside = [fr.outside_fraction(theta[b:b + 1], flow[b:b + 1], mshape, scale) for b in range(2)]
    print(f"{name} {'world' if world else 'ones'}: {100 * dropped:.3f} % left out, outside {outside[0]:.3f} / {outside[1]:.3f}")
    assert dropped <= 0.005
    assert all(0.05 <= o <= 0.50 for o in outside)
    assert (theta[0] - theta[1]).abs().max().item() > 0.05 and (flow - flow.round()).abs().mean().item() > 0.1
    if len(tshape) == 3:      # every entry of theta's matrix is non-zero in at least one pair
        assert bool(((theta[0, :, :3] != 0) | (theta[1, :, :3] != 0)).all())


@pytest.mark.parametrize("name", list(fr.LOOPS))
def test_arbiter_descends_and_its_precisions_stay_together(name):
    """Every row of the loop table: the fp64 loss falls in every one of the 10 iterations, and the fp32 run stays within 1e-5 of its loss curve."""
    (l64, p64), (l32, p32) = fr.loop_pair(name)
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    print(f"{name}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, lgap {lgap:.1e}, pgap {pgap:.1e}")
    assert len(l64) == fr.ITERS and np.all(np.isfinite(l64)) and np.all(np.diff(l64) < 0), l64
    assert lgap <= 1e-5, lgap


def test_loop_samples_leave_the_moving_field_of_view():
    for name in fr.LOOPS:
        mov, tgt, theta, _, _, ctrl0 = fr.loop_setup(name)
        import bspline_ref
        flow = bspline_ref.expand(ctrl0, tuple(tgt.shape[2:]), fr.LOOPS[name][2])
        assert 0.02 <= fr.outside_fraction(theta, flow, mov.shape[2:]) <= 0.5, name


# ---------------------------------------------------------------------------------------------------------------------------------------
# what it is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_interpolation_beats_resample_then_deform():
    """The world phantom of tests/affine_mi_grids_ref.py (10x30x30 @ 3x1x1 mm against 26x22x18 @ 1.2x1.4x1.7 mm, WORLD_POSE, no intensity map), a
    smooth flow of amplitude 1.5 target voxels, against the analytic image: sampling the moving image once through theta o (id + flow) has less
    than half the rms error of resampling with theta first and deforming the copy (0.0021 against 0.0060 of a signal range of 0.35)."""
    (rms1, max1), (rms2, max2), span = fr.world_errors()
    print(f"one interpolation: rms {rms1:.4f} max {max1:.4f}; resample then deform: rms {rms2:.4f} max {max2:.4f}; signal range {span:.2f}")
    assert rms1 < 0.5 * rms2 and max1 < max2 and span > 0.3
