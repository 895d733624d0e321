"""Dense-flow composition and fixed-point inversion on the GPU (trx_flow_compose, trx_flow_invert) against tests/flowops_ref.py;
tests/test_flowops_host.py asserts what these tests rest on."""
import math

import numpy as np
import pytest
import torch

import flowops_ref as fr
import jacobian_ref as jr
import phantoms as ph
from conftest import bar
from test_flowops_host import check_refusals
from test_gpu_bspline import _Guarded

pytestmark = pytest.mark.gpu

CASE_IDS = list(fr.CASES)


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _np(t):
    return t.detach().cpu().double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. compose
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding", ["border", "zeros"])
@pytest.mark.parametrize("case", CASE_IDS)
def test_compose_against_the_restatement(tr, case, padding):
    """Floor: 1e-6 * max(1, max |c|), a handful of fp32 roundings of a sum of eight products of values of that size."""
    r = fr.reference(case)
    u, s = fr.field(case).cuda(), fr.second_field(case).cuda()
    got = tr.compose_flows(u, s, padding)
    c32, c64 = _np(r["c32", padding]), _np(r["c64", padding])
    assert got.shape == u.shape and got.dtype == torch.float32
    e, b = np.abs(_np(got) - c64).max(), bar(c32, c64, 1e-6 * max(1.0, np.abs(c64).max()))
    print(f"{case} compose {padding}: err {e:.3e} bar {b:.3e} (restatement fp32-fp64 {np.abs(c32 - c64).max():.3e})")
    assert e <= b
    if padding == "border":
        assert torch.equal(tr.compose_flows(u, s), got)      # the default


@pytest.mark.parametrize("case", CASE_IDS)
def test_compose_with_itself_is_one_squaring(tr, case):
    u = fr.field(case).cuda()
    assert torch.equal(tr.compose_flows(u, u, "zeros"), tr.svf_exp(2 * u, 1))


@pytest.mark.parametrize("padding", [0, 1])
@pytest.mark.parametrize("case", ["a", "c"])
def test_compose_into_second(tr, case, padding):
    """out may be `second` itself: the bits of the call with a buffer of its own."""
    from torchregister_amd import _lib
    lib = _lib.load()
    u, s = fr.field(case).cuda(), fr.second_field(case).cuda()
    want = tr.compose_flows(u, s, "border" if padding else "zeros")
    geom = (u.shape[1], u.shape[0]) + tr._engine._dhw(u.shape[2:])
    buf = s.clone()
    _lib.check(lib.trx_flow_compose(_lib.ptr(u), _lib.ptr(buf), _lib.ptr(buf), *geom, padding, _lib.current_stream(u.device)), "trx_flow_compose")
    assert torch.equal(buf, want)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. invert
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_IDS)
def test_invert_fixed_count_against_the_restatement(tr, case):
    """tol = 0, 12 updates: v and residual against the restatement run for the same count.  Floor: 1e-5 * max(1, max |u|) - an update's rounding of a
    few 1e-7 max |u| carried through 12 updates of a map whose Lipschitz constant is below one."""
    r = fr.reference(case)
    u = fr.field(case).cuda()
    v, res = tr.invert_flow(u, fr.FIXED_K, 0.0, return_residual=True)
    assert v.shape == u.shape and res.shape == (u.shape[0], 1) + tuple(u.shape[2:])
    floor = 1e-5 * max(1.0, u.abs().max().item())
    ev, bv = np.abs(_np(v) - _np(r["v64"])).max(), bar(_np(r["v32"]), _np(r["v64"]), floor)
    er, br = np.abs(_np(res[:, 0]) - _np(r["r64"])).max(), bar(_np(r["r32"]), _np(r["r64"]), floor)
    print(f"{case} invert K={fr.FIXED_K}: v err {ev:.3e} bar {bv:.3e}; residual err {er:.3e} bar {br:.3e}")
    assert ev <= bv and er <= br
    assert torch.equal(tr.invert_flow(u, fr.FIXED_K, 0.0), v)


@pytest.mark.parametrize("case", CASE_IDS)
def test_invert_to_a_tolerance(tr, case):
    """tol = 1e-3 (the defaults): every voxel converges, and the fp64 right-inverse residual |v + Sb(u, y + v)| of the GPU's v, formed by the restatement,
    is at most tol + 1.5e-4 on every voxel.  Not compared element by element with the early-stopping restatement: a stop that falls one update apart in
    two precisions is legitimate."""
    u = fr.field(case)
    v, res = tr.invert_flow(u.cuda(), return_residual=True)
    assert torch.equal(tr.invert_flow(u.cuda(), fr.ITERATIONS, fr.TOL, return_residual=True)[1], res)
    rr = fr.right_residual(u, v.cpu())
    print(f"{case} invert tol={fr.TOL:g}: residual max {res.max().item():.3e}, |v + Sb(u, y + v)| max {rr.max().item():.3e} (restatement {fr.TABLE[case][1]:.1e})")
    assert bool((res <= fr.TOL).all())
    assert rr.max().item() <= fr.TOL + fr.SLACK


@pytest.mark.parametrize("case", ["a", "c", "e"])
def test_split_runs_give_the_bits_of_one_run(tr, case):
    """5 updates and 7 more from that result are 12 updates, also with `inverse` aliased to `init`."""
    from torchregister_amd import _lib
    lib = _lib.load()
    u = fr.field(case).cuda()
    v12, r12 = tr.invert_flow(u, 12, 0.0, return_residual=True)
    v5 = tr.invert_flow(u, 5, 0.0)
    v57, r57 = tr.invert_flow(u, 7, 0.0, init=v5, return_residual=True)
    assert torch.equal(v57, v12) and torch.equal(r57, r12) and not torch.equal(v5, v12)
    geom = (u.shape[1], u.shape[0]) + tr._engine._dhw(u.shape[2:])
    buf, res = v5.clone(), torch.empty_like(r12)
    _lib.check(lib.trx_flow_invert(_lib.ptr(u), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(res), *geom, 7, 0.0, _lib.current_stream(u.device)), "trx_flow_invert")
    assert torch.equal(buf, v12) and torch.equal(res, r12)


def test_same_bits_on_every_call_and_in_every_batch(tr):
    """Two calls; a pair alone and inside B = 3, next to a pair that holds NaN and Inf: that pair gets NaN in v and residual at the voxels that meet the
    values and nowhere else - a voxel of it that is not NaN has the bits of the clean field - and the other pairs do not notice."""
    one = fr.field("a")
    B, sp = 1, tuple(one.shape[2:])
    bad = one.clone()
    bad[0, 1, 4, 5, 6] = float("nan")
    bad[0, 2, 9, 12, 20] = float("inf")
    other = fr.second_field("a")
    batch = torch.cat([one, bad, other]).cuda()
    for kw in (dict(iterations=fr.FIXED_K, tol=0.0), dict(iterations=fr.ITERATIONS, tol=fr.TOL)):
        v, r = tr.invert_flow(batch, return_residual=True, **kw)
        v2, r2 = tr.invert_flow(batch, return_residual=True, **kw)
        assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(r.view(torch.int32), r2.view(torch.int32))
        for b, alone in ((0, one), (2, other)):
            va, ra = tr.invert_flow(alone.cuda(), return_residual=True, **kw)
            assert torch.equal(va[0], v[b]) and torch.equal(ra[0], r[b])
            assert bool(torch.isfinite(v[b]).all()) and bool(torch.isfinite(r[b]).all())
        nanmap = torch.isnan(r[1, 0])
        assert bool(nanmap[4, 5, 6]) and bool(nanmap[9, 12, 20]) and 2 <= int(nanmap.sum()) < 200
        assert torch.equal(torch.isnan(v[1]).all(0), nanmap) and torch.equal(torch.isnan(v[1]).any(0), nanmap)
        keep = ~nanmap[None].expand_as(v[1])
        assert torch.equal(v[1][keep], v[0][keep]) and torch.equal(r[1, 0][~nanmap], r[0, 0][~nanmap])
    # compose: the same, and a non-finite `second` stays in its own voxel
    c, c2 = tr.compose_flows(batch, batch.flip(0)), tr.compose_flows(batch, batch.flip(0))
    assert torch.equal(c.view(torch.int32), c2.view(torch.int32))
    assert torch.equal(tr.compose_flows(batch[:1], batch[2:]), c[:1]) and torch.equal(tr.compose_flows(batch[2:], batch[:1]), c[2:])
    assert bool(torch.isfinite(c[0]).all()) and bool(torch.isfinite(c[2]).all()) and not bool(torch.isfinite(c[1]).all())


def test_a_constant_field_inverts_exactly(tr):
    u = fr.constant_field().cuda()
    v, r = tr.invert_flow(u, return_residual=True)
    assert torch.equal(v, -u) and not bool(r.any())
    v, r = tr.invert_flow(u, 2, 0.0, return_residual=True)
    assert torch.equal(v, -u) and not bool(r.any())
    v, r = tr.invert_flow(u, 1, 0.0, return_residual=True)
    assert torch.equal(v, -u) and torch.equal(r, torch.full_like(r, 2.5))


def test_the_fold_field(tr):
    """Finite outputs; the share of voxels that converge is the host test's to +-0.02; the voxels that do not converge overlap those whose determinant
    is <= 0 (the host test establishes the overlap for the restatement)."""
    u = fr.fold_field().cuda()
    v, r = tr.invert_flow(u, return_residual=True)
    share = (r <= fr.TOL).float().mean().item()
    folded = tr.jacobian_determinant(u) <= 0
    print(f"fold: {100 * share:.1f} % converge, largest residual {r.max().item():.2f}, {int(((r > fr.TOL) & folded).sum())} voxels neither converge nor have det > 0")
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(r).all())
    assert abs(share - fr.FOLD_CONVERGED) <= 0.02
    assert bool(((r > fr.TOL) & folded).any())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. memory contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "c", "d"])
def test_kernels_stay_inside_their_buffers(tr, case):
    """out, inverse and residual between canaries (the inputs too); the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    u, s = fr.field(case).cuda(), fr.second_field(case).cuda()
    B, nd, sp = u.shape[0], u.shape[1], tuple(u.shape[2:])
    geom = (nd, B) + tr._engine._dhw(sp)
    n = math.prod(sp)
    gu, gs = _Guarded(u.numel() * 4, 0x69), _Guarded(u.numel() * 4, 0x66)
    gu.region.copy_(u.view(torch.uint8).reshape(-1))
    gs.region.copy_(s.view(torch.uint8).reshape(-1))
    stream = _lib.current_stream(torch.device("cuda"))
    outs = {pad: _Guarded(u.numel() * 4, 0x96) for pad in (0, 1)}
    for pad, g in outs.items():
        _lib.check(lib.trx_flow_compose(_lib.ptr(gu.region), _lib.ptr(gs.region), _lib.ptr(g.region), *geom, pad, stream), "trx_flow_compose")
    inv, res, inv2 = _Guarded(u.numel() * 4, 0x3C), _Guarded(B * n * 4, 0xC3), _Guarded(u.numel() * 4, 0x5A)
    _lib.check(lib.trx_flow_invert(_lib.ptr(gu.region), None, _lib.ptr(inv.region), _lib.ptr(res.region), *geom, fr.ITERATIONS, fr.TOL, stream), "trx_flow_invert")
    _lib.check(lib.trx_flow_invert(_lib.ptr(gu.region), _lib.ptr(gs.region), _lib.ptr(inv2.region), None, *geom, 3, 0.0, stream), "trx_flow_invert")
    torch.cuda.synchronize()
    for buf, what in ((gu, "flow"), (gs, "second / init"), (outs[0], "out (zeros)"), (outs[1], "out (border)"), (inv, "inverse"), (res, "residual"),
                      (inv2, "inverse (with init, without residual)")):
        buf.check(what)
    assert torch.equal(gu.floats(tuple(u.shape)), u) and torch.equal(gs.floats(tuple(u.shape)), s)
    assert torch.equal(outs[0].floats(tuple(u.shape)), tr.compose_flows(u, s, "zeros")) and torch.equal(outs[1].floats(tuple(u.shape)), tr.compose_flows(u, s, "border"))
    v, r = tr.invert_flow(u, return_residual=True)
    assert torch.equal(inv.floats(tuple(u.shape)), v) and torch.equal(res.floats((B, 1) + sp), r)
    assert torch.equal(inv2.floats(tuple(u.shape)), tr.invert_flow(u, 3, 0.0, init=s))


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. what they are for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_one_resampling_is_closer_than_two(tr):
    """On an analytic image and two analytic flows, flow_warp(img, compose_flows(a, b)) is closer (rms, interior) to the analytically composed image
    than flow_warp(flow_warp(img, a), b) - the ordering the host test establishes in fp64 (0.094 against 0.162)."""
    img, a, b, truth = (t.cuda() for t in fr.use_inputs(torch.float32))
    warp = tr._engine.flow_warp
    for padding in ("border", "zeros"):
        once, twice = fr.interior_rms(warp(img, tr.compose_flows(a, b, padding)).cpu(), truth.cpu()), fr.interior_rms(warp(warp(img, a), b).cpu(), truth.cpu())
        print(f"{padding}: one resampling {once:.4f}, two {twice:.4f}")
        assert once < twice


def test_compose_with_the_inverse_is_the_identity(tr):
    """compose_flows(u, invert_flow(u)) is the right-inverse residual: at most tol + 1.5e-4 everywhere (the fp32 form of the test above)."""
    for case in ("a", "c", "g"):
        u = fr.field(case).cuda()
        c = tr.compose_flows(u, tr.invert_flow(u))
        assert c.abs().max().item() <= fr.TOL + fr.SLACK


def test_register_invert_flow(tr):
    """The NCC B-spline phantom of tests/test_gpu_bspline.py::test_register_bspline_single_level: reg.invert_flow() converges on every voxel whose
    reg.jacobian() > 0.3, and warping reg(moving) with the inverse flow is closer to moving (interior mse) than reg(moving) itself.  Without the
    feature: AttributeError."""
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, ph.flow_field(shape)).cuda()
    tgt = tgt.cuda()
    reg = tr.Register("flow", criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, optimizer="adam")
    reg.optim(mov, tgt, lr=0.1, max_epochs=15)
    v, res = reg.invert_flow()
    assert v.shape == reg.theta.shape and res.shape == (1, 1) + shape
    v2, res2 = tr.invert_flow(reg.theta, return_residual=True)
    assert torch.equal(v, v2) and torch.equal(res, res2)
    det = reg.jacobian()
    print(f"min det {det.min().item():.3f}, {100 * (res <= fr.TOL).float().mean().item():.1f} % converge, largest residual {res.max().item():.3e}, "
          f"largest where det > 0.3: {res[det > 0.3].max().item():.3e}")
    assert bool((res[det > 0.3] <= fr.TOL).all()) and bool(torch.isfinite(v).all())
    warped = reg(mov)
    back = tr._engine.flow_warp(warped, v)
    inner = (Ellipsis,) + (slice(4, -4),) * 3
    mse = lambda x, y: (x[inner] - y[inner]).pow(2).mean().item()  # noqa: E731
    print(f"interior mse against moving: reg(moving) {mse(warped, mov):.5f}, carried back {mse(back, mov):.5f}")
    assert mse(back, mov) < mse(warped, mov)
    # flow_register carries the same method
    fl = tr.flow_register(shape, flow_model="bspline", criterions=[tr.NCCLoss()], weights=[1.0], spacing=6, optimizer="adam", lr=0.1, max_epochs=3).cuda()
    fl.optimize(mov, tgt, debug=False)
    vf, rf = fl.invert_flow(20, 1e-4)
    assert torch.equal(vf, tr.invert_flow(fl.flow, 20, 1e-4)) and rf.shape == (1, 1) + shape
    # carrying a label map back: nearest-neighbour resampling through the inverse
    labels = (tgt > tgt.mean()).float()
    carried = tr.resample(labels, flow=v, interpolation="nearest")
    assert carried.shape == labels.shape and set(carried.unique().tolist()) <= {0.0, 1.0}
