"""GPU checks of points and target-space images through the whole transform (trx_transform_points, trx_affine_then_flow_resample and the public interface
over them) against tests/chain_ref.py.  The shapes are the smallest at which the kernels can still go wrong: odd sizes with W
below one wave, unequal lattices, more than one block per pair, B = 2 with a theta per pair, 2 channels, 2-D, an axis of one voxel.
tests/test_chain_host.py asserts the conditions on the inputs (which voxels the comparisons leave out, how many samples leave the field of view).
Every test here fails without the feature: the functions do not exist."""
import ctypes
import math

import numpy as np
import pytest
import torch

import affine_flow_ref as afr
import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import chain_ref as cr
import flowops_ref as fr
import phantoms as ph
import spline_ref as sr
from conftest import bar
from test_chain_host import check_refusals
from test_gpu_bspline import _Guarded

pytestmark = pytest.mark.gpu

ORDERS = {0: "nearest", 1: "linear", 3: "cubic"}
CHAIN = {0: "flow_then_affine", 1: "affine_then_flow"}


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _cuda(t):
    return None if t is None else t.cuda()


def _point_lattices(name, which):
    """(from, to) of a case for chain `which`: the flow lives on the source lattice, which chain 0 starts from and chain 1 ends on."""
    out_shape, src_shape = cr.CASES[name][:2]
    return (src_shape, out_shape) if which == 0 else (out_shape, src_shape)


def _point_err(got, r32, r64, floor):
    """(largest difference to the fp64 restatement over the points that are not NaN there, the bar); the NaN points must agree."""
    nan = torch.isnan(r64).any(-1)
    assert torch.equal(torch.isnan(got).all(-1), nan) and torch.equal(torch.isnan(got).any(-1), nan)
    keep = ~nan
    return (got[keep].double() - r64[keep]).abs().max().item(), bar(r32[keep].numpy(), r64[keep].numpy(), floor)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. points
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", list(cr.CASES))
def test_points_against_the_restatement(tr, name, which):
    """P in {1, 63, 65, 1000}, both paddings: points on faces, several voxels outside the lattice and one NaN point against the fp64 restatement, within
    bar(restatement fp32, restatement fp64, 1e-5 x the largest lattice size); the NaN point gives NaN and its neighbours are untouched."""
    _, theta, flow = cr.case(name)
    a, b = _point_lattices(name, which)
    floor = 1e-5 * max(a + b)
    for P in cr.POINT_COUNTS:
        for padding in ("border", "zeros") if flow is not None else ("border",):
            p = cr.points_for(a, P, 100 + P, nan_at=17)
            r64, r32 = (cr.chain(p, theta, flow, a, b, which, padding, dt) for dt in (torch.float64, torch.float32))
            got = tr.transform_points(p.cuda(), theta=_cuda(theta), flow=_cuda(flow), from_shape=a, to_shape=b, chain=CHAIN[which], padding=padding).cpu()
            err, limit = _point_err(got, r32, r64, floor)
            print(f"{name} chain {which} P {P} {padding}: {err:.3e} bar {limit:.3e}")
            assert err <= limit
            if P > 17:      # the NaN point gives NaN, and the clean set gives the neighbours' bits
                assert bool(torch.isnan(got[0, 17]).all())
                clean = tr.transform_points(cr.points_for(a, P, 100 + P).cuda(), theta=_cuda(theta), flow=_cuda(flow), from_shape=a, to_shape=b,
                                            chain=CHAIN[which], padding=padding).cpu()
                keep = torch.ones(2, P, dtype=torch.bool)
                keep[0, 17] = False
                assert torch.equal(got[keep], clean[keep])


@pytest.mark.parametrize("padding", ["border", "zeros"])
@pytest.mark.parametrize("name", ["9x11x13", "2d", "1x12x20", "20x18x16"])
def test_points_at_lattice_points_without_theta_are_grid_plus_flow(tr, name, padding):
    """A weight of exactly 1 on the voxel's own corner: bit for bit, both paddings, both chains."""
    _, _, flow = cr.case(name)
    S = tuple(flow.shape[2:])
    grid = cr.lattice_points(S, 2, torch.float32)
    want = grid + flow.reshape(2, len(S), -1).transpose(1, 2)
    for which in (0, 1):
        got = tr.transform_points(grid.cuda(), flow=flow.cuda(), chain=CHAIN[which], padding=padding).cpu()
        assert torch.equal(got, want), which


def test_points_feed_the_positions_of_the_nearest_resample(tr):
    """transform_points at the target's lattice points gives the positions whose order-0 sample is tr.resample(..., 'nearest') on the kept voxels."""
    x, theta, flow = sr.case("composed")
    tshape, mshape = sr.CASES["composed"][:2]
    pos = tr.transform_points(cr.lattice_points(tshape, 2, torch.float32).cuda(), theta=theta.cuda(), flow=flow.cuda(), to_shape=mshape).cpu()
    pos = pos.flip(-1).reshape((2,) + tshape + (3,))
    got = sr.sample_nearest(x, pos)
    want = tr.resample(x.cuda(), theta=theta.cuda(), flow=flow.cuda(), interpolation="nearest").cpu()
    keep = sr.kept(sr.case_positions("composed"), mshape, nearest=True)[:, None].expand_as(want)
    assert torch.equal(got[keep], want[keep])
    print(f"positions of transform_points reproduce resample('nearest'): all voxels agree: {torch.equal(got, want)}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. images
# ---------------------------------------------------------------------------------------------------------------------------------------
def _image_cases():
    for name in cr.CASES:
        for order in ORDERS:
            for padding in ("border", "zeros") if cr.CASES[name][3] is not None else ("border",):
                yield name, order, padding


def _positions(name, padding):
    out_shape, src_shape = cr.CASES[name][:2]
    _, theta, flow = cr.case(name)
    return cr.image_positions(theta, flow, out_shape, src_shape, padding)


def _run(tr, name, order, padding, x=None):
    x0, theta, flow = cr.case(name)
    return tr.resample_affine_then_flow((x0 if x is None else x).cuda(), theta=_cuda(theta), flow=_cuda(flow), size=cr.CASES[name][0],
                                        interpolation=ORDERS[order], padding=padding).cpu()


@pytest.mark.parametrize("name,order,padding", list(_image_cases()))
def test_images_against_the_restatement(tr, name, order, padding):
    """Orders 1 and 3: within bar(restatement fp32, restatement fp64, 1e-5 x range) on the kept voxels; order 0: no kept voxel differs; voxels outside the
    field of view (orders 0, 3: beyond half a voxel; order 1: beyond a whole voxel, where the last corner has left) are exactly 0."""
    out_shape, src_shape = cr.CASES[name][:2]
    x = cr.case(name)[0]
    r64, r32 = cr.reference(name, order, padding)
    got = _run(tr, name, order, padding)
    pos = _positions(name, padding)
    assert got.shape == (2, 2) + out_shape and bool(torch.isfinite(got).all())
    fig = {}
    msgs, n_outside = cr.check_image(got, r64, r32, pos, src_shape, order, (x.max() - x.min()).item(), fig)
    print(f"{name} order {order} {padding}: {fig}")
    assert not msgs, msgs
    assert n_outside > 0


@pytest.mark.parametrize("name", ["9x11x13", "2d", "flow-only"])
def test_a_label_volume_comes_back_with_no_invented_value(tr, name):
    lab = cr.labels(cr.CASES[name][1])
    got = _run(tr, name, 0, "border", lab)
    values = set(got.unique().tolist())
    assert values <= set(float(v) for v in range(8)) and 0.0 in values and len(values) >= 7
    r64 = cr.resample(lab, *cr.case(name)[1:], cr.CASES[name][0], 0)
    keep = sr.kept(_positions(name, "border"), cr.CASES[name][1], nearest=True)[:, None].expand_as(got)
    assert torch.equal(got[keep].double(), r64[keep])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. against the existing kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("name,zero_flow", [("theta-only", False), ("9x11x13", True), ("2d", True)])
def test_without_a_flow_it_is_the_existing_resample(tr, name, order, zero_flow):
    """flow NULL or a zero flow: tr.resample(theta=, size=) for orders 0 and 3, affine_warp(size=) (resample 'linear') for order 1, within the bar of the
    restatement; the positions are formed by the same statements, so the bits are reported."""
    out_shape, src_shape = cr.CASES[name][:2]
    x, theta, flow = cr.case(name)
    fl = torch.zeros_like(flow).cuda() if zero_flow else None
    got = tr.resample_affine_then_flow(x.cuda(), theta=theta.cuda(), flow=fl, size=out_shape, interpolation=ORDERS[order]).cpu()
    want = tr.resample(x.cuda(), theta=theta.cuda(), size=out_shape, interpolation=ORDERS[order]).cpu()
    r64, r32 = (cr.resample(x, theta, None, out_shape, order, dtype=dt) for dt in (torch.float64, torch.float32))
    pos = cr.image_positions(theta, None, out_shape, src_shape)
    keep = sr.kept(pos, src_shape, nearest=order == 0)[:, None].expand_as(got)
    limit = bar(r32[keep].numpy(), r64[keep].numpy(), 1e-5 * (x.max() - x.min()).item())
    err = (got - want)[keep].abs().max().item()
    print(f"{name} order {order}{' zero flow' if zero_flow else ''}: |new - existing| {err:.3e} bar {limit:.3e}; bits agree: {torch.equal(got, want)}")
    assert err <= (0.0 if order == 0 else limit)


@pytest.mark.parametrize("order", list(ORDERS))
def test_with_the_identity_theta_it_is_the_existing_flow_resample(tr, order):
    """theta = I on equal lattices: tr.resample(flow=) within the bar on the kept voxels (q = unnorm(norm(y)) is y up to a rounding)."""
    name = "flow-only"
    S = cr.CASES[name][0]
    x, _, flow = cr.case(name)
    eye = torch.eye(3, 4)[None].expand(2, 3, 4).contiguous()
    got = tr.resample_affine_then_flow(x.cuda(), theta=eye.cuda(), flow=flow.cuda(), size=S, interpolation=ORDERS[order]).cpu()
    want = tr.resample(x.cuda(), flow=flow.cuda(), interpolation=ORDERS[order]).cpu()
    r64, r32 = (cr.resample(x, eye, flow, S, order, dtype=dt) for dt in (torch.float64, torch.float32))
    keep = sr.kept(cr.image_positions(eye, flow, S, S), S, nearest=order == 0)[:, None].expand_as(got)
    limit = bar(r32[keep].numpy(), r64[keep].numpy(), 1e-5 * (x.max() - x.min()).item())
    err = (got - want)[keep].abs().max().item()
    print(f"theta = I order {order}: |new - existing| {err:.3e} bar {limit:.3e}; bits agree: {torch.equal(got, want)}")
    assert err <= (0.0 if order == 0 else limit)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. determinism, isolation, memory
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x11x13", "20x18x16", "2d"])
def test_same_bits_on_every_call_for_every_channel_and_every_batch(tr, name):
    out_shape, src_shape = cr.CASES[name][:2]
    x, theta, flow = (t.cuda() for t in cr.case(name))
    for order in ORDERS:
        kw = dict(size=out_shape, interpolation=ORDERS[order])
        a = tr.resample_affine_then_flow(x, theta=theta, flow=flow, **kw)
        assert torch.equal(a, tr.resample_affine_then_flow(x, theta=theta, flow=flow, **kw))
        assert torch.equal(a[:, 1:], tr.resample_affine_then_flow(x[:, 1:], theta=theta, flow=flow, **kw))      # channels share coordinates
        assert torch.equal(a[:1], tr.resample_affine_then_flow(x[:1], theta=theta[:1], flow=flow[:1], **kw))    # pair 0 alone
        assert torch.equal(a[1:], tr.resample_affine_then_flow(x[1:], theta=theta[1:], flow=flow[1:], **kw))
    for which in (0, 1):
        a_, b_ = _point_lattices(name, which)
        p = cr.points_for(a_, 65, 7).cuda()
        kw = dict(from_shape=a_, to_shape=b_, chain=CHAIN[which])
        out = tr.transform_points(p, theta=theta, flow=flow, **kw)
        assert torch.equal(out, tr.transform_points(p, theta=theta, flow=flow, **kw))
        assert torch.equal(out[:1], tr.transform_points(p[:1], theta=theta[:1], flow=flow[:1], **kw))
        assert torch.equal(out[0], tr.transform_points(p[0], theta=theta[:1], flow=flow[:1], **kw))      # [P, nd]
        # a theta and a flow of batch 1 serve every pair
        assert torch.equal(tr.transform_points(p, theta=theta[:1], flow=flow[:1], **kw)[1], tr.transform_points(p[1:], theta=theta[:1], flow=flow[:1], **kw)[0])


@pytest.mark.parametrize("name", ["9x11x13", "2d", "1x12x20"])
def test_calls_stay_inside_their_buffers(tr, name):
    """Both entry points called directly with every output inside a guarded buffer: the canaries are intact, the results are the wrappers', and
    trx_transform_points may write over its own input."""
    from torchregister_amd import _lib
    lib = _lib.load()
    out_shape, src_shape = cr.CASES[name][:2]
    nd = len(out_shape)
    x, theta, flow = (t.cuda() for t in cr.case(name))
    th = tr._engine.pad_theta(theta, nd)
    stream = _lib.current_stream(torch.device("cuda"))
    size = lambda s: (ctypes.c_int * 3)(*((1,) * (3 - len(s)) + tuple(s)))  # noqa: E731
    for order in ORDERS:
        src = tr.spline_coefficients(x) if order == 3 else x
        g = _Guarded(2 * 2 * math.prod(out_shape) * 4, 0x5A)
        rc = lib.trx_affine_then_flow_resample(_lib.ptr(src), src[0].numel(), size(src_shape), _lib.ptr(th), _lib.ptr(flow), nd, 2, 2, size(out_shape), order, 1,
                                               ctypes.c_void_p(g.region.data_ptr()), stream)
        torch.cuda.synchronize()
        assert rc == 0
        g.check(f"out of order {order}")
        assert torch.equal(g.floats((2, 2) + out_shape), tr.resample_affine_then_flow(x, theta=theta, flow=flow, size=out_shape, interpolation=ORDERS[order]))
    for which in (0, 1):
        a, b = _point_lattices(name, which)
        p = cr.points_for(a, 65, 7, nan_at=17).cuda()
        want = tr.transform_points(p, theta=theta, flow=flow, from_shape=a, to_shape=b, chain=CHAIN[which])
        g = _Guarded(p.numel() * 4, 0xA5)
        g.floats(tuple(p.shape)).copy_(p)
        ptr = ctypes.c_void_p(g.region.data_ptr())
        rc = lib.trx_transform_points(ptr, ptr, nd, 2, 65, _lib.ptr(th), _lib.ptr(flow), size(a), size(b), which, 1, stream)      # in place
        torch.cuda.synchronize()
        assert rc == 0
        g.check(f"points of chain {which}")
        got = g.floats(tuple(p.shape))
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(), want.nan_to_num())


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. what it is for: landmarks and target-space images through a finished registration, both ways
# ---------------------------------------------------------------------------------------------------------------------------------------
def _interior_points(shape, P=400, seed=21, margin=3.0):
    S = torch.tensor(shape, dtype=torch.float32)
    return (torch.rand((1, P, len(shape)), generator=torch.Generator().manual_seed(seed)) * (S - 1.0 - 2.0 * margin) + margin)


def _check_registration(tr, reg, tshape, mshape, what):
    """transform_points, inverse_transform and to_moving of a finished Register against the restatement applied to its own pieces."""
    theta = reg.initial if reg.mode == "flow" else reg.theta
    theta = None if theta is None else theta.detach().cpu()
    flow = reg.theta.detach().cpu() if reg.mode == "flow" else None
    floor = 1e-5 * max(tshape + mshape)
    assert reg.moving_shape == mshape
    # forward: target voxels to moving voxels, anywhere
    p = cr.points_for(tshape, 1000, 31, B=1)
    got = reg.transform_points(p.cuda()).cpu()
    r64, r32 = (cr.chain(p, theta, flow, tshape, mshape, 0, dtype=dt) for dt in (torch.float64, torch.float32))
    err, limit = _point_err(got, r32, r64, floor)
    print(f"{what}: transform_points {err:.3e} bar {limit:.3e}")
    assert err <= limit
    # the pieces of the inverse
    th_inv, fl_inv, res = reg.inverse_transform()
    if theta is None:
        assert th_inv is None
    else:
        assert torch.equal(th_inv, tr.invert_theta(theta))
    if flow is None:
        assert fl_inv is None and res is None
    else:
        assert fl_inv.shape == flow.shape
        rr = fr.right_residual(flow, fl_inv.cpu()).max().item()
        print(f"{what}: |v + Sb(u, y + v)| of the inverted flow {rr:.3e}" + ("" if res is None else f", largest last update {res.max().item():.3e}"))
        if res is not None:      # the fixed-point inverse: converged everywhere, and a right inverse to tol + the fp32 slack of tests/flowops_ref.py
            assert bool((res <= fr.TOL).all()) and rr <= fr.TOL + fr.SLACK
    fl_inv = None if fl_inv is None else fl_inv.cpu()
    # inverse points against the restatement on the SAME pieces
    q = cr.points_for(mshape, 1000, 32, B=1)
    got = reg.transform_points(q.cuda(), inverse=True).cpu()
    r64, r32 = (cr.chain(q, th_inv, fl_inv, mshape, tshape, 1, dtype=dt) for dt in (torch.float64, torch.float32))
    err, limit = _point_err(got, r32, r64, floor)
    print(f"{what}: transform_points(inverse=True) {err:.3e} bar {limit:.3e}")
    assert err <= limit
    # to_moving against the restatement on the same pieces
    x = ph.blobs(tshape, 77) + 0.3 * torch.rand((1, 1) + tshape, generator=torch.Generator().manual_seed(5))
    x = torch.cat([x, cr.labels(tshape)[:1, :1]], dim=1)
    pos = cr.image_positions(th_inv, fl_inv, mshape, tshape)
    for order in ORDERS:
        got = reg.to_moving(x.cuda(), interpolation=ORDERS[order]).cpu()
        assert got.shape == (1, 2) + mshape
        r64, r32 = (cr.resample(x, th_inv, fl_inv, mshape, order, dtype=dt) for dt in (torch.float64, torch.float32))
        keep = sr.kept(pos, tshape, nearest=order == 0)[:, None].expand_as(got)
        if order == 0:
            assert torch.equal(got[keep].double(), r64[keep]) and set(got[:, 1].unique().tolist()) <= set(float(v) for v in range(8))
        else:
            err, limit = (got.double() - r64)[keep].abs().max().item(), bar(r32[keep].numpy(), r64[keep].numpy(), 1e-5 * (x.max() - x.min()).item())
            print(f"{what}: to_moving order {order} {err:.3e} bar {limit:.3e}")
            assert err <= limit
    # there and back: interior points return to within twice the fp64 restatement's round trip on the same theta and flow, plus the point bar
    p = _interior_points(tshape)
    back = reg.transform_points(reg.transform_points(p.cuda()), inverse=True).cpu()
    if flow is None:
        v64 = None
    elif res is None:
        v64 = fl_inv.double()      # diffeomorphic: the inverse is exp(-velocity), a given field - the restatement's round trip uses it as it is
    else:
        v64 = fr.invert(flow.double(), fr.ITERATIONS, fr.TOL)[0]
    th64 = None if theta is None else tr.invert_theta(theta)
    fwd64 = cr.chain(p, theta, flow, tshape, mshape, 0)
    back64 = cr.chain(fwd64, th64, v64, mshape, tshape, 1)
    back32 = cr.chain(cr.chain(p, theta, flow, tshape, mshape, 0, dtype=torch.float32), th64, None if v64 is None else v64.float(), mshape, tshape, 1, dtype=torch.float32)
    e64 = (back64 - p.double()).abs().max().item()
    limit = 2.0 * e64 + bar(back32.numpy(), back64.numpy(), floor)
    err = (back.double() - p.double()).abs().max().item()
    print(f"{what}: there and back {err:.3e} voxels; the fp64 restatement's round trip {e64:.3e}, limit {limit:.3e}")
    assert err <= limit


def test_register_through_an_initial_affine_both_ways(tr):
    """affine_flow_ref's loop phantom, a short ffd.optim(..., initial=theta): the multimodal pipeline's transform carries points both ways and an image
    from the target lattice onto the moving one, which Register.invert_flow() still refuses."""
    tshape, mshape = afr.LOOPS["adam"][:2]
    mov, tgt, theta, _, _, _ = afr.loop_setup("adam")
    ffd = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4)
    ffd.optim(mov.cuda(), tgt.cuda(), lr=0.05, max_epochs=6, initial=theta)
    assert ffd.target_shape == tshape and ffd.moving_shape == mshape and ffd.theta.abs().max().item() > 0.01
    with pytest.raises(ValueError, match="initial"):
        ffd.invert_flow()
    _check_registration(tr, ffd, tshape, mshape, "flow through initial=")
    # the new kernel is the one that ran: to_moving is resample_affine_then_flow of the pieces
    th_inv, fl_inv, _ = ffd.inverse_transform()
    x = tgt.cuda()
    assert torch.equal(ffd.to_moving(x, "nearest"), tr.resample_affine_then_flow(x, theta=th_inv, flow=fl_inv, size=mshape, interpolation="nearest"))


def test_register_affine_both_ways(tr):
    tshape, mshape = (16, 18, 20), (22, 20, 17)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    reg = tr.Register("affine", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=aref.theta0(3))
    reg.optim(mov, tgt, lr=0.005, max_epochs=4, moving_voxel=(1.1, 0.9, 1.2), target_voxel=(1.5, 1.0, 1.0))
    _check_registration(tr, reg, tshape, mshape, "affine")
    x = tgt
    assert torch.equal(reg.to_moving(x, "cubic"), tr.resample(x, theta=tr.invert_theta(reg.theta).float(), size=mshape, interpolation="cubic"))


@pytest.mark.parametrize("diffeomorphic", [False, True])
def test_register_flow_both_ways(tr, diffeomorphic):
    """Flow without initial= (one lattice): the fixed-point inverse, or exp(-velocity) under diffeomorphic=True."""
    from oracle import compose
    shape = (16, 18, 20)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, ph.flow_field(shape)).cuda()
    reg = tr.Register("flow", criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, optimizer="adam", diffeomorphic=diffeomorphic)
    reg.optim(mov, tgt.cuda(), lr=0.1, max_epochs=8)
    _check_registration(tr, reg, shape, shape, "diffeomorphic flow" if diffeomorphic else "flow")
    _, fl_inv, res = reg.inverse_transform()
    if diffeomorphic:
        assert res is None and torch.equal(fl_inv, reg.inverse_flow)
    else:
        v, r = reg.invert_flow()
        assert torch.equal(fl_inv, v) and torch.equal(res, r)
    assert torch.equal(reg.to_moving(tgt.cuda(), "nearest"), tr.resample(tgt.cuda(), flow=fl_inv, interpolation="nearest"))
