"""GPU checks of the composed warp (trx_affine_flow_warp, trx_affine_flow_warp_backward), the B-spline mutual-information loop over it
(trx_bspline_mi_run_grids) and initial= of the public interface, against tests/affine_flow_ref.py.  The shapes are the
smallest at which the kernels can still go wrong: odd sizes, W below one wave, more than one block per pair, B = 2 with a theta per pair, 2
channels, 2-D.  tests/test_affine_flow_host.py asserts the conditions on the inputs (which voxels the backward comparisons leave out, how many
samples leave the moving field of view, that the arbiter's loss curves descend)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import affine_flow_ref as fr
import affine_mi_grids_ref as gref
import phantoms as ph
from test_affine_flow_host import check_refusals
from test_gpu_bspline import _Guarded
from test_gpu_mi import _arbiter_pair, _loop_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


@functools.lru_cache(maxsize=None)
def _reference(name, world):
    """(forward fp64, backward fp64, backward fp32 on the CPU, kept voxels [2,1,*S_t]) of a case: computed once, shared, never written to."""
    x, theta, flow, go = fr.case(name, world)
    scale = fr.case_scale(name, world)
    keep = fr.kept_voxels(theta, flow, x.shape[2:], scale)[:, None]
    return (fr.warp(x, theta, flow, scale), fr.backward(x, theta, flow, go, scale), fr.backward(x, theta, flow, go, scale, torch.float32).double(), keep)


def _scale32(name, world):
    return fr.case_scale(name, world).float()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. forward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("name", list(fr.CASES))
def test_forward_against_the_fp64_reference(tr, name, world):
    """<= 1e-5 of the moving range, the bar of trx_affine_warp_grids."""
    x, theta, flow, _ = fr.case(name, world)
    want = _reference(name, world)[0]
    got = tr.affine_flow_warp(x.cuda(), theta.cuda(), flow.cuda(), _scale32(name, world) if world else None)
    assert got.shape == want.shape and got.dtype == torch.float32
    err, bar = (got.cpu().double() - want).abs().max().item(), 1e-5 * (x.max() - x.min()).item()
    print(f"{name} {'world' if world else 'ones'}: forward err {err:.3e} bar {bar:.3e}")
    assert err <= bar
    assert torch.equal(got, tr.affine_flow_warp(x.cuda(), theta.cuda(), flow.cuda(), _scale32(name, world) if world else None))
    assert torch.equal(got[:, 1:], tr.affine_flow_warp(x[:, 1:].cuda(), theta.cuda(), flow.cuda(), _scale32(name, world) if world else None))   # channels share coordinates


@pytest.mark.parametrize("name", list(fr.CASES))
def test_zero_flow_is_the_cross_lattice_affine_warp(tr, name):
    """flow = 0 against trx_affine_warp_grids, within the forward bar (the coordinates are formed differently: closed form against tables)."""
    x, theta, flow, _ = fr.case(name, True)
    scale = _scale32(name, True)
    got = tr.affine_flow_warp(x.cuda(), theta.cuda(), torch.zeros_like(flow).cuda(), scale)
    pair_mg = tr._engine._moving_grid(tuple(x.shape[2:]), scale)
    xc, B, C, nd = x.cuda().contiguous(), x.shape[0], x.shape[1], x.dim() - 2
    from torchregister_amd import _lib
    v = _lib.Volumes()
    v.moving, v.moving_stride, v.ndim, v.B = xc.data_ptr(), xc[0].numel(), nd, B
    v.D, v.H, v.W = tr._engine._dhw(tuple(flow.shape[2:]))
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    want = torch.empty_like(got)
    _lib.check(_lib.load().trx_affine_warp_grids(ctypes.byref(v), ctypes.byref(pair_mg), _lib.ptr(th), C, _lib.ptr(want), _lib.current_stream(xc.device)),
               "trx_affine_warp_grids")
    err, bar = (got - want).abs().max().item(), 1e-5 * (x.max() - x.min()).item()
    print(f"{name}: flow = 0 against trx_affine_warp_grids: {err:.3e} bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("name", list(fr.CASES))
def test_identity_on_equal_lattices_is_the_flow_warp(tr, name):
    """theta = I, equal lattices, scale 1 against trx_flow_warp, within the forward bar."""
    _, _, flow, _ = fr.case(name)
    nd = flow.shape[1]
    x = torch.cat([torch.cat([ph.blobs(tuple(flow.shape[2:]), 40 + 2 * b + c) for c in range(2)], dim=1) for b in range(2)]).cuda()
    eye = torch.eye(nd, nd + 1)[None].expand(2, -1, -1).cuda()
    got, want = tr.affine_flow_warp(x, eye, flow.cuda()), tr._engine.flow_warp(x, flow.cuda())
    err, bar = (got - want).abs().max().item(), 1e-5 * (x.max() - x.min()).item()
    print(f"{name}: theta = I against trx_flow_warp: {err:.3e} bar {bar:.3e}")
    assert err <= bar


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. backward
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("name", list(fr.CASES))
def test_backward_against_the_fp64_reference(tr, name, world):
    """On the kept voxels, the bar tests/test_gpu_flow.py holds trx_flow_warp_backward to: max(1e-4 max |d64|, 2 x the reference's own fp32 - fp64
    gap).  The same bits on two consecutive calls, and through autograd."""
    x, theta, flow, go = fr.case(name, world)
    _, d64, d32, keep = _reference(name, world)
    scale = _scale32(name, world) if world else None
    got = tr.affine_flow_warp_backward(x.cuda(), theta.cuda(), flow.cuda(), go.cuda(), scale)
    assert got.shape == flow.shape and got.dtype == torch.float32
    k = keep.expand_as(d64)
    err = (got.cpu().double() - d64)[k].abs().max().item()
    gap = (d32 - d64)[k].abs().max().item()
    bar = max(1e-4 * d64.abs().max().item(), 2.0 * gap)
    print(f"{name} {'world' if world else 'ones'}: backward err {err:.3e} bar {bar:.3e} (reference fp32 - fp64 {gap:.3e}, max |d| {d64.abs().max().item():.3e})")
    assert err <= bar
    assert torch.equal(got, tr.affine_flow_warp_backward(x.cuda(), theta.cuda(), flow.cuda(), go.cuda(), scale))
    fl = flow.cuda().requires_grad_()
    tr.affine_flow_warp(x.cuda(), theta.cuda(), fl, scale).backward(go.cuda())
    assert torch.equal(fl.grad, got)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, name, capacity=fr.ITERS):
    _, _, spacing, optimizer, lr, _, lam = fr.LOOPS[name]
    mov, tgt, theta, mask, _, ctrl0 = fr.loop_setup(name)
    return tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=ctrl0, capacity=capacity, bending_weight=lam, mi=dict(bins=32),
                            mask=None if mask is None else mask.cuda(), initial=theta)


@pytest.mark.parametrize("name", list(fr.LOOPS))
def test_loop_vs_torch_autograd(tr, name):
    """trx_bspline_mi_run_grids, 10 iterations from a random control tensor of amplitude 0.2, against the arbiter in fp64 with the bars of the
    other loops (2e-5 of the loss, 2e-4 on the parameters, or 4 x the arbiter's own fp32 - fp64 gap)."""
    r64, r32 = fr.loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    s = _solver(tr, name)
    theta0 = s.initial.clone()
    s.run(fr.ITERS)
    torch.cuda.synchronize()
    assert int(s.step[0]) == fr.ITERS and torch.equal(s.initial, theta0)
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), r64, r32, f"bspline grids {name}")
    tshape, _, spacing = fr.LOOPS[name][:3]
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, tshape, spacing))


def test_split_runs_give_the_bits_of_one_run(tr):
    one, two = _solver(tr, "adam"), _solver(tr, "adam")
    one.run(10)
    two.run(4)
    two.run(6)
    torch.cuda.synchronize()
    assert torch.equal(one.losses, two.losses) and torch.equal(one.ctrl, two.ctrl) and torch.equal(one.flow, two.flow) and torch.equal(one.adam_v, two.adam_v)


def test_identity_on_equal_lattices_tracks_the_one_lattice_loop(tr):
    """theta = I on equal lattices: the loss curve and the control tensor stay within the loop bars of trx_bspline_mi_run's arbiter (in fp64 the two
    definitions coincide), and next to trx_bspline_mi_run itself."""
    shape, spacing, iters = (12, 14, 16), 4, 10
    mov, tgt, p0, _, r64, r32 = _arbiter_pair((shape, "adam", 0.1, False, spacing, False, 0.0, 0.0, iters))
    kw = dict(optimizer="adam", lr=0.1, init=p0, capacity=iters, mi=dict(bins=32))
    grids = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, initial=torch.eye(3, 4)[None], **kw)
    plain = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, **kw)
    grids.run(iters)
    plain.run(iters)
    torch.cuda.synchronize()
    _loop_bars(grids.losses[0].cpu().numpy(), grids.ctrl.cpu().numpy(), r64, r32, "bspline grids at theta = I")
    _loop_bars(grids.losses[0].cpu().numpy(), grids.ctrl.cpu().numpy(), (plain.losses[0].cpu().double().numpy(), plain.ctrl.cpu().double().numpy()), r32,
               "bspline grids at theta = I against trx_bspline_mi_run")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. memory contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["9x11x13", "17x19"])
def test_warps_stay_inside_their_buffers(tr, name):
    """out, dflow and the moving volume between canaries: nothing outside them changes, the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    x, theta, flow, go = (t.cuda() for t in fr.case(name, True))
    scale = _scale32(name, True)
    B, C, nd = x.shape[0], x.shape[1], x.dim() - 2
    tshape, mshape = tuple(flow.shape[2:]), tuple(x.shape[2:])
    gmov = _Guarded(x.numel() * 4, 0x69)
    gmov.region.copy_(x.contiguous().view(torch.uint8).reshape(-1))
    out, dflow = _Guarded(B * C * math.prod(tshape) * 4, 0x96), _Guarded(B * nd * math.prod(tshape) * 4, 0xC3)
    v = _lib.Volumes()
    v.moving, v.moving_stride, v.ndim, v.B = gmov.region.data_ptr(), C * math.prod(mshape), nd, B
    v.D, v.H, v.W = tr._engine._dhw(tshape)
    mg = tr._engine._moving_grid(mshape, scale)
    th = tr._engine.pad_theta(theta.reshape(B, -1), nd)
    keep = [t.clone() for t in (th, flow, go)]
    stream = _lib.current_stream(torch.device("cuda"))
    _lib.check(lib.trx_affine_flow_warp(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), _lib.ptr(flow), C, _lib.ptr(out.region), stream), "trx_affine_flow_warp")
    _lib.check(lib.trx_affine_flow_warp_backward(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), _lib.ptr(flow), C, _lib.ptr(go), _lib.ptr(dflow.region), stream),
               "trx_affine_flow_warp_backward")
    torch.cuda.synchronize()
    for buf, what in ((out, "out"), (dflow, "dflow"), (gmov, "moving")):
        buf.check(what)
    assert torch.equal(out.floats((B, C) + tshape), tr.affine_flow_warp(x, theta, flow, scale))
    assert torch.equal(dflow.floats((B, nd) + tshape), tr.affine_flow_warp_backward(x, theta, flow, go, scale))
    assert torch.equal(gmov.floats(tuple(x.shape)), x) and all(torch.equal(a, b) for a, b in zip((th, flow, go), keep))


def test_loop_stays_inside_its_buffers(tr):
    """The workspace at exactly trx_bspline_mi_workspace_bytes(target lattice) - one byte less is TRX_ERR_WORKSPACE -, the moving volume and the
    state between canaries; theta is unchanged after the run; the bits of the solver."""
    from torchregister_amd import _lib
    lib = _lib.load()
    name, iters = "adam", 3
    tshape, mshape, spacing, optimizer, lr = fr.LOOPS[name][:5]
    mov, tgt, theta, _, _, ctrl0 = fr.loop_setup(name)
    mov, tgt = mov.cuda(), tgt.cuda()
    want = tr.BSplineSolver(mov, tgt, spacing, optimizer=optimizer, lr=lr, init=ctrl0, capacity=iters, mi=dict(bins=32), initial=theta)
    G = want.grid
    gmov = _Guarded(mov.numel() * 4, 0x69)
    gmov.region.copy_(mov.view(torch.uint8).reshape(-1))
    pair = tr._engine._GridPair(gmov.floats(tuple(mov.shape)), tgt)
    vol, mg = pair.vol(), pair.grid()
    nctrl, nflow = 3 * math.prod(G) * 4, 3 * math.prod(tshape) * 4
    g = dict(ctrl=_Guarded(nctrl, 0x3C), adam_m=_Guarded(nctrl, 0x3C), adam_v=_Guarded(nctrl, 0x3C), flow=_Guarded(nflow, 0xA5), dflow=_Guarded(nflow, 0xC3),
             losses=_Guarded(iters * 4, 0x96), step=_Guarded(4, 0x96))
    for k in ("ctrl", "adam_m", "adam_v", "losses", "step"):
        g[k].region.copy_(getattr(want, k).contiguous().view(torch.uint8).reshape(-1))
    st = _lib.BSplineState()
    for k in g:
        setattr(st, k, g[k].region.data_ptr())
    st.losses_capacity, st.bending_weight = iters, 0.0
    th = _Guarded(48, 0x11)
    th.region.copy_(want.initial.view(torch.uint8).reshape(-1))
    ws_bytes = lib.trx_bspline_mi_workspace_bytes(3, 1, *tshape, spacing, spacing, spacing, 32)
    assert ws_bytes == want.ws_bytes > 0
    ws = _Guarded(ws_bytes, 0x5A)
    d3 = (ctypes.c_int * 3)(spacing, spacing, spacing)
    run = lambda n: lib.trx_bspline_mi_run_grids(ctypes.byref(vol), ctypes.byref(mg), _lib.ptr(th.region), ctypes.byref(want.mi), ctypes.byref(want.opt),  # noqa: E731
                                                 ctypes.byref(st), d3, iters, _lib.ptr(ws.region), n, _lib.current_stream(torch.device("cuda")))
    assert run(ws_bytes - 1) == -3
    _lib.check(run(ws_bytes), "trx_bspline_mi_run_grids")
    torch.cuda.synchronize()
    for k in g:
        g[k].check(k)
    for buf, what in ((ws, "the workspace"), (gmov, "moving"), (th, "theta")):
        buf.check(what)
    assert torch.equal(th.region, want.initial.view(torch.uint8).reshape(-1)) and torch.equal(gmov.floats(tuple(mov.shape)), mov)
    want.run(iters)
    torch.cuda.synchronize()
    for k in ("ctrl", "adam_m", "adam_v", "losses", "step"):
        assert torch.equal(g[k].region, getattr(want, k).contiguous().view(torch.uint8).reshape(-1)), k
    assert int(want.step[0]) == iters


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stages(tr, levels=1):
    tshape, mshape = (16, 18, 20), (22, 20, 17)
    tvox, mvox = (1.5, 1.0, 1.0), (1.1, 0.9, 1.2)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    rigid = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6))
    rigid.optim(mov, tgt, lr=0.01, max_epochs=8, moving_voxel=mvox, target_voxel=tvox)
    reg = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4, levels=levels)
    return mov, tgt, rigid, reg


def test_register_bspline_through_an_initial_rigid(tr):
    """The test that fails without the feature (optim has no `initial` there): a rigid stage on two lattices, then the B-spline stage composed with it -
    the original moving image is sampled once."""
    mov, tgt, rigid, reg = _stages(tr)
    tshape = tuple(tgt.shape[2:])
    reg.optim(mov, tgt, lr=0.05, max_epochs=8, initial=rigid)
    ls = reg.losses.cpu().numpy()
    print(f"Register bspline + MILoss through an initial rigid: {ls[0, 0]:.5f} -> {ls[0, -1]:.5f}")
    assert ls.shape == (1, 8) and np.all(np.isfinite(ls)) and ls[0, -1] < ls[0, 0]
    assert torch.equal(reg.initial, rigid.theta) and reg.target_shape == tshape
    assert reg.theta.shape == (1, 3) + tshape and reg.final_theta.shape == (1, 3) + tshape and reg.control.shape[:2] == (1, 3)
    x = torch.cat([mov, mov * mov], dim=1)
    out = reg(x)
    assert out.shape == (1, 2) + tshape and torch.equal(out[:, :1], reg(mov))
    want = fr.warp(x.cpu(), rigid.theta.cpu(), reg.theta.cpu())
    err, bar = (out.cpu().double() - want).abs().max().item(), 1e-5 * (x.max() - x.min()).item()
    print(f"reg(x) against the reference's composed warp of reg.theta: {err:.3e} bar {bar:.3e}")
    assert err <= bar
    # the same run through the solver, and an effective theta tensor in place of the Register
    s = tr.BSplineSolver(mov, tgt, 4, optimizer="adam", lr=0.05, capacity=8, stop_crit=1e-4, keep_last=True, mi=dict(bins=32), initial=rigid.theta)
    s.run(8)
    assert torch.equal(reg.losses, s.losses) and torch.equal(reg.control, s.ctrl)
    again = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4)
    again.optim(mov, tgt, lr=0.05, max_epochs=8, initial=rigid.theta.clone())
    assert torch.equal(again.losses, reg.losses) and torch.equal(again(mov), reg(mov))
    # without initial the same object is the one-lattice flow path again, and two lattices are refused as before
    with pytest.raises(ValueError, match="lattice of its own"):
        reg.optim(mov, tgt, lr=0.05, max_epochs=2)
    reg.optim(tgt, tgt, lr=0.05, max_epochs=2)
    assert reg.initial is None and torch.equal(reg(tgt), tr._engine.flow_warp(tgt, reg.theta))


def test_register_two_levels_through_an_initial_rigid(tr):
    """levels=2 runs: each image gets its own pyramid, the coarse level runs with level_theta of the rigid result (replayed with the solver), and
    reg(x) uses the full-resolution theta."""
    from torchregister_amd.pyramid import level_theta
    mov, tgt, rigid, reg = _stages(tr, levels=2)
    tshape, mshape = tuple(tgt.shape[2:]), tuple(mov.shape[2:])
    reg.optim(mov, tgt, lr=0.05, max_epochs=[6, 6], initial=rigid)
    assert reg.level_shapes == tr.pyramid_shapes(tshape, 2) and reg.target_shape == tshape
    assert [tuple(ls.shape) for ls in reg.level_losses] == [(1, 6), (1, 6)] and all(bool(torch.isfinite(ls).all()) for ls in reg.level_losses)
    mc, tc = tr.pyramid(mov, 2, align_corners=True)[0], tr.pyramid(tgt, 2, align_corners=True)[0]
    coarse = tr.BSplineSolver(mc, tc, 4, optimizer="adam", lr=0.05, capacity=6, stop_crit=1e-4, keep_last=True, mi=dict(bins=32),
                              initial=level_theta(rigid.theta, tshape, tc.shape[2:], mshape, mc.shape[2:]))
    coarse.run(6)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    assert torch.equal(reg.initial, rigid.theta) and reg(mov).shape == (1, 1) + tshape
    want = fr.warp(mov.cpu(), rigid.theta.cpu(), reg.theta.cpu())
    assert (reg(mov).cpu().double() - want).abs().max().item() <= 1e-5 * (mov.max() - mov.min()).item()
