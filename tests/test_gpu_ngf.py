"""Normalised gradient field criterion on the GPU: trx_ngf_loss_grad against its CPU restatement (tests/ngf_ref.py), its bit-level promises, its
buffers, the Python face, trx_bspline_ngf_run against the CPU reference loop of tests/test_ngf_host.py, and Register end to end.

Bars follow tests/test_gpu_mi.py: error against the fp64 restatement <= 4 x (the restatement's own fp32 - fp64 gap on that case) + a floor - 1e-6 |alpha|
for the loss, 1e-6 max|grad64| for the gradient; loops: max(2e-5 max|l64|, 4 gap) for the loss curve, max(2e-4, 4 gap) for the control tensor.  Every
case prints error, gap and bar (pytest -s; kept in profiles/ngf_gpu_tests.txt)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import affine_flow_ref as fr
import bspline_ref
import ngf_ref
import phantoms as ph
import test_ngf_host as host
from test_gpu_bspline import _Guarded

pytestmark = pytest.mark.gpu

VOXEL = host.VOXEL


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _images(shape, B=1, seed=0):
    """target: a blob phantom; warped: another blob phantom plus a ripple, through the non-monotone map 4x(1 - x) (tests/test_gpu_mi.py::_images)."""
    tgt = torch.cat([ph.blobs(shape, 31 + 7 * b + seed) for b in range(B)])
    w = torch.cat([ph.blobs(shape, 32 + 7 * b + seed) + 0.05 * ph.vol(shape, 0.029, "cos") for b in range(B)])
    return tgt, (4.0 * w * (1.0 - w)).float()


def _ball(shape, B=1, r=0.42):
    idx = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) - (s - 1) / 2 for s in shape], indexing="ij")
    return (sum((i / max(r * s, 0.6)) ** 2 for i, s in zip(idx, shape)) <= 1.0)[None, None].expand(B, 1, *shape).clone()


def _check(tr, tgt, wrp, eps, alpha, voxel, mask, what):
    """One call against the restatement; returns the kernel's (loss, grad)."""
    l64, g64 = host.autograd_grad(tgt, wrp, eps, voxel, mask, alpha, torch.float64)
    l32, g32 = host.autograd_grad(tgt, wrp, eps, voxel, mask, alpha, torch.float32)
    loss, grad = tr.ngf_loss_grad(tgt.cuda(), wrp.cuda(), eps.cuda(), alpha, voxel, True, None if mask is None else mask.cuda())
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    for b in range(tgt.shape[0]):
        gap, err = abs(l32[b].item() - l64[b].item()), abs(loss[b].item() - l64[b].item())
        bar = 4.0 * gap + 1e-6 * abs(alpha)
        print(f"{what} pair {b}: loss {l64[b].item():.6f} err {err:.2e} (fp32 gap {gap:.2e}, bar {bar:.2e})")
        assert err <= bar, (what, b, err, bar)
        gmax = g64[b].abs().max().item()
        ggap = (g32[b].double() - g64[b]).abs().max().item()
        gerr = (grad[b].double().cpu() - g64[b]).abs().max().item()
        gbar = 4.0 * ggap + 1e-6 * gmax
        print(f"{what} pair {b}: max|grad| {gmax:.3e} err {gerr:.2e} (fp32 gap {ggap:.2e}, bar {gbar:.2e})")
        assert gerr <= gbar, (what, b, gerr, gbar)
    return loss, grad


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. trx_ngf_loss_grad against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 6, 7), (2, 3, 130), (1, 9, 70), (9, 17, 65), (20, 40, 70), (13, 17), (1, 300)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_match_the_restatement(tr, shape):
    """5x6x7: less than a block; 2x3x130: rows crossing 64 and 128 lanes; 1x9x70: D = 1 in 3-D; 20x40x70 = 56000 voxels: 28 chunks of 2048, the last
    one partial; 13x17 and 1x300: 2-D.  Fitted eps."""
    tgt, wrp = _images(shape)
    _check(tr, tgt, wrp, ngf_ref.fit_eps(tgt, wrp), 1.0, None, None, f"{shape}")


def test_three_pairs_with_three_eps_alpha_and_voxel_sizes(tr):
    tgt, wrp = _images((9, 17, 65), B=3)
    eps = ngf_ref.fit_eps(tgt, wrp) * torch.tensor([[1.0, 1.0], [0.25, 2.0], [3.0, 0.1]])
    _check(tr, tgt, wrp, eps, 2.5, None, None, "B=3 alpha=2.5")
    _check(tr, tgt, wrp, ngf_ref.fit_eps(tgt, wrp, voxel=VOXEL), 2.5, VOXEL, None, "B=3 voxel")
    t2, w2 = _images((13, 17), B=2)
    _check(tr, t2, w2, ngf_ref.fit_eps(t2, w2, voxel=(3.0, 0.7)), -1.5, (3.0, 0.7), None, "2-D voxel (3.0, 0.7)")


def test_masks_a_ball_a_single_voxel_and_an_empty_one(tr):
    shape = (9, 17, 65)
    tgt, wrp = _images(shape, B=3)
    mask = _ball(shape, B=3)
    mask[1] = False
    mask[1, 0, 4, 8, 30] = True      # one voxel
    mask[2] = False                  # none: loss and gradient 0, the other pairs untouched
    eps = ngf_ref.fit_eps(tgt, wrp)
    loss, grad = _check(tr, tgt, wrp, eps, 2.5, None, mask, "masks")
    assert loss[2].item() == 0.0 and torch.count_nonzero(grad[2]).item() == 0
    alone, galone = tr.ngf_loss_grad(tgt[:2].cuda(), wrp[:2].cuda(), eps[:2].cuda(), 2.5, None, True, mask[:2].cuda())
    assert torch.equal(alone, loss[:2]) and torch.equal(galone, grad[:2])
    reach = host.stencil_reach(mask).cuda()
    assert torch.count_nonzero(grad[~reach]).item() == 0      # q is 0 outside the mask: nothing beyond the face neighbours of its voxels
    assert torch.count_nonzero(grad[1]).item() <= 7
    _check(tr, tgt, wrp, ngf_ref.fit_eps(tgt, wrp, voxel=VOXEL, mask=mask), 1.0, VOXEL, mask, "masks + voxel")
    t2, w2 = _images((13, 17))
    _check(tr, t2, w2, ngf_ref.fit_eps(t2, w2), 1.0, None, _ball((13, 17)), "2-D ball")


def test_a_constant_image_and_zero_eps(tr):
    """a b == 0 everywhere: r = 0 by the select - loss == alpha, gradient 0, no NaN; and eps = 0 against a real image: finite wherever it has an edge."""
    tgt, wrp = _images((5, 6, 7), B=2)
    const = torch.full_like(wrp, 0.37)
    eps = ngf_ref.fit_eps(tgt, const)
    assert bool((eps[:, 1] == 0).all())
    loss, grad = tr.ngf_loss_grad(tgt.cuda(), const.cuda(), eps.cuda(), 2.5)
    assert loss.cpu().tolist() == [2.5, 2.5] and torch.count_nonzero(grad).item() == 0
    assert torch.equal(tr.ngf_edge_parameters(tgt.cuda(), const.cuda()).cpu()[:, 1], eps[:, 1])
    _check(tr, tgt, wrp, torch.zeros(2, 2), 1.0, None, None, "eps = 0")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(20, 40, 70), (13, 17)], ids=["3d", "2d"])
def test_bits(tr, shape):
    """Two calls give the same bits; a pair alone gives the bits it has in a batch; an all-ones mask gives the bits of no mask; a loss-only call gives
    the bits of the call with a gradient; with a mask the gradient is 0 beyond the reach of the mask's stencils."""
    B = 3
    tgt, wrp = (t.cuda() for t in _images(shape, B=B))
    eps = tr.ngf_edge_parameters(tgt, wrp) * torch.tensor([[1.0, 1.0], [0.5, 2.0], [2.0, 0.5]], device="cuda")
    voxel = VOXEL[-len(shape):]
    loss, grad = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel)
    again, gagain = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel)
    assert torch.equal(loss, again) and torch.equal(grad, gagain)
    for b in range(B):
        one, gone = tr.ngf_loss_grad(tgt[b:b + 1], wrp[b:b + 1], eps[b:b + 1], 2.5, voxel)
        assert torch.equal(one, loss[b:b + 1]) and torch.equal(gone, grad[b:b + 1]), b
    ones, gones = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel, True, torch.ones_like(tgt, dtype=torch.uint8))
    assert torch.equal(ones, loss) and torch.equal(gones, grad)
    only, none = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel, need_grad=False)
    assert none is None and torch.equal(only, loss)
    mask = _ball(shape, B=B).cuda()
    mloss, mgrad = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel, True, mask)
    monly, _ = tr.ngf_loss_grad(tgt, wrp, eps, 2.5, voxel, False, mask)
    assert torch.equal(monly, mloss) and not torch.equal(mloss, loss)
    assert torch.count_nonzero(mgrad[~host.stencil_reach(mask)]).item() == 0 and torch.count_nonzero(mgrad[mask]).item() > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. buffers and status codes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,shape,masked", [(2, (12, 14, 16), False), (1, (20, 40, 70), True), (3, (13, 17), True)])
def test_calls_stay_inside_their_buffers(tr, B, shape, masked):
    """The workspace at exactly trx_ngf_workspace_bytes, loss and grad at their sizes: canaries intact, bits of the wrapper."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd = len(shape)
    dhw = (1,) * (3 - nd) + shape
    tgt, wrp = (t.cuda() for t in _images(shape, B=B))
    eps = tr.ngf_edge_parameters(tgt, wrp)
    mask = _ball(shape, B=B).to(device="cuda", dtype=torch.uint8).contiguous() if masked else None
    ws_bytes = lib.trx_ngf_workspace_bytes(nd, B, *dhw)
    assert ws_bytes > 0
    ws, loss, grad = _Guarded(ws_bytes, 0x5A), _Guarded(B * 4, 0xA5), _Guarded(B * math.prod(shape) * 4, 0xC3)
    cfg = host.ngf_cfg(_lib, 1.0, eps.data_ptr(), VOXEL[-nd:], None if mask is None else mask.data_ptr())
    stream = _lib.current_stream(torch.device("cuda"))
    rc = lib.trx_ngf_loss_grad(_lib.ptr(tgt), _lib.ptr(wrp), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(loss.region), _lib.ptr(grad.region),
                               _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_ngf_loss_grad")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (loss, "loss"), (grad, "grad")):
        buf.check(what)
    want_l, want_g = tr.ngf_loss_grad(tgt, wrp, eps, 1.0, VOXEL[-nd:], True, mask)
    assert torch.equal(loss.floats((B,)), want_l) and torch.equal(grad.floats(wrp.shape), want_g)
    only = _Guarded(B * 4, 0x3C)
    rc = lib.trx_ngf_loss_grad(_lib.ptr(tgt), _lib.ptr(wrp), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(only.region), None, _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_ngf_loss_grad")
    torch.cuda.synchronize()
    ws.check("the workspace")
    only.check("loss")
    assert torch.equal(only.floats((B,)), want_l)


def test_status_codes_come_before_any_launch(tr):
    host.check_refusals()
    from torchregister_amd import _lib
    lib = _lib.load()
    shape = (12, 14, 16)
    tgt, wrp = (t.cuda() for t in _images(shape))
    eps = tr.ngf_edge_parameters(tgt, wrp)
    n = lib.trx_ngf_workspace_bytes(3, 1, *shape)
    ws, loss, grad = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.full((1,), 7.0, device="cuda"), torch.full_like(wrp, 7.0)
    stream = _lib.current_stream(torch.device("cuda"))
    P = _lib.ptr

    def call(cfg, nd=3, nbytes=n):
        return lib.trx_ngf_loss_grad(P(tgt), P(wrp), nd, 1, *shape, ctypes.byref(cfg), P(loss), P(grad), P(ws), nbytes, stream)

    assert call(host.ngf_cfg(_lib, float("nan"), eps.data_ptr())) == host.ARG and call(host.ngf_cfg(_lib, 1.0, eps.data_ptr(), (1.0, 0.0, 1.0))) == host.ARG
    assert call(host.ngf_cfg(_lib, 1.0, None)) == host.ARG and call(host.ngf_cfg(_lib, 1.0, eps.data_ptr()), nd=2) == host.NDIM
    assert call(host.ngf_cfg(_lib, 1.0, eps.data_ptr()), nbytes=n - 1) == host.WS
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and bool((grad == 7.0).all())           # nothing ran
    assert call(host.ngf_cfg(_lib, 1.0, eps.data_ptr())) == host.OK
    torch.cuda.synchronize()
    assert torch.equal(loss, tr.ngf_loss_grad(tgt, wrp, eps)[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the Python face
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_ngfloss_module_against_autograd_of_the_restatement(tr):
    """NGFLoss is an autograd criterion: the batch mean of the kernel's losses with eps fitted to the call (held constant under the gradient), its
    gradient the restatement's autograd within the gradient bar; contrast inversion costs nothing, within the loss bar."""
    tgt, wrp = _images((9, 17, 65), B=2)
    mask = _ball((9, 17, 65), B=2)
    for kw, m in ((dict(), None), (dict(eta=0.5, alpha=2.5, voxel=VOXEL), None), (dict(alpha=2.5), mask)):
        crit = tr.NGFLoss(**kw)
        alpha, voxel = kw.get("alpha", 1.0), kw.get("voxel")
        w = wrp.cuda().requires_grad_()
        v = crit(tgt.cuda(), w) if m is None else crit(tgt.cuda(), w, mask=m.cuda())
        v.backward()
        eps = ngf_ref.fit_eps(tgt, wrp, kw.get("eta", 1.0), voxel, m)
        l64, g64 = host.autograd_grad(tgt, wrp, eps, voxel, m, alpha, torch.float64)
        l32, g32 = host.autograd_grad(tgt, wrp, eps, voxel, m, alpha, torch.float32)
        err, bar = abs(v.item() - l64.mean().item()), 4.0 * abs(l32.mean().item() - l64.mean().item()) + 1e-6 * abs(alpha)
        gerr = (w.grad.double().cpu() - g64 / 2).abs().max().item()
        gbar = 4.0 * (g32.double() - g64).abs().max().item() / 2 + 1e-6 * g64.abs().max().item() / 2
        print(f"NGFLoss {kw}: loss {v.item():.6f} err {err:.2e} (bar {bar:.2e}); grad err {gerr:.2e} (bar {gbar:.2e})")
        assert err <= bar and gerr <= gbar
        inv = crit(tgt.cuda(), 1.0 - wrp.cuda()) if m is None else crit(tgt.cuda(), 1.0 - wrp.cuda(), mask=m.cuda())
        print(f"NGFLoss {kw}: loss(T, 1 - W) - loss(T, W) = {inv.item() - v.item():.2e}")
        assert abs(inv.item() - l64.mean().item()) <= bar
    assert "NGFLoss" in dir(__import__("TorchRegister"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. trx_bspline_ngf_run against the CPU loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def _loop_bars(got_losses, got_param, r64, r32, what):
    """tests/test_gpu_mi.py::_loop_bars."""
    (l64, p64), (l32, p32) = r64, r32
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    e, b = np.max(np.abs(got_losses - l64)), max(2e-5 * np.max(np.abs(l64)), 4.0 * lgap)
    print(f"{what} loss curve {l64[0]:.5f} -> {l64[-1]:.5f}: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {lgap:.3e})")
    assert e <= b, (what, "loss curve", e, b)
    e, b = np.max(np.abs(got_param - p64)), max(2e-4, 4.0 * pgap)
    print(f"{what} parameters: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {pgap:.3e})")
    assert e <= b, (what, "parameters", e, b)


CONFIGS = [("adam", {}), ("sgd", {}), ("2d-adam", {}), ("2d-sgd", {}), ("adam", dict(with_base=True, lam=50.0)), ("adam", dict(masked=True)),
           ("2d-adam", dict(masked=True, lam=50.0))]


@pytest.mark.parametrize("name,kw", CONFIGS, ids=["adam", "sgd", "2d-adam", "2d-sgd", "base-bending", "mask", "2d-mask-bending"])
def test_bspline_ngf_loop_vs_torch_autograd(tr, name, kw):
    """trx_bspline_ngf_run, 10 iterations from a random control tensor of amplitude 0.2, against the arbiter in fp64; eps fitted by the solver."""
    shape, spacing, optimizer, lr = host.LOOPS[name]
    mov, tgt, eps, p0, base, mask, r64, r32 = host.arbiter_pair(name, **kw)
    if not kw:
        assert np.all(np.diff(r64[0]) < 0)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=p0, base=None if base is None else base.cuda(), capacity=host.ITERS,
                         bending_weight=kw.get("lam", 0.0), mask=mask, ngf=dict())
    assert torch.allclose(s.ngf_eps.cpu(), eps, rtol=1e-5, atol=0)
    s.run(host.ITERS)
    torch.cuda.synchronize()
    assert int(s.step[0]) == host.ITERS
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), r64, r32, f"bspline ngf {name} {kw}")
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing, base=None if base is None else base.cuda()))


def test_bspline_ngf_loop_with_the_folding_penalty(tr):
    """folding_weight 5 with the threshold at 1.05, where a lattice of amplitude 0.2 has active voxels from the first iteration: against the
    arbiter with tests/jacobian_ref.py::penalty; weight 0 is the unpenalised loop, bit for bit."""
    shape, spacing, optimizer, lr = host.LOOPS["adam"]
    mov, tgt, eps, p0, _, _, r64, r32 = host.arbiter_pair("adam", fold=5.0, fold_eps=1.05)
    pen = host.jr.penalty(bspline_ref.expand(p0, shape, spacing), 1.05).item()
    assert pen > 1e-4 and abs(r64[0][0] - host.arbiter_pair("adam")[6][0][0] - 5.0 * pen) < 1e-9
    kw = dict(optimizer=optimizer, lr=lr, init=p0, capacity=host.ITERS, ngf=dict())
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, folding_weight=5.0, folding_threshold=1.05, **kw)
    s.run(host.ITERS)
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), r64, r32, "bspline ngf folding")
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing))


def test_bspline_ngf_loop_through_an_initial_affine(tr):
    """initial=: a rotation by 0.1 rad about the first axis, the moving image on a lattice of its own (13x12x18 under a 12x14x16 target): one
    interpolation through theta, against the arbiter with tests/affine_flow_ref.py::warp.  eps_w is fitted to the moving image as theta puts it on
    the target lattice."""
    tshape, mshape, spacing = (12, 14, 16), (13, 12, 18), 4
    tgt = ph.blobs(tshape, 3)
    m = ph.blobs(mshape, 3)
    mov = (4.0 * m * (1.0 - m)).float()
    c, s_ = math.cos(0.1), math.sin(0.1)
    theta = torch.tensor([[[c, -s_, 0.0, 0.02], [s_, c, 0.0, -0.03], [0.0, 0.0, 1.0, 0.01]]])
    eps = ngf_ref.fit_eps(tgt, fr.warp(mov, theta, torch.zeros((1, 3) + tshape), None, torch.float32))
    p0 = host.ctrl0(tshape, spacing)
    r64, r32 = (host.arbiter(mov, tgt, eps, host.ITERS, "adam", 0.1, dt, spacing, p0, theta=theta) for dt in (torch.float64, torch.float32))
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer="adam", lr=0.1, init=p0, capacity=host.ITERS, ngf=dict(), initial=theta.cuda())
    print(f"initial=: fitted eps {s.ngf_eps.cpu().tolist()} (restatement {eps.tolist()})")
    assert torch.allclose(s.ngf_eps.cpu(), eps, rtol=1e-4, atol=0)
    s.run(host.ITERS)
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), r64, r32, "bspline ngf initial=")
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, tshape, spacing))


def test_bspline_ngf_loop_stops_where_the_arbiter_does(tr):
    """stop_crit between two losses of pair 0's arbiter: every pair stops exactly where its arbiter does (pair 1, misaligned further, runs on), the
    losses behind a pair's stop stay NaN, and an un-stopped run gives the same bits up to there."""
    shape, spacing, N, k = (12, 14, 16), 4, 10, 4
    mov, tgt = host.multimodal(shape, B=2)
    tgt = torch.cat([tgt[:1], torch.roll(tgt[1:], 3, dims=4)])
    eps = ngf_ref.fit_eps(tgt, mov)
    p0 = host.ctrl0(shape, spacing, B=2)
    run = lambda b, crit: host.arbiter(mov[b:b + 1], tgt[b:b + 1], eps[b:b + 1], N, "adam", 0.1, torch.float64, spacing, p0[b:b + 1], stop_crit=crit)[0]  # noqa: E731
    free0 = run(0, None)
    assert np.all(np.diff(free0[: k + 2]) < 0)
    crit = 0.5 * (free0[k] + free0[k - 1])
    want = [len(run(b, crit)) for b in range(2)]
    assert want == [k + 1, N]
    kw = dict(optimizer="adam", lr=0.1, init=p0, capacity=N, ngf=dict())
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, stop_crit=crit, **kw)
    s.run(3)
    s.run(N - 3)
    free = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, **kw)
    free.run(N)
    torch.cuda.synchronize()
    assert s.step.cpu().tolist() == want and (s.stopped.cpu() != 0).tolist() == [True, False]
    assert torch.equal(s.losses[0, : k + 1], free.losses[0, : k + 1]) and bool(torch.isnan(s.losses[0, k + 1:]).all())
    assert torch.equal(s.losses[1], free.losses[1]) and torch.equal(s.ctrl[1], free.ctrl[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. Register end to end
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register_ngf(tr, levels, **kw):
    return tr.Register("flow", criterion=[tr.NGFLoss()], weight=[1.0], flow_model="bspline", spacing=4, optimizer="adam", levels=levels, **kw)


def _arbiter_level(mov, tgt, base, iters=10):
    """fp64 and fp32 arbiter runs of one level as flow_register runs it: eps fitted to that level's (target, moving), a zero lattice on `base`."""
    shape = tuple(mov.shape[2:])
    eps = ngf_ref.fit_eps(tgt, mov)
    p0 = torch.zeros((1, 3) + bspline_ref.grid(shape, 4))
    return [host.arbiter(mov, tgt, eps, iters, "adam", 0.1, dt, 4, p0, base=base) for dt in (torch.float64, torch.float32)]


def test_register_bspline_with_ngf(tr):
    """Register('flow', criterion=[NGFLoss()], flow_model='bspline') on the multimodal pair, one level, Adam 0.1, 10 iterations from zero: the loss
    falls, loss curve and control tensor are the arbiter's within the loop bars, reg(moving) is the warp by reg.theta; then mask= and initial= reach
    the solver.  From a ZERO lattice Adam normalises gradients that sit at rounding level and the arbiter's own fp32 and fp64 control tensors part by
    0.9 (tests/test_gpu_mi.py found the same on its coarse level), so the control bar is wide here and the check that binds is the loss curve
    (measured: err 4.9e-8, bar 7.9e-4; control err 4.5e-2).  So the same route is run once more from a control tensor of amplitude 0.2
    (flow_register.init_control, which Register's levels use too), where both bars bind: the arbiter's fp32 and fp64 runs stay within 5e-8 / 3e-6."""
    shape = (12, 14, 16)
    mov, tgt = host.multimodal(shape)
    reg = _register_ngf(tr, 1)
    reg.optim(mov.cuda(), tgt.cuda(), lr=0.1, max_epochs=10)
    losses = reg.losses[0].cpu().numpy()
    assert losses.shape == (10,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 4) and reg.theta.shape == (1, 3) + shape
    assert torch.equal(reg(mov.cuda()), tr._engine.flow_warp(mov.cuda(), reg.theta))
    assert torch.equal(reg.final_theta, tr.bspline_expand(reg.control, shape, 4))
    r64, r32 = _arbiter_level(mov, tgt, None)
    _loop_bars(losses, reg.control.cpu().numpy(), r64, r32, "Register")
    _, _, eps, p0, _, _, a64, a32 = host.arbiter_pair("adam")
    ffd = tr.flow_register(shape, criterions=[tr.NGFLoss()], weights=[1.0], lr=0.1, max_epochs=host.ITERS, stop_crit=-1.0, flow_model="bspline", spacing=4,
                           optimizer="adam")
    ffd.init_control = p0
    ffd.optimize(mov.cuda(), tgt.cuda(), debug=False)
    assert ffd.losses.shape == (1, host.ITERS)
    _loop_bars(ffd.losses[0].cpu().numpy(), ffd.control.cpu().numpy(), a64, a32, "flow_register from amplitude 0.2")
    mask = _ball(shape)
    theta = torch.tensor([[[1.0, 0.02, 0.0, 0.01], [-0.02, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, -0.01]]])
    reg.optim(mov.cuda(), tgt.cuda(), lr=0.1, max_epochs=5, mask=mask, initial=theta)      # mask= and initial= reach the solver
    assert reg.losses.shape[-1] == 5 and bool(torch.isfinite(reg.losses).all()) and reg.initial is not None


def test_register_bspline_with_ngf_two_levels(tr):
    """levels=2 on 24x28x32, as tests/test_gpu_mi.py does for mutual information: the coarse level is bit for bit a single-level Register on the
    pyramid's coarse images; the fine level is checked against the arbiter started from the coarse level's handed-up flow, with eps refitted to the
    fine images."""
    shape = (24, 28, 32)
    mov, tgt = host.multimodal(shape)
    m, t = mov.cuda(), tgt.cuda()
    reg = _register_ngf(tr, 2)
    reg.optim(m, t, lr=0.1, max_epochs=10)
    assert [ls.shape[-1] for ls in reg.level_losses] == [10, 10]
    l0, l1 = (ls[0].cpu().numpy() for ls in reg.level_losses)
    print(f"coarse {l0[0]:.5f} -> {l0[-1]:.5f}, fine {l1[0]:.5f} -> {l1[-1]:.5f}")
    assert np.all(np.isfinite(l0)) and np.all(np.isfinite(l1)) and l0[-1] < l0[0] and l1[-1] < l1[0]
    mc, tc = tr.pyramid(m, 2, align_corners=True)[0], tr.pyramid(t, 2, align_corners=True)[0]
    coarse = _register_ngf(tr, 1)
    coarse.optim(mc, tc, lr=0.1, max_epochs=10)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    base = tr.upsample_flow(coarse.final_theta, shape)
    r64, r32 = _arbiter_level(mov, tgt, base.cpu())
    _loop_bars(l1, reg.control.cpu().numpy(), r64, r32, "fine level")
    assert torch.equal(reg.final_theta, tr.bspline_expand(reg.control, shape, 4, base=base))


def test_ngfloss_in_the_generic_affine_loop(tr):
    from oracle import compose
    shape = (16, 18, 20)
    t = ph.blobs(shape, 5)
    m = compose.affine_warp(torch.tensor(ph.THETA_STAR3), t)
    m = (4.0 * m * (1.0 - m)).float()
    reg = tr.Register("affine", criterion=[tr.NGFLoss()], weight=[1.0], honor_criterion=True, optimizer="adam")
    reg.optim(m.cuda(), t.cuda(), lr=0.005, max_epochs=12)
    ls = reg.losses.detach().flatten().cpu().numpy()
    print(f"affine + NGFLoss: {ls[0]:.5f} -> {ls[-1]:.5f}")
    assert len(ls) == 12 and np.all(np.isfinite(ls)) and ls[-1] < ls[0]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. recorded, not asserted
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_record_bias_field_recovery(tr):
    """The multimodal phantom with a multiplicative bias field 1 + 0.5 ramp on the moving image: mean end-point error of the recovered flow after
    100 Adam iterations under NGFLoss and under MILoss.  Printed for DESIGN.md section 4.24; only finiteness is asserted."""
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 3)
    flow = ph.flow_field(shape, amp=1.2, f=0.013)
    w = compose.flow_warp(tgt, flow)
    ramp = torch.linspace(0.0, 1.0, shape[2]).view(1, 1, 1, 1, -1) * torch.linspace(0.0, 1.0, shape[1]).view(1, 1, 1, -1, 1)
    mov = ((4.0 * w * (1.0 - w)) * (1.0 + 0.5 * ramp)).float()
    truth = tr.invert_flow(flow.cuda(), iterations=50, tol=1e-5)
    for name, crit in (("NGFLoss", tr.NGFLoss()), ("MILoss", tr.MILoss())):
        reg = tr.Register("flow", criterion=[crit], weight=[1.0], flow_model="bspline", spacing=4, optimizer="adam")
        reg.optim(mov.cuda(), tgt.cuda(), lr=0.1, max_epochs=100)
        epe = (reg.final_theta - truth).square().sum(1).sqrt().mean().item()
        start = truth.square().sum(1).sqrt().mean().item()
        print(f"bias field, {name}: mean end-point error {epe:.4f} voxels (zero flow: {start:.4f}); loss {reg.losses[0, 0].item():.5f} -> {reg.losses[0, -1].item():.5f}")
        assert math.isfinite(epe)
