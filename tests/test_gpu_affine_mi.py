"""GPU checks of the fused rigid / affine mutual-information entry points (csrc/affine_mi.hip: trx_affine_mi_loss_grad, trx_affine_mi_run) against
the arbiter tests/affine_mi_ref.py (oracle/compose.py::affine_warp + tests/mi_ref.py under torch autograd and torch.optim, fp64): single
evaluations, batch independence and determinism, the loops, split runs, the memory contract and the public interface.

Bars.  Loss: the project's loop bar max(2e-5 |l64|, 4 |l32 - l64|).  dtheta: max(4 |g32 - g64|, 2 e_chain) with e_chain the error, against the same
arbiter, of the chain of entry points the fused pass replaces (affine_warp -> mi_loss_grad -> affine_warp_backward), measured in the test: the
fused pass may be no worse than twice what the project already ships.  Joint table: sum |P - P64| <= max(4 sum |P32 - P64|, 2 x the same sum for
trx_mi_histogram on the chain's warped volume).  Loops: test_gpu_mi.py's _loop_bars; tests/test_affine_mi_host.py asserts that the arbiter's own
fp32-fp64 gaps stay below 1e-5 (loss) and 2e-5 (parameters) for every configuration, so the floors 2e-5 |loss| and 2e-4 are the bars that bind."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import affine_mi_ref as aref
import mi_ref
import phantoms as ph
from test_gpu_bspline import _Guarded
from test_gpu_mi import _loop_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _cfg(_lib, rng, bins=32, alpha=1.0, normalized=False):
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, alpha, int(normalized), rng.data_ptr()
    return cfg


def _fused(tr, mov, tgt, theta, rng, bins, alpha=1.0, normalized=False, need_grad=True, tables=True):
    """trx_affine_mi_loss_grad through the C ABI (CUDA tensors in): (loss [B], dtheta [B,nd,nd+1] or None, counts [B,K,K] int64 from the workspace)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    batch = tr._engine._Batch(mov, tgt, tables=tables)
    B, nd = batch.B, batch.nd
    vol = batch.vol()
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    assert n > 0
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    loss, dth = torch.empty(B, device="cuda"), torch.zeros(B, 12, device="cuda") if need_grad else None
    cfg = _cfg(_lib, rng, bins, alpha, normalized)
    _lib.check(lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n,
                                           _lib.current_stream(torch.device("cuda"))), "trx_affine_mi_loss_grad")
    torch.cuda.synchronize()
    counts = ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()
    return loss, (dth[:, : nd * (nd + 1)].reshape(B, nd, nd + 1) if need_grad else None), counts


def _chain(tr, mov, tgt, theta, rng, bins, alpha, normalized):
    """The entry points the fused pass replaces: (loss, dtheta, counts of trx_mi_histogram on the warped volume)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    warped = tr._engine.affine_warp(theta.cuda(), mov)
    loss, gw = tr._engine.mi_loss_grad(tgt, warped, rng, bins, alpha, normalized)
    dth = tr._engine.affine_warp_backward(theta.cuda(), mov, gw)
    B, nd = mov.shape[0], mov.dim() - 2
    dhw = (1,) * (3 - nd) + tuple(mov.shape[2:])
    n = lib.trx_mi_workspace_bytes(nd, B, *dhw, bins)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    cfg = _cfg(_lib, rng, bins, alpha, normalized)
    _lib.check(lib.trx_mi_histogram(_lib.ptr(tgt), _lib.ptr(warped), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(ws), n, _lib.current_stream(torch.device("cuda"))),
               "trx_mi_histogram")
    torch.cuda.synchronize()
    return loss, dth, ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()


@functools.lru_cache(maxsize=None)
def _arbiter(shape, bins, normalized):
    mov, tgt = aref.pair(shape)
    rng = mi_ref.fit_range(tgt, mov)
    th = aref.theta0(len(shape))[None]
    return tuple(aref.evaluate(mov, tgt, th, rng, bins, 1.0, normalized, dt) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. single evaluation
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("shape", [(5, 6, 7), (12, 14, 16), (40, 40, 40), (13, 17)], ids=lambda s: "x".join(map(str, s)))
def test_single_evaluation_against_the_arbiter(tr, shape, bins, normalized):
    """5x6x7: less than one block; 40^3 = 64000 voxels: four blocks and partial rows per pair, the last one ragged; 13x17: 2-D.  8 and 32 bins: one LDS
    table per wave, 64: two.  Measured on the CPU, the arbiter's own fp32-fp64 gap of dtheta: 1.7e-6 at 12x14x16, 2.0e-4 at 40^3, 8.7e-6 at 13x17
    with |dtheta| up to 0.7, 1.1 and 2.3."""
    N = math.prod(shape)
    mov, tgt = aref.pair(shape)
    rng = mi_ref.fit_range(tgt, mov)
    th = aref.theta0(len(shape))[None]
    (l64, g64, P64), (l32, g32, P32) = _arbiter(shape, bins, normalized)
    m, t, r = mov.cuda(), tgt.cuda(), rng.cuda()
    loss, dth, counts = _fused(tr, m, t, th, r, bins, 1.0, normalized)
    c_loss, c_dth, c_counts = _chain(tr, m, t, th, r, bins, 1.0, normalized)
    what = f"{shape} K={bins} {'normalized' if normalized else 'plain'}"

    err, bar = abs(loss[0].item() - l64[0].item()), max(2e-5 * abs(l64[0].item()), 4.0 * abs(l32[0].item() - l64[0].item()))
    print(f"{what}: loss {l64[0].item():.6f} err {err:.2e} bar {bar:.2e} (chain err {abs(c_loss[0].item() - l64[0].item()):.2e})")
    assert err <= bar, (what, "loss", err, bar)

    gerr, ggap = (dth.double().cpu() - g64).abs().max().item(), (g32 - g64).abs().max().item()
    e_chain = (c_dth.double().cpu() - g64).abs().max().item()
    print(f"{what}: max|dtheta| {g64.abs().max().item():.3e} err {gerr:.2e}, arbiter fp32-fp64 {ggap:.2e}, chain err {e_chain:.2e}")
    assert gerr <= max(4.0 * ggap, 2.0 * e_chain), (what, "dtheta", gerr, ggap, e_chain)

    assert (counts >= 0).all() and counts.sum((1, 2)).tolist() == [N * 2 ** 31]
    P, Pc = counts.double().cpu() / (N * 2.0 ** 31), c_counts.double().cpu() / (N * 2.0 ** 31)
    perr, pgap, pchain = (P - P64).abs().sum().item(), (P32 - P64).abs().sum().item(), (Pc - P64).abs().sum().item()
    print(f"{what}: sum|P - P64| {perr:.2e}, arbiter fp32-fp64 {pgap:.2e}, chain histogram {pchain:.2e}")
    assert perr <= max(4.0 * pgap, 2.0 * pchain), (what, "table", perr, pgap, pchain)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. batch and determinism
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [32, 64])
def test_pairs_do_not_see_each_other_and_calls_repeat(tr, bins):
    """B = 3 at 40^3 (four blocks per pair), three images, three thetas, three ranges (fitted, narrower than the data, wider), tables present: every
    pair's loss and dtheta are bit for bit those of the pair run alone, two calls agree bit for bit, the loss-only call has the same loss bits."""
    shape = (40, 40, 40)
    pairs = [aref.pair(shape, seed) for seed in (5, 6, 7)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    theta = torch.stack([aref.theta0(3), torch.tensor(ph.THETA_STAR3), torch.tensor(ph.THETA_A)])
    rng = mi_ref.fit_range(tgt.cpu(), mov.cpu())
    rng[1] = torch.tensor([0.15, 0.7, 0.1, 0.8])
    rng[2] = torch.tensor([-0.5, 1.5, -1.0, 2.0])
    rng = rng.cuda()
    for normalized in (False, True):
        l1, g1, c1 = _fused(tr, mov, tgt, theta, rng, bins, 1.5, normalized)
        l2, g2, c2 = _fused(tr, mov, tgt, theta, rng, bins, 1.5, normalized)
        assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(c1, c2)
        assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and len(set(l1.tolist())) == 3
        l0, none, c0 = _fused(tr, mov, tgt, theta, rng, bins, 1.5, normalized, need_grad=False)
        assert none is None and torch.equal(l0, l1) and torch.equal(c0, c1)
        for b in range(3):
            ls, gs, cs = _fused(tr, mov[b:b + 1], tgt[b:b + 1], theta[b:b + 1], rng[b:b + 1].contiguous(), bins, 1.5, normalized)
            assert torch.equal(ls, l1[b:b + 1]) and torch.equal(gs, g1[b:b + 1]) and torch.equal(cs, c1[b:b + 1]), b
        wl, wg = tr.affine_mi_loss_grad(mov, tgt, theta, rng, bins, 1.5, normalized)
        assert torch.equal(wl, l1) and torch.equal(wg, g1)


def test_closed_form_coordinates_and_strides(tr):
    """Without the tables xn / yn / zn the closed form (2i + 1) / S - 1 serves: the arbiter's bars hold as with them.  A moving_stride of 0 shares one
    moving volume among the pairs, a target_stride larger than the volume skips a channel: both equal the dense call bit for bit."""
    from torchregister_amd import _lib
    lib = _lib.load()
    shape, bins = (12, 14, 16), 32
    mov, tgt = aref.pair(shape)
    rng = mi_ref.fit_range(tgt, mov).cuda()
    th = aref.theta0(3)[None]
    (l64, g64, _), (l32, g32, _) = _arbiter(shape, bins, False)
    loss, dth, _ = _fused(tr, mov.cuda(), tgt.cuda(), th, rng, bins, tables=False)
    assert abs(loss[0].item() - l64[0].item()) <= max(2e-5 * abs(l64[0].item()), 4.0 * abs(l32[0].item() - l64[0].item()))
    _, c_dth, _ = _chain(tr, mov.cuda(), tgt.cuda(), th, rng, bins, 1.0, False)
    e_chain = (c_dth.double().cpu() - g64).abs().max().item()
    assert (dth.double().cpu() - g64).abs().max().item() <= max(4.0 * (g32 - g64).abs().max().item(), 2.0 * e_chain)

    tgt2 = torch.cat([tgt, aref.pair(shape, 6)[1]], dim=1).repeat(2, 1, 1, 1, 1).cuda().contiguous()      # [2, 2, ...]: channel 0 is the target
    theta = torch.stack([aref.theta0(3), torch.tensor(ph.THETA_STAR3)])
    rng2 = rng.repeat(2, 1).contiguous()
    dense = _fused(tr, mov.cuda().repeat(2, 1, 1, 1, 1), tgt2[:, :1].contiguous(), theta, rng2, bins)
    batch = tr._engine._Batch(mov.cuda().repeat(2, 1, 1, 1, 1), tgt2[:, :1].contiguous())
    vol = batch.vol(moving_stride=0, target_stride=2 * math.prod(shape))
    vol.target = tgt2.data_ptr()
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws, loss, dth = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(2, device="cuda"), torch.zeros(2, 12, device="cuda")
    cfg = _cfg(_lib, rng2, bins)
    pth = tr._engine.pad_theta(theta.cuda().reshape(2, -1), 3)
    _lib.check(lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), _lib.ptr(pth), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n,
                                           _lib.current_stream(torch.device("cuda"))), "trx_affine_mi_loss_grad")
    torch.cuda.synchronize()
    assert torch.equal(loss, dense[0]) and torch.equal(dth.reshape(2, 3, 4), dense[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the loops, 4. split runs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, name, capacity=aref.ITERS):
    shape, mode, optimizer, lr, normalized = aref.LOOPS[name]
    mov, tgt = aref.pair(shape)
    return tr.AffineMISolver(mov.cuda(), tgt.cuda(), mode=mode, mi=dict(bins=32, normalized=normalized), optimizer=optimizer, lr=lr,
                             init=aref.start_of(shape, mode)[None], capacity=capacity)


@pytest.mark.parametrize("name", list(aref.LOOPS))
def test_loop_vs_torch_autograd(tr, name):
    """trx_affine_mi_run, 10 iterations from a start off the identity, against the arbiter in fp64 (its loss falls in every iteration: asserted);
    step, the NaN tail of the loss curve, and best_idx / best_loss / best_theta = the first strict minimum of the returned curve and the theta of
    that forward (the thetas of the forwards come from a second solver stepped one iteration per call, whose curve has the same bits)."""
    iters = aref.ITERS
    shape, mode, optimizer, lr, normalized = aref.LOOPS[name]
    nd = len(shape)
    r64, r32 = aref.loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    s = _solver(tr, name, capacity=iters + 3)
    assert torch.equal(s.mi_range.cpu(), mi_ref.fit_range(*reversed(aref.pair(shape))))
    s.run(iters)
    torch.cuda.synchronize()
    npar = (6 if nd == 3 else 3) if mode == "rigid" else nd * (nd + 1)
    _loop_bars(s.losses[0, :iters].cpu().numpy(), s.param[0, :npar].cpu().numpy().reshape(r64[1].shape), r64, r32, name)
    assert s.step.tolist() == [iters] and bool(torch.isnan(s.losses[:, iters:]).all()) and s.losses.shape == (1, iters + 3)
    if mode == "rigid":
        assert torch.allclose(s.current_theta, tr._engine.pose_to_theta(s.param[:, :npar].double()).float().reshape(1, nd, nd + 1), rtol=0.0, atol=1e-7)
    else:
        assert torch.equal(s.current_theta, s.param[:, :npar].reshape(1, nd, nd + 1))
    one = _solver(tr, name)
    thetas = []
    for _ in range(iters):
        thetas.append(one.current_theta)
        one.run(1)
    torch.cuda.synchronize()
    assert torch.equal(one.losses[:, :iters], s.losses[:, :iters]) and torch.equal(one.theta, s.theta)
    curve = s.losses[0, :iters].cpu().numpy()
    k = int(np.argmin(curve))                                  # the first of equal minima: the first strict minimum
    assert s.best_idx.tolist() == [k] and s.best_loss[0].item() == curve[k] and torch.equal(s.best, thetas[k])
    assert k == iters - 1                                      # the arbiter descends throughout, and so does the kernel within the bars


@pytest.mark.parametrize("name", ["affine-adam", "rigid-sgd", "2d-rigid"])
def test_split_runs_give_the_bits_of_one_run(tr, name):
    whole, split = _solver(tr, name), _solver(tr, name)
    whole.run(10)
    split.run(4)
    split.run(6)
    torch.cuda.synchronize()
    for f in ("losses", "param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad"):
        assert torch.equal(getattr(whole, f), getattr(split, f)), f
    with pytest.raises(tr._lib.TrxError, match="capacity"):
        split.run(1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. memory contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,shape,bins,mode", [(2, (12, 14, 16), 32, "affine"), (3, (13, 17), 8, "rigid")])
def test_calls_stay_inside_their_buffers(tr, B, shape, bins, mode):
    """The workspace at exactly trx_affine_mi_workspace_bytes, outputs and state at their sizes, all between canaries: nothing outside them changes
    (inputs included), and the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd = len(shape)
    npose = 6 if nd == 3 else 3
    pairs = [aref.pair(shape, 5 + b) for b in range(B)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    rng = tr._engine.mi_range(tgt, mov)
    theta = torch.stack([aref.theta0(nd) * (1.0 + 0.01 * b) for b in range(B)])
    batch = tr._engine._Batch(mov, tgt)
    vol = batch.vol()
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    keep = [x.clone() for x in (mov, tgt, rng, th)]
    ws_bytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    assert ws_bytes > 0
    stream = _lib.current_stream(torch.device("cuda"))
    cfg = _cfg(_lib, rng, bins)

    ws, loss, dth = _Guarded(ws_bytes, 0x5A), _Guarded(B * 4, 0xA5), _Guarded(B * 12 * 4, 0xC3)
    _lib.check(lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss.region), _lib.ptr(dth.region), _lib.ptr(ws.region),
                                           ws_bytes, stream), "trx_affine_mi_loss_grad")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (loss, "loss"), (dth, "dtheta")):
        buf.check(what)
    want_l, want_g = tr.affine_mi_loss_grad(mov, tgt, theta, rng, bins)
    nt = nd * (nd + 1)
    assert torch.equal(loss.floats((B,)), want_l) and torch.equal(dth.floats((B, 12))[:, :nt].reshape(B, nd, nd + 1), want_g)
    assert bool((dth.floats((B, 12))[:, nt:].view(torch.uint8) == 0xC3).all())          # the padding of a row is not written

    iters, cap = 3, 4
    init = torch.stack([aref.pose0(nd) * (1.0 + 0.1 * b) for b in range(B)]) if mode == "rigid" else theta
    want = tr.AffineMISolver(mov, tgt, mode=mode, mi=dict(bins=bins), optimizer="adam", lr=0.005, init=init, capacity=cap)
    sizes = dict(param=B * 48, theta=B * 48, adam_m=B * 48, adam_v=B * 48, best_theta=B * 48, best_loss=B * 4, best_idx=B * 4, losses=B * cap * 4, step=B * 4,
                 grad=B * 48)
    g = {k: _Guarded(n, 0x3C) for k, n in sizes.items()}
    for k in sizes:
        g[k].region.copy_(getattr(want, k).contiguous().view(torch.uint8).reshape(-1))
    st = _lib.AffineState()
    st.mode = _lib.PARAM_RIGID if mode == "rigid" else _lib.PARAM_AFFINE
    for k in sizes:
        setattr(st, k, g[k].region.data_ptr())
    st.losses_capacity = cap
    ws = _Guarded(ws_bytes, 0x5A)
    opt = tr._engine.opt_cfg("adam", 0.005)
    _lib.check(lib.trx_affine_mi_run(ctypes.byref(vol), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(st), iters, _lib.ptr(ws.region), ws_bytes, stream),
               "trx_affine_mi_run")
    torch.cuda.synchronize()
    ws.check("the workspace")
    for k in sizes:
        g[k].check(k)
    want.run(iters)
    torch.cuda.synchronize()
    for k in sizes:
        assert torch.equal(g[k].region, getattr(want, k).contiguous().view(torch.uint8).reshape(-1)), k
    assert want.step.tolist() == [iters] * B
    for x, k in zip((mov, tgt, rng, th), keep):
        assert torch.equal(x, k)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register(tr, mode="rigid", crit=None, weight=1.0, init=None, levels=1):
    return tr.Register(mode, criterion=[crit or tr.MILoss()], weight=[weight], optimizer="adam", device_loop=True, init=init, levels=levels)


def test_register_rigid_with_the_device_loop(tr):
    shape = (16, 18, 20)
    mov, tgt = (x.cuda() for x in aref.pair(shape))
    pose = aref.pose0(3)
    reg = _register(tr, init=pose)
    reg.optim(mov, tgt, lr=0.01, max_epochs=12)
    ls = reg.losses.cpu().numpy()
    print(f"Register rigid + MILoss, device loop: {ls[0, 0]:.5f} -> {ls[0, -1]:.5f}")
    assert ls.shape == (1, 12) and np.all(np.isfinite(ls)) and ls[0, -1] < ls[0, 0]
    assert reg.theta.shape == (1, 3, 4) and torch.equal(reg(mov), tr.get_affine_warp(reg.theta, mov))
    # the same run through the solver: Register adds nothing to the numbers
    s = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=12)
    s.run(12)
    assert torch.equal(reg.losses, s.losses) and torch.equal(reg.final_theta, s.current_theta) and torch.equal(reg.theta, s.best)
    # alpha 2 at weight 0.5 is alpha 1 at weight 1
    half = _register(tr, crit=tr.MILoss(alpha=2.0), weight=0.5, init=pose)
    half.optim(mov, tgt, lr=0.01, max_epochs=12)
    assert torch.equal(half.losses, reg.losses)


def test_register_two_levels_and_a_batch(tr):
    shape = (16, 18, 20)
    mov, tgt = (x.cuda() for x in aref.pair(shape))
    pose = aref.pose0(3)
    reg = _register(tr, init=pose, levels=2)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[6, 6])
    assert len(reg.level_losses) == 2 and [tuple(ls.shape) for ls in reg.level_losses] == [(1, 6), (1, 6)]
    assert all(bool(torch.isfinite(ls).all()) for ls in reg.level_losses)
    # the second level starts from the first level's final pose: replay both levels with the solver on the package's own pyramid images
    mc, tc = tr.pyramid(mov, 2, align_corners=False)[0], tr.pyramid(tgt, 2, align_corners=False)[0]
    coarse = tr.AffineMISolver(mc, tc, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6)
    coarse.run(6)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    fine = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=coarse.param[:, :6].clone(), capacity=6)
    fine.run(6)
    assert torch.equal(fine.losses, reg.level_losses[1]) and torch.equal(fine.current_theta, reg.final_theta)
    assert torch.equal(reg(mov), tr.get_affine_warp(reg.theta, mov))

    # B = 2, affine: two independent pairs end at different thetas, each the theta of its own single-pair run
    m2 = torch.cat([mov, aref.pair(shape, 6)[0].cuda()])
    t2 = torch.cat([tgt, aref.pair(shape, 6)[1].cuda()])
    both = _register(tr, mode="affine", init=aref.theta0(3))
    both.optim(m2, t2, lr=0.005, max_epochs=8)
    assert both.final_theta.shape == (2, 3, 4) and not torch.equal(both.final_theta[0], both.final_theta[1])
    for b in range(2):
        alone = _register(tr, mode="affine", init=aref.theta0(3))
        alone.optim(m2[b:b + 1], t2[b:b + 1], lr=0.005, max_epochs=8)
        assert torch.equal(alone.final_theta[0], both.final_theta[b]) and torch.equal(alone.losses[0], both.losses[b])
