"""GPU checks of world-geometry registration (trx_moving_grid.world, trx_affine_world_theta, trx_image_moments) against the
arbiter tests/affine_mi_world_ref.py (L, R, l restated; theta_eff = (L Theta R)[:nd] under torch autograd; F.affine_grid + F.grid_sample on the moving
lattice + tests/mi_ref.py, fp64).

Bars: those of tests/test_gpu_affine_mi_grids.py.  Loss: max(2e-5 |l64|, 4 |l32 - l64|).  Joint table: max(4 sum |P32 - P64|, 2 x the same sum for
trx_mi_histogram on the chain's warped volume).  dtheta: max(4 |g32 - g64|, 2 e_chain), the chain being the scale-1 call's chain at theta_eff
(trx_affine_warp_grids -> trx_mi_loss_grad -> torch autograd, fp32 on the GPU) sent through the host fp64 chain rule.  Loops: test_gpu_mi.py's
_loop_bars, whose floors bind because tests/test_affine_mi_world_host.py holds the arbiter's own fp32-fp64 gaps below 1e-5 and 2e-5."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import affine_mi_world_ref as wref
import mi_mask_ref as mref
import mi_ref
from test_affine_mi_world_host import check_refusals
from test_gpu_affine_mi_grids import SHAPES, _call, _cfg, _chain, _ids, _mask8
from test_gpu_bspline import _Guarded
from test_gpu_mi import _loop_bars

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _case(tshape, mshape):
    """(mov, tgt, rec [1,32], theta [1,nd,nd+1] fp32, (A_m, A_t)): affine_mi_grids_ref's pair under oblique headers with 'centers' as T0, at the
    unscaled theta whose theta_eff is affine_mi_ref.theta0 (off the identity, no sample on a voxel centre) up to its rounding to fp32."""
    nd = len(tshape)
    mov, tgt = gref.pair(tshape, mshape)
    Am, At = wref.oblique_pair(tshape, mshape)
    T0 = wref.translation(wref.centre_of(mshape, Am) - wref.centre_of(tshape, At))
    rec = wref.record(mshape, tshape, Am, At, T0)
    return mov, tgt, rec, wref.theta_for(aref.theta0(nd), rec), (Am, At)


def _world(tr, mov, tgt, theta, rec, rng, bins=32, need_grad=True, mask=None, overlap=False, mmask=None, scale=None):
    """trx_affine_mi_loss_grad_grids through the C ABI (CUDA tensors in).  rec: the records [B,32] or None (then scale, None = ones)."""
    from torchregister_amd import _lib
    pair = tr._engine._GridPair(mov, tgt, scale)
    th = tr._engine.pad_theta(theta.cuda().reshape(pair.B, -1), pair.nd)
    m8, mm8 = _mask8(mask), _mask8(mmask)
    r = None if rec is None else rec.cuda().contiguous()
    out = _call(pair.vol(), pair.grid(overlap, mm8, r), _cfg(_lib, rng, bins, mask=m8), th, pair.B, pair.nd, bins, need_grad)
    del r, m8, mm8
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. interchangeable, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["plain", "target-mask", "overlap-moving-mask"])
@pytest.mark.parametrize("pair", SHAPES, ids=_ids)
def test_record_and_effective_theta_are_interchangeable(tr, pair, case):
    """A call with the record against a call without it at theta = trx_affine_world_theta(...) and scale 1: the same samples, so the same loss bits
    and the same counts - alone, under a target mask, under the overlap rule with a moving mask.  The effective theta has the bits of the host
    restatement of the device function (IEEE multiplies and adds in a stated order), and dtheta is the host chain rule of the scale-1 call's
    dtheta_eff to 1e-6 relative (one rounding to fp32 each)."""
    tshape, mshape = pair
    nd = len(tshape)
    mov, tgt, rec, th, _ = _case(tshape, mshape)
    m, t = mov.cuda(), tgt.cuda()
    mask = mref.ellipsoid(tshape) if case == "target-mask" else None
    ov = case == "overlap-moving-mask"
    mmask = mref.ellipsoid(mshape, 0.9) if ov else None
    rng = tr._engine.mi_range(t, m, mask=None if mask is None else mask.cuda(), overlap=ov, moving_mask=None if mmask is None else mmask.cuda())
    te = tr.affine_world_theta(th.cuda(), rec)
    assert te.dtype == torch.float32 and torch.equal(te.cpu(), tr._engine.world_theta_host(th, rec, nd))
    assert (te.cpu().double() - aref.theta0(nd).double()).abs().max().item() <= 1e-5
    l, g, c = _world(tr, m, t, th, rec, rng, mask=mask, overlap=ov, mmask=mmask)
    le, ge, ce = _world(tr, m, t, te, None, rng, mask=mask, overlap=ov, mmask=mmask)
    assert torch.equal(l, le) and torch.equal(c, ce) and bool(torch.isfinite(l).all()) and int(c.sum()) > 0
    if ov:
        assert int(c.sum()) < math.prod(tshape) * 2 ** 31      # the rule rejects some samples: it is on in both calls
    want = tr._engine.world_chain_host(ge, rec, nd)
    rel = (g.double().cpu() - want).abs().max().item() / want.abs().max().item()
    print(f"{tshape} from {mshape} {case}: loss {l.item():.6f}, dtheta against the chain rule of dtheta_eff {rel:.2e} relative")
    assert want.abs().max().item() > 0 and rel <= 1e-6
    # the wrapper is the same call; a garbage scale next to a record is not read
    wl, wg = tr.affine_mi_loss_grad(m, t, th, rng, mask=mask, overlap=ov or None, moving_mask=mmask, world=rec)
    assert torch.equal(wl, l) and torch.equal(wg, g)
    l2, g2, c2 = _world(tr, m, t, th, rec, rng, mask=mask, overlap=ov, mmask=mmask, scale=torch.full((nd, nd + 1), float("nan")))
    assert torch.equal(l2, l) and torch.equal(g2, g) and torch.equal(c2, c)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. single evaluations against the arbiter
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _arbiter(tshape, mshape, masked):
    mov, tgt, rec, th, _ = _case(tshape, mshape)
    mask = mref.ellipsoid(tshape) if masked else None
    rng = mref.fit_range(tgt, mov, mask) if masked else mi_ref.fit_range(tgt, mov)
    return rng, tuple(wref.evaluate(mov, tgt, th, rec, rng, 32, 1.0, False, dt, mask) for dt in (torch.float64, torch.float32))


def _loss_bar(l64, l32):
    return max(2e-5 * abs(l64), 4.0 * abs(l32 - l64))


@pytest.mark.parametrize("masked", [False, True], ids=["all-voxels", "masked"])
@pytest.mark.parametrize("pair", SHAPES, ids=_ids)
def test_single_evaluation_against_the_arbiter(tr, pair, masked):
    tshape, mshape = pair
    nd, N, bins = len(tshape), math.prod(tshape), 32
    mov, tgt, rec, th, _ = _case(tshape, mshape)
    mask = mref.ellipsoid(tshape) if masked else None
    rng, ((l64, g64, P64, _), (l32, g32, P32, _)) = _arbiter(tshape, mshape, masked)
    m, t, rng = mov.cuda(), tgt.cuda(), rng.cuda()
    loss, dth, counts = _world(tr, m, t, th, rec, rng, bins, mask=mask)
    te = tr.affine_world_theta(th.cuda(), rec)
    c_loss, c_dte, c_counts = _chain(tr, m, t, te.cpu(), gref.scale_of(mshape, tshape), rng, bins, mask)
    c_dth = tr._engine.world_chain_host(c_dte, rec, nd)
    what = f"{tshape} from {mshape}{' masked' if masked else ''}"

    err, bar = abs(loss[0].item() - l64[0].item()), _loss_bar(l64[0].item(), l32[0].item())
    print(f"{what}: loss {l64[0].item():.6f} err {err:.2e} bar {bar:.2e} (chain err {abs(c_loss[0].item() - l64[0].item()):.2e})")
    assert err <= bar, (what, "loss", err, bar)

    gerr, ggap = (dth.double().cpu() - g64).abs().max().item(), (g32 - g64).abs().max().item()
    e_chain = (c_dth - g64).abs().max().item()
    print(f"{what}: max|dtheta| {g64.abs().max().item():.3e} err {gerr:.2e}, arbiter fp32-fp64 {ggap:.2e}, chain err {e_chain:.2e}")
    assert g64.abs().max().item() > 0 and gerr <= max(4.0 * ggap, 2.0 * e_chain), (what, "dtheta", gerr, ggap, e_chain)

    Nm = int(mask.sum()) if masked else N
    assert (counts >= 0).all() and counts.sum((1, 2)).tolist() == [Nm * 2 ** 31]
    P, Pc = counts.double().cpu() / (Nm * 2.0 ** 31), c_counts.double().cpu() / (Nm * 2.0 ** 31)
    perr, pgap, pchain = (P - P64).abs().sum().item(), (P32 - P64).abs().sum().item(), (Pc - P64).abs().sum().item()
    print(f"{what}: sum|P - P64| {perr:.2e}, arbiter fp32-fp64 {pgap:.2e}, chain histogram {pchain:.2e}")
    assert perr <= max(4.0 * pgap, 2.0 * pchain), (what, "table", perr, pgap, pchain)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. layout invariance
# ---------------------------------------------------------------------------------------------------------------------------------------
def _layout_solver(tr, mov, tgt, Am, At, T0, c, start):
    geo = tr.world_geometry(mov.shape[2:], tgt.shape[2:], Am, At, init=T0, center=c)
    return tr.AffineMISolver(mov.cuda(), tgt.cuda(), mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=start[None], capacity=wref.ITERS, world=geo)


@pytest.mark.parametrize("which", ["moving", "target"])
def test_layout_invariance(tr, which):
    """Axis 0 of one tensor flipped, its axes 1 and 2 swapped, its header changed to match: the same physical image, T0 and c held.  theta_eff
    un-normalises to the same physical sample positions (no interpolation between the layouts), so the loss agrees within the loss bar of test 2, and a
    10-iteration rigid run ends at the same world matrix: each run lies within _loop_bars' pose floor 2e-4 of the arbiter, so the two poses differ by at
    most 4e-4 per parameter; an entry of the rotation block depends on three angles with derivatives of at most 1 each, and the translation column is
    (I - R) c + l (.) t with t = 0.25 tanh(p): bars 3 x 4e-4 and 3 x 4e-4 sum|c| + 0.25 x 4e-4 max l.  For the target the voxel walk changes: the integer
    histogram does not care beyond the rounding of the coordinates."""
    name = "rigid-adam"
    mov, tgt, rec, rng, start, (Am, At, T0) = wref.loop_setup(name)
    tshape, mshape = wref.LOOPS[name][:2]
    c = wref.centre_of(tshape, At)
    (l64, _, _, _), (l32, _, _, _) = (wref.evaluate(mov, tgt, gref.pose_to_theta(start.double()).float(), rec, rng, dtype=dt) for dt in (torch.float64, torch.float32))
    if which == "moving":
        mov2, Am2 = wref.relayout(mov, Am)
        tgt2, At2 = tgt, At
    else:
        tgt2, At2 = wref.relayout(tgt, At)
        mov2, Am2 = mov, Am
    a, b = _layout_solver(tr, mov, tgt, Am, At, T0, c, start), _layout_solver(tr, mov2, tgt2, Am2, At2, T0, c, start)
    assert torch.equal(a.mi_range, b.mi_range)
    a.run(wref.ITERS)
    b.run(wref.ITERS)
    torch.cuda.synchronize()
    la, lb = a.losses[0, 0].item(), b.losses[0, 0].item()
    bar = _loss_bar(l64.item(), l32.item())
    print(f"layout of the {which}: first loss {la:.7f} / {lb:.7f} (arbiter {l64.item():.7f}), apart {abs(la - lb):.2e}, bar {bar:.2e}")
    assert abs(la - l64.item()) <= bar and abs(lb - l64.item()) <= bar and abs(la - lb) <= bar
    Ma, Mb = a.world_matrix(a.current_theta)[0].cpu(), b.world_matrix(b.current_theta)[0].cpu()
    lin, trans = (Ma[:3, :3] - Mb[:3, :3]).abs().max().item(), (Ma[:3, 3] - Mb[:3, 3]).abs().max().item()
    ext = a.world.extent[0]
    bar_lin, bar_trans = 3 * 4e-4, 3 * 4e-4 * c.abs().sum().item() + 0.25 * 4e-4 * ext.max().item()
    print(f"layout of the {which}: world matrices apart by {lin:.2e} (bar {bar_lin:.1e}) and {trans:.2e} mm (bar {bar_trans:.1e})")
    assert lin <= bar_lin and trans <= bar_trans
    assert (Ma - torch.eye(4, dtype=torch.float64)).abs().max().item() > 1e-2      # the run went somewhere


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the loops
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, name, capacity=wref.ITERS):
    tshape, mshape, mode, optimizer, lr = wref.LOOPS[name]
    mov, tgt, _, _, start, (Am, At, T0) = wref.loop_setup(name)
    return tr.AffineMISolver(mov.cuda(), tgt.cuda(), mode=mode, mi=dict(bins=32), optimizer=optimizer, lr=lr, init=start[None], capacity=capacity,
                             moving_affine=Am, target_affine=At, world_init=T0)


STATE = ("losses", "param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad")


@pytest.mark.parametrize("name", list(wref.LOOPS))
def test_loop_vs_torch_autograd(tr, name):
    """trx_affine_mi_run_grids under a record, 10 iterations from a start off the identity, against the arbiter in fp64 (its loss falls in every
    iteration: asserted); the state is the unscaled theta; a run split over two calls has the bits of one run."""
    iters = wref.ITERS
    tshape, mshape, mode, _, _ = wref.LOOPS[name]
    nd = len(tshape)
    r64, r32 = wref.loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    _, _, rec, rng, _, _ = wref.loop_setup(name)
    s = _solver(tr, name, capacity=iters + 3)
    assert s.grid is not None and s.grid.world == s.world_record.data_ptr() and torch.equal(s.mi_range.cpu(), rng)
    assert torch.allclose(s.world.record, rec, rtol=0, atol=1e-11 * rec.abs().max().item())
    s.run(iters)
    torch.cuda.synchronize()
    npar = (6 if nd == 3 else 3) if mode == "rigid" else nd * (nd + 1)
    _loop_bars(s.losses[0, :iters].cpu().numpy(), s.param[0, :npar].cpu().numpy().reshape(r64[1].shape), r64, r32, name)
    assert s.step.tolist() == [iters] and bool(torch.isnan(s.losses[:, iters:]).all())
    if mode == "rigid":
        assert torch.allclose(s.current_theta, tr._engine.pose_to_theta(s.param[:, :npar].double()).float().reshape(1, nd, nd + 1), rtol=0.0, atol=1e-7)
    else:
        assert torch.equal(s.current_theta, s.param[:, :npar].reshape(1, nd, nd + 1))
    assert torch.equal(s.effective(s.current_theta).cpu(), tr._engine.world_theta_host(s.current_theta, s.world.record, nd))
    whole, split = _solver(tr, name), _solver(tr, name)
    whole.run(10)
    split.run(4)
    split.run(6)
    torch.cuda.synchronize()
    for f in STATE:
        assert torch.equal(getattr(whole, f), getattr(split, f)), f
    assert torch.equal(whole.losses[:, :iters], s.losses[:, :iters])


def test_every_pair_of_a_batch_has_its_own_header(tr):
    """B = 2 with two different headers (and two different images): each pair has the bits of its B = 1 run."""
    name = "rigid-adam"
    tshape, mshape, mode, optimizer, lr = wref.LOOPS[name]
    _, _, _, _, start, (Am, At, T0) = wref.loop_setup(name)
    pairs = [gref.pair(tshape, mshape, seed) for seed in (5, 6)]
    Am2 = wref.header(mshape, (1.1, 1.0, 0.9), wref.rotation(-0.2, 0.1, 0.25), flip=2, centre=(-12.0, 40.0, 7.0))
    At2 = wref.header(tshape, (2.0, 1.2, 1.0), centre=(-11.0, 39.0, 6.5))
    kw = dict(mode=mode, mi=dict(bins=32), optimizer=optimizer, lr=lr, capacity=6)
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    both = tr.AffineMISolver(mov, tgt, init=torch.stack([start, 0.5 * start]), moving_affine=torch.stack([Am, Am2]), target_affine=torch.stack([At, At2]),
                             world_init="centers", **kw)
    both.run(6)
    singles = [tr.AffineMISolver(mov[:1], tgt[:1], init=start[None], moving_affine=Am, target_affine=At, world_init="centers", **kw),
               tr.AffineMISolver(mov[1:], tgt[1:], init=0.5 * start[None], moving_affine=Am2, target_affine=At2, world_init="centers", **kw)]
    for b, one in enumerate(singles):
        one.run(6)
        torch.cuda.synchronize()
        assert torch.equal(one.world.record, both.world.record[b:b + 1])
        for f in STATE:
            assert torch.equal(getattr(one, f), getattr(both, f)[b:b + 1]), (b, f)
        assert torch.equal(one.world_matrix(one.best), both.world_matrix(both.best)[b:b + 1])
    assert not torch.equal(both.losses[0], both.losses[1]) and bool(torch.isfinite(both.losses).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. levels
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register(tr, mode="rigid", init=None, levels=1, **kw):
    return tr.Register(mode, criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=init, levels=levels, **kw)


def test_register_two_levels_share_one_record(tr):
    """levels=2 under headers (anisotropic voxels, an oblique header, 'centers'): replayed level by level with the solver and the same record; the rotation
    block of reg.world_matrix is orthonormal in mode 'rigid'."""
    tshape, mshape = (16, 18, 20), (22, 20, 17)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    Am, At = wref.oblique_pair(tshape, mshape)
    pose = aref.pose0(3)
    reg = _register(tr, init=pose, levels=2)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[6, 6], moving_affine=Am, target_affine=At, world_init="centers")
    assert [tuple(ls.shape) for ls in reg.level_losses] == [(1, 6), (1, 6)] and all(bool(torch.isfinite(ls).all()) for ls in reg.level_losses)
    assert reg.level_shapes == tr.pyramid_shapes(tshape, 2) and reg.target_shape == tshape
    geo = tr.world_setup(mov, tgt, Am, At, "centers")
    assert torch.equal(reg.world_init, geo.init) and torch.equal(reg.world_center, geo.center)
    mc, tc = tr.pyramid(mov, 2, align_corners=False)[0], tr.pyramid(tgt, 2, align_corners=False)[0]
    kw = dict(mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, capacity=6, world=geo)
    coarse = tr.AffineMISolver(mc, tc, init=pose[None], **kw)
    coarse.run(6)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    fine = tr.AffineMISolver(mov, tgt, init=coarse.param[:, :6].clone(), **kw)
    fine.run(6)
    assert torch.equal(fine.losses, reg.level_losses[1]) and torch.equal(fine.effective(fine.current_theta), reg.final_theta)
    assert torch.equal(fine.effective(fine.best), reg.theta) and torch.equal(reg.final_pose, fine.param[:, :6])
    M = reg.world_matrix
    assert M.shape == (1, 4, 4) and M.dtype == torch.float64 and M[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0] and torch.equal(M, fine.world_matrix(fine.best))
    R = M[0, :3, :3]
    assert (R @ R.T - torch.eye(3, dtype=R.dtype, device=R.device)).abs().max().item() <= 1e-5
    assert reg(mov).shape == (1, 1) + tshape
    # with mask=, overlap= and moving_mask= the keywords still go together
    reg2 = _register(tr, init=pose, levels=2)
    reg2.optim(mov, tgt, lr=0.01, max_epochs=[3, 3], moving_affine=Am, target_affine=At, world_init="moments", mask=mref.ellipsoid(tshape, 0.9),
               moving_mask=mref.ellipsoid(mshape, 0.95))
    assert bool(torch.isfinite(reg2.losses).all()) and 0.0 < reg2.valid_fraction.item() <= 1.0 and reg2.world_matrix.shape == (1, 4, 4)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. moments and reach
# ---------------------------------------------------------------------------------------------------------------------------------------
def _moments_call(x, mask, offset):
    """trx_image_moments through the C ABI: out [N, 1+nd] fp64."""
    from torchregister_amd import _lib
    lib = _lib.load()
    N, nd = x.shape[0], x.dim() - 2
    dhw = (1,) * (3 - nd) + tuple(x.shape[2:])
    n = lib.trx_image_moments_workspace_bytes(nd, N, *dhw)
    assert n > 0
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((N, 1 + nd), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(lib.trx_image_moments(_lib.ptr(x), _lib.ptr(mask), _lib.ptr(offset), nd, N, *dhw, _lib.ptr(out), _lib.ptr(ws), n,
                                     _lib.current_stream(torch.device("cuda"))), "trx_image_moments")
    torch.cuda.synchronize()
    return out


def _moments_numpy(x, mask, offset):
    v = x[:, 0].double().cpu().numpy()
    N, nd = v.shape[0], v.ndim - 1
    m = np.ones_like(v, dtype=bool) if mask is None else mask.reshape(v.shape).cpu().numpy() != 0
    w = np.where(m, v - offset.double().cpu().numpy().reshape((N,) + (1,) * nd), 0.0)
    idx = np.meshgrid(*[np.arange(s, dtype=np.float64) for s in v.shape[1:]], indexing="ij")
    cols = [w.reshape(N, -1).sum(1)] + [(w * idx[a][None]).reshape(N, -1).sum(1) for a in reversed(range(nd))]      # x, y(, z) = the last axis first
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("shape", [(5, 6, 7), (19, 23, 41), (40, 40, 40), (13, 17), (150, 131)], ids=lambda s: "x".join(map(str, s)))
def test_image_moments_against_numpy(tr, shape):
    """Raw and masked volumes, N = 3 with three offsets: 1e-6 relative against numpy fp64, two calls with the same bits, every volume the bits of the
    volume alone.  (5,6,7): less than a block; (19,23,41): two chunks, the second ragged; (40,40,40) and (150,131): four / two chunks."""
    nd = len(shape)
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(3, 1, *shape, generator=g) * torch.tensor([1.0, 100.0, 0.01]).reshape(3, 1, *([1] * nd)) + torch.tensor([0.0, -50.0, 3.0]).reshape(3, 1, *([1] * nd))).cuda()
    mask = (torch.rand(3, 1, *shape, generator=g) < 0.4).to(torch.uint8).cuda()
    for mk in (None, mask):
        flat = x.reshape(3, -1)
        offset = (flat.amin(1) if mk is None else torch.where(mk.reshape(3, -1) != 0, flat, torch.full_like(flat, float("inf"))).amin(1)).contiguous()
        a, b = _moments_call(x, mk, offset), _moments_call(x, mk, offset)
        assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        want = _moments_numpy(x, mk, offset)
        rel = np.max(np.abs(a.cpu().numpy() - want) / np.abs(want))
        print(f"{shape}{' masked' if mk is not None else ''}: moments against numpy {rel:.1e} relative")
        assert np.all(np.abs(want) > 0) and rel <= 1e-6
        for n in range(3):
            assert torch.equal(_moments_call(x[n:n + 1].contiguous(), None if mk is None else mk[n:n + 1].contiguous(), offset[n:n + 1].contiguous()), a[n:n + 1])
        mass, centre = tr.image_moments(x, mk)
        assert torch.equal(mass, a[:, 0]) and torch.equal(centre, (a[:, 1:] / a[:, :1]).flip(1)) and centre.dtype == torch.float64
    raw = _moments_call(x, None, None)      # offset NULL = 0
    assert np.max(np.abs(raw.cpu().numpy() - _moments_numpy(x, None, torch.zeros(3))) / np.abs(_moments_numpy(x, None, torch.zeros(3)))) <= 1e-6
    with pytest.raises(ValueError):
        tr.image_moments(torch.full((1, 1) + shape, 2.0, device="cuda"))
    with pytest.raises(ValueError):
        tr.image_moments(x, torch.zeros_like(mask))


def test_reach_beyond_the_rigid_cap(tr):
    """Contents 40 mm apart: beyond 0.25 l of the moving lattice (asserted), so the header-trusting rigid loop cannot bring them together whatever it does -
    its world matrix keeps |t| < 0.25 l - while world_init='moments' starts on top of them and the loop ends at the arbiter's pose."""
    mov, tgt, Am, At = wref.reach_pair()
    ms, ts = wref.REACH_MSHAPE, wref.REACH_TSHAPE
    shift = torch.tensor(wref.REACH_SHIFT, dtype=torch.float64)
    ext = tr.world_geometry(ms, ts, Am, At).extent[0]
    cm, ct = wref.centre_of_mass_world(mov, Am), wref.centre_of_mass_world(tgt, At)
    assert math.isclose(float(shift.norm()), 40.0) and bool(((cm - ct).abs()[:2] > 0.25 * ext[:2]).all())
    m, t = mov.cuda(), tgt.cuda()
    reg = _register(tr, init=torch.zeros(6))
    reg.optim(m, t, lr=0.01, max_epochs=wref.ITERS, moving_affine=Am, target_affine=At, world_init="moments")
    want_T0 = wref.translation(cm - ct)
    print("world_init translation", reg.world_init[0, :3, 3].tolist(), "expected", (cm - ct).tolist())
    assert (reg.world_init[0] - want_T0).abs().max().item() <= 1e-4 and (reg.world_center[0] - ct).abs().max().item() <= 1e-4
    rec = wref.record(ms, ts, Am, At, want_T0, ct)
    rng = mi_ref.fit_range(tgt, mov)
    mi = dict(bins=32, alpha=1.0, normalized=False)
    r64, r32 = (wref.loop(mov, tgt, rng, rec, "rigid", "adam", 0.01, wref.ITERS, torch.zeros(6), mi, dt) for dt in (torch.float64, torch.float32))
    _loop_bars(reg.losses[0].cpu().numpy(), reg.final_pose[0].cpu().numpy(), r64, r32, "reach, world_init='moments'")
    assert r64[0][-1] < r64[0][0]
    # the same run trusting the headers: whatever it finds, its translation is capped
    cap = _register(tr, init=torch.zeros(6))
    cap.optim(m, t, lr=0.01, max_epochs=wref.ITERS, moving_affine=Am, target_affine=At, world_init=None)
    assert torch.equal(cap.world_init[0], torch.eye(4, dtype=torch.float64))
    M, c = cap.world_matrix[0].cpu(), cap.world_center[0]
    tcol = M[:3, 3] - (c - M[:3, :3] @ c)               # T = Tr(c) Theta Tr(-c): the translation column of Theta = l (.) theta[:, 3]
    print("header-trusting run: l (.) t =", tcol.tolist(), "cap", (0.25 * ext).tolist(), "needed", (cm - ct).tolist())
    assert bool((tcol.abs() < 0.25 * ext).all()) and bool(((cm - ct).abs()[:2] > tcol.abs()[:2]).all())
    assert reg.losses.min().item() < cap.losses.min().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. what it is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_what_it_is_for(tr):
    """The world phantom under two headers (tests/affine_mi_world_ref.py: the moving header oblique, offset, one axis flipped) through Register with the
    two headers and nothing else: rigid, Adam 0.01, 32 bins, zero start, 120 iterations end at the arbiter's pose within the loop bar 2e-4 (the
    arbiter: 5.8e-3 from the true pose; with the voxel sizes alone 1.39 - tests/test_affine_mi_world_host.py); then the deformable stage through
    initial=reg and the cubic resample, which only ever see the effective theta."""
    _, pose_h, err_h, best_h = wref.world_run(True)
    (ts, _), (ms, _) = gref.WORLD_TARGET, gref.WORLD_MOVING
    Am, At, T = wref.world_headers()
    mov, tgt = (x.cuda() for x in wref.world_pair())
    reg = _register(tr, init=torch.zeros(6))
    reg.optim(mov, tgt, lr=gref.WORLD_LR, max_epochs=gref.WORLD_ITERS, moving_affine=Am, target_affine=At)
    pose = reg.final_pose[0].double().cpu().numpy()
    gap, err = float(np.max(np.abs(pose - pose_h))), float(np.max(np.abs(pose - np.asarray(wref.WORLD_POSE))))
    print(f"max |pose - true|: arbiter {err_h:.4f} (best loss {best_h:.4f}); GPU {err:.4f} (best loss {reg.losses.min().item():.4f}), GPU against the "
          f"arbiter's pose {gap:.2e}; |world_matrix - T_true| {(reg.world_matrix[0].cpu() - T).abs().max().item():.3f} mm")
    assert gap <= 2e-4
    assert (reg.world_matrix[0].cpu() - T).abs().max().item() <= 0.1      # the arbiter's own world matrix lies 0.033 mm from the truth; a tenth of the finest voxel
    x = torch.cat([mov, mov * mov], dim=1)
    out = reg(x)
    want = F.grid_sample(x, F.affine_grid(reg.theta, [1, 2, *ts], align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    assert out.shape == (1, 2) + ts and (out - want).abs().max().item() <= 1e-5 * (x.max() - x.min()).item()
    # the world matrix and the effective theta say the same thing (the converter is host fp64, theta fp32)
    assert (tr.world_from_theta(reg.theta.cpu(), Am, At, ms, ts) - reg.world_matrix.cpu()).abs().max().item() <= 1e-3
    ffd = tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", flow_model="bspline", spacing=6)
    ffd.optim(mov, tgt, lr=0.01, max_epochs=3, initial=reg)
    assert bool(torch.isfinite(ffd.losses).all()) and ffd(mov, interpolation="cubic").shape == (1, 1) + ts
    assert reg(mov, interpolation="nearest").shape == (1, 1) + ts


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. buffers and refusals
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,pair,mode", [(2, SHAPES[1], "affine"), (3, SHAPES[3], "rigid")], ids=["3d", "2d"])
def test_calls_stay_inside_their_buffers(tr, B, pair, mode):
    """The workspace at exactly its size (one byte less: TRX_ERR_WORKSPACE), the records, both masks, the moving volume, loss, dtheta, theta_eff and the
    moments' workspace and output between canaries: nothing outside them changes, the inputs keep their bytes, the guarded calls give the wrappers' bits."""
    from torchregister_amd import _lib
    lib = _lib.load()
    tshape, mshape = pair
    nd, bins = len(tshape), 32
    pairs = [gref.pair(tshape, mshape, 5 + b) for b in range(B)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    _, _, rec1, th1, _ = _case(tshape, mshape)
    rec = rec1.repeat(B, 1)
    theta = torch.cat([th1 * (1.0 + 0.01 * b) for b in range(B)])
    mask, mmask = torch.cat([mref.ellipsoid(tshape)] * B), torch.cat([mref.ellipsoid(mshape, 0.9)] * B)
    rng = tr._engine.mi_range(tgt, mov, mask=mask.cuda(), overlap=True, moving_mask=mmask.cuda())
    stream = _lib.current_stream(torch.device("cuda"))

    def guarded(t, fill):
        g = _Guarded(t.numel() * t.element_size(), fill)
        g.region.copy_(t.contiguous().view(torch.uint8).reshape(-1))
        return g
    gmov, grec = guarded(mov, 0x69), guarded(rec.cuda(), 0x77)
    gmask, gmmask = guarded(_mask8(mask), 0x11), guarded(_mask8(mmask), 0x22)
    gpair = tr._engine._GridPair(gmov.floats(tuple(mov.shape)), tgt, None)
    vol, mg = gpair.vol(), gpair.grid(True, gmmask.region, grec.region)
    assert mg.world == grec.region.data_ptr() and mg.mask == gmmask.region.data_ptr()
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    cfg = _cfg(_lib, rng, bins, mask=gmask.region)
    ws_bytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws, loss, dth = _Guarded(ws_bytes, 0x5A), _Guarded(B * 4, 0xA5), _Guarded(B * 12 * 4, 0xC3)
    call = lambda n: lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss.region),  # noqa: E731
                                                       _lib.ptr(dth.region), _lib.ptr(ws.region), n, stream)
    assert call(ws_bytes - 1) == -3
    _lib.check(call(ws_bytes), "trx_affine_mi_loss_grad_grids")
    torch.cuda.synchronize()
    inputs = ((gmov, "moving"), (grec, "the records"), (gmask, "the mask"), (gmmask, "the moving mask"))
    for buf, what in ((ws, "the workspace"), (loss, "loss"), (dth, "dtheta")) + inputs:
        buf.check(what)
    want_l, want_g = tr.affine_mi_loss_grad(mov, tgt, theta, rng, bins, mask=mask, moving_mask=mmask, world=rec)
    nt = nd * (nd + 1)
    assert torch.equal(loss.floats((B,)), want_l) and torch.equal(dth.floats((B, 12))[:, :nt].reshape(B, nd, nd + 1), want_g)

    te = _Guarded(B * 12 * 4, 0x3C)
    _lib.check(lib.trx_affine_world_theta(ctypes.byref(mg), nd, B, _lib.ptr(th), _lib.ptr(te.region), stream), "trx_affine_world_theta")
    torch.cuda.synchronize()
    te.check("theta_eff")
    grec.check("the records")
    assert torch.equal(te.floats((B, 12))[:, :nt].reshape(B, nd, nd + 1), tr.affine_world_theta(theta.cuda(), rec))
    assert bool((te.floats((B, 12))[:, nt:] == 0).all())

    iters, cap = 3, 4
    init = torch.stack([aref.pose0(nd) * (1.0 + 0.1 * b) for b in range(B)]) if mode == "rigid" else theta
    geo = tr.WorldGeometry(rec, torch.zeros(B, nd, dtype=torch.float64), torch.eye(nd + 1, dtype=torch.float64).repeat(B, 1, 1), rec[:, 24:24 + nd])
    want = tr.AffineMISolver(mov, tgt, mode=mode, mi=dict(bins=bins), optimizer="adam", lr=0.005, init=init, capacity=cap, mask=mask, moving_mask=mmask, world=geo)
    assert torch.equal(want.mi_range, rng)
    sizes = dict(param=B * 48, theta=B * 48, adam_m=B * 48, adam_v=B * 48, best_theta=B * 48, best_loss=B * 4, best_idx=B * 4, losses=B * cap * 4, step=B * 4,
                 grad=B * 48)
    g = {k: guarded(getattr(want, k), 0x3C) for k in sizes}
    st = _lib.AffineState()
    st.mode = _lib.PARAM_RIGID if mode == "rigid" else _lib.PARAM_AFFINE
    for k in sizes:
        assert g[k].n == sizes[k]
        setattr(st, k, g[k].region.data_ptr())
    st.losses_capacity = cap
    ws = _Guarded(ws_bytes, 0x5A)
    opt = tr._engine.opt_cfg("adam", 0.005)
    run = lambda n: lib.trx_affine_mi_run_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(st), iters,  # noqa: E731
                                                _lib.ptr(ws.region), n, stream)
    assert run(ws_bytes - 1) == -3
    _lib.check(run(ws_bytes), "trx_affine_mi_run_grids")
    torch.cuda.synchronize()
    ws.check("the workspace")
    for buf, what in inputs:
        buf.check(what)
    for k in sizes:
        g[k].check(k)
    want.run(iters)
    torch.cuda.synchronize()
    for k in sizes:
        assert torch.equal(g[k].region, getattr(want, k).contiguous().view(torch.uint8).reshape(-1)), k
    assert torch.equal(gmov.floats(tuple(mov.shape)), mov) and torch.equal(grec.region.view(torch.float64).view(B, 32).cpu(), rec)
    assert torch.equal(gmask.region, _mask8(mask).reshape(-1)) and torch.equal(gmmask.region, _mask8(mmask).reshape(-1))

    # trx_image_moments: the partial rows and the output between canaries
    dhw = (1,) * (3 - nd) + tuple(mshape)
    n = lib.trx_image_moments_workspace_bytes(nd, B, *dhw)
    mws, mout = _Guarded(n, 0x5A), _Guarded(B * (1 + nd) * 8, 0xA5)
    mcall = lambda k: lib.trx_image_moments(gmov.region.data_ptr(), gmmask.region.data_ptr(), None, nd, B, *dhw, mout.region.data_ptr(), mws.region.data_ptr(), k, stream)  # noqa: E731
    assert n > 0 and mcall(n - 1) == -3
    _lib.check(mcall(n), "trx_image_moments")
    torch.cuda.synchronize()
    for buf, what in ((mws, "the moments' workspace"), (mout, "the moments"), (gmov, "moving"), (gmmask, "the moving mask")):
        buf.check(what)
    assert bool(torch.isfinite(mout.region.view(torch.float64)).all())


def test_c_statuses(tr):
    """Every new status, before any HIP call: `world` given to an entry point that does not honour it, NULL outputs, N < 1, sizes."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ARG, NDIM, WS = -1, -2, -3
    tshape, mshape = SHAPES[0]
    mov, tgt, rec1, th1, _ = _case(tshape, mshape)
    m, t, rec = mov.cuda(), tgt.cuda(), rec1.cuda()
    stream = _lib.current_stream(torch.device("cuda"))
    pair = tr._engine._GridPair(m, t, None)
    vol, th = pair.vol(), tr._engine.pad_theta(th1.cuda().reshape(1, -1), 3)
    with_world, without = pair.grid(False, None, rec), pair.grid()
    out = torch.empty(1, 1, *tshape, device="cuda")
    flow = torch.zeros(1, 3, *tshape, device="cuda")
    valid = torch.empty(1, 1, *tshape, dtype=torch.uint8, device="cuda")
    B = ctypes.byref
    # honoured by the two mutual-information entry points only
    for mg, rc in ((without, 0), (with_world, ARG)):
        assert lib.trx_affine_warp_grids(B(vol), B(mg), _lib.ptr(th), 1, _lib.ptr(out), stream) == rc
        assert lib.trx_affine_flow_warp(B(vol), B(mg), _lib.ptr(th), _lib.ptr(flow), 1, _lib.ptr(out), stream) == rc
        assert lib.trx_affine_flow_warp_backward(B(vol), B(mg), _lib.ptr(th), _lib.ptr(flow), 1, _lib.ptr(out), _lib.ptr(torch.empty_like(flow)), stream) == rc
        assert lib.trx_affine_flow_valid(B(vol), B(mg), _lib.ptr(th), _lib.ptr(flow), None, _lib.ptr(valid), stream) == rc
        assert lib.trx_transform_resample(B(vol), B(mg), _lib.ptr(th), None, 1, 0, _lib.ptr(out), stream) == rc
    torch.cuda.synchronize()
    # trx_affine_world_theta
    te = torch.empty(1, 12, device="cuda")
    ok = lambda mg, nd, n, a, b: lib.trx_affine_world_theta(None if mg is None else B(mg), nd, n, a, b, stream)  # noqa: E731
    assert ok(with_world, 3, 1, _lib.ptr(th), _lib.ptr(te)) == 0
    assert ok(None, 3, 1, _lib.ptr(th), _lib.ptr(te)) == ARG and ok(without, 3, 1, _lib.ptr(th), _lib.ptr(te)) == ARG
    assert ok(with_world, 3, 1, None, _lib.ptr(te)) == ARG and ok(with_world, 3, 1, _lib.ptr(th), None) == ARG
    assert ok(with_world, 3, 0, _lib.ptr(th), _lib.ptr(te)) == ARG and ok(with_world, 3, 65536, _lib.ptr(th), _lib.ptr(te)) == ARG
    assert ok(with_world, 4, 1, _lib.ptr(th), _lib.ptr(te)) == NDIM and ok(with_world, 1, 1, _lib.ptr(th), _lib.ptr(te)) == NDIM
    # trx_image_moments
    n = lib.trx_image_moments_workspace_bytes(3, 1, *mshape)
    ws, mo = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(1, 4, dtype=torch.float64, device="cuda")
    mom = lambda x, o, w, nd, N, d, h, ww, k: lib.trx_image_moments(x, None, None, nd, N, d, h, ww, o, w, k, stream)  # noqa: E731
    good = (_lib.ptr(m), _lib.ptr(mo), _lib.ptr(ws), 3, 1) + tuple(mshape) + (n,)
    assert n == 32 and mom(*good) == 0
    assert mom(None, *good[1:]) == ARG and mom(good[0], None, *good[2:]) == ARG and mom(*good[:2], None, *good[3:]) == ARG
    assert mom(*good[:4], 0, *good[5:]) == ARG and mom(*good[:4], 65536, *good[5:]) == ARG and mom(*good[:5], 0, *good[6:]) == ARG
    assert mom(*good[:3], 4, *good[4:]) == NDIM and mom(*good[:3], 2, *good[4:]) == NDIM      # ndim 2 with D != 1
    assert mom(*good[:8], n - 1) == WS
    for bad in ((4, 1, 2, 2, 2), (2, 1, 2, 2, 2), (3, 0, 2, 2, 2), (3, 65536, 2, 2, 2), (3, 1, 0, 2, 2), (3, 1, 2048, 1024, 1024)):
        assert lib.trx_image_moments_workspace_bytes(*bad) == 0
    assert lib.trx_image_moments_workspace_bytes(2, 2, 1, 150, 131) == 2 * 2 * 32      # two volumes, ceil(19650 / 16384) partial rows of four doubles
    torch.cuda.synchronize()


def test_refusals_hold_next_to_a_device(tr):
    check_refusals("cuda")
