"""GPU checks of the cross-lattice rigid / affine mutual-information entry points (csrc/affine_mi.hip: trx_affine_mi_loss_grad_grids,
trx_affine_mi_run_grids, trx_affine_warp_grids) against the arbiter tests/affine_mi_grids_ref.py (F.affine_grid(theta * scale,
target) + F.grid_sample on the moving lattice + tests/mi_ref.py under torch autograd and torch.optim, fp64): exact identities with the one-lattice
entry points, single evaluations, the warp, the loops, the memory contract, the public interface and the registration the feature is for.

Bars: those of tests/test_gpu_affine_mi.py.  Loss: max(2e-5 |l64|, 4 |l32 - l64|).  dtheta: max(4 |g32 - g64|, 2 e_chain) with e_chain the error,
against the same arbiter, of the chain the fused passes replace, run in fp32 on the GPU: trx_affine_warp_grids -> trx_mi_loss_grad -> torch autograd
of (grid_sample(mov, affine_grid(theta * scale, target)) * grad_warped).sum().  Joint table: max(4 sum |P32 - P64|, 2 x the same sum for
trx_mi_histogram on the chain's warped volume).  Loops: test_gpu_mi.py's _loop_bars, whose floors (2e-5 |loss|, 2e-4) bind because
tests/test_affine_mi_grids_host.py holds the arbiter's own fp32-fp64 gaps below 1e-5 and 2e-5."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import mi_mask_ref as mref
import mi_ref
import phantoms as ph
from test_affine_mi_grids_host import check_dispatch, check_refusals
from test_gpu_bspline import _Guarded
from test_gpu_mi import _loop_bars

pytestmark = pytest.mark.gpu

# target / moving: less than one block with finer and coarser axes mixed; two chunks, the second ragged; four chunks; 2-D
SHAPES = [((5, 6, 7), (9, 7, 6)), ((19, 23, 41), (24, 20, 30)), ((40, 40, 40), (25, 33, 52)), ((13, 17), (21, 15))]
_ids = lambda p: "x".join(map(str, p[0])) + "-from-" + "x".join(map(str, p[1]))  # noqa: E731


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _scale(tshape, mshape, world):
    """fp64 [nd, nd+1]: ones, or the world scale of the anisotropic voxel sizes of affine_mi_grids_ref."""
    if not world:
        return gref.scale_of(mshape, tshape)
    return gref.scale_of(mshape, tshape, *((gref.VOXEL_M3, gref.VOXEL_T3) if len(tshape) == 3 else (gref.VOXEL_M2, gref.VOXEL_T2)))


def _cfg(_lib, rng, bins=32, alpha=1.0, normalized=False, mask=None):
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, alpha, int(normalized), rng.data_ptr()
    cfg.mask = None if mask is None else mask.data_ptr()
    return cfg


def _mask8(mask):
    return None if mask is None else (mask != 0).to(device="cuda", dtype=torch.uint8).contiguous()


def _call(vol, mg, cfg, theta, B, nd, bins, need_grad):
    """One evaluation through the C ABI: (loss [B], dtheta [B,nd,nd+1] or None, counts [B,K,K] int64 from the workspace).  mg None: the
    one-lattice entry point."""
    from torchregister_amd import _lib
    lib = _lib.load()
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    assert n > 0
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    loss, dth = torch.empty(B, device="cuda"), torch.zeros(B, 12, device="cuda") if need_grad else None
    args = (_lib.ptr(theta), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n, _lib.current_stream(torch.device("cuda")))
    if mg is None:
        _lib.check(lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), *args), "trx_affine_mi_loss_grad")
    else:
        _lib.check(lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), *args), "trx_affine_mi_loss_grad_grids")
    torch.cuda.synchronize()
    counts = ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()
    return loss, (dth[:, : nd * (nd + 1)].reshape(B, nd, nd + 1) if need_grad else None), counts


def _grids(tr, mov, tgt, theta, scale, rng, bins=32, alpha=1.0, normalized=False, need_grad=True, mask=None):
    """trx_affine_mi_loss_grad_grids (CUDA tensors in; scale [nd,nd+1] or None = ones)."""
    from torchregister_amd import _lib
    pair = tr._engine._GridPair(mov, tgt, scale)
    th = tr._engine.pad_theta(theta.cuda().reshape(pair.B, -1), pair.nd)
    m8 = _mask8(mask)
    return _call(pair.vol(), pair.grid(), _cfg(_lib, rng, bins, alpha, normalized, m8), th, pair.B, pair.nd, bins, need_grad)


def _one_lattice(tr, mov, tgt, theta, rng, bins=32, alpha=1.0, normalized=False, need_grad=True, mask=None):
    """trx_affine_mi_loss_grad, the entry point of before."""
    from torchregister_amd import _lib
    batch = tr._engine._Batch(mov, tgt)
    th = tr._engine.pad_theta(theta.cuda().reshape(batch.B, -1), batch.nd)
    m8 = _mask8(mask)
    return _call(batch.vol(), None, _cfg(_lib, rng, bins, alpha, normalized, m8), th, batch.B, batch.nd, bins, need_grad)


def _warp_grids(tr, theta, mov, size, scale=None):
    """trx_affine_warp_grids through the C ABI: mov [B,C,*moving] -> [B,C,*size] at theta * scale (scale None: ones)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    eng = tr._engine
    B, C, nd = mov.shape[0], mov.shape[1], mov.dim() - 2
    th = eng.pad_theta(theta.cuda().reshape(B, -1), nd)
    out = torch.empty((B, C) + tuple(size), device="cuda")
    tables = eng.base_tables(tuple(size), mov.device)
    v = _lib.Volumes()
    v.moving, v.moving_stride, v.ndim, v.B = mov.data_ptr(), mov[0].numel(), nd, B
    v.D, v.H, v.W = eng._dhw(tuple(size))
    if nd == 3:
        v.zn, v.yn, v.xn = (t.data_ptr() for t in tables)
    else:
        v.yn, v.xn = (t.data_ptr() for t in tables)
    mg = eng._moving_grid(tuple(mov.shape[2:]), None if scale is None else scale.float())
    _lib.check(lib.trx_affine_warp_grids(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), C, _lib.ptr(out), _lib.current_stream(torch.device("cuda"))),
               "trx_affine_warp_grids")
    torch.cuda.synchronize()
    return out


def _chain(tr, mov, tgt, theta, scale, rng, bins, mask=None):
    """What the fused passes replace, in fp32 on the GPU: (loss, dtheta, counts of trx_mi_histogram on the warped volume)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    s32 = scale.float().cuda()
    warped = _warp_grids(tr, theta, mov, tgt.shape[2:], scale)
    loss, gw = tr._engine.mi_loss_grad(tgt, warped, rng, bins, mask=mask)
    th = theta.float().cuda().clone().requires_grad_()
    w = F.grid_sample(mov, F.affine_grid(th * s32, list(tgt.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    (dth,) = torch.autograd.grad((w * gw).sum(), th)
    B, nd = tgt.shape[0], tgt.dim() - 2
    dhw = (1,) * (3 - nd) + tuple(tgt.shape[2:])
    n = lib.trx_mi_workspace_bytes(nd, B, *dhw, bins)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    m8 = _mask8(mask)
    cfg = _cfg(_lib, rng, bins, mask=m8)
    _lib.check(lib.trx_mi_histogram(_lib.ptr(tgt), _lib.ptr(warped), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(ws), n, _lib.current_stream(torch.device("cuda"))),
               "trx_mi_histogram")
    torch.cuda.synchronize()
    return loss, dth, ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()


@functools.lru_cache(maxsize=None)
def _arbiter(tshape, mshape, world, bins, masked=False):
    mov, tgt = gref.pair(tshape, mshape)
    mask = mref.ellipsoid(tshape) if masked else None
    rng = mref.fit_range(tgt, mov, mask) if masked else mi_ref.fit_range(tgt, mov)
    th = aref.theta0(len(tshape))[None]
    scale = _scale(tshape, mshape, world)
    return tuple(gref.evaluate(mov, tgt, th, scale, rng, bins, 1.0, False, dt, mask) for dt in (torch.float64, torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. exact identities
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["all-voxels", "masked"])
@pytest.mark.parametrize("shape", [(19, 23, 41), (13, 17)], ids=lambda s: "x".join(map(str, s)))
def test_same_lattice_has_the_bits_of_the_one_lattice_entry_points(tr, shape, masked):
    """Equal sizes and scale 1: loss, dtheta and counts of trx_affine_mi_loss_grad bit for bit; 6 iterations of trx_affine_mi_run_grids (rigid Adam,
    affine SGD) leave every state array with the bits of trx_affine_mi_run.  (The second solver is a one-lattice solver handed a trx_moving_grid of
    the same sizes and ones: its run() then goes through the cross-lattice entry point.)"""
    nd = len(shape)
    mov, tgt = (x.cuda() for x in aref.pair(shape))
    mask = mref.ellipsoid(shape) if masked else None
    rng = tr._engine.mi_range(tgt, mov, mask=None if mask is None else mask.cuda())
    th = aref.theta0(nd)[None]
    for bins in (32, 64):
        a, b = _one_lattice(tr, mov, tgt, th, rng, bins, mask=mask), _grids(tr, mov, tgt, th, None, rng, bins, mask=mask)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), bins
        assert torch.isfinite(a[0]).all() and a[1].abs().max().item() > 0
    for mode, optimizer, lr, init in (("rigid", "adam", 0.01, aref.pose0(nd)[None]), ("affine", "sgd", 0.01 if nd == 3 else 0.005, th)):
        kw = dict(mode=mode, mi=dict(bins=32), optimizer=optimizer, lr=lr, init=init, capacity=6, mask=mask)
        one, two = tr.AffineMISolver(mov, tgt, **kw), tr.AffineMISolver(mov, tgt, **kw)
        assert one.grid is None and two.grid is None
        two.grid = tr._engine._moving_grid(shape)
        assert (two.grid.D, two.grid.H, two.grid.W) == tr._engine._dhw(shape) and list(two.grid.scale)[: nd * (nd + 1)] == [1.0] * (nd * (nd + 1))
        one.run(6)
        two.run(6)
        torch.cuda.synchronize()
        for f in ("losses", "param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad"):
            assert torch.equal(getattr(one, f), getattr(two, f)), (mode, f)
        assert one.step.tolist() == [6] and bool(torch.isfinite(one.losses[:, :6]).all())


@pytest.mark.parametrize("pair", [SHAPES[1], SHAPES[3]], ids=_ids)
def test_scale_and_theta_are_interchangeable(tr, pair):
    """(theta, scale s) against (fl32(theta s), 1) on two lattices: the same samples, so loss and counts bit for bit; dtheta = dtheta_eff s to 1e-6 relative
    (the reduction behind pass 2 multiplies once, in fp64, in front of the one rounding to fp32)."""
    tshape, mshape = pair
    nd = len(tshape)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    rng = mi_ref.fit_range(tgt.cpu(), mov.cpu()).cuda()
    s32 = _scale(tshape, mshape, True).float()
    th = aref.theta0(nd)[None]
    l, g, c = _grids(tr, mov, tgt, th, s32, rng)
    le, ge, ce = _grids(tr, mov, tgt, th * s32, None, rng)
    assert torch.equal(l, le) and torch.equal(c, ce)
    want = ge.double().cpu() * s32.double()
    rel = ((g.double().cpu() - want).abs() / want.abs().clamp(min=1e-300)).max().item()
    print(f"{tshape} from {mshape}: dtheta against dtheta_eff * s: {rel:.2e} relative")
    assert want.abs().min().item() > 0 and rel <= 1e-6


@pytest.mark.parametrize("bins", [32, 64])
def test_counts_determinism_and_batch_independence(tr, bins):
    """B = 3 on 19x23x41 from 24x20x30 (two chunks per pair), three images, three thetas, three ranges, the world scale: sum(counts) = N_target 2^31, and
    N_m 2^31 under a mask; two calls agree bit for bit; the loss-only call has the same loss bits; every pair has the bits of the pair run alone."""
    tshape, mshape = SHAPES[1]
    N = math.prod(tshape)
    pairs = [gref.pair(tshape, mshape, seed) for seed in (5, 6, 7)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    theta = torch.stack([aref.theta0(3), torch.tensor(ph.THETA_STAR3), torch.tensor(ph.THETA_A)])
    rng = mi_ref.fit_range(tgt.cpu(), mov.cpu())
    rng[1] = torch.tensor([0.15, 0.7, 0.1, 0.8])
    rng[2] = torch.tensor([-0.5, 1.5, -1.0, 2.0])
    rng = rng.cuda()
    scale = _scale(tshape, mshape, True)
    masks = torch.cat([mref.ellipsoid(tshape), mref.checkerboard(tshape), mref.ellipsoid(tshape, 0.5)])
    for mask in (None, masks):
        l1, g1, c1 = _grids(tr, mov, tgt, theta, scale, rng, bins, 1.5, mask=mask)
        l2, g2, c2 = _grids(tr, mov, tgt, theta, scale, rng, bins, 1.5, mask=mask)
        assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(c1, c2)
        assert torch.isfinite(l1).all() and torch.isfinite(g1).all() and len(set(l1.tolist())) == 3
        want = [N * 2 ** 31] * 3 if mask is None else [int(m.sum()) * 2 ** 31 for m in masks]
        assert (c1 >= 0).all() and c1.sum((1, 2)).tolist() == want
        l0, none, c0 = _grids(tr, mov, tgt, theta, scale, rng, bins, 1.5, need_grad=False, mask=mask)
        assert none is None and torch.equal(l0, l1) and torch.equal(c0, c1)
        for b in range(3):
            ls, gs, cs = _grids(tr, mov[b:b + 1], tgt[b:b + 1], theta[b:b + 1], scale, rng[b:b + 1].contiguous(), bins, 1.5,
                                mask=None if mask is None else mask[b:b + 1])
            assert torch.equal(ls, l1[b:b + 1]) and torch.equal(gs, g1[b:b + 1]) and torch.equal(cs, c1[b:b + 1]), b
        wl, wg = tr.affine_mi_loss_grad(mov, tgt, theta, rng, bins, 1.5, mask=mask, scale=scale)
        assert torch.equal(wl, l1) and torch.equal(wg, g1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. single evaluations against the arbiter
# ---------------------------------------------------------------------------------------------------------------------------------------
def _against_the_arbiter(tr, tshape, mshape, world, bins, masked):
    N = math.prod(tshape)
    mov, tgt = gref.pair(tshape, mshape)
    mask = mref.ellipsoid(tshape) if masked else None
    rng = (mref.fit_range(tgt, mov, mask) if masked else mi_ref.fit_range(tgt, mov)).cuda()
    th = aref.theta0(len(tshape))[None]
    scale = _scale(tshape, mshape, world)
    (l64, g64, P64), (l32, g32, P32) = _arbiter(tshape, mshape, world, bins, masked)
    m, t = mov.cuda(), tgt.cuda()
    loss, dth, counts = _grids(tr, m, t, th, scale, rng, bins, mask=mask)
    c_loss, c_dth, c_counts = _chain(tr, m, t, th, scale, rng, bins, mask)
    what = f"{tshape} from {mshape} K={bins} {'world' if world else 'ones'}{' masked' if masked else ''}"

    err, bar = abs(loss[0].item() - l64[0].item()), max(2e-5 * abs(l64[0].item()), 4.0 * abs(l32[0].item() - l64[0].item()))
    print(f"{what}: loss {l64[0].item():.6f} err {err:.2e} bar {bar:.2e} (chain err {abs(c_loss[0].item() - l64[0].item()):.2e})")
    assert err <= bar, (what, "loss", err, bar)

    gerr, ggap = (dth.double().cpu() - g64).abs().max().item(), (g32 - g64).abs().max().item()
    e_chain = (c_dth.double().cpu() - g64).abs().max().item()
    print(f"{what}: max|dtheta| {g64.abs().max().item():.3e} err {gerr:.2e}, arbiter fp32-fp64 {ggap:.2e}, chain err {e_chain:.2e}")
    assert g64.abs().max().item() > 0 and gerr <= max(4.0 * ggap, 2.0 * e_chain), (what, "dtheta", gerr, ggap, e_chain)

    Nm = int(mask.sum()) if masked else N
    assert (counts >= 0).all() and counts.sum((1, 2)).tolist() == [Nm * 2 ** 31]
    P, Pc = counts.double().cpu() / (Nm * 2.0 ** 31), c_counts.double().cpu() / (Nm * 2.0 ** 31)
    perr, pgap, pchain = (P - P64).abs().sum().item(), (P32 - P64).abs().sum().item(), (Pc - P64).abs().sum().item()
    print(f"{what}: sum|P - P64| {perr:.2e}, arbiter fp32-fp64 {pgap:.2e}, chain histogram {pchain:.2e}")
    assert perr <= max(4.0 * pgap, 2.0 * pchain), (what, "table", perr, pgap, pchain)


@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("pair", SHAPES, ids=_ids)
def test_single_evaluation_against_the_arbiter(tr, pair, bins, world):
    """theta = affine_mi_ref.THETA0_*: off the identity, no sample on a voxel centre.  `world`: the scale of 3x1x1 mm target voxels against 1.2x0.9x0.8 mm
    moving voxels (2-D: 2x1 against 0.9x1.3) - entries between 0.6 and 3.5, part of the target outside the moving field of view.  Measured: loss errors
    1e-9 .. 2e-7 against bars of 4e-6 .. 1e-4; dtheta errors at or below the chain's and the arbiter's own fp32-fp64 gap on every case (at 19x23x41 under
    the world scale that gap is 6e-4 .. 1.2e-3 on |dtheta| up to 0.23, and the kernel's and the chain's errors equal it to two digits: the three fp32
    computations agree with one another there and differ from fp64 together)."""
    _against_the_arbiter(tr, pair[0], pair[1], world, bins, False)


def test_single_evaluation_under_a_mask(tr):
    """The ellipsoid of tests/test_gpu_mi_mask.py on the target lattice, two chunks, the world scale."""
    _against_the_arbiter(tr, SHAPES[1][0], SHAPES[1][1], True, 32, True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the warp
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [False, True], ids=["ones", "world"])
@pytest.mark.parametrize("pair", SHAPES, ids=_ids)
def test_warp_against_grid_sample(tr, pair, world):
    """B = 2, two channels sharing coordinates, against F.grid_sample in fp64 on the CPU: at most 1e-5 of the value range."""
    tshape, mshape = pair
    nd = len(tshape)
    mov = torch.cat([torch.cat([gref.pair(tshape, mshape, 5 + 2 * b + c)[0] for c in range(2)], dim=1) for b in range(2)])      # [2, 2, *mshape]
    theta = torch.stack([aref.theta0(nd), torch.tensor(ph.THETA_A if nd == 3 else ph.THETA_B)])
    scale = _scale(tshape, mshape, world)
    want = gref.warp(theta.double(), gref.kernel_scale(scale), mov, tshape)
    got = _warp_grids(tr, theta, mov.cuda(), tshape, scale)
    assert got.shape == (2, 2) + tshape
    err, span = (got.double().cpu() - want).abs().max().item(), (mov.max() - mov.min()).item()
    print(f"{tshape} from {mshape} {'world' if world else 'ones'}: warp err {err:.2e} of range {span:.3f}")
    assert err <= 1e-5 * span
    if not world:      # the public wrapper: theta is the effective one
        assert torch.equal(tr._engine.affine_warp(theta.cuda(), mov.cuda(), size=tshape), got)


@pytest.mark.parametrize("shape", [(19, 23, 41), (13, 17)], ids=lambda s: "x".join(map(str, s)))
def test_warp_on_one_lattice_is_trx_affine_warp(tr, shape):
    nd = len(shape)
    mov = torch.cat([aref.pair(shape, 5)[0], aref.pair(shape, 6)[0]], dim=1).repeat(2, 1, *([1] * nd)).cuda().contiguous()
    theta = torch.stack([aref.theta0(nd), torch.tensor(ph.THETA_A if nd == 3 else ph.THETA_B)]).cuda()
    assert torch.equal(_warp_grids(tr, theta, mov, shape), tr._engine.affine_warp(theta, mov))
    assert torch.equal(tr._engine.affine_warp(theta, mov, size=shape), tr._engine.affine_warp(theta, mov))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the loops
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, name, capacity=gref.ITERS):
    tshape, mshape, mode, optimizer, lr, voxels, masked = gref.LOOPS[name]
    mov, tgt, _, mask, _, start = gref.loop_setup(name)
    kw = {} if voxels is None else dict(moving_voxel=voxels[0], target_voxel=voxels[1])
    return tr.AffineMISolver(mov.cuda(), tgt.cuda(), mode=mode, mi=dict(bins=32), optimizer=optimizer, lr=lr, init=start[None], capacity=capacity, mask=mask, **kw)


@pytest.mark.parametrize("name", list(gref.LOOPS))
def test_loop_vs_torch_autograd(tr, name):
    """trx_affine_mi_run_grids, 10 iterations from a start off the identity, against the arbiter in fp64 (its loss falls in every iteration: asserted);
    the state is the unscaled theta, the best record is the first strict minimum, a run stepped one iteration per call has the same bits."""
    iters = gref.ITERS
    tshape, mshape, mode, _, _, voxels, _ = gref.LOOPS[name]
    nd = len(tshape)
    r64, r32 = gref.loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    mov, tgt, scale, mask, rng, _ = gref.loop_setup(name)
    s = _solver(tr, name, capacity=iters + 3)
    assert s.grid is not None and torch.equal(s.mi_range.cpu(), rng) and torch.equal(s.scale.cpu(), scale.float())
    s.run(iters)
    torch.cuda.synchronize()
    npar = (6 if nd == 3 else 3) if mode == "rigid" else nd * (nd + 1)
    _loop_bars(s.losses[0, :iters].cpu().numpy(), s.param[0, :npar].cpu().numpy().reshape(r64[1].shape), r64, r32, name)
    assert s.step.tolist() == [iters] and bool(torch.isnan(s.losses[:, iters:]).all()) and s.losses.shape == (1, iters + 3)
    if mode == "rigid":      # the state's theta is Theta(pose) itself: the scale lives in the sampler alone
        assert torch.allclose(s.current_theta, tr._engine.pose_to_theta(s.param[:, :npar].double()).float().reshape(1, nd, nd + 1), rtol=0.0, atol=1e-7)
    else:
        assert torch.equal(s.current_theta, s.param[:, :npar].reshape(1, nd, nd + 1))
    assert torch.equal(s.effective(s.current_theta), s.current_theta * s.scale)
    assert (s.world_matrix(s.best) is None) == (voxels is None)
    one = _solver(tr, name)
    thetas = []
    for _ in range(iters):
        thetas.append(one.current_theta)
        one.run(1)
    torch.cuda.synchronize()
    assert torch.equal(one.losses[:, :iters], s.losses[:, :iters]) and torch.equal(one.theta, s.theta)
    curve = s.losses[0, :iters].cpu().numpy()
    k = int(np.argmin(curve))
    assert s.best_idx.tolist() == [k] and s.best_loss[0].item() == curve[k] and torch.equal(s.best, thetas[k])
    assert k == iters - 1


@pytest.mark.parametrize("name", ["affine-adam", "rigid-voxels", "2d-rigid"])
def test_split_runs_give_the_bits_of_one_run(tr, name):
    whole, split = _solver(tr, name), _solver(tr, name)
    whole.run(10)
    split.run(4)
    split.run(6)
    torch.cuda.synchronize()
    for f in ("losses", "param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad"):
        assert torch.equal(getattr(whole, f), getattr(split, f)), f


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. memory contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,pair,bins,mode", [(2, SHAPES[1], 32, "affine"), (3, SHAPES[3], 8, "rigid")], ids=["3d", "2d"])
def test_calls_stay_inside_their_buffers(tr, B, pair, bins, mode):
    """The workspace at exactly trx_affine_mi_workspace_bytes(target lattice) - one byte less is TRX_ERR_WORKSPACE -, the moving volume, out, dtheta and
    the state at their sizes, all between canaries: nothing outside them changes (inputs included), and the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    tshape, mshape = pair
    nd = len(tshape)
    pairs = [gref.pair(tshape, mshape, 5 + b) for b in range(B)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    rng = tr._engine.mi_range(tgt, mov)
    theta = torch.stack([aref.theta0(nd) * (1.0 + 0.01 * b) for b in range(B)])
    scale = _scale(tshape, mshape, True)
    gmov = _Guarded(mov.numel() * 4, 0x69)                      # the moving volume itself between canaries: a sampler that ran past it would read them
    gmov.region.copy_(mov.view(torch.uint8).reshape(-1))
    gpair = tr._engine._GridPair(gmov.floats(tuple(mov.shape)), tgt, scale)
    vol, mg = gpair.vol(), gpair.grid()
    assert vol.moving == gmov.region.data_ptr() and (vol.D, vol.H, vol.W) == tr._engine._dhw(tshape) and (mg.D, mg.H, mg.W) == tr._engine._dhw(mshape)
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    keep = [x.clone() for x in (mov, tgt, rng, th)]
    ws_bytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    one = tr._engine._Batch(tgt, tgt).vol()
    assert ws_bytes > 0 and ws_bytes == lib.trx_affine_mi_workspace_bytes(ctypes.byref(one), bins)      # the target lattice alone
    stream = _lib.current_stream(torch.device("cuda"))
    cfg = _cfg(_lib, rng, bins)

    ws, loss, dth = _Guarded(ws_bytes, 0x5A), _Guarded(B * 4, 0xA5), _Guarded(B * 12 * 4, 0xC3)
    call = lambda n: lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss.region),  # noqa: E731
                                                       _lib.ptr(dth.region), _lib.ptr(ws.region), n, stream)
    assert call(ws_bytes - 1) == -3
    _lib.check(call(ws_bytes), "trx_affine_mi_loss_grad_grids")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (loss, "loss"), (dth, "dtheta"), (gmov, "moving")):
        buf.check(what)
    want_l, want_g = tr.affine_mi_loss_grad(mov, tgt, theta, rng, bins, scale=scale)
    nt = nd * (nd + 1)
    assert torch.equal(loss.floats((B,)), want_l) and torch.equal(dth.floats((B, 12))[:, :nt].reshape(B, nd, nd + 1), want_g)
    assert bool((dth.floats((B, 12))[:, nt:].view(torch.uint8) == 0xC3).all())          # the padding of a row is not written

    C = 2                                                       # the warp: [B][C][moving] -> [B][C][target]
    mov2 = torch.cat([mov, mov.flip(-1)], dim=1).contiguous()
    gmov2 = _Guarded(mov2.numel() * 4, 0x69)
    gmov2.region.copy_(mov2.view(torch.uint8).reshape(-1))
    out = _Guarded(B * C * math.prod(tshape) * 4, 0x96)
    wvol = tr._engine._GridPair(gmov.floats(tuple(mov.shape)), tgt, scale).vol()
    wvol.moving, wvol.moving_stride, wvol.target = gmov2.region.data_ptr(), C * math.prod(mshape), None
    _lib.check(lib.trx_affine_warp_grids(ctypes.byref(wvol), ctypes.byref(mg), _lib.ptr(th), C, _lib.ptr(out.region), stream), "trx_affine_warp_grids")
    torch.cuda.synchronize()
    out.check("out")
    gmov2.check("moving")
    assert torch.equal(out.floats((B, C) + tshape), _warp_grids(tr, theta, mov2, tshape, scale))

    iters, cap = 3, 4
    init = torch.stack([aref.pose0(nd) * (1.0 + 0.1 * b) for b in range(B)]) if mode == "rigid" else theta
    vox = (gref.VOXEL_M3, gref.VOXEL_T3) if nd == 3 else (gref.VOXEL_M2, gref.VOXEL_T2)
    want = tr.AffineMISolver(mov, tgt, mode=mode, mi=dict(bins=bins), optimizer="adam", lr=0.005, init=init, capacity=cap, moving_voxel=vox[0], target_voxel=vox[1])
    assert torch.equal(want.scale.cpu(), scale.float())
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
    run = lambda n: lib.trx_affine_mi_run_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(st), iters,  # noqa: E731
                                                _lib.ptr(ws.region), n, stream)
    assert run(ws_bytes - 1) == -3
    _lib.check(run(ws_bytes), "trx_affine_mi_run_grids")
    torch.cuda.synchronize()
    ws.check("the workspace")
    gmov.check("moving")
    for k in sizes:
        g[k].check(k)
    want.run(iters)
    torch.cuda.synchronize()
    for k in sizes:
        assert torch.equal(g[k].region, getattr(want, k).contiguous().view(torch.uint8).reshape(-1)), k
    assert want.step.tolist() == [iters] * B
    for x, k in zip((mov, tgt, rng, th), keep):
        assert torch.equal(x, k)
    assert torch.equal(gmov.floats(tuple(mov.shape)), mov)


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register(tr, mode="rigid", init=None, levels=1, **kw):
    return tr.Register(mode, criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=init, levels=levels, **kw)


def _grid_sample(theta, x, size):
    return F.grid_sample(x, F.affine_grid(theta, [x.shape[0], x.shape[1], *size], align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)


def test_register_on_two_lattices_in_millimetres(tr):
    """The test that fails without the feature: a moving image on a lattice of its own is a ValueError there."""
    tshape, mshape = (16, 18, 20), (22, 20, 17)
    tvox, mvox = (1.5, 1.0, 1.0), (1.1, 0.9, 1.2)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    pose = aref.pose0(3)
    reg = _register(tr, init=pose)
    reg.optim(mov, tgt, lr=0.01, max_epochs=12, moving_voxel=mvox, target_voxel=tvox)
    ls = reg.losses.cpu().numpy()
    print(f"Register rigid + MILoss on two lattices: {ls[0, 0]:.5f} -> {ls[0, -1]:.5f}")
    assert ls.shape == (1, 12) and np.all(np.isfinite(ls)) and ls[0, -1] < ls[0, 0]
    assert reg.theta.shape == (1, 3, 4) and reg.target_shape == tshape and reg.final_pose.shape == (1, 6)
    # the same run through the solver: Register adds nothing to the numbers, and hands out the EFFECTIVE thetas
    s = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=12, moving_voxel=mvox, target_voxel=tvox)
    s.run(12)
    assert torch.equal(reg.losses, s.losses) and torch.equal(reg.final_theta, s.effective(s.current_theta)) and torch.equal(reg.theta, s.effective(s.best))
    assert torch.equal(reg.final_pose, s.param[:, :6]) and torch.equal(s.scale.cpu(), tr.grid_scale(mshape, tshape, mvox, tvox).float())
    # reg(x) lands on the target lattice and is what torch makes of reg.theta, for any channel count
    x = torch.cat([mov, mov * mov], dim=1)
    out = reg(x)
    assert out.shape == (1, 2) + tshape and torch.equal(out[:, :1], reg(mov))
    err = (out - _grid_sample(reg.theta, x, tshape)).abs().max().item()
    assert err <= 1e-5 * (x.max() - x.min()).item(), err
    # rigid in the world: the matrix part of world_matrix is orthonormal, its last row is (0, 0, 0, 1)
    M = reg.world_matrix
    assert M.shape == (1, 4, 4) and M[0, 3].tolist() == [0.0, 0.0, 0.0, 1.0]
    R = M[0, :3, :3]
    assert (R @ R.T - torch.eye(3, dtype=R.dtype, device=R.device)).abs().max().item() <= 1e-5
    assert torch.equal(M, s.world_matrix(s.best))
    # no voxel sizes: theta acts between the normalised cubes, no world matrix
    cube = _register(tr, init=pose)
    cube.optim(mov, tgt, lr=0.01, max_epochs=4)
    assert cube.world_matrix is None and cube.target_shape == tshape and cube(mov).shape == (1, 1) + tshape and cube.losses.shape == (1, 4)
    # a mask on the target lattice; affine mode
    aff = _register(tr, mode="affine", init=aref.theta0(3))
    aff.optim(mov, tgt, lr=0.005, max_epochs=4, moving_voxel=mvox, target_voxel=tvox, mask=mref.ellipsoid(tshape, 0.9))
    assert bool(torch.isfinite(aff.losses).all()) and aff(mov).shape == (1, 1) + tshape and aff.final_pose is None
    # a later one-lattice optim of the same object is the one-lattice path again
    reg.optim(tgt, tgt, lr=0.01, max_epochs=2)
    assert reg.world_matrix is None and reg.warp is tr.get_affine_warp and torch.equal(reg(tgt), tr.get_affine_warp(reg.theta, tgt))


def test_register_two_levels_on_two_lattices(tr):
    """Each image gets its own pyramid, the pose handed up is the unscaled one: replayed level by level with the solver."""
    tshape, mshape = (16, 18, 20), (22, 20, 17)
    tvox, mvox = (1.5, 1.0, 1.0), (1.1, 0.9, 1.2)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    pose = aref.pose0(3)
    reg = _register(tr, init=pose, levels=2)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[6, 6], moving_voxel=mvox, target_voxel=tvox)
    assert len(reg.level_losses) == 2 and [tuple(ls.shape) for ls in reg.level_losses] == [(1, 6), (1, 6)]
    assert all(bool(torch.isfinite(ls).all()) for ls in reg.level_losses)
    assert reg.level_shapes == tr.pyramid_shapes(tshape, 2) and reg.target_shape == tshape
    mc, tc = tr.pyramid(mov, 2, align_corners=False)[0], tr.pyramid(tgt, 2, align_corners=False)[0]
    cvox = lambda vox, full, lvl: tuple(v * s / c for v, s, c in zip(vox, full, lvl.shape[2:]))  # noqa: E731
    coarse = tr.AffineMISolver(mc, tc, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6,
                               moving_voxel=cvox(mvox, mshape, mc), target_voxel=cvox(tvox, tshape, tc))
    fine = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6, moving_voxel=mvox, target_voxel=tvox)
    assert torch.allclose(coarse.scale, fine.scale, rtol=1e-6, atol=0.0)          # the same fields of view at every level: the same scale
    coarse.run(6)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    fine = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=coarse.param[:, :6].clone(), capacity=6,
                             moving_voxel=mvox, target_voxel=tvox)
    fine.run(6)
    assert torch.equal(fine.losses, reg.level_losses[1]) and torch.equal(fine.effective(fine.current_theta), reg.final_theta)
    assert reg(mov).shape == (1, 1) + tshape


def test_everything_else_refuses_two_lattices(tr):
    check_dispatch(torch.zeros(1, 1, 9, 7, 6, device="cuda"), torch.zeros(1, 1, 5, 6, 7, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. what it is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_what_it_is_for(tr):
    """tests/affine_mi_grids_ref.py's world phantom through Register: 10x30x30 @ 3x1x1 mm against 26x22x18 @ 1.2x1.4x1.7 mm, rigid, Adam 0.01, 32 bins, zero
    start, 120 iterations.  In the arbiter (fp64) the pose error under the world scale is at most half the error under scale 1; the GPU run ends at
    the arbiter's pose within the loop bar 2e-4."""
    _, pose_w, err_w, best_w = gref.world_run(True)
    _, _, err_1, best_1 = gref.world_run(False)
    assert err_w <= 0.5 * err_1
    (ts, tv), (ms, mv) = gref.WORLD_TARGET, gref.WORLD_MOVING
    mov, tgt = (x.cuda() for x in gref.world_pair())
    reg = _register(tr, init=torch.zeros(6))
    reg.optim(mov, tgt, lr=gref.WORLD_LR, max_epochs=gref.WORLD_ITERS, moving_voxel=mv, target_voxel=tv)
    pose = reg.final_pose[0].double().cpu().numpy()
    gap, err = float(np.max(np.abs(pose - pose_w))), float(np.max(np.abs(pose - np.asarray(gref.WORLD_POSE))))
    print(f"max |pose - true|: arbiter world {err_w:.4f} (best loss {best_w:.4f}), arbiter scale 1 {err_1:.4f} (best loss {best_1:.4f}); "
          f"GPU world {err:.4f} (best loss {reg.losses.min().item():.4f}), GPU against the arbiter's pose {gap:.2e}")
    assert gap <= 2e-4
    R = reg.world_matrix[0, :3, :3]
    assert (R @ R.T - torch.eye(3, dtype=R.dtype, device=R.device)).abs().max().item() <= 1e-5
