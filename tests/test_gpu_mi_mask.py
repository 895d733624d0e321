"""GPU checks of the region-of-interest mask of the mutual information (trx_mi_cfg.mask; csrc/mi.hip, csrc/affine_mi.hip) against the restatement
tests/mi_mask_ref.py (select the voxels inside the mask, hand them to tests/mi_ref.py; fp64).

Shapes, for the 16 384-voxel chunk of the passes: 5x6x7 less than one block; 19x23x41 = 17 917 voxels, two chunks, the second ragged, rows no
multiple of the wave; 40^3 four chunks; 131x127 = 16 637 voxels, 2-D, two chunks.  Bins 8 / 32 / 64: four / four / two LDS tables.  Masks
(mi_mask_ref.MASKS): an ellipsoid (3 249 of 17 917 voxels at 19x23x41), "first chunk empty", a checkerboard, a single voxel, all ones, all zeros.

1. Exact identities, no tolerance: an all-ones mask gives the bits of mask = NULL; the masked call equals the unmasked call on the compacted
   arrays (the selected voxels as a 1 x N_m image) cell for cell and bit for bit; the counts sum to N_m 2^31; an empty mask gives zeros and leaves
   the other pairs alone; pairs do not see each other; the direct-flow loop leaves the flow at exactly 0 outside the mask.
2. Against the arbiter with the bars of tests/test_gpu_mi.py and tests/test_gpu_affine_mi.py (N_m for N); tests/test_mi_mask_host.py asserts that
   the arbiter's own fp32-fp64 gaps stay below the floors and that the masked and unmasked answers differ by far more than any bar.
3. What the mask is for: an occluder in the target. 4. The public interface."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import affine_mi_ref as aref
import mi_mask_ref as mref
import mi_ref
import phantoms as ph
from test_gpu_mi import FIXED_P, _loop_bars

pytestmark = pytest.mark.gpu

SHAPES = [(5, 6, 7), (19, 23, 41), (40, 40, 40), (131, 127)]
ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)  # noqa: E731


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _dhw(shape):
    return (1,) * (3 - len(shape)) + tuple(shape)


def _cfg(_lib, rng, bins, alpha=1.0, normalized=False, mask=None):
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, alpha, int(normalized), rng.data_ptr()
    if mask is not None:
        cfg.mask = mask.data_ptr()
    return cfg


def _u8(tr, mask, like):
    return None if mask is None else tr._engine._mask_u8(mask, like).cuda()


def _hist(tr, tgt, wrp, rng, bins, mask=None):
    """trx_mi_histogram through the C ABI (CUDA tensors in): counts [B,K,K] int64."""
    from torchregister_amd import _lib
    lib = _lib.load()
    B, nd = tgt.shape[0], tgt.dim() - 2
    dhw = _dhw(tgt.shape[2:])
    n = lib.trx_mi_workspace_bytes(nd, B, *dhw, bins)
    assert n > 0
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    m8 = _u8(tr, mask, tgt)
    cfg = _cfg(_lib, rng, bins, mask=m8)
    _lib.check(lib.trx_mi_histogram(_lib.ptr(tgt), _lib.ptr(wrp), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(ws), n, _lib.current_stream(torch.device("cuda"))),
               "trx_mi_histogram")
    torch.cuda.synchronize()
    return ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()


def _fused(tr, mov, tgt, theta, rng, bins, alpha=1.0, normalized=False, mask=None):
    """trx_affine_mi_loss_grad through the C ABI: (loss [B], dtheta [B,nd,nd+1], counts [B,K,K] int64 from the workspace)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    batch = tr._engine._Batch(mov, tgt)
    B, nd = batch.B, batch.nd
    vol = batch.vol()
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    assert n > 0
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    loss, dth = torch.full((B,), 7.0, device="cuda"), torch.full((B, 12), 7.0, device="cuda")
    m8 = _u8(tr, mask, tgt)
    cfg = _cfg(_lib, rng, bins, alpha, normalized, m8)
    _lib.check(lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n,
                                           _lib.current_stream(torch.device("cuda"))), "trx_affine_mi_loss_grad")
    torch.cuda.synchronize()
    counts = ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()
    return loss, dth[:, : nd * (nd + 1)].reshape(B, nd, nd + 1), counts


@functools.lru_cache(maxsize=None)
def _gpu_pair(shape, seed=5):
    """(moving, target, theta0) on the GPU; the moving image doubles as the warped volume of the warped-volume entry points."""
    mov, tgt = aref.pair(shape, seed)
    return mov.cuda(), tgt.cuda(), aref.theta0(len(shape))[None]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. exact identities
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_an_all_ones_mask_gives_the_bits_of_no_mask(tr, shape, bins):
    """(a) trx_mi_histogram counts, trx_mi_loss_grad loss and gradient, trx_affine_mi_loss_grad loss, dtheta and counts: N_m = N, derived on the
    device from the counts, and every operation behind it is the unmasked call's."""
    mov, tgt, th = _gpu_pair(shape)
    rng = tr._engine.mi_range(tgt, mov)
    ones = mref.ones(shape)
    assert torch.equal(tr._engine.mi_range(tgt, mov, mask=ones), rng)
    assert torch.equal(_hist(tr, tgt, mov, rng, bins, ones), _hist(tr, tgt, mov, rng, bins))
    for normalized in (False, True):
        l0, g0 = tr._engine.mi_loss_grad(tgt, mov, rng, bins, 1.5, normalized)
        l1, g1 = tr._engine.mi_loss_grad(tgt, mov, rng, bins, 1.5, normalized, mask=ones)
        assert torch.equal(l0, l1) and torch.equal(g0, g1), ("mi_loss_grad", normalized)
        f0, f1 = _fused(tr, mov, tgt, th, rng, bins, 1.5, normalized), _fused(tr, mov, tgt, th, rng, bins, 1.5, normalized, ones)
        assert all(torch.equal(a, b) for a, b in zip(f0, f1)), ("affine_mi_loss_grad", normalized)
        w = tr.affine_mi_loss_grad(mov, tgt, th, rng, bins, 1.5, normalized, mask=ones)
        assert torch.equal(w[0], f0[0]) and torch.equal(w[1], f0[1])


@pytest.mark.parametrize("name", ["rigid-adam", "affine-sgd", "2d-affine", "rigid-normalized"])
def test_an_all_ones_mask_gives_the_bits_of_no_mask_affine_run(tr, name):
    """(a) a 6-iteration trx_affine_mi_run: losses, parameters, theta, best_*."""
    shape, mode, optimizer, lr, normalized = aref.LOOPS[name]
    mov, tgt, _ = _gpu_pair(shape)
    runs = []
    for mask in (None, mref.ones(shape)):
        s = tr.AffineMISolver(mov, tgt, mode=mode, mi=dict(bins=32, normalized=normalized), optimizer=optimizer, lr=lr, init=aref.start_of(shape, mode)[None],
                              capacity=6, mask=mask)
        s.run(6)
        runs.append(s)
    torch.cuda.synchronize()
    assert runs[0].mask is None and runs[1].mask.dtype == torch.uint8 and runs[1].mi.mask == runs[1].mask.data_ptr()
    assert bool(torch.isfinite(runs[0].losses).all())
    for f in ("losses", "param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad", "mi_range"):
        assert torch.equal(getattr(runs[0], f), getattr(runs[1], f)), f


@pytest.mark.parametrize("shape,spacing", [((12, 14, 16), 4), ((24, 28), 5)], ids=["3d", "2d"])
def test_an_all_ones_mask_gives_the_bits_of_no_mask_bspline_run(tr, shape, spacing):
    """(a) a 4-iteration trx_bspline_mi_run with a bending weight."""
    mov, tgt = (x.cuda() for x in mref.multimodal(shape))
    runs = []
    for mask in (None, mref.ones(shape)):
        s = tr.BSplineSolver(mov, tgt, spacing, optimizer="adam", lr=0.1, capacity=4, bending_weight=20.0, mi=dict(bins=32), mask=mask)
        s.run(4)
        runs.append(s)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(runs[0].losses).all()) and runs[0].losses[0, 3] < runs[0].losses[0, 0]
    for f in ("losses", "ctrl", "flow", "step"):
        assert torch.equal(getattr(runs[0], f), getattr(runs[1], f)), f


def _masks_for(shape):
    names = ["ellipsoid", "checkerboard", "single-voxel"] + (["first-chunk-empty"] if math.prod(shape) > mref.CHUNK else [])
    return [(n, mref.MASKS[n](shape)) for n in names]


@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_the_masked_call_is_the_unmasked_call_on_the_selected_voxels(tr, shape, bins):
    """(b), (c): counts cell for cell, loss bit for bit, gradient bit for bit at the selected voxels and exactly 0 elsewhere, against the unmasked
    entry points on the compacted arrays (a 2-D image 1 x N_m) with the same range; sum(counts) = N_m 2^31."""
    mov, tgt, _ = _gpu_pair(shape)
    rng = tr._engine.mi_range(tgt, mov)
    for name, mask in _masks_for(shape):
        sel = mask.flatten().cuda()
        n_m = int(sel.sum())
        ct, cw = tgt.flatten()[sel].reshape(1, 1, 1, n_m).contiguous(), mov.flatten()[sel].reshape(1, 1, 1, n_m).contiguous()
        counts = _hist(tr, tgt, mov, rng, bins, mask)
        assert counts.sum().item() == n_m * 2 ** 31 and bool((counts >= 0).all()), name
        assert torch.equal(counts, _hist(tr, ct, cw, rng, bins)), name
        for normalized in (False, True):
            loss, grad = tr._engine.mi_loss_grad(tgt, mov, rng, bins, 1.5, normalized, mask=mask)
            closs, cgrad = tr._engine.mi_loss_grad(ct, cw, rng, bins, 1.5, normalized)
            assert torch.equal(loss, closs), (name, normalized, loss.item(), closs.item())
            assert torch.equal(grad.flatten()[sel], cgrad.flatten()), (name, normalized)
            assert torch.count_nonzero(grad.flatten()[~sel]).item() == 0 and bool(torch.isfinite(grad).all()), (name, normalized)
            only, none = tr._engine.mi_loss_grad(tgt, mov, rng, bins, 1.5, normalized, need_grad=False, mask=mask)
            assert none is None and torch.equal(only, loss)
        # the fused passes count the same voxels: their table sums to N_m 2^31 too
        assert _fused(tr, mov, tgt, aref.theta0(len(shape))[None], rng, bins, mask=mask)[2].sum().item() == n_m * 2 ** 31, name


@pytest.mark.parametrize("shape", [(19, 23, 41), (131, 127)], ids=ids)
def test_an_empty_mask_gives_zeros_and_leaves_the_other_pairs_alone(tr, shape):
    """(d) B = 3, the middle pair's mask all zeros: loss 0, gradient 0, dtheta 0, theta unchanged after a run, no NaN anywhere; the other two pairs
    are bit for bit their solo results."""
    nd = len(shape)
    pairs = [aref.pair(shape, seed) for seed in (5, 6, 7)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    mask = torch.cat([mref.ellipsoid(shape), mref.zeros(shape), mref.checkerboard(shape)])
    rng = tr._engine.mi_range(tgt, mov, mask=mask)
    assert torch.equal(rng[1], tr._engine.mi_range(tgt[1:2], mov[1:2])[0])               # the empty pair falls back to its whole target
    theta = torch.stack([aref.theta0(nd) * (1.0 + 0.01 * b) for b in range(3)])
    for normalized in (False, True):
        loss, grad = tr._engine.mi_loss_grad(tgt, mov, rng, 32, 1.0, normalized, mask=mask)
        fl, fg, fc = _fused(tr, mov, tgt, theta, rng, 32, 1.0, normalized, mask)
        assert loss[1].item() == 0.0 and torch.count_nonzero(grad[1]).item() == 0 and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
        assert fl[1].item() == 0.0 and torch.count_nonzero(fg[1]).item() == 0 and torch.count_nonzero(fc[1]).item() == 0 and bool(torch.isfinite(fg).all())
        for b in (0, 2):
            sl, sg = tr._engine.mi_loss_grad(tgt[b:b + 1], mov[b:b + 1], rng[b:b + 1], 32, 1.0, normalized, mask=mask[b:b + 1])
            assert torch.equal(sl[0], loss[b]) and torch.equal(sg[0], grad[b]) and loss[b].item() > 0.0, b
            s = _fused(tr, mov[b:b + 1], tgt[b:b + 1], theta[b:b + 1], rng[b:b + 1].contiguous(), 32, 1.0, normalized, mask[b:b + 1])
            assert torch.equal(s[0][0], fl[b]) and torch.equal(s[1][0], fg[b]) and torch.equal(s[2][0], fc[b]), b
    mode = "rigid"
    init = torch.stack([aref.pose0(nd) * (1.0 + 0.1 * b) for b in range(3)])
    kw = dict(mode=mode, mi=dict(bins=32), optimizer="adam", lr=0.01, capacity=4)
    s = tr.AffineMISolver(mov, tgt, init=init, mask=mask, **kw)
    theta_before, param_before = s.theta.clone(), s.param.clone()
    s.run(4)
    torch.cuda.synchronize()
    assert torch.equal(s.theta[1], theta_before[1]) and torch.equal(s.param[1], param_before[1]) and s.losses[1].tolist() == [0.0] * 4
    assert torch.count_nonzero(s.grad[1]).item() == 0 and s.step.tolist() == [4, 4, 4]
    for f in ("losses", "param", "theta", "best_theta", "grad"):
        assert bool(torch.isfinite(getattr(s, f)).all()), f
    for b in (0, 2):
        solo = tr.AffineMISolver(mov[b:b + 1], tgt[b:b + 1], init=init[b:b + 1], mask=mask[b:b + 1], **kw)
        solo.run(4)
        for f in ("losses", "param", "theta", "best_theta", "best_loss", "best_idx", "grad"):
            assert torch.equal(getattr(solo, f)[0], getattr(s, f)[b]), (b, f)
        assert not torch.equal(s.param[b], param_before[b])


@pytest.mark.parametrize("bins", [32, 64])
def test_masked_pairs_do_not_see_each_other_and_calls_repeat(tr, bins):
    """(e) B = 3 at 40^3 with three masks, three thetas, three ranges: every pair's results are bit for bit those of the pair run alone, and two
    calls agree bit for bit - tests/test_gpu_affine_mi.py's test with masks."""
    shape = (40, 40, 40)
    pairs = [aref.pair(shape, seed) for seed in (5, 6, 7)]
    mov, tgt = torch.cat([p[0] for p in pairs]).cuda(), torch.cat([p[1] for p in pairs]).cuda()
    theta = torch.stack([aref.theta0(3), torch.tensor(ph.THETA_STAR3), torch.tensor(ph.THETA_A)])
    mask = torch.cat([mref.ellipsoid(shape), mref.first_chunk_empty(shape), mref.checkerboard(shape)])
    rng = mref.fit_range(tgt.cpu(), mov.cpu(), mask)
    rng[1] = torch.tensor([0.15, 0.7, 0.1, 0.8])
    rng[2] = torch.tensor([-0.5, 1.5, -1.0, 2.0])
    rng = rng.cuda()
    for normalized in (False, True):
        f1, f2 = _fused(tr, mov, tgt, theta, rng, bins, 1.5, normalized, mask), _fused(tr, mov, tgt, theta, rng, bins, 1.5, normalized, mask)
        assert all(torch.equal(a, b) for a, b in zip(f1, f2))
        assert bool(torch.isfinite(f1[0]).all()) and bool(torch.isfinite(f1[1]).all()) and len(set(f1[0].tolist())) == 3
        m1, m2 = (tr._engine.mi_loss_grad(tgt, mov, rng, bins, 1.5, normalized, mask=mask) for _ in range(2))
        assert torch.equal(m1[0], m2[0]) and torch.equal(m1[1], m2[1])
        for b in range(3):
            s = _fused(tr, mov[b:b + 1], tgt[b:b + 1], theta[b:b + 1], rng[b:b + 1].contiguous(), bins, 1.5, normalized, mask[b:b + 1])
            assert all(torch.equal(x[0], y[b]) for x, y in zip(s, f1)), b
            sl, sg = tr._engine.mi_loss_grad(tgt[b:b + 1], mov[b:b + 1], rng[b:b + 1], bins, 1.5, normalized, mask=mask[b:b + 1])
            assert torch.equal(sl[0], m1[0][b]) and torch.equal(sg[0], m1[1][b]), b


@pytest.mark.parametrize("optimizer,lr", [("sgd", 3.0), ("adam", 0.05)])
def test_the_flow_stays_zero_outside_the_mask(tr, optimizer, lr):
    """(f) trx_flow_mi_run, smooth_weight 0, 3 iterations from a zero flow: the gradient lives on the target lattice, so the flow is exactly 0 at
    every voxel outside the mask (and moves inside it)."""
    shape = (19, 23, 41)
    mov, tgt = (x.cuda() for x in mref.multimodal(shape))
    for name in ("ellipsoid", "first-chunk-empty", "checkerboard"):
        mask = mref.MASKS[name](shape)
        s = tr.FlowSolver(mov, tgt, optimizer=optimizer, lr=lr, capacity=3, mi=dict(bins=32), mask=mask)
        s.run(3)
        torch.cuda.synchronize()
        out = ~mask.cuda().expand(1, 3, *shape)
        assert torch.count_nonzero(s.flow[out]).item() == 0, name
        assert torch.count_nonzero(s.flow[~out]).item() > 0.5 * int((~out).sum()) and bool(torch.isfinite(s.flow).all()) and bool(torch.isfinite(s.losses).all()), name


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. against the arbiter
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _arbiter(shape, name, bins, normalized):
    """The restatement of one (shape, mask, bins, criterion) in fp64 and fp32: warped-volume form (loss, grad) and affine form (loss, dtheta, P)."""
    mov, tgt = aref.pair(shape)
    mask = mref.MASKS[name](shape)
    rng = mref.fit_range(tgt, mov, mask)
    th = aref.theta0(len(shape))[None]
    vol = tuple(mref.loss_grad(tgt, mov, mask, rng, bins, 1.0, normalized, dt) for dt in (torch.float64, torch.float32))
    aff = tuple(mref.evaluate(mov, tgt, th, rng, mask, bins, 1.0, normalized, dt) for dt in (torch.float64, torch.float32))
    return mask, rng, vol, aff


CASES = [((5, 6, 7), "ellipsoid"), ((19, 23, 41), "ellipsoid"), ((19, 23, 41), "first-chunk-empty"), ((19, 23, 41), "checkerboard"),
         ((40, 40, 40), "ellipsoid"), ((131, 127), "ellipsoid"), ((131, 127), "checkerboard")]


@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("shape,name", CASES, ids=ids)
def test_masked_loss_and_gradient_match_the_restatement(tr, shape, name, bins, normalized):
    """trx_mi_loss_grad with a mask, the bars of tests/test_gpu_mi.py with N_m for N: loss 4 x (fp32 - fp64 of the restatement) + the fixed-point bound,
    gradient 4 x the same gap + 1e-6 max|G| s_w / N_m.  Ranges fitted inside the mask."""
    mask, rng, ((l64, g64), (l32, g32)), _ = _arbiter(shape, name, bins, normalized)
    mov, tgt, _ = _gpu_pair(shape)
    assert torch.equal(tr._engine.mi_range(tgt, mov, mask=mask).cpu(), rng)
    loss, grad = tr._engine.mi_loss_grad(tgt, mov, rng.cuda(), bins, 1.0, normalized, mask=mask)
    n_m = int(mask.sum())
    P = mref.joint(tgt.cpu(), mov.cpu(), mask, bins, rng)
    h_tw = -(P * torch.log(torch.where(P > 0, P, torch.ones_like(P)))).sum().item()
    gmax = mi_ref.grad_table(P, 1.0, normalized).abs().max().item()
    e_h = FIXED_P * (math.log(n_m) + 31.0 * math.log(2.0) + 1.0)
    fixed = 4.0 * e_h / h_tw if normalized else 2.0 * e_h
    what = f"{shape} {name} K={bins} {'normalized' if normalized else 'plain'}"
    err, gap = abs(loss[0].item() - l64[0].item()), abs(l32[0].item() - l64[0].item())
    print(f"{what}: loss {l64[0].item():.6f} err {err:.2e} bar {4.0 * gap + fixed:.2e} (fp32 gap {gap:.2e}, fixed point {fixed:.2e})")
    assert err <= 4.0 * gap + fixed, (what, err, gap, fixed)
    _, s_w = mi_ref.scales(rng, bins)
    gfix = 1e-6 * gmax * s_w[0].item() / n_m
    gerr, ggap = (grad.double().cpu() - g64).abs().max().item(), (g32 - g64).abs().max().item()
    print(f"{what}: max|grad| {g64.abs().max().item():.3e} err {gerr:.2e} bar {4.0 * ggap + gfix:.2e} (fp32 gap {ggap:.2e}, fixed point {gfix:.2e})")
    assert gerr <= 4.0 * ggap + gfix, (what, gerr, ggap, gfix)
    assert torch.count_nonzero(grad[~mask.cuda()]).item() == 0


@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("bins", [8, 32, 64])
@pytest.mark.parametrize("shape,name", CASES, ids=ids)
def test_masked_fused_evaluation_against_the_arbiter(tr, shape, name, bins, normalized):
    """trx_affine_mi_loss_grad with a mask, the bars of tests/test_gpu_affine_mi.py: loss max(2e-5 |l64|, 4 |l32 - l64|); dtheta max(4 |g32 - g64|,
    2 e_chain) with e_chain measured here from the masked chain affine_warp -> mi_loss_grad(mask) -> affine_warp_backward; the joint table likewise
    against the chain's trx_mi_histogram(mask)."""
    mask, rng, _, ((l64, g64, P64), (l32, g32, P32)) = _arbiter(shape, name, bins, normalized)
    mov, tgt, th = _gpu_pair(shape)
    r = rng.cuda()
    n_m = int(mask.sum())
    loss, dth, counts = _fused(tr, mov, tgt, th, r, bins, 1.0, normalized, mask)
    warped = tr._engine.affine_warp(th.cuda(), mov)
    c_loss, gw = tr._engine.mi_loss_grad(tgt, warped, r, bins, 1.0, normalized, mask=mask)
    c_dth = tr._engine.affine_warp_backward(th.cuda(), mov, gw)
    c_counts = _hist(tr, tgt, warped, r, bins, mask)
    what = f"{shape} {name} K={bins} {'normalized' if normalized else 'plain'}"

    err, bar = abs(loss[0].item() - l64[0].item()), max(2e-5 * abs(l64[0].item()), 4.0 * abs(l32[0].item() - l64[0].item()))
    print(f"{what}: loss {l64[0].item():.6f} err {err:.2e} bar {bar:.2e} (chain err {abs(c_loss[0].item() - l64[0].item()):.2e})")
    assert err <= bar, (what, "loss", err, bar)

    gerr, ggap = (dth.double().cpu() - g64).abs().max().item(), (g32 - g64).abs().max().item()
    e_chain = (c_dth.double().cpu() - g64).abs().max().item()
    print(f"{what}: max|dtheta| {g64.abs().max().item():.3e} err {gerr:.2e}, arbiter fp32-fp64 {ggap:.2e}, chain err {e_chain:.2e}")
    assert gerr <= max(4.0 * ggap, 2.0 * e_chain), (what, "dtheta", gerr, ggap, e_chain)

    assert counts.sum().item() == n_m * 2 ** 31
    P, Pc = counts.double().cpu() / (n_m * 2.0 ** 31), c_counts.double().cpu() / (n_m * 2.0 ** 31)
    perr, pgap, pchain = (P - P64).abs().sum().item(), (P32 - P64).abs().sum().item(), (Pc - P64).abs().sum().item()
    print(f"{what}: sum|P - P64| {perr:.2e}, arbiter fp32-fp64 {pgap:.2e}, chain histogram {pchain:.2e}")
    assert perr <= max(4.0 * pgap, 2.0 * pchain), (what, "table", perr, pgap, pchain)


@pytest.mark.parametrize("name", list(aref.LOOPS))
def test_masked_affine_loop_vs_torch_autograd(tr, name):
    """trx_affine_mi_run under mi_mask_ref.loop_mask (the radius-1.1 ellipsoid), affine_mi_ref.LOOPS' configurations (rigid + affine, SGD + Adam, 2-D + 3-D), 10 iterations, against
    the masked arbiter in fp64 with test_gpu_mi.py's loop bars; the solver fits its ranges inside the mask."""
    iters = aref.ITERS
    shape, mode, optimizer, lr, normalized = aref.LOOPS[name]
    nd = len(shape)
    r64, r32 = mref.loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    mov, tgt, _ = _gpu_pair(shape)
    mask = mref.loop_mask(shape)
    s = tr.AffineMISolver(mov, tgt, mode=mode, mi=dict(bins=32, normalized=normalized), optimizer=optimizer, lr=lr, init=aref.start_of(shape, mode)[None],
                          capacity=iters, mask=mask)
    assert torch.equal(s.mi_range.cpu(), mref.fit_range(tgt.cpu(), mov.cpu(), mask))
    s.run(iters)
    torch.cuda.synchronize()
    npar = (6 if nd == 3 else 3) if mode == "rigid" else nd * (nd + 1)
    _loop_bars(s.losses[0, :iters].cpu().numpy(), s.param[0, :npar].cpu().numpy().reshape(r64[1].shape), r64, r32, f"masked {name}")
    assert s.step.tolist() == [iters]


@pytest.mark.parametrize("name", list(mref.FLOW_LOOPS))
def test_masked_flow_and_bspline_loops_vs_torch_autograd(tr, name):
    """trx_bspline_mi_run (2-D and 3-D, with a bending weight) and trx_flow_mi_run under mi_mask_ref.loop_mask, 10 iterations, against the masked
    arbiter in fp64 with test_gpu_mi.py's loop bars: cfg->mask reaches trx_mi_loss_grad on every iteration."""
    shape, spacing, optimizer, lr, lam = mref.FLOW_LOOPS[name]
    mov, tgt, mask, p0, r64, r32 = mref.flow_loop_pair(name)
    assert np.all(np.diff(r64[0]) < 0)
    if spacing is None:
        s = tr.FlowSolver(mov.cuda(), tgt.cuda(), optimizer=optimizer, lr=lr, init=p0, capacity=mref.FLOW_ITERS, mi=dict(bins=32), mask=mask)
    else:
        s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=p0, capacity=mref.FLOW_ITERS, bending_weight=lam,
                             mi=dict(bins=32), mask=mask)
    assert torch.equal(s.mi_range.cpu(), mref.fit_range(tgt, mov, mask))
    s.run(mref.FLOW_ITERS)
    torch.cuda.synchronize()
    assert int(s.step[0]) == mref.FLOW_ITERS
    _loop_bars(s.losses[0].cpu().numpy(), (s.flow if spacing is None else s.ctrl).cpu().numpy(), r64, r32, f"masked {name}")


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. what the mask is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_mask_restores_the_pose_an_occluder_spoils(tr):
    """The target of affine_mi_ref.pair at 24x28x32 with a bright block (1.5; the phantom stays below 1.2) pasted over the corner region
    [0:10, 0:12, 0:14] - 1 680 of 21 504 voxels - that the moving image lacks.  Rigid, Adam, lr 0.01, 120 iterations from affine_mi_ref.pose0 through
    Register(device_loop=True).optim, with and without a mask that excludes the block.  The pose error is max |pose - p*| with p* the pose the fp64
    arbiter reaches on the clean pair (mi_mask_ref.OCC_TRUTH).  Block and iteration count were chosen on the CPU with the fp64 arbiter
    (tests/test_mi_mask_host.py asserts it): its pose error is 0.00126 with the mask and 0.00799 without, a ratio of 0.16 (fp32 arbiter: the same to
    2e-5).  Asserted here for the GPU run: the same inequality, masked error <= half the unmasked error."""
    mov, tgt, mask = mref.occluded_pair()
    errs = []
    for m in (mask, None):
        reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=aref.pose0(3))
        reg.optim(mov.cuda(), tgt.cuda(), lr=mref.OCC_LR, max_epochs=mref.OCC_ITERS, mask=m)
        assert bool(torch.isfinite(reg.losses).all()) and reg.final_pose.shape == (1, 6)
        errs.append(mref.pose_error(reg.final_pose[0].cpu().numpy()))
    print(f"max|pose - p*|: masked {errs[0]:.5f} unmasked {errs[1]:.5f} (fp64 arbiter: 0.00126, 0.00799)")
    assert errs[0] <= 0.5 * errs[1], errs


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_register_with_a_mask(tr):
    shape = (16, 18, 20)
    mov, tgt, _ = _gpu_pair(shape)
    mask = mref.ellipsoid(shape, 0.8)
    pose = aref.pose0(3)
    # one level: Register adds nothing to the solver's numbers; bool, float and [B,*spatial] masks are one mask
    ref = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6, mask=mask)
    ref.run(6)
    free = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6)
    free.run(6)
    assert not torch.equal(ref.losses, free.losses)
    for m in (mask, mask.float() * 3.0, mask[:, 0].to(torch.uint8).cuda()):
        reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=pose)
        reg.optim(mov, tgt, lr=0.01, max_epochs=6, mask=m)
        assert torch.equal(reg.losses, ref.losses) and torch.equal(reg.final_theta, ref.current_theta) and torch.equal(reg.theta, ref.best)
    # two levels: the coarse level's mask is the pyramid of the float mask at >= 0.5, its ranges are fitted inside it
    reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=pose, levels=2)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[6, 6], mask=mask)
    assert [tuple(ls.shape) for ls in reg.level_losses] == [(1, 6), (1, 6)] and all(bool(torch.isfinite(ls).all()) for ls in reg.level_losses)
    mc, tc = tr.pyramid(mov, 2, align_corners=False)[0], tr.pyramid(tgt, 2, align_corners=False)[0]
    kc = tr.pyramid(mask.float().cuda(), 2, align_corners=False)[0] >= 0.5
    assert 0 < int(kc.sum()) < kc.numel() and tuple(kc.shape[2:]) == (8, 9, 10)
    coarse = tr.AffineMISolver(mc, tc, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose[None], capacity=6, mask=kc)
    coarse.run(6)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    fine = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=coarse.param[:, :6].clone(), capacity=6, mask=mask)
    fine.run(6)
    assert torch.equal(fine.losses, reg.level_losses[1]) and torch.equal(fine.current_theta, reg.final_theta)
    # a mask that empties at the coarse level
    tiny = mref.single_voxel(shape)
    with pytest.raises(ValueError, match=r"pair 0 .* level 1"):
        reg.optim(mov, tgt, lr=0.01, max_epochs=[2, 2], mask=tiny)


def test_flow_register_and_miloss_with_a_mask(tr):
    shape = (12, 14, 16)
    mov, tgt = (x.cuda() for x in mref.multimodal(shape))
    mask = mref.ellipsoid(shape, 0.8)
    reg = tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline", spacing=4, optimizer="adam")
    reg.optim(mov, tgt, lr=0.1, max_epochs=5, mask=mask)
    s = tr.BSplineSolver(mov, tgt, 4, optimizer="adam", lr=0.1, capacity=5, mi=dict(bins=32), mask=mask, stop_crit=1e-4, keep_last=True)
    s.run(5)
    assert torch.equal(reg.losses, s.losses) and torch.equal(reg.control, s.ctrl) and reg.losses[0, -1] < reg.losses[0, 0]
    two = tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline", spacing=4, optimizer="adam", levels=2)
    m24, t24 = (x.cuda() for x in mref.multimodal((24, 28, 32)))
    two.optim(m24, t24, lr=0.1, max_epochs=4, mask=mref.ellipsoid((24, 28, 32), 0.8))
    assert [ls.shape[-1] for ls in two.level_losses] == [4, 4] and all(bool(torch.isfinite(ls).all()) for ls in two.level_losses)
    fr = tr.flow_register(shape, criterions=[tr.MILoss()], weights=[1.0], lr=0.05, max_epochs=3, flow_model="direct", optimizer="adam", stop_crit=-1.0)
    fr.optimize(mov, tgt, debug=False, mask=mask)
    assert torch.count_nonzero(fr.final_flow[~mask.cuda().expand(1, 3, *shape)]).item() == 0 and torch.count_nonzero(fr.final_flow).item() > 0
    # MILoss as an autograd criterion: value and gradient are the kernel's, the range is fitted inside the mask, the mask gets no gradient
    w = mov.clone().requires_grad_()
    fmask = mask.float().cuda().requires_grad_()
    crit = tr.MILoss(bins=16, alpha=1.5, normalized=True)
    v = crit(tgt, w, mask=fmask)
    v.backward()
    rng = tr._engine.mi_range(tgt, mov, mask=mask)
    assert rng[0, :2].tolist() == [tgt[mask.cuda()].min().item(), tgt[mask.cuda()].max().item()]
    loss, grad = tr._engine.mi_loss_grad(tgt, mov, rng, 16, 1.5, True, mask=mask)
    assert torch.equal(v.detach(), loss.mean()) and torch.equal(w.grad, grad) and fmask.grad is None
