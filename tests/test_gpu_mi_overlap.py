"""GPU checks of the overlap rule (trx_moving_grid.overlap / .mask: trx_affine_mi_loss_grad_grids, trx_affine_mi_run_grids, trx_affine_flow_valid,
trx_bspline_mi_run_grids) against the restatement tests/mi_overlap_ref.py.

Exact identities (bit for bit): the rule on against the restatement's validity uploaded as cfg->mask with the rule off; every sample valid against
the rule off; sum(counts) = N_valid 2^31; a pair without a valid sample; trx_affine_flow_valid byte for byte on every voxel; determinism and batch
independence.
Against the fp64 arbiter: single evaluations with the bars of tests/test_gpu_affine_mi_grids.py - loss max(2e-5 |l64|, 4 |l32 - l64|), dtheta
max(4 |g32 - g64|, 2 e_chain), table max(4 sum |P32 - P64|, 2 x the chain's) with e_chain the error of the fp32 GPU chain trx_affine_warp_grids ->
trx_mi_loss_grad under the validity mask -> torch autograd; loops with test_gpu_mi.py's _loop_bars rule, restated below.  The identities are exact
because tests/test_mi_overlap_host.py holds every sample of every case and of every arbiter iteration at least 1e-4 voxel away from a decision."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import affine_mi_grids_ref as gref
import mi_overlap_ref as oref
from test_gpu_bspline import _Guarded
from test_mi_overlap_host import check_python_refusals, check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _loop_bars(got_losses, got_param, r64, r32, what):
    """The rule of tests/test_gpu_mi.py::_loop_bars: loss curve within max(2e-5 max|l64|, 4 x the arbiter's fp32-fp64 gap), parameters within
    max(2e-4, 4 x the arbiter's gap)."""
    (l64, p64), (l32, p32) = r64[:2], r32[:2]
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    e, b = np.max(np.abs(got_losses - l64)), max(2e-5 * np.max(np.abs(l64)), 4.0 * lgap)
    print(f"{what} loss curve {l64[0]:.5f} -> {l64[-1]:.5f}: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {lgap:.3e})")
    assert e <= b, (what, "loss curve", e, b)
    e, b = np.max(np.abs(got_param - p64)), max(2e-4, 4.0 * pgap)
    print(f"{what} parameters: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {pgap:.3e})")
    assert e <= b, (what, "parameters", e, b)


def _u8(x):
    return None if x is None else (x != 0).to(device="cuda", dtype=torch.uint8).contiguous()


def _call(tr, mov, tgt, theta, scale, rng, tmask=None, mmask=None, overlap=False, bins=32, alpha=1.0, need_grad=True):
    """One evaluation through the C ABI: (loss [B], dtheta [B,nd,nd+1] or None, counts [B,K,K] int64)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    pair = tr._engine._GridPair(mov, tgt, scale)
    B, nd = pair.B, pair.nd
    th = tr._engine.pad_theta(theta.cuda().reshape(B, -1), nd)
    t8, m8 = _u8(tmask), _u8(mmask)
    cfg = tr._engine._mi_cfg_c(bins, alpha, False, rng, t8)
    vol, mg = pair.vol(), pair.grid(overlap, m8)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    loss, dth = torch.empty(B, device="cuda"), torch.zeros(B, 12, device="cuda") if need_grad else None
    _lib.check(lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n,
                                                 _lib.current_stream(torch.device("cuda"))), "trx_affine_mi_loss_grad_grids")
    torch.cuda.synchronize()
    counts = ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()
    return loss, (dth[:, : nd * (nd + 1)].reshape(B, nd, nd + 1) if need_grad else None), counts


def _gpu_case(name):
    mov, tgt, theta, scale, tmask, mmask, rng = oref.case(name)
    return mov.cuda(), tgt.cuda(), theta, scale, tmask, mmask, rng.cuda()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. exact identities
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oref.CASES))
def test_rule_on_is_the_validity_as_a_target_mask(tr, name):
    """(a) single evaluation, (c), (f): the rule on has the bits of the rule off with the restatement's validity uploaded as cfg->mask - counts, loss,
    dtheta -; sum(counts) = N_valid 2^31 with N_valid from the restatement; two calls agree; the loss-only call agrees; a pair alone has its bits."""
    mov, tgt, theta, scale, tmask, mmask, rng = _gpu_case(name)
    valid = oref.case_arbiter(name)[0][3]
    on = _call(tr, mov, tgt, theta, scale, rng, tmask, mmask, overlap=True)
    off = _call(tr, mov, tgt, theta, scale, rng, valid)
    assert _same(on, off)
    nvalid = valid.flatten(1).sum(1).tolist()
    assert (on[2] >= 0).all() and on[2].sum((1, 2)).tolist() == [n * 2 ** 31 for n in nvalid] and 0 < min(nvalid)
    assert torch.isfinite(on[0]).all() and on[1].abs().amax((1, 2)).min().item() > 0
    assert _same(on, _call(tr, mov, tgt, theta, scale, rng, tmask, mmask, overlap=True))
    lo = _call(tr, mov, tgt, theta, scale, rng, tmask, mmask, overlap=True, need_grad=False)
    assert lo[1] is None and torch.equal(lo[0], on[0]) and torch.equal(lo[2], on[2])
    for b in range(2):
        one = _call(tr, mov[b:b + 1], tgt[b:b + 1], theta[b:b + 1], scale, rng[b:b + 1].contiguous(), None if tmask is None else tmask[b:b + 1],
                    None if mmask is None else mmask[b:b + 1], overlap=True)
        assert _same(one, [x[b:b + 1] for x in on]), b
    wl, wg, wc = tr.affine_mi_loss_grad(mov, tgt, theta, rng, mask=tmask, scale=scale, overlap=True, moving_mask=mmask, return_counts=True)
    assert _same((wl, wg, wc), on)


def test_every_sample_valid_has_the_bits_of_the_rule_off(tr):
    """(b) and (d): B = 2 under scale 1 - pair 0 zooms into the moving image (every sample valid), pair 1 is shifted out of it (none valid).  With the
    same range, pair 0 has the bits of the rule off (one evaluation and a 6-iteration run); pair 1 has loss 0, dtheta 0, counts 0 and a run leaves its
    theta where it was; pair 0 next to it has the bits of pair 0 alone."""
    tshape, mshape = (12, 14, 16), (15, 13, 18)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    mov, tgt = (mov + 0.25).repeat(2, 1, 1, 1, 1), tgt.repeat(2, 1, 1, 1, 1)
    theta = torch.cat([oref.special_pair("all"), oref.special_pair("none")])
    rng = oref.fit_range(tgt.cpu(), mov.cpu()).cuda()
    on = _call(tr, mov, tgt, theta, None, rng, overlap=True)
    off = _call(tr, mov, tgt, theta, None, rng)
    assert _same([x[:1] for x in on], [x[:1] for x in off]) and on[2][0].sum().item() == math.prod(tshape) * 2 ** 31
    assert on[0][1].item() == 0.0 and not on[1][1].any() and not on[2][1].any() and off[0][1].item() != 0.0
    alone = _call(tr, mov[:1], tgt[:1], theta[:1], None, rng[:1].contiguous(), overlap=True)
    assert _same(alone, [x[:1] for x in on])
    kw = dict(mode="affine", mi=dict(bins=32, moving_range=(rng[0, 2].item(), rng[0, 3].item())), optimizer="adam", lr=0.002, init=theta, capacity=6)
    a, b = tr.AffineMISolver(mov, tgt, overlap=True, **kw), tr.AffineMISolver(mov, tgt, **kw)
    assert torch.equal(a.mi_range, b.mi_range)
    a.run(6)
    b.run(6)
    torch.cuda.synchronize()
    for f in ("losses", "theta", "param", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "grad"):
        assert torch.equal(getattr(a, f)[:1], getattr(b, f)[:1]), f
    assert torch.equal(a.theta[1, :12].cpu(), theta[1].reshape(-1)) and not a.losses[1, :6].any() and not a.grad[1].any() and a.step.tolist() == [6, 6]
    assert a.valid_fraction(a.theta[:, :12].reshape(2, 3, 4)).tolist() == [1.0, 0.0]


@pytest.mark.parametrize("name", list(oref.LOOPS))
def test_ten_iterations_are_the_validity_replayed_as_masks(tr, name):
    """(a) for a run: 10 iterations with the rule on, stepped one call at a time, against the rule off with, in front of every iteration, the fp64
    arbiter's validity of that iteration uploaded into the cfg->mask buffer: every state array bit for bit."""
    _, _, mode, optimizer, lr, voxels = oref.LOOPS[name][:6]
    mov, tgt, _, tmask, mmask, rng, start = oref.loop_setup(name)
    valids = oref.loop_pair(name)[0][2]
    kw = dict(mode=mode, mi=dict(bins=32, moving_range=(rng[0, 2].item(), rng[0, 3].item()), target_range=(rng[0, 0].item(), rng[0, 1].item())),
              optimizer=optimizer, lr=lr, init=start[None], capacity=oref.ITERS)
    if voxels is not None:
        kw.update(moving_voxel=voxels[0], target_voxel=voxels[1])
    on = tr.AffineMISolver(mov.cuda(), tgt.cuda(), mask=tmask, overlap=True, moving_mask=mmask, **kw)
    off = tr.AffineMISolver(mov.cuda(), tgt.cuda(), mask=valids[0], **kw)
    assert torch.equal(on.mi_range, off.mi_range) and torch.equal(on.mi_range.cpu(), rng)
    for k in range(oref.ITERS):
        off.mask.copy_(valids[k].to(torch.uint8))
        on.run(1)
        off.run(1)
    torch.cuda.synchronize()
    for f in ("losses", "theta", "param", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "step", "grad"):
        assert getattr(on, f) is None and getattr(off, f) is None or torch.equal(getattr(on, f), getattr(off, f)), (name, f)
    assert on.step.tolist() == [oref.ITERS]


def _valid_call(tr, mshape, theta, flow, scale=None, tmask=None, mmask=None):
    return tr.affine_flow_valid(mshape, theta, flow.cuda(), scale, tmask, mmask).cpu()


@pytest.mark.parametrize("name", list(oref.VALID_CASES))
def test_flow_valid_is_the_restatement_byte_for_byte(tr, name):
    """(e) on the warp cases of tests/affine_flow_ref.py (B = 2, a theta per pair, a flow off the voxel lattice; scale 1 or the world scale), each
    held 1e-4 voxel away from every decision by tests/test_mi_overlap_host.py: trx_affine_flow_valid equals the restatement on EVERY voxel, without
    masks and with both; repeated calls and a pair alone have the same bytes."""
    mshape, theta, flow, scale, tmask, mmask = oref.valid_case(name)
    i = oref.flow_coords(theta, flow, mshape, scale)
    for tm, mm in ((None, None), (tmask, mmask)):
        want = oref.valid_of(i, mshape, tm, mm)
        got = _valid_call(tr, mshape, theta, flow, scale, tm, mm)
        assert got.shape == want.shape and got.dtype == torch.uint8 and set(got.unique().tolist()) == {0, 1}
        assert torch.equal(got.bool(), want), (name, tm is not None, int((got.bool() != want).sum()))
        assert torch.equal(got, _valid_call(tr, mshape, theta, flow, scale, tm, mm))
        assert torch.equal(got[1:], _valid_call(tr, mshape, theta[1:], flow[1:], scale, None if tm is None else tm[1:], None if mm is None else mm[1:]))


@pytest.mark.parametrize("name", list(oref.FLOW_LOOPS))
def test_flow_valid_at_the_first_forward_of_the_loops(tr, name):
    """(e) on the flow the B-spline loops start from (trx_bspline_expand of the starting control tensor, fp32 on the GPU): the bytes of
    trx_affine_flow_valid equal the validity the fp64 arbiter takes in its first iteration, voxel for voxel."""
    mov, _, theta, mmask = oref.flow_loop_setup(name)[:4]
    want = oref.flow_loop_pair(name)[0][2][0]
    s = _flow_solver(tr, name)
    got = _valid_call(tr, tuple(mov.shape[2:]), theta, s.flow, None, None, mmask)
    assert torch.equal(got.bool(), want) and 0 < int(want.sum()) < want.numel()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. against the fp64 arbiter
# ---------------------------------------------------------------------------------------------------------------------------------------
def _chain(tr, mov, tgt, theta, scale, rng, valid, bins):
    """What the fused passes replace, in fp32 on the GPU, under the validity mask: (loss, dtheta, counts of trx_mi_histogram on the warped volume)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    eng = tr._engine
    s32 = scale.float().cuda()
    B, nd = tgt.shape[0], tgt.dim() - 2
    pair = eng._GridPair(mov, tgt, scale)
    th = eng.pad_theta(theta.cuda().reshape(B, -1), nd)
    warped = torch.empty_like(tgt)
    vol, mg = pair.vol(), pair.grid()
    _lib.check(lib.trx_affine_warp_grids(ctypes.byref(vol), ctypes.byref(mg), _lib.ptr(th), 1, _lib.ptr(warped), _lib.current_stream(torch.device("cuda"))),
               "trx_affine_warp_grids")
    loss, gw = eng.mi_loss_grad(tgt, warped, rng, bins, mask=valid)
    t = theta.float().cuda().clone().requires_grad_()
    w = F.grid_sample(mov, F.affine_grid(t * s32, list(tgt.shape), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
    (dth,) = torch.autograd.grad((w * gw).sum(), t)
    dhw = (1,) * (3 - nd) + tuple(tgt.shape[2:])
    n = lib.trx_mi_workspace_bytes(nd, B, *dhw, bins)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    cfg = eng._mi_cfg_c(bins, 1.0, False, rng, _u8(valid))
    _lib.check(lib.trx_mi_histogram(_lib.ptr(tgt), _lib.ptr(warped), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(ws), n, _lib.current_stream(torch.device("cuda"))),
               "trx_mi_histogram")
    torch.cuda.synchronize()
    return loss, dth, ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).clone()


@pytest.mark.parametrize("name", list(oref.CASES))
def test_single_evaluation_against_the_arbiter(tr, name):
    mov, tgt, theta, scale, tmask, mmask, rng = _gpu_case(name)
    (l64, g64, P64, valid), (l32, g32, P32, v32) = oref.case_arbiter(name)
    assert torch.equal(valid, v32)
    loss, dth, counts = _call(tr, mov, tgt, theta, scale, rng, tmask, mmask, overlap=True)
    c_loss, c_dth, c_counts = _chain(tr, mov, tgt, theta, scale, rng, valid, 32)
    nv = valid.flatten(1).sum(1).double()
    for b in range(2):
        err, bar = abs(loss[b].item() - l64[b].item()), max(2e-5 * abs(l64[b].item()), 4.0 * abs(l32[b].item() - l64[b].item()))
        print(f"{name}[{b}]: loss {l64[b].item():.6f} err {err:.2e} bar {bar:.2e} (chain err {abs(c_loss[b].item() - l64[b].item()):.2e})")
        assert err <= bar, (name, b, "loss", err, bar)
        gerr, ggap = (dth[b].double().cpu() - g64[b]).abs().max().item(), (g32[b] - g64[b]).abs().max().item()
        e_chain = (c_dth[b].double().cpu() - g64[b]).abs().max().item()
        print(f"{name}[{b}]: max|dtheta| {g64[b].abs().max().item():.3e} err {gerr:.2e}, arbiter fp32-fp64 {ggap:.2e}, chain err {e_chain:.2e}")
        assert g64[b].abs().max().item() > 0 and gerr <= max(4.0 * ggap, 2.0 * e_chain), (name, b, "dtheta", gerr, ggap, e_chain)
        P, Pc = counts[b].double().cpu() / (nv[b] * 2.0 ** 31), c_counts[b].double().cpu() / (nv[b] * 2.0 ** 31)
        perr, pgap, pchain = (P - P64[b]).abs().sum().item(), (P32[b] - P64[b]).abs().sum().item(), (Pc - P64[b]).abs().sum().item()
        print(f"{name}[{b}]: sum|P - P64| {perr:.2e}, arbiter fp32-fp64 {pgap:.2e}, chain histogram {pchain:.2e}")
        assert perr <= max(4.0 * pgap, 2.0 * pchain), (name, b, "table", perr, pgap, pchain)


def _affine_solver(tr, name, capacity=oref.ITERS):
    _, _, mode, optimizer, lr, voxels = oref.LOOPS[name][:6]
    mov, tgt, _, tmask, mmask, rng, start = oref.loop_setup(name)
    kw = {} if voxels is None else dict(moving_voxel=voxels[0], target_voxel=voxels[1])
    s = tr.AffineMISolver(mov.cuda(), tgt.cuda(), mode=mode, mi=dict(bins=32), optimizer=optimizer, lr=lr, init=start[None], capacity=capacity, mask=tmask,
                          overlap=True, moving_mask=mmask, **kw)
    assert torch.equal(s.mi_range.cpu(), rng)      # the solver's own fit: not widened to 0, inside both masks
    return s


@pytest.mark.parametrize("name", list(oref.LOOPS))
def test_affine_loop_vs_torch_autograd(tr, name):
    """trx_affine_mi_run_grids with the rule, 10 iterations: rigid / affine, Adam / SGD, 2-D, voxel sizes, both masks - against the fp64 arbiter, which
    re-decides validity in every iteration and holds it constant under autograd.  valid_fraction at the final theta is the restatement's."""
    r64, r32 = oref.loop_pair(name)
    s = _affine_solver(tr, name)
    s.run(oref.ITERS)
    torch.cuda.synchronize()
    mode = oref.LOOPS[name][2]
    nd = s.nd
    param = s.param[0, : (6 if nd == 3 else 3)] if mode == "rigid" else s.param[0, : nd * (nd + 1)]
    _loop_bars(s.losses[0, : oref.ITERS].cpu().double().numpy(), param.cpu().double().numpy().reshape(r64[1].shape), r64, r32, name)
    mov, tgt, scale, tmask, mmask, _, _ = oref.loop_setup(name)
    th = s.current_theta.cpu()
    valid = oref.valid_of(oref.affine_coords(th, scale, mov.shape[2:], tgt.shape[2:]), mov.shape[2:], tmask, mmask)
    total = tgt[0].numel() if tmask is None else int(tmask.sum())
    got = s.valid_fraction(s.current_theta).item()
    print(f"{name}: valid fraction {got:.6f}, restatement {int(valid.sum())} / {total}")
    assert abs(got * total - int(valid.sum())) <= 2      # (the final theta is not held away from the border planes: a sample or two may differ)


def _flow_solver(tr, name, capacity=oref.ITERS):
    mov, tgt, theta, mmask, rng, ctrl0, spacing, optimizer, lr = oref.flow_loop_setup(name)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=ctrl0, capacity=capacity, mi=dict(bins=32), initial=theta,
                         overlap=True, moving_mask=mmask)
    assert torch.equal(s.mi_range.cpu(), rng)
    return s


@pytest.mark.parametrize("name", list(oref.FLOW_LOOPS))
def test_bspline_loop_through_initial_vs_torch_autograd(tr, name):
    """trx_bspline_mi_run_grids with the rule on affine_flow_ref.LOOPS shapes, with and without a moving mask, 10 iterations; a run stepped one
    iteration per call has the same bits; the solver's valid_fraction is the byte count of trx_affine_flow_valid at its flow."""
    r64, r32 = oref.flow_loop_pair(name)
    s = _flow_solver(tr, name)
    s.run(oref.ITERS)
    torch.cuda.synchronize()
    _loop_bars(s.losses[0, : oref.ITERS].cpu().double().numpy(), s.ctrl.cpu().double().numpy(), r64, r32, name)
    t = _flow_solver(tr, name)
    for _ in range(oref.ITERS):
        t.run(1)
    assert torch.equal(t.losses, s.losses) and torch.equal(t.ctrl, s.ctrl)
    mov, tgt, theta, mmask = oref.flow_loop_setup(name)[:4]
    want = oref.valid_of(oref.flow_coords(theta, s.flow.cpu(), mov.shape[2:]), mov.shape[2:], None, mmask)
    assert abs(s.valid_fraction().item() * tgt[0].numel() - int(want.sum())) <= 2


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. memory
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_bspline_loop_stays_inside_its_buffers(tr):
    """The workspace at exactly trx_bspline_mi_grids_workspace_bytes - the validity bytes are its tail; one byte less is TRX_ERR_WORKSPACE - and the
    moving mask between canaries: 3 iterations leave the canaries intact and have the bits of the solver.  trx_affine_flow_valid writes exactly B N
    bytes."""
    from torchregister_amd import _lib
    lib = _lib.load()
    name, iters = "bspline-mmask", 3
    mov, tgt, theta, mmask, rng, ctrl0, spacing, optimizer, lr = oref.flow_loop_setup(name)
    want = _flow_solver(tr, name, capacity=iters)
    want.run(iters)
    tshape, mshape = tuple(tgt.shape[2:]), tuple(mov.shape[2:])
    gmask = _Guarded(math.prod(mshape), 0x69)
    gmask.region.copy_(_u8(mmask).reshape(-1))
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=ctrl0, capacity=iters, mi=dict(bins=32, moving_range=(rng[0, 2].item(), rng[0, 3].item())),
                         initial=theta, overlap=True)
    assert torch.equal(s.mi_range, want.mi_range)
    s.moving_grid.mask = gmask.region.data_ptr()
    n = lib.trx_bspline_mi_grids_workspace_bytes(3, 1, *tshape, *s.sp3, 32, ctypes.byref(s.moving_grid))
    base = lib.trx_bspline_mi_workspace_bytes(3, 1, *tshape, *s.sp3, 32)
    assert n == s.ws_bytes == base + ((math.prod(tshape) + 255) // 256) * 256
    ws = _Guarded(n, 0x5A)
    stream = _lib.current_stream(torch.device("cuda"))
    args = (ctypes.byref(s.vol), ctypes.byref(s.moving_grid), _lib.ptr(s.initial), ctypes.byref(s.mi), ctypes.byref(s.opt), ctypes.byref(s.state), s.sp3, iters)
    assert lib.trx_bspline_mi_run_grids(*args, _lib.ptr(ws.region), n - 1, stream) == -3
    _lib.check(lib.trx_bspline_mi_run_grids(*args, _lib.ptr(ws.region), n, stream), "trx_bspline_mi_run_grids")
    torch.cuda.synchronize()
    ws.check("the workspace")
    gmask.check("the moving mask")
    assert torch.equal(gmask.region, _u8(mmask).reshape(-1))
    assert torch.equal(s.losses, want.losses) and torch.equal(s.ctrl, want.ctrl)
    # the validity bytes of the last iteration are the tail of the workspace: the bytes of trx_affine_flow_valid at the last forward's flow
    tail = ws.region[base: base + math.prod(tshape)].cpu().reshape((1, 1) + tshape)
    assert torch.equal(tail, _valid_call(tr, mshape, theta, s.flow, None, None, mmask))      # (the direct call leaves s.flow at the last forward's flow)
    gv = _Guarded(math.prod(tshape), 0xC3)
    pair = tr._engine._GridPair(mov.cuda(), tgt.cuda())
    vol, mg = pair.vol(), pair.grid(True, gmask.region)
    fl = want.flow.contiguous()
    _lib.check(lib.trx_affine_flow_valid(ctypes.byref(vol), ctypes.byref(mg), _lib.ptr(want.initial), _lib.ptr(fl), None, _lib.ptr(gv.region), stream), "trx_affine_flow_valid")
    torch.cuda.synchronize()
    gv.check("the validity bytes")
    assert torch.equal(gv.region.cpu().reshape((1, 1) + tshape), _valid_call(tr, mshape, theta, fl, None, None, mmask))


def test_refusals_hold_on_the_gpu_machine(tr):
    check_refusals()
    check_python_refusals(torch.zeros(1, 1, 9, 7, 6, device="cuda"), torch.zeros(1, 1, 5, 6, 7, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair(tshape=(16, 18, 20), mshape=(22, 20, 17)):
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    return mov + 0.25, tgt


def test_register_end_to_end(tr):
    """The test that fails without the feature (optim has no `overlap` keyword there): a rigid device_loop stage with the rule on two lattices with
    voxel sizes, then the B-spline stage composed with it under the rule and a moving mask.  Each is the solver's run bit for bit, and
    reg.valid_fraction is the restatement's count at the returned transform."""
    import mi_mask_ref as mref
    mov, tgt = _pair()
    tshape, mshape = tuple(tgt.shape[2:]), tuple(mov.shape[2:])
    tvox, mvox = (1.5, 1.0, 1.0), (1.1, 0.9, 1.2)
    mmask = mref.ellipsoid(mshape, 1.1)
    rigid = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6))
    rigid.optim(mov, tgt, lr=0.01, max_epochs=8, moving_voxel=mvox, target_voxel=tvox, overlap=True)
    s = tr.AffineMISolver(mov, tgt, mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=torch.zeros(1, 6), capacity=8, moving_voxel=mvox,
                          target_voxel=tvox, overlap=True)
    s.run(8)
    assert torch.equal(rigid.losses, s.losses[:, :8]) and torch.equal(rigid.theta, s.effective(s.best))
    assert s.mi_range[0, 2].item() == mov.min().item() and s.mi_range[0, 3].item() == mov.max().item()      # the image's own range, whatever its sign
    ones = torch.ones(3, 4, dtype=torch.float64)
    want = oref.valid_of(oref.affine_coords(rigid.theta.cpu(), ones, mshape, tshape), mshape)
    got = rigid.valid_fraction
    print(f"rigid stage: valid fraction {got.tolist()}, restatement {int(want.sum())} / {want.numel()}")
    assert got.shape == (1,) and abs(got.item() * want.numel() - int(want.sum())) <= 2 and 0.3 < got.item() <= 1.0
    plain = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6))
    plain.optim(mov, tgt, lr=0.01, max_epochs=8, moving_voxel=mvox, target_voxel=tvox)
    assert plain.valid_fraction is None and not torch.equal(plain.losses, rigid.losses)

    reg = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4)
    reg.optim(mov, tgt, lr=0.05, max_epochs=8, initial=rigid, overlap=True, moving_mask=mmask)
    b = tr.BSplineSolver(mov, tgt, 4, optimizer="adam", lr=0.05, capacity=8, stop_crit=1e-4, keep_last=True, mi=dict(bins=32), initial=rigid.theta,
                         moving_mask=mmask)
    b.run(8)
    assert b.overlap and torch.equal(reg.losses, b.losses) and torch.equal(reg.control, b.ctrl) and torch.isfinite(reg.losses).all()
    want = oref.valid_of(oref.flow_coords(rigid.theta.cpu(), reg.theta.cpu(), mshape), mshape, None, mmask)
    got = reg.valid_fraction
    print(f"B-spline stage: valid fraction {got.tolist()}, restatement {int(want.sum())} / {want.numel()}")
    assert got.shape == (1,) and abs(got.item() * want.numel() - int(want.sum())) <= 2
    assert reg(mov).shape == (1, 1) + tshape
    reg.optim(mov, tgt, lr=0.05, max_epochs=2, initial=rigid)      # the rule is per call: off again, nothing left behind
    assert reg.valid_fraction is None


def test_register_two_levels_replayed_level_by_level(tr):
    """levels=2, rigid, both lattices, a moving mask: the coarse level is the solver on the two pyramids' coarse images with pyramid_masks of the moving
    mask over the MOVING pyramid; the fine level starts from its final pose; each level fits its own range."""
    import mi_mask_ref as mref
    from torchregister_amd.pyramid import pyramid_masks
    mov, tgt = _pair()
    mmask = mref.ellipsoid(tuple(mov.shape[2:]), 1.1).cuda()
    reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6), levels=2)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[6, 6], moving_mask=mmask)
    movs, tgts, mms = tr.pyramid(mov, 2), tr.pyramid(tgt, 2), pyramid_masks(mmask.to(torch.uint8), 2)
    assert tuple(mms[0].shape[2:]) == tuple(movs[0].shape[2:]) != tuple(tgts[0].shape[2:])
    pose = torch.zeros(1, 6)
    for k in range(2):
        s = tr.AffineMISolver(movs[k], tgts[k], mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=pose, capacity=6, moving_mask=mms[k])
        s.run(6)
        assert torch.equal(s.losses[:, :6], reg.level_losses[k]), k
        sel = movs[k][mms[k] != 0]
        assert s.mi_range[0, 2].item() == sel.min().item() and s.mi_range[0, 3].item() == sel.max().item()
        pose = s.param[:, :6].clone()
    assert torch.equal(reg.theta, s.effective(s.best)) and torch.equal(reg.valid_fraction, s.valid_fraction(s.best))
