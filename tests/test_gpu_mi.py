"""GPU checks of the Parzen joint-histogram mutual information (csrc/mi.hip) and of the two device-side loops over it (trx_flow_mi_run,
trx_bspline_mi_run): parity with the fp64 restatement (tests/mi_ref.py) at the shapes and ranges where the binning can go wrong, determinism and
batch independence, guard bytes, status codes, the loops against torch autograd on the CPU, the early stop, and the public surface (MILoss,
FlowSolver(mi=), BSplineSolver(mi=), Register).

Bars.  Kernel against restatement: 4 x (restatement in fp32 against restatement in fp64, same inputs: the kernel sums in another order) plus the
fixed-point bound of the histogram (include/trx.h: sum over cells of |P - exact| <= 3 * 2^-31):
  entropies   |dH| <= 3 * 2^-31 (ln N + ln 2^31 + 1) = E_H       (|d(p ln p)| <= |dp| (|ln p| + 1), no non-empty cell is below 1 / (N 2^31))
  loss        plain 2 alpha E_H,  normalized 4 alpha E_H / H_TW   ((H_T + H_W) / H_TW <= 2)
  gradient    1e-6 max|G| s_w / N: an outer weight r^3 / 6 below 2^-32 (r < 1.1e-3) adds nothing, a cell fed by such weights alone reads P = 0 and
              G = 0; those voxels lose G beta' with |beta'| = r^2 / 2 < 6.3e-7 on at most one tap, rounded up to 1e-6.
Measured on the CPU over the 8, 32 and 64 bin cases of the first test (fitted ranges): fp32-vs-fp64 gap of the loss 2e-9 .. 3.5e-6 (largest: 40^3, 8 bins,
normalized), of the gradient 2e-7 .. 1.1e-5 of its maximum; the loss bounds are 3.5e-8 .. 1.2e-7, the gradient bounds 2e-6 .. 2e-5 of its maximum.
On the MI355X the kernel's own errors were 1e-9 .. 5e-8 on the loss and 1e-7 .. 8e-6 of the maximum on the gradient.  Loops: max(floor of
test_gpu_bspline.py's loop test, 4 x the arbiter's own fp32-vs-fp64 gap); the arbiter's gaps: loss 2e-7 .. 4e-6, parameters 8e-7 .. 2.4e-4."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import bspline_bending_ref as bref
import bspline_ref
import mi_ref
import phantoms as ph
from test_gpu_bspline import _Guarded

pytestmark = pytest.mark.gpu

FIXED_P = 3.0 * 2.0 ** -31


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _images(shape, B=1, seed=0):
    """target: a blob phantom; warped: another blob phantom plus a ripple, through the non-monotone map 4x(1 - x)."""
    tgt = torch.cat([ph.blobs(shape, 31 + 7 * b + seed) for b in range(B)])
    w = torch.cat([ph.blobs(shape, 32 + 7 * b + seed) + 0.05 * ph.vol(shape, 0.029, "cos") for b in range(B)])
    return tgt, (4.0 * w * (1.0 - w)).float()


def _reference(tgt, wrp, rng, bins, alpha, normalized, dtype):
    """(loss [B], grad like wrp, max|G|, H_TW [B]) of the restatement with its weights and sums in `dtype`; the inputs stay fp32, so the bins and
    the coordinate are the kernel's."""
    w = wrp.clone().requires_grad_()
    loss = mi_ref.loss(tgt, w, bins, alpha, normalized, rng, dtype)
    (grad,) = torch.autograd.grad(loss.sum(), w)
    P = mi_ref.joint(tgt, wrp, bins, rng, torch.float64)
    gmax = mi_ref.grad_table(P, alpha, normalized).abs().flatten(1).amax(1)
    safe = torch.where(P > 0, P, torch.ones_like(P))
    return loss.detach().double(), grad.double(), gmax, -(P * torch.log(safe)).sum((1, 2))


def _check(tr, tgt, wrp, rng, bins, alpha, normalized, what):
    """One call against the restatement; returns the kernel's (loss, grad) and per pair max|G| s_w / N, the scale of a voxel's gradient."""
    l64, g64, gmax, h_tw = _reference(tgt, wrp, rng, bins, alpha, normalized, torch.float64)
    l32, g32, _, _ = _reference(tgt, wrp, rng, bins, alpha, normalized, torch.float32)
    loss, grad = tr._engine.mi_loss_grad(tgt.cuda(), wrp.cuda(), rng.cuda(), bins, alpha, normalized)
    B, N = tgt.shape[0], tgt[0].numel()
    e_h = FIXED_P * (math.log(N) + 31.0 * math.log(2.0) + 1.0)
    _, s_w = mi_ref.scales(rng, bins)
    for b in range(B):
        fixed = abs(alpha) * (4.0 * e_h / h_tw[b].item() if normalized else 2.0 * e_h)
        gap = abs(l32[b].item() - l64[b].item())
        err = abs(loss[b].item() - l64[b].item())
        print(f"{what} pair {b}: loss {l64[b].item():.6f} err {err:.2e} (fp32 gap {gap:.2e}, fixed point {fixed:.2e})")
        assert err <= 4.0 * gap + fixed, (what, b, err, gap, fixed)
        gfix = 1e-6 * gmax[b].item() * s_w[b].item() / N
        ggap = (g32[b] - g64[b]).abs().max().item()
        gerr = (grad[b].double().cpu() - g64[b]).abs().max().item()
        print(f"{what} pair {b}: max|grad| {g64[b].abs().max().item():.3e} err {gerr:.2e} (fp32 gap {ggap:.2e}, fixed point {gfix:.2e})")
        assert gerr <= 4.0 * ggap + gfix, (what, b, gerr, ggap, gfix)
    return loss, grad, gmax * s_w.double() / N


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. trx_mi_loss_grad against the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
@pytest.mark.parametrize("bins", [8, 32, 48, 64])
@pytest.mark.parametrize("shape", [(5, 6, 7), (12, 14, 16), (40, 40, 40), (13, 17)], ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradient_match_the_restatement(tr, shape, bins, normalized):
    """Fitted ranges.  5x6x7: less than one block; 40^3 = 64000 voxels: four blocks of 16384, the last one partial; 13x17: 2-D; 8 and 32 bins: one
    table per wave; 48: three tables, waves 0 and 3 share one; 64: two tables."""
    tgt, wrp = _images(shape)
    _check(tr, tgt, wrp, mi_ref.fit_range(tgt, wrp), bins, 1.0, normalized, f"{shape} K={bins}")


@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
def test_three_pairs_with_three_ranges(tr, normalized):
    """B = 3: a fitted range, one narrower than the data on both images (values outside fall into the end bins and get a zero gradient) and one
    wider than the data; alpha = 2.5."""
    tgt, wrp = _images((12, 14, 16), B=3)
    rng = mi_ref.fit_range(tgt, wrp)
    rng[1] = torch.tensor([0.15, 0.7, 0.1, 0.8])
    rng[2] = torch.tensor([-0.5, 1.5, -1.0, 2.0])
    _, grad, _ = _check(tr, tgt, wrp, rng, 32, 2.5, normalized, "three ranges")
    outside = (wrp[1] < 0.1) | (wrp[1] > 0.8)
    assert outside.any() and not outside.all()
    assert grad[1].cpu()[outside].abs().max().item() == 0.0


@pytest.mark.parametrize("normalized", [False, True], ids=["plain", "normalized"])
def test_values_on_the_ends_of_the_range_and_a_constant_image(tr, normalized):
    """Voxels exactly on lo_t, hi_t, lo_w and hi_w (the top end lands in the last bin: r = 1 on c = K - 3) against the restatement, whose
    inclusive clamp mask the kernel shares; then a constant warped image, with a fitted range (empty at 0: s_w = 0 ... the constant) and with
    a given one: the loss is finite and the gradient is zero to the rounding of the fp32 table (four taps, |beta'| <= 1, each entry of G off by
    at most 2^-24 max|G|: 2^-22 max|G| s_w / N)."""
    tgt, wrp = _images((12, 14, 16))
    rng = torch.tensor([[0.2, 0.6, 0.1, 0.7]])
    t, w = tgt.clone().flatten(), wrp.clone().flatten()
    t[0:40:4], t[1:40:4] = 0.2, 0.6
    w[100:140:4], w[101:140:4], w[2:40:4], w[3:40:4] = 0.1, 0.7, 0.1, 0.7
    _check(tr, t.view_as(tgt), w.view_as(wrp), rng, 32, 1.0, normalized, "range ends")
    for value, r in ((0.37, None), (0.0, None), (0.37, torch.tensor([[0.0, 1.0, 0.0, 1.0]]))):
        const = torch.full_like(wrp, value)
        rr = mi_ref.fit_range(tgt, const) if r is None else r
        loss, grad, scale = _check(tr, tgt, const, rr, 32, 1.0, normalized, f"constant {value}")
        assert torch.isfinite(loss).all() and grad.abs().max().item() <= 2.0 ** -22 * scale[0].item()


def test_loss_only_call_gives_the_same_bits(tr):
    tgt, wrp = (t.cuda() for t in _images((12, 14, 16), B=2))
    rng = tr._engine.mi_range(tgt, wrp)
    for normalized in (False, True):
        with_grad, _ = tr._engine.mi_loss_grad(tgt, wrp, rng, 32, 1.0, normalized)
        alone, none = tr._engine.mi_loss_grad(tgt, wrp, rng, 32, 1.0, normalized, need_grad=False)
        assert none is None and torch.equal(with_grad, alone)


def test_fitted_ranges_match_the_restatement(tr):
    tgt, wrp = _images((12, 14, 16), B=2)
    wrp[1] = wrp[1] + 0.5                      # strictly positive: the range is widened down to 0
    assert torch.equal(tr._engine.mi_range(tgt.cuda(), wrp.cuda()).cpu(), mi_ref.fit_range(tgt, wrp))
    assert tr._engine.mi_range(tgt.cuda(), wrp.cuda(), (0.0, 2.0), (-1.0, 1.0)).cpu().tolist() == [[0.0, 2.0, -1.0, 1.0]] * 2


@pytest.mark.parametrize("bins", [32, 48, 64])
def test_histogram_pass_alone(tr, bins):
    """trx_mi_histogram: the 64-bit counts of every pair sum to N * 2^31 exactly (each voxel adds exactly one), equal the restatement's table
    within the fixed-point bound plus the fp32 rounding of the weights (per cell 1.5 * 2^-31 + 2^-22 of the cell's share of voxels, bounded here by
    2^-21 overall), and the call has trx_mi_loss_grad's status codes."""
    from torchregister_amd import _lib
    lib = _lib.load()
    B, shape = 2, (40, 40, 40)
    N = math.prod(shape)
    tgt, wrp = _images(shape, B=B)
    rng = mi_ref.fit_range(tgt, wrp)
    t, w, r = tgt.cuda(), wrp.cuda(), rng.cuda()
    n = lib.trx_mi_workspace_bytes(3, B, *shape, bins)
    ws = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    cfg = _cfg(_lib, r, bins)
    stream = _lib.current_stream(torch.device("cuda"))
    args = (_lib.ptr(t), _lib.ptr(w), 3, B, *shape, ctypes.byref(cfg))
    assert lib.trx_mi_histogram(*args, None, n, stream) == -1 and lib.trx_mi_histogram(*args, _lib.ptr(ws), n - 1, stream) == -3
    assert lib.trx_mi_histogram(_lib.ptr(t), _lib.ptr(w), 4, B, *shape, ctypes.byref(cfg), _lib.ptr(ws), n, stream) == -2
    assert lib.trx_mi_histogram(_lib.ptr(t), _lib.ptr(w), 3, B, *shape, ctypes.byref(_cfg(_lib, r, 65)), _lib.ptr(ws), n, stream) == -1
    torch.cuda.synchronize()
    assert bool((ws == 0x5A).all())
    _lib.check(lib.trx_mi_histogram(*args, _lib.ptr(ws), n, stream), "trx_mi_histogram")
    torch.cuda.synchronize()
    counts = ws[: B * bins * bins * 8].view(torch.int64).view(B, bins, bins).cpu()
    assert (counts >= 0).all() and counts.sum((1, 2)).tolist() == [N * 2 ** 31] * B
    P = counts.double() / (N * 2.0 ** 31)
    want = mi_ref.joint(tgt, wrp, bins, rng)
    err = (P - want).abs().max().item()
    print(f"K={bins}: max|P - restatement| {err:.2e}")
    assert err <= 2.0 ** -21
    assert bool(((P == 0) | (want > 0)).all())                   # no weight lands in a cell the restatement leaves empty


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. reproducibility
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [32, 64])
def test_two_calls_give_equal_bits_and_pairs_do_not_see_each_other(tr, bins):
    tgt, wrp = (t.cuda() for t in _images((40, 40, 40), B=3))
    rng = tr._engine.mi_range(tgt, wrp)
    for normalized in (False, True):
        l1, g1 = tr._engine.mi_loss_grad(tgt, wrp, rng, bins, 1.0, normalized)
        l2, g2 = tr._engine.mi_loss_grad(tgt, wrp, rng, bins, 1.0, normalized)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)
        ls, gs = tr._engine.mi_loss_grad(tgt[1:2], wrp[1:2], rng[1:2], bins, 1.0, normalized)
        assert torch.equal(l1[1:2], ls) and torch.equal(g1[1:2], gs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. guard bytes and status codes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cfg(_lib, rng, bins=32, alpha=1.0, normalized=0):
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, alpha, normalized, rng.data_ptr() if rng is not None else None
    return cfg


@pytest.mark.parametrize("B,shape,bins", [(2, (12, 14, 16), 32), (1, (40, 40, 40), 64), (3, (13, 17), 8)])
def test_calls_stay_inside_their_buffers(tr, B, shape, bins):
    """The workspace at exactly trx_mi_workspace_bytes, loss and grad at their sizes: canaries intact, bits of the wrapper."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd = len(shape)
    dhw = (1,) * (3 - nd) + shape
    tgt, wrp = (t.cuda() for t in _images(shape, B=B))
    rng = tr._engine.mi_range(tgt, wrp)
    ws_bytes = lib.trx_mi_workspace_bytes(nd, B, *dhw, bins)
    assert ws_bytes > 0
    ws, loss, grad = _Guarded(ws_bytes, 0x5A), _Guarded(B * 4, 0xA5), _Guarded(B * math.prod(shape) * 4, 0xC3)
    cfg = _cfg(_lib, rng, bins)
    rc = lib.trx_mi_loss_grad(_lib.ptr(tgt), _lib.ptr(wrp), nd, B, *dhw, ctypes.byref(cfg), _lib.ptr(loss.region), _lib.ptr(grad.region),
                              _lib.ptr(ws.region), ws_bytes, _lib.current_stream(torch.device("cuda")))
    _lib.check(rc, "trx_mi_loss_grad")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (loss, "loss"), (grad, "grad")):
        buf.check(what)
    want_l, want_g = tr._engine.mi_loss_grad(tgt, wrp, rng, bins)
    assert torch.equal(loss.floats((B,)), want_l) and torch.equal(grad.floats(wrp.shape), want_g)


def test_status_codes_come_before_any_launch(tr):
    from torchregister_amd import _lib
    lib = _lib.load()
    OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5
    shape, B = (12, 14, 16), 1
    tgt, wrp = (t.cuda() for t in _images(shape))
    rng = tr._engine.mi_range(tgt, wrp)
    n = lib.trx_mi_workspace_bytes(3, B, *shape, 32)
    ws, loss, grad = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.full((B,), 7.0, device="cuda"), torch.full_like(wrp, 7.0)
    stream = _lib.current_stream(torch.device("cuda"))
    P = _lib.ptr

    def call(t=tgt, w=wrp, nd=3, b=B, dhw=shape, cfg=_cfg(_lib, rng), lo=loss, ws_=ws, nbytes=n):
        c = ctypes.byref(cfg) if cfg is not None else None
        return lib.trx_mi_loss_grad(P(t), P(w), nd, b, *dhw, c, P(lo), P(grad), P(ws_), nbytes, stream)

    assert [lib.trx_mi_workspace_bytes(3, B, *shape, k) for k in (7, 65)] == [0, 0] and lib.trx_mi_workspace_bytes(2, B, *shape, 32) == 0
    assert lib.trx_mi_workspace_bytes(3, B, *shape, 8) > 0 and lib.trx_mi_workspace_bytes(3, B, *shape, 64) > 0
    assert call(t=None) == ARG and call(w=None) == ARG and call(cfg=None) == ARG and call(lo=None) == ARG and call(ws_=None) == ARG
    assert call(cfg=_cfg(_lib, None)) == ARG
    assert call(cfg=_cfg(_lib, rng, bins=7)) == ARG and call(cfg=_cfg(_lib, rng, bins=65)) == ARG
    assert call(cfg=_cfg(_lib, rng, alpha=float("nan"))) == ARG
    assert call(b=0) == ARG and call(dhw=(0, 14, 16)) == ARG
    assert call(nd=4) == NDIM and call(nd=2) == NDIM
    assert call(nbytes=n - 1) == WS
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and bool((grad == 7.0).all())           # nothing ran
    assert call() == OK

    # the loops
    mov = wrp
    batch = tr._engine._Batch(mov, tgt, tables=False)
    vol = batch.vol()
    opt = tr._engine.opt_cfg("adam", 0.1)
    flow = torch.zeros((1, 3) + shape, device="cuda")
    m, v = torch.zeros_like(flow), torch.zeros_like(flow)
    step, losses = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1, 2), float("nan"), device="cuda")
    st = _lib.FlowState()
    st.flow, st.adam_m, st.adam_v, st.losses, st.losses_capacity, st.step = flow.data_ptr(), m.data_ptr(), v.data_ptr(), losses.data_ptr(), 2, step.data_ptr()
    nf = lib.trx_flow_mi_workspace_bytes(ctypes.byref(vol), 32)
    assert nf > 0 and lib.trx_flow_mi_workspace_bytes(ctypes.byref(vol), 65) == 0
    wf = torch.zeros(nf, dtype=torch.uint8, device="cuda")
    cfg = _cfg(_lib, rng)

    def frun(vol_=vol, cfg_=cfg, iters=1, nbytes=nf):
        return lib.trx_flow_mi_run(ctypes.byref(vol_), ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(opt), ctypes.byref(st), iters,
                                   P(wf), nbytes, stream)

    t2, w2 = (t.cuda() for t in _images((13, 17)))
    vol2 = tr._engine._Batch(w2, t2, tables=False).vol()
    assert lib.trx_flow_mi_workspace_bytes(ctypes.byref(vol2), 32) == 0 and frun(vol_=vol2) == NDIM
    assert frun(cfg_=None) == ARG and frun(cfg_=_cfg(_lib, None)) == ARG and frun(cfg_=_cfg(_lib, rng, bins=65)) == ARG and frun(iters=-1) == ARG
    assert frun(nbytes=nf - 1) == WS and frun(iters=3) == CAP

    d3 = (ctypes.c_int * 3)(4, 4, 4)
    G = bspline_ref.grid(shape, 4)
    ctrl = torch.zeros((1, 3) + G, device="cuda")
    cm, cv, dflow = torch.zeros_like(ctrl), torch.zeros_like(ctrl), torch.zeros_like(flow)
    bs = _lib.BSplineState()
    bs.ctrl, bs.adam_m, bs.adam_v, bs.flow, bs.dflow = ctrl.data_ptr(), cm.data_ptr(), cv.data_ptr(), flow.data_ptr(), dflow.data_ptr()
    bs.losses, bs.losses_capacity, bs.step = losses.data_ptr(), 2, step.data_ptr()
    nb = lib.trx_bspline_mi_workspace_bytes(3, 1, *shape, 4, 4, 4, 32)
    assert nb > 0 and lib.trx_bspline_mi_workspace_bytes(3, 1, *shape, 4, 4, 4, 7) == 0 and lib.trx_bspline_mi_workspace_bytes(3, 1, *shape, 0, 4, 4, 32) == 0
    wb = torch.zeros(nb, dtype=torch.uint8, device="cuda")

    def brun(cfg_=cfg, iters=1, nbytes=nb, lam=0.0, vol_=vol):
        bs.bending_weight = lam
        return lib.trx_bspline_mi_run(ctypes.byref(vol_), ctypes.byref(cfg_) if cfg_ is not None else None, ctypes.byref(opt), ctypes.byref(bs), d3, iters,
                                      P(wb), nbytes, stream)

    assert brun(cfg_=None) == ARG and brun(cfg_=_cfg(_lib, None)) == ARG and brun(cfg_=_cfg(_lib, rng, bins=7)) == ARG and brun(lam=-1.0) == ARG
    assert brun(iters=-1) == ARG and brun(nbytes=nb - 1) == WS and brun(iters=3) == CAP
    bad = tr._engine._Batch(mov, tgt, tables=False).vol()
    bad.ndim = 4
    assert brun(vol_=bad) == NDIM
    torch.cuda.synchronize()
    assert step.item() == 0 and bool(torch.isnan(losses).all()) and torch.count_nonzero(flow).item() == 0 and torch.count_nonzero(ctrl).item() == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the loops against torch autograd on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def _multimodal(shape, B=1):
    """The pair of tests/test_mi_host.py: a blob phantom; the same phantom warped by a small flow and sent through 4x(1 - x)."""
    from oracle import compose
    tgt = torch.cat([ph.blobs(shape, 3 + b) for b in range(B)])
    flow = ph.flow_field(shape, amp=1.2, f=0.013).expand(B, -1, *shape)
    w = compose.flow_warp(tgt, flow)
    return (4.0 * w * (1.0 - w)).float(), tgt


def _arbiter(mov, tgt, rng, iters, optimizer, lr, dtype, mi, spacing=None, param0=None, base=None, lam=0.0, smooth=0.0):
    """oracle/compose.py::flow_warp + mi_ref.loss (+ bspline_ref.expand, bspline_bending_ref, smooth_regulariser) under torch autograd +
    torch.optim on the CPU: spacing None optimises the flow itself.  Returns (losses [iters], final parameter)."""
    from oracle import compose
    sp = tuple(mov.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    p = param0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        flow = p if spacing is None else bspline_ref.expand(p, sp, spacing, base=None if base is None else base.to(dtype), dtype=dtype)
        e = mi_ref.loss(tgt, compose.flow_warp(mov, flow), rng=rng, dtype=dtype, **mi).sum()
        if lam:
            e = e + lam * bref.energy_squares(p, sp, spacing, dtype=dtype).sum()
        if smooth:
            e = e + compose.smooth_regulariser(p, smooth)
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy()


@functools.lru_cache(maxsize=None)
def _arbiter_pair(key):
    """fp64 and fp32 runs of one loop configuration, computed once."""
    shape, optimizer, lr, normalized, spacing, with_base, lam, smooth, iters = key
    mov, tgt = _multimodal(shape)
    rng = mi_ref.fit_range(tgt, mov)
    nd = len(shape)
    if spacing is None:
        p0 = 0.3 * ph.flow_field(shape, 1.0, 0.05) + 0.17            # off the voxel lattice, where the trilinear derivative is one-sided
    else:
        g = torch.Generator().manual_seed(7)
        p0 = (torch.rand((1, nd) + bspline_ref.grid(shape, spacing), generator=g) - 0.5) * 0.4
    base = 0.3 * ph.flow_field(shape, 1.0, 0.05) if with_base else None
    kw = dict(mi=dict(bins=32, alpha=1.0, normalized=normalized), spacing=spacing, param0=p0, base=base, lam=lam, smooth=smooth)
    r64 = _arbiter(mov, tgt, rng, iters, optimizer, lr, torch.float64, **kw)
    r32 = _arbiter(mov, tgt, rng, iters, optimizer, lr, torch.float32, **kw)
    return mov, tgt, p0, base, r64, r32


def _loop_bars(got_losses, got_param, r64, r32, what):
    (l64, p64), (l32, p32) = r64, r32
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    e, b = np.max(np.abs(got_losses - l64)), max(2e-5 * np.max(np.abs(l64)), 4.0 * lgap)
    print(f"{what} loss curve {l64[0]:.5f} -> {l64[-1]:.5f}: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {lgap:.3e})")
    assert e <= b, (what, "loss curve", e, b)
    e, b = np.max(np.abs(got_param - p64)), max(2e-4, 4.0 * pgap)
    print(f"{what} parameters: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {pgap:.3e})")
    assert e <= b, (what, "parameters", e, b)


# learning rates chosen on the CPU so that the arbiter's loss falls in every iteration (asserted) and its fp32 and fp64 runs stay together (direct
# flow: Adam 0.1 or SGD 10 and above move single voxels by whole voxels per step and the two precisions part by 0.06 .. 3 voxels within 10
# iterations; lattice: SGD 15 and above overshoots, the loss rises in between)
FLOW_LOOPS = [((12, 14, 16), "adam", 0.05, False, 0.0), ((12, 14, 16), "sgd", 3.0, False, 0.0), ((12, 14, 16), "adam", 0.05, True, 0.05)]


@pytest.mark.parametrize("shape,optimizer,lr,normalized,smooth", FLOW_LOOPS, ids=["adam", "sgd", "adam-normalized-smooth"])
def test_flow_mi_loop_vs_torch_autograd(tr, shape, optimizer, lr, normalized, smooth):
    """trx_flow_mi_run, 10 iterations from a small flow off the voxel lattice, against the arbiter in fp64."""
    iters = 10
    mov, tgt, p0, _, r64, r32 = _arbiter_pair((shape, optimizer, lr, normalized, None, False, 0.0, smooth, iters))
    assert np.all(np.diff(r64[0]) < 0)
    s = tr.FlowSolver(mov.cuda(), tgt.cuda(), optimizer=optimizer, lr=lr, init=p0, capacity=iters, smooth_weight=smooth,
                      mi=dict(bins=32, normalized=normalized))
    s.run(iters)
    torch.cuda.synchronize()
    assert int(s.step[0]) == iters
    _loop_bars(s.losses[0].cpu().numpy(), s.flow.cpu().numpy(), r64, r32, f"flow {optimizer}")


BSPLINE_LOOPS = [((12, 14, 16), 4, "adam", 0.1, False, False, 0.0), ((12, 14, 16), 4, "sgd", 10.0, False, False, 0.0),
                 ((24, 28), 5, "adam", 0.1, False, False, 0.0), ((12, 14, 16), 4, "adam", 0.1, True, True, 0.0),
                 ((12, 14, 16), 4, "adam", 0.1, False, False, 50.0), ((24, 28), 5, "adam", 0.1, True, True, 50.0)]


@pytest.mark.parametrize("shape,spacing,optimizer,lr,normalized,with_base,lam", BSPLINE_LOOPS,
                         ids=["adam", "sgd", "2d", "base-normalized", "bending", "2d-base-bending-normalized"])
def test_bspline_mi_loop_vs_torch_autograd(tr, shape, spacing, optimizer, lr, normalized, with_base, lam):
    """trx_bspline_mi_run, 10 iterations from a random control tensor of amplitude 0.2, against the arbiter in fp64."""
    iters = 10
    mov, tgt, p0, base, r64, r32 = _arbiter_pair((shape, optimizer, lr, normalized, spacing, with_base, lam, 0.0, iters))
    assert np.all(np.diff(r64[0]) < 0)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=p0, base=None if base is None else base.cuda(), capacity=iters,
                         bending_weight=lam, mi=dict(bins=32, normalized=normalized))
    s.run(iters)
    torch.cuda.synchronize()
    assert int(s.step[0]) == iters
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), r64, r32, f"bspline {optimizer}")
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing, base=None if base is None else base.cuda()))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. early stop, bit for bit against uninterrupted runs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, kind, mov, tgt, **kw):
    if kind == "flow":
        return tr.FlowSolver(mov, tgt, optimizer="adam", lr=0.05, mi=dict(bins=32), **kw)
    return tr.BSplineSolver(mov, tgt, 4, optimizer="adam", lr=0.1, mi=dict(bins=32), bending_weight=20.0, **kw)


@pytest.mark.parametrize("calls", ["one", "split"])
@pytest.mark.parametrize("kind", ["flow", "bspline"])
def test_mi_loops_stop_exactly(tr, kind, calls):
    """stop_crit between two recorded losses of a probe run: step = index + 1, that iteration's update has been applied, flow_last is the flow of
    that forward, nothing changes afterwards - bit for bit against un-stopped solvers run k + 1 and k iterations.  B = 2 with the second pair
    scaled so that it never meets the threshold: it runs on."""
    N, k = 10, 4
    mov, tgt = (t.cuda() for t in _multimodal((12, 14, 16), B=2))
    tgt = torch.cat([tgt[:1], torch.roll(tgt[1:], 3, dims=4)])            # pair 1 is misaligned further: its loss stays above pair 0's
    free = _solver(tr, kind, mov, tgt, capacity=N)
    free.run(N)
    L = free.losses.cpu().numpy().astype(np.float64)
    assert np.all(np.diff(L[0, : k + 2]) < 0), "the probe run must descend so that a threshold between two losses is well defined"
    crit = 0.5 * (L[0, k] + L[0, k - 1])
    assert L[1].min() > crit
    s = _solver(tr, kind, mov, tgt, capacity=N, stop_crit=crit)
    if calls == "one":
        s.run(N)
    else:
        s.run(3)
        s.run(4)
        s.run(N - 7)
    torch.cuda.synchronize()
    assert s.step.cpu().tolist() == [k + 1, N] and (s.stopped.cpu() != 0).tolist() == [True, False]
    assert torch.equal(s.losses[0, : k + 1], free.losses[0, : k + 1]) and bool(torch.isnan(s.losses[0, k + 1:]).all())
    assert torch.equal(s.losses[1], free.losses[1])
    after, before = _solver(tr, kind, mov, tgt, capacity=N, keep_last=True), _solver(tr, kind, mov, tgt, capacity=N)
    after.run(k + 1)
    before.run(k)
    torch.cuda.synchronize()
    param = (lambda x: x.flow) if kind == "flow" else (lambda x: x.ctrl)
    assert torch.equal(param(s)[0], param(after)[0]) and torch.equal(param(s)[1], param(free)[1])
    assert torch.equal(s.flow_last[0], before.flow[0]) and torch.equal(s.flow_last[0], after.flow_last[0])
    assert not torch.equal(s.flow_last[0], s.flow[0])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. public surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register_mi(tr, levels):
    return tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="bspline", spacing=4, optimizer="adam", levels=levels)


def _arbiter_level(mov, tgt, base, iters=10):
    """fp64 and fp32 arbiter runs of one level as flow_register runs it: ranges fitted to that level's (target, moving), a zero lattice on `base`."""
    shape = tuple(mov.shape[2:])
    rng = mi_ref.fit_range(tgt, mov)
    kw = dict(mi=dict(bins=32, alpha=1.0, normalized=False), spacing=4, param0=torch.zeros((1, 3) + bspline_ref.grid(shape, 4)), base=base)
    return [_arbiter(mov, tgt, rng, iters, "adam", 0.1, dt, **kw) for dt in (torch.float64, torch.float32)]


def test_register_bspline_with_mutual_information(tr):
    """Register('flow', criterion=[MILoss()], flow_model='bspline') on the multimodal pair, one level: the loss falls, the loss curve and the
    control tensor are the arbiter's (Adam, lr 0.1, 10 iterations from zero) within the loop bars, reg(moving) is the warp by reg.theta."""
    shape = (12, 14, 16)
    mov, tgt = _multimodal(shape)
    reg = _register_mi(tr, 1)
    reg.optim(mov.cuda(), tgt.cuda(), lr=0.1, max_epochs=10)
    losses = reg.losses[0].cpu().numpy()
    assert losses.shape == (10,) and np.all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 4) and reg.theta.shape == (1, 3) + shape
    assert torch.equal(reg(mov.cuda()), tr._engine.flow_warp(mov.cuda(), reg.theta))
    assert torch.equal(reg.final_theta, tr.bspline_expand(reg.control, shape, 4))
    r64, r32 = _arbiter_level(mov, tgt, None)
    _loop_bars(losses, reg.control.cpu().numpy(), r64, r32, "Register")


def test_register_bspline_with_mutual_information_two_levels(tr):
    """levels=2 on 24x28x32.  The arbiter follows the levels on the package's own pyramid images (tr.pyramid; the resampling has its own tests):
    coarse level - ranges fitted to the coarse (target, moving), zero lattice, no base - against a single-level Register on those images, whose
    loss curve is bit for bit level_losses[0]; fine level - ranges fitted to the fine images, zero lattice on base = upsample_flow(coarse final
    flow) - against reg.level_losses[1] and reg.control, both within the loop bars.  A level that fitted its ranges to other images or took
    another base would miss them.  Measured: fine level, loss curve err 1.3e-8 (bar 5.7e-6), control err 7.6e-5 (bar 3.2e-4).  On the blurred
    coarse images the arbiter's own fp32 and fp64 control tensors part by 0.6 within the 10 iterations (Adam normalises gradients that sit at
    rounding level), so there the control bar is wide and the check that binds is the loss curve (err 7e-7, bar 1.1e-3)."""
    shape = (24, 28, 32)
    mov, tgt = _multimodal(shape)
    m, t = mov.cuda(), tgt.cuda()
    reg = _register_mi(tr, 2)
    reg.optim(m, t, lr=0.1, max_epochs=10)
    assert [ls.shape[-1] for ls in reg.level_losses] == [10, 10]
    l0, l1 = (ls[0].cpu().numpy() for ls in reg.level_losses)
    print(f"coarse {l0[0]:.5f} -> {l0[-1]:.5f}, fine {l1[0]:.5f} -> {l1[-1]:.5f}")
    assert np.all(np.isfinite(l0)) and np.all(np.isfinite(l1)) and l0[-1] < l0[0] and l1[-1] < l1[0]
    assert torch.equal(reg(m), tr._engine.flow_warp(m, reg.theta))
    assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 4)
    mc, tc = tr.pyramid(m, 2, align_corners=True)[0], tr.pyramid(t, 2, align_corners=True)[0]
    coarse = _register_mi(tr, 1)
    coarse.optim(mc, tc, lr=0.1, max_epochs=10)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    r64, r32 = _arbiter_level(mc.cpu(), tc.cpu(), None)
    _loop_bars(l0, coarse.control.cpu().numpy(), r64, r32, "coarse level")
    base = tr.upsample_flow(coarse.final_theta, shape)
    r64, r32 = _arbiter_level(mov, tgt, base.cpu())
    _loop_bars(l1, reg.control.cpu().numpy(), r64, r32, "fine level")
    assert torch.equal(reg.final_theta, tr.bspline_expand(reg.control, shape, 4, base=base))


def test_flow_register_dispatch(tr):
    """MILoss alone: direct flow in 3-D runs trx_flow_mi_run with alpha * weight folded; mixed lists take the generic path for 'direct' and raise
    for 'bspline'; 2-D direct takes the generic path with the same criterion."""
    import torch.nn as nn
    shape = (12, 14, 16)
    mov, tgt = (t.cuda() for t in _multimodal(shape))
    fr = tr.flow_register(shape, criterions=[tr.MILoss(alpha=2.0)], weights=[0.5], lr=0.1, max_epochs=5, flow_model="direct", optimizer="adam", stop_crit=-1.0)
    fr.optimize(mov, tgt, debug=False)
    s = tr.FlowSolver(mov, tgt, optimizer="adam", lr=0.1, capacity=5, mi=dict(bins=32, alpha=1.0))
    s.run(5)
    torch.cuda.synchronize()
    assert fr.solver.mi is not None and torch.equal(fr.losses, s.losses) and torch.equal(fr.final_flow, s.flow)
    mixed = tr.flow_register(shape, criterions=[tr.MILoss(), nn.MSELoss()], weights=[1.0, 1.0], lr=0.1, max_epochs=2, flow_model="direct", optimizer="adam",
                             stop_crit=-1.0)
    mixed.optimize(mov, tgt, debug=False)
    assert not hasattr(mixed, "solver") and mixed.losses.shape == (1, 2)
    with pytest.raises(ValueError, match="MILoss alone"):
        tr.flow_register(shape, criterions=[tr.MILoss(), nn.MSELoss()], weights=[1.0, 1.0], flow_model="bspline", spacing=4)
    with pytest.raises(ValueError):
        tr.MILoss(bins=7)
    with pytest.raises(ValueError, match="data term of its own"):
        tr.FlowSolver(mov, tgt, loss=tr.LossSpec(w_mse=1.0), mi=dict(bins=32))
    with pytest.raises(ValueError, match="data term of its own"):
        tr.BSplineSolver(mov, tgt, 4, loss=tr.LossSpec(w_mse=1.0), mi=dict(bins=32))
    m2, t2 = (t.cuda() for t in _multimodal((24, 28)))
    two = tr.flow_register((24, 28), criterions=[tr.MILoss()], weights=[1.0], lr=0.1, max_epochs=3, flow_model="direct", optimizer="adam", stop_crit=-1.0)
    two.optimize(m2, t2, debug=False)
    ls = two.losses[0].numpy()
    assert ls.shape == (3,) and np.all(np.isfinite(ls)) and ls[-1] < ls[0]


def test_miloss_module_and_the_generic_affine_loop(tr):
    """MILoss is an autograd criterion: its value is the batch mean of the kernel's losses with ranges fitted to the call, its gradient the
    kernel's divided by B; inside Register('affine', honor_criterion=True) it drives the generic loop to a finite, decreasing loss."""
    tgt, wrp = (t.cuda() for t in _images((12, 14, 16), B=2))
    w = wrp.clone().requires_grad_()
    crit = tr.MILoss(bins=16, alpha=1.5, normalized=True)
    v = crit(tgt, w)
    v.backward()
    loss, grad = tr._engine.mi_loss_grad(tgt, wrp, tr._engine.mi_range(tgt, wrp), 16, 1.5, True)
    assert torch.equal(v.detach(), loss.mean()) and torch.allclose(w.grad, grad / 2, rtol=1e-6, atol=0.0)
    assert "MILoss" in dir(__import__("TorchRegister"))
    from oracle import compose
    shape = (16, 18, 20)
    t = ph.blobs(shape, 5)
    m = compose.affine_warp(torch.tensor(ph.THETA_STAR3), t)
    m = (4.0 * m * (1.0 - m)).float()
    reg = tr.Register("affine", criterion=[tr.MILoss()], weight=[1.0], honor_criterion=True, optimizer="adam")
    reg.optim(m.cuda(), t.cuda(), lr=0.005, max_epochs=12)
    ls = reg.losses.detach().flatten().cpu().numpy()
    print(f"affine + MILoss: {ls[0]:.5f} -> {ls[-1]:.5f}")
    assert len(ls) == 12 and np.all(np.isfinite(ls)) and ls[-1] < ls[0]
