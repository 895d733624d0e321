"""GPU checks of the cubic B-spline free-form deformation (csrc/bspline.hip): trx_bspline_expand / _reduce against the fp64 restatement
(tests/bspline_ref.py) at the shapes where the edge handling can go wrong, the adjoint property and closed forms on the device, determinism
and batch independence, guard bytes, the device-side loop against torch autograd on the CPU, the early stop, and the public surface
(BSplineSolver, flow_register(flow_model='bspline'), Register(..., flow_model='bspline', levels=L))."""
import math
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

import bspline_ref as ref
import phantoms as ph
from conftest import bar
from loop_arbiters import bspline_arbiter as _arbiter, bspline_ctrl0 as _ctrl0, loop_pair as _pair, rand as _rand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1, 2. expand and reduce against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cases(n=60, seed=1999):
    """(B, spatial, spacing, with_base): the fixed cases, then seeded random ones up to n."""
    fixed = [(1, (13, 18, 23), (4, 5, 3)),      # no size a multiple of its spacing
             (1, (17, 17, 17), (4, 4, 4)),      # S - 1 divisible by the spacing: the last voxel has t = 0
             (1, (5, 6, 7), (8, 8, 8)),         # the spacing is larger than the volume
             (1, (9, 10, 11), (1, 1, 1)),       # spacing 1: every voxel is a lattice point
             (1, (1, 12, 20), (3, 3, 4)),       # an axis of one voxel
             (1, (19, 26), (4, 6)),             # 2-D
             (3, (13, 18, 23), (4, 5, 3))]      # B = 3
    cases = [c + (False,) for c in fixed] + [c + (True,) for c in fixed]
    rng = random.Random(seed)
    pool = [1, 2, 3, 4, 5] + list(range(7, 41))
    while len(cases) < n:
        nd = rng.choice((2, 3))
        sp = tuple(rng.choice(pool) for _ in range(nd))
        if math.prod(sp) > 40000:
            continue
        cases.append((rng.randint(1, 3), sp, tuple(rng.randint(1, 9) for _ in range(nd)), rng.random() < 0.5))
    return cases


CASES = _cases()
CASE_IDS = ["%dx%s-d%s-%s" % (c[0], "x".join(map(str, c[1])), "x".join(map(str, c[2])), "base" if c[3] else "nobase") for c in CASES]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: CASE_IDS[i])
def test_expand_and_reduce_match_the_restatement(tr, case):
    """trx_bspline_expand to 1e-5 max|ctrl| (+ max|base|), trx_bspline_reduce to bar(ref32, ref64, 1e-5 dz dy dx max|dflow|): the weights of
    one control point sum to at most d per axis, so dz dy dx max|dflow| bounds |dctrl|.  Uniform noise in, so every weight is checked tap
    by tap.  Fixed cases first (see _cases), then seeded random ones: sizes from {1..5, 7..40}, spacings 1..9, B 1..3, <= 40000 voxels."""
    B, sp, d, with_base = CASES[case]
    nd = len(sp)
    ctrl = _rand((B, nd) + ref.grid(sp, d), 10 + case)
    base = _rand((B, nd) + sp, 500 + case, -2.0, 2.0) if with_base else None
    got = tr.bspline_expand(ctrl.cuda(), sp, d, base=None if base is None else base.cuda())
    assert got.shape == (B, nd) + sp
    want = ref.expand(ctrl, sp, d, base)
    err, tol = (got.double().cpu() - want).abs().max().item(), 1e-5 * (ctrl.abs().max().item() + (base.abs().max().item() if with_base else 0.0))
    print(f"expand {CASE_IDS[case]}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)

    dflow = _rand((B, nd) + sp, 900 + case)
    got = tr.bspline_reduce(dflow.cuda(), d)
    assert got.shape == ctrl.shape
    r64, r32 = ref.reduce(dflow, d), ref.reduce(dflow, d, dtype=torch.float32)
    err, tol = (got.double().cpu() - r64).abs().max().item(), bar(r32.numpy(), r64.numpy(), 1e-5 * math.prod(d) * dflow.abs().max().item())
    print(f"reduce {CASE_IDS[case]}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the adjoint on the device
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp,d", [((13, 18, 23), (4, 5, 3)), ((19, 26), (4, 6))])
def test_reduce_is_the_adjoint_of_expand_on_the_device(tr, sp, d):
    """<expand(c), g> = <c, reduce(g)> to 1e-5 relative, both dot products formed in fp64 from the GPU's outputs."""
    nd = len(sp)
    c, g = _rand((2, nd) + ref.grid(sp, d), 1).cuda(), _rand((2, nd) + sp, 2).cuda()
    lhs = (tr.bspline_expand(c, sp, d).double() * g.double()).sum().item()
    rhs = (c.double() * tr.bspline_reduce(g, d).double()).sum().item()
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs)), (lhs, rhs)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. closed forms, without the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_constant_and_linear_control_lattices(tr):
    """Partition of unity and linear reproduction on the GPU: constant ctrl -> constant flow; ctrl_i = a . (i - 1) d + b -> a . x + b."""
    sp, d = (14, 15, 16), (3, 4, 5)
    G = tr.bspline_grid(sp, d)
    flow = tr.bspline_expand(torch.full((1, 3) + G, -1.37).cuda(), sp, d)
    assert (flow + 1.37).abs().max().item() <= 1e-5 * 1.37
    a, b = [0.31, -0.17, 0.23], 0.4
    pts = torch.meshgrid(*[(torch.arange(g, dtype=torch.float64) - 1) * s for g, s in zip(G, d)], indexing="ij")
    vox = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in sp], indexing="ij")
    ctrl = torch.stack([(c + 1) * (sum(a[i] * pts[i] for i in range(3)) + b) for c in range(3)])[None]      # a different scale per channel
    want = torch.stack([(c + 1) * (sum(a[i] * vox[i] for i in range(3)) + b) for c in range(3)])[None]
    got = tr.bspline_expand(ctrl.float().cuda(), sp, d).double().cpu()
    assert (got - want).abs().max().item() <= 1e-5 * want.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. determinism and batch independence
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_pairs_do_not_see_each_other(tr):
    sp, d = (13, 18, 23), (4, 5, 3)
    c, base, g = _rand((2, 3) + ref.grid(sp, d), 3).cuda(), _rand((2, 3) + sp, 4).cuda(), _rand((2, 3) + sp, 5).cuda()
    e1, e2 = tr.bspline_expand(c, sp, d, base=base), tr.bspline_expand(c, sp, d, base=base)
    r1, r2 = tr.bspline_reduce(g, d), tr.bspline_reduce(g, d)
    assert torch.equal(e1, e2) and torch.equal(r1, r2)
    assert torch.equal(e1[1:], tr.bspline_expand(c[1:], sp, d, base=base[1:])) and torch.equal(r1[1:], tr.bspline_reduce(g[1:], d))

    shape, spacing = (20, 24, 28), (5, 4, 6)
    mov, tgt = _pair(shape, B=2)
    c0 = _ctrl0(2, shape, spacing, 8)
    kw = dict(loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.1, capacity=5)
    runs = []
    for sl in (slice(0, 2), slice(0, 2), slice(1, 2)):
        s = tr.BSplineSolver(mov[sl].cuda(), tgt[sl].cuda(), spacing, init=c0[sl], **kw)
        s.run(5)
        runs.append(s)
    torch.cuda.synchronize()
    a, b, solo = runs
    assert torch.equal(a.ctrl, b.ctrl) and torch.equal(a.losses, b.losses) and torch.equal(a.flow, b.flow)
    assert torch.equal(a.ctrl[1:], solo.ctrl) and torch.equal(a.losses[1:], solo.losses) and torch.equal(a.flow[1:], solo.flow)
    assert not torch.equal(a.ctrl[1:].cpu(), c0[1:]) and torch.isfinite(a.losses).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. guard bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096


class _Guarded:
    """`nbytes` inside a larger buffer filled with a byte pattern."""

    def __init__(self, nbytes, fill):
        self.n, self.fill = nbytes, fill
        self.buf = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
        self.region = self.buf[GUARD:GUARD + nbytes]

    def floats(self, shape):
        return self.region.view(torch.float32).view(shape)

    def check(self, what):
        assert bool((self.buf[:GUARD] == self.fill).all()), f"bytes written in front of {what}"
        assert bool((self.buf[GUARD + self.n:] == self.fill).all()), f"bytes written behind {what}"


@pytest.mark.parametrize("B,sp,d", [(2, (13, 18, 23), (4, 5, 3)), (1, (5, 6, 7), (8, 8, 8)), (3, (19, 26), (4, 6))])
def test_calls_stay_inside_their_buffers(tr, B, sp, d):
    """Expand, reduce and a 3-iteration run with the workspace at exactly trx_bspline_workspace_bytes: canaries around flow, dflow, dctrl /
    ctrl and the workspace are intact, and the guarded calls give the bits of the wrappers."""
    import ctypes
    from torchregister_amd import _lib
    lib = _lib.load()
    nd = len(sp)
    G = ref.grid(sp, d)
    dhw, d3 = (1,) * (3 - nd) + sp, (1,) * (3 - nd) + d
    ws_bytes = lib.trx_bspline_workspace_bytes(nd, B, *dhw, *d3)
    assert ws_bytes > 0
    nflow, nctrl = B * nd * math.prod(sp) * 4, B * nd * math.prod(G) * 4
    ws, flow, dflow, dctrl = _Guarded(ws_bytes, 0x5A), _Guarded(nflow, 0xA5), _Guarded(nflow, 0xC3), _Guarded(nctrl, 0x3C)
    stream = _lib.current_stream(torch.device("cuda"))
    ctrl, base = _rand((B, nd) + G, 6).cuda(), _rand((B, nd) + sp, 7).cuda()
    rc = lib.trx_bspline_expand(_lib.ptr(ctrl), _lib.ptr(base), _lib.ptr(flow.region), nd, B, *dhw, *d3, _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_bspline_expand")
    torch.cuda.synchronize()
    assert torch.equal(flow.floats((B, nd) + sp), tr.bspline_expand(ctrl, sp, d, base=base))
    g = _rand((B, nd) + sp, 8).cuda()
    rc = lib.trx_bspline_reduce(_lib.ptr(g), _lib.ptr(dctrl.region), nd, B, *dhw, *d3, _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_bspline_reduce")
    torch.cuda.synchronize()
    assert torch.equal(dctrl.floats((B, nd) + G), tr.bspline_reduce(g, d))
    for buf, what in ((ws, "the workspace"), (flow, "flow"), (dctrl, "dctrl")):
        buf.check(what)

    # the loop: ctrl (in the dctrl buffer), flow and dflow guarded, Adam moments and the rest plain tensors
    mov, tgt = _pair(sp, B=B)
    batch = tr._engine._Batch(mov.cuda(), tgt.cuda(), tables=False)
    vol = batch.vol()
    cg = dctrl.floats((B, nd) + G)
    c0 = _ctrl0(B, sp, d, 9).cuda()
    cg.copy_(c0)
    m, v = torch.zeros_like(c0), torch.zeros_like(c0)
    losses, step = torch.full((B, 3), float("nan"), device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    st = _lib.BSplineState()
    st.ctrl, st.adam_m, st.adam_v, st.base = cg.data_ptr(), m.data_ptr(), v.data_ptr(), base.data_ptr()
    st.flow, st.dflow = flow.region.data_ptr(), dflow.region.data_ptr()
    st.losses, st.losses_capacity, st.step = losses.data_ptr(), 3, step.data_ptr()
    loss, opt = tr.LossSpec(w_mse=1.0, w_ncc=0.01).c(), tr._engine.opt_cfg("adam", 0.05)
    rc = lib.trx_bspline_run(ctypes.byref(vol), ctypes.byref(loss), ctypes.byref(opt), ctypes.byref(st), (ctypes.c_int * 3)(*d3), 3,
                             _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_bspline_run")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (flow, "flow"), (dflow, "dflow"), (dctrl, "ctrl")):
        buf.check(what)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), d, loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01), optimizer="adam", lr=0.05, init=c0, base=base, capacity=3)
    s.run(3)
    torch.cuda.synchronize()
    assert step.tolist() == [3] * B and torch.equal(cg, s.ctrl) and torch.equal(losses, s.losses)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the loop against torch autograd on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,spacing,optimizer,lr,loss_kw", [((20, 24, 28), (5, 4, 6), "adam", 0.1, dict(w_ncc=1.0)),
                                                                ((20, 24, 28), (5, 4, 6), "sgd", 1000.0, dict(w_mse=1.0)),
                                                                ((40, 44), (5, 6), "adam", 0.05, dict(w_mse=1.0, w_ncc=0.01))])
def test_bspline_loop_vs_torch_autograd(tr, shape, spacing, optimizer, lr, loss_kw):
    """trx_bspline_run (expand -> fused loss and dL/dflow -> reduce -> SGD / Adam, all on the device) against the same objective under
    torch autograd in fp64, 12 iterations from a random control tensor of amplitude 0.4; bars = max(floor, 2 x the arbiter's own
    fp32-vs-fp64 gap) with the floors of the local-NCC loop test.  Each lr was chosen on the CPU so that the arbiter's loss falls in
    every iteration (NCC + Adam 99.17 -> 90.61, MSE + SGD 0.010635 -> 0.008974, 2-D 0.5355 -> 0.4625)."""
    iters = 12
    mov, tgt = _pair(shape)
    c0 = _ctrl0(1, shape, spacing, 7)
    l64, c64 = _arbiter(mov, tgt, spacing, c0, lr, iters, optimizer, torch.float64, **loss_kw)
    l32, c32 = _arbiter(mov, tgt, spacing, c0, lr, iters, optimizer, torch.float32, **loss_kw)
    assert np.all(np.diff(l64) < 0)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, loss=tr.LossSpec(**loss_kw), optimizer=optimizer, lr=lr, init=c0, capacity=iters)
    s.run(iters)
    torch.cuda.synchronize()
    e, b = np.max(np.abs(s.losses[0].cpu().numpy() - l64)), bar(l32, l64, 2e-5 * np.max(np.abs(l64)))
    print(f"loss curve: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {np.max(np.abs(l32 - l64)):.3e})")
    assert e <= b, ("loss curve", e, b)
    e, b = np.max(np.abs(s.ctrl.cpu().numpy() - c64)), bar(c32, c64, 2e-4)
    print(f"ctrl: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {np.max(np.abs(c32 - c64)):.3e})")
    assert e <= b, ("ctrl", e, b)
    assert int(s.step[0]) == iters
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 8. early stop
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", ["one", "split", "single"])
@pytest.mark.parametrize("shape,spacing,optimizer,lr,with_base", [((20, 24, 28), (5, 4, 6), "adam", 0.1, False), ((20, 24, 28), 6, "sgd", 1000.0, True),
                                                                  ((40, 44), (5, 6), "adam", 0.05, False)])
def test_bspline_loop_stops_exactly(tr, shape, spacing, optimizer, lr, with_base, calls):
    """stop_crit between two recorded losses of a probe run: step = index + 1, the update of that iteration has been applied, flow_last is
    the flow of that forward, nothing is recorded or changed afterwards - bit for bit against un-stopped solvers run k + 1 and k iterations."""
    mov, tgt = (t.cuda() for t in _pair(shape))
    N, k = 12, 5
    base = (0.3 * ph.flow_field(shape, 1.0, 0.05)).cuda() if with_base else None
    loss = tr.LossSpec(w_mse=1.0) if optimizer == "sgd" else tr.LossSpec(w_mse=1.0, w_ncc=0.01)     # (each descends under the CPU arbiter)
    kw = dict(loss=loss, optimizer=optimizer, lr=lr, init=_ctrl0(1, shape, spacing, 7), base=base, capacity=N)
    free = tr.BSplineSolver(mov, tgt, spacing, **kw)
    free.run(N)
    L = free.losses[0].cpu().numpy().astype(np.float64)
    assert np.all(np.diff(L[: k + 2]) < 0), "the probe run must descend so that a threshold between two losses is well defined"
    crit = 0.5 * (L[k] + L[k - 1])
    s = tr.BSplineSolver(mov, tgt, spacing, stop_crit=crit, **kw)
    if calls == "one":
        s.run(N)
    elif calls == "split":
        s.run(4)
        s.run(5)
        s.run(N - 9)
    else:
        for _ in range(N):
            s.run(1)
    torch.cuda.synchronize()
    assert int(s.step[0]) == k + 1 and int(s.stopped[0]) != 0
    got = s.losses[0].cpu().numpy()
    assert np.array_equal(got[: k + 1], free.losses[0, : k + 1].cpu().numpy()) and np.all(np.isnan(got[k + 1:]))
    after, before = tr.BSplineSolver(mov, tgt, spacing, **kw), tr.BSplineSolver(mov, tgt, spacing, **kw)
    after.run(k + 1)
    before.run(k)
    torch.cuda.synchronize()
    assert torch.equal(s.ctrl, after.ctrl) and torch.equal(s.flow, after.flow)
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing, base=base))
    assert torch.equal(s.flow_last, before.flow) and not torch.equal(s.flow_last, s.flow)
    if optimizer == "adam":
        assert torch.equal(s.adam_m, after.adam_m) and torch.equal(s.adam_v, after.adam_v)


def test_pairs_of_a_bspline_batch_stop_independently(tr):
    """B = 2, a threshold only pair 0 meets: pair 0 stops there, pair 1 runs all iterations; each equals its un-stopped run to that point."""
    shape, spacing, N = (20, 24, 28), (5, 4, 6), 10
    mov, tgt = (t.cuda() for t in _pair(shape, B=2))
    tgt = torch.cat([tgt[:1], 3.0 * tgt[1:]])          # MSE grows with the intensity scale: pair 1 stays far above pair 0's losses
    mov = torch.cat([mov[:1], 3.0 * mov[1:]])
    kw = dict(loss=tr.LossSpec(w_mse=1.0), optimizer="adam", lr=0.1, init=_ctrl0(2, shape, spacing, 7), capacity=N)
    free = tr.BSplineSolver(mov, tgt, spacing, **kw)
    free.run(N)
    L = free.losses.cpu().numpy().astype(np.float64)
    k = 4
    assert np.all(np.diff(L[0, : k + 2]) < 0)
    crit = 0.5 * (L[0, k] + L[0, k - 1])
    assert L[1].min() > crit
    s = tr.BSplineSolver(mov, tgt, spacing, stop_crit=crit, **kw)
    s.run(6)
    s.run(N - 6)
    torch.cuda.synchronize()
    assert s.step.cpu().tolist() == [k + 1, N] and (s.stopped.cpu() != 0).tolist() == [True, False]
    assert torch.equal(s.losses[0, : k + 1], free.losses[0, : k + 1]) and bool(torch.isnan(s.losses[0, k + 1:]).all())
    assert torch.equal(s.losses[1], free.losses[1]) and torch.equal(s.ctrl[1], free.ctrl[1])
    one = tr.BSplineSolver(mov, tgt, spacing, **kw)
    one.run(k)
    torch.cuda.synchronize()
    assert torch.equal(s.flow_last[0], one.flow[0])
    one.run(1)
    torch.cuda.synchronize()
    assert torch.equal(s.ctrl[0], one.ctrl[0]) and torch.equal(s.flow[0], one.flow[0])


def test_flow_register_bspline_stops_and_keeps_the_last_forward(tr):
    shape, spacing, N, k = (20, 24, 28), (5, 4, 6), 12, 5
    mov, tgt = (t.cuda() for t in _pair(shape))
    kw = dict(criterions=[nn.MSELoss(), tr.NCCLoss()], weights=[1.0, 0.01], lr=0.1, max_epochs=N, flow_model="bspline", spacing=spacing, optimizer="adam")
    probe = tr.flow_register(shape, stop_crit=-1.0, **kw)
    probe.init_control = _ctrl0(1, shape, spacing, 7)
    probe.optimize(mov, tgt, debug=False)
    L = probe.losses[0].cpu().numpy().astype(np.float64)
    assert probe.losses.shape[1] == N and int(probe.iterations[0]) == N and np.all(np.diff(L[: k + 2]) < 0)
    fr = tr.flow_register(shape, stop_crit=0.5 * (L[k] + L[k - 1]), **kw)
    fr.init_control = _ctrl0(1, shape, spacing, 7)
    fr.optimize(mov, tgt, debug=False)
    assert fr.losses.shape[1] == k + 1 and int(fr.iterations[0]) == k + 1
    assert fr.control.shape == (1, 3) + tr.bspline_grid(shape, spacing)
    assert torch.equal(fr.final_flow, tr.bspline_expand(fr.control, shape, spacing))       # expand of ctrl AFTER that iteration's update
    before = tr.BSplineSolver(mov, tgt, spacing, loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01, ncc_alpha=tr.NCCLoss().alpha), optimizer="adam", lr=0.1,
                              init=_ctrl0(1, shape, spacing, 7), capacity=N)
    before.run(k)
    torch.cuda.synchronize()
    assert torch.equal(fr.flow, before.flow) and not torch.equal(fr.flow, fr.final_flow)   # .flow: the expanded flow BEFORE the update
    assert torch.equal(fr.deform(mov), tr.SpatialTransformer(shape)(mov, fr.flow))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. public surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _smooth_flow(shape, amp=1.0):
    ax = [torch.arange(n, dtype=torch.float64) for n in shape]
    comp = lambda a, b, c: (torch.sin(a * ax[0])[:, None, None] + torch.cos(b * ax[1])[None, :, None] + torch.sin(c * ax[2] + 0.4)[None, None, :])  # noqa: E731
    return (amp * torch.stack([comp(0.21, 0.17, 0.13), 0.75 * comp(0.11, 0.23, 0.19), 0.9 * comp(0.15, 0.12, 0.27)])).float()[None]


def test_register_bspline_single_level(tr):
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, ph.flow_field(shape)).cuda()
    tgt = tgt.cuda()
    reg = tr.Register("flow", criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, optimizer="adam")
    reg.optim(mov, tgt, lr=0.1, max_epochs=15)
    losses = reg.losses[0].cpu().numpy()
    assert losses.shape == (15,) and losses[-1] < losses[0]          # CPU arbiter: 3.537 -> 0.819
    assert reg.theta.shape == (1, 3) + shape and reg.final_theta.shape == (1, 3) + shape
    assert torch.equal(reg(mov), tr._engine.flow_warp(mov, reg.theta))
    assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 6)
    assert torch.equal(reg.final_theta, tr.bspline_expand(reg.control, shape, 6))
    two = torch.cat([mov, 0.5 * mov], dim=1)
    out = reg(two)
    assert out.shape == two.shape and torch.equal(out[:, :1], reg(mov))


def test_register_bspline_levels(tr):
    """levels=2 with the same spacing in voxels at both levels.  max_epochs=[15, 0]: the fine level's lattice stays zero, so its flow is
    its base, upsample_flow of the coarse level's final flow, bit for bit.  max_epochs=[15, 10] on a smooth deformation (blobs warped by a
    sum of low-frequency sines, about 2 voxels): the fine level starts below where the coarse level started - CPU arbiter (bspline_ref +
    resample_ref + oracle/compose under Adam, lr 0.1): coarse 9.60 -> 1.58, fine 2.31 -> 0.53; the fine level from a zero flow starts at
    11.75.  (ph.flow_field is not smooth: there the arbiter's coarse level starts at 0.115, its blur having removed the difference, and
    the fine level at 2.05.)"""
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, _smooth_flow(shape)).cuda()
    tgt = tgt.cuda()
    kw = dict(criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, optimizer="adam")
    coarse_shape = tr.pyramid_shapes(shape, 2)[0]
    reg = tr.Register("flow", levels=2, **kw)
    reg.optim(mov, tgt, lr=0.1, max_epochs=[15, 0])
    assert [ls.shape[-1] for ls in reg.level_losses] == [15, 0]
    coarse = tr.Register("flow", **kw)
    coarse.optim(tr.pyramid(mov, 2, align_corners=True)[0], tr.pyramid(tgt, 2, align_corners=True)[0], lr=0.1, max_epochs=15)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    assert torch.equal(reg.final_theta, tr.upsample_flow(coarse.final_theta, shape)) and torch.equal(reg.theta, reg.final_theta)
    assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 6) and torch.count_nonzero(reg.control).item() == 0
    assert coarse.control.shape == (1, 3) + tr.bspline_grid(coarse_shape, 6)

    reg = tr.Register("flow", levels=2, **kw)
    reg.optim(mov, tgt, lr=0.1, max_epochs=[15, 10])
    l0, l1 = (ls[0].cpu().numpy() for ls in reg.level_losses)
    assert l0.shape == (15,) and l1.shape == (10,)
    print(f"levels: coarse {l0[0]:.4f} -> {l0[-1]:.4f}, fine {l1[0]:.4f} -> {l1[-1]:.4f}")
    assert l1[0] < l0[0] and l1[-1] < l1[0]
    assert torch.count_nonzero(reg.control).item() > 0 and torch.equal(reg(mov), tr._engine.flow_warp(mov, reg.theta))
