"""The Jacobian determinant map and the folding penalty on the GPU (trx_flow_jacobian, trx_flow_folding, trx_bspline_run_fold,
trx_bspline_mi_run_fold) against tests/jacobian_ref.py; tests/test_jacobian_host.py asserts what these tests rest on."""
import ctypes
import math

import numpy as np
import pytest
import torch

import affine_flow_ref as fr
import jacobian_ref as jr
from conftest import bar
from test_gpu_bspline import _Guarded
from test_gpu_mi import _loop_bars
from test_jacobian_host import check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the map
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jr.CASES, ids=jr.case_id)
def test_map_against_the_fp64_restatement(tr, case):
    """Floor: 1e-5 * max(1, max |det|), about 170 fp32 roundings of a sum of triple products."""
    r = jr.reference(case)
    got = tr.jacobian_determinant(jr.field(case).cuda())
    assert got.shape == (case[0], 1) + tuple(case[1])
    e, b = np.abs(got[:, 0].cpu().double().numpy() - r["det64"]).max(), bar(r["det32"], r["det64"], 1e-5 * max(1.0, np.abs(r["det64"]).max()))
    print(f"{jr.case_id(case)} map: err {e:.3e} bar {b:.3e} (restatement fp32-fp64 {np.abs(r['det32'] - r['det64']).max():.3e})")
    assert e <= b


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the penalty and its gradient
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jr.CASES, ids=jr.case_id)
def test_penalty_and_gradient_against_autograd(tr, case):
    """P against fp64 (floor 1e-5 P), dflow against autograd on EVERY voxel - the hinge is C^1, no voxel is left out - (floor 1e-4 max |g64|, the
    flow-gradient floor of the loop arbiters); accumulate adds onto a non-zero dflow; weight scales dflow and not the penalty; autograd through
    tr.folding_penalty gives the bits of the direct call."""
    r = jr.reference(case)
    fl = jr.field(case).cuda()
    p, g = tr.folding_penalty_grad(fl, jr.EPS)
    gmax = np.abs(r["g64"]).max()
    for b_ in range(case[0]):
        e, b = abs(p[b_].item() - r["p64"][b_]), bar(r["p32"][b_], r["p64"][b_], 1e-5 * r["p64"][b_])
        print(f"{jr.case_id(case)} pair {b_}: P {r['p64'][b_]:.6f} err {e:.3e} bar {b:.3e}")
        assert e <= b
    e, b = np.abs(g.cpu().double().numpy() - r["g64"]).max(), bar(r["g32"], r["g64"], 1e-4 * gmax)
    print(f"{jr.case_id(case)} dflow: max {gmax:.3e} err {e:.3e} bar {b:.3e} (autograd fp32-fp64 {np.abs(r['g32'] - r['g64']).max():.3e})")
    assert e <= b
    assert torch.equal(tr.folding_penalty(fl, jr.EPS), p) and torch.equal(tr.folding_penalty_grad(fl, jr.EPS, need_grad=False)[0], p)
    # accumulate = 1 onto a non-zero field of the gradient's size
    gen = torch.Generator().manual_seed(5)
    g0 = ((torch.rand(fl.shape, generator=gen) - 0.5) * 2 * gmax).float()
    into = g0.clone().cuda()
    p2, out = tr.folding_penalty_grad(fl, jr.EPS, into=into)
    assert out is into and torch.equal(p2, p)
    e = np.abs(into.cpu().double().numpy() - (g0.double().numpy() + r["g64"])).max()
    print(f"{jr.case_id(case)} accumulate: err {e:.3e} bar {b:.3e}")
    assert e <= b and not torch.equal(into.cpu(), g0)
    # weight
    p3, g3 = tr.folding_penalty_grad(fl, jr.EPS, weight=3.0)
    assert torch.equal(p3, p)
    e = np.abs(g3.cpu().double().numpy() - 3.0 * r["g64"]).max()
    assert e <= 3.0 * b
    p0, gz = tr.folding_penalty_grad(fl, jr.EPS, weight=0.0)
    assert torch.equal(p0, p) and not bool(gz.any())
    # autograd
    x = fl.clone().requires_grad_()
    pa = tr.folding_penalty(x, jr.EPS)
    pa.sum().backward()
    assert torch.equal(pa.detach(), p) and torch.equal(x.grad, g)


def test_blocks_without_an_active_voxel_in_reach(tr):
    """The gather's early exit: on the bump field most blocks find every partial sum within reach at 0 and leave; the gradient still matches autograd on
    every voxel, those of inactive chunks next to active ones included, and accumulating leaves the voxels of the blocks that left bit for bit as they were."""
    fl = jr.bump_field()
    p64, g64 = jr.penalty_grad(fl)
    _, g32 = jr.penalty_grad(fl, dtype=torch.float32)
    p, g = tr.folding_penalty_grad(fl.cuda(), jr.EPS)
    gmax = g64.abs().max().item()
    e, b = (g.cpu().double() - g64).abs().max().item(), bar(g32.double().numpy(), g64.numpy(), 1e-4 * gmax)
    print(f"bump: P {float(p64):.6e} err {abs(float(p) - float(p64)):.3e}; dflow max {gmax:.3e} err {e:.3e} bar {b:.3e}")
    assert abs(float(p) - float(p64)) <= 1e-5 * float(p64) and e <= b
    zero = g64 == 0
    assert zero.double().mean().item() > 0.5 and not bool(g.cpu()[zero].any())
    gen = torch.Generator().manual_seed(9)
    g0 = ((torch.rand(fl.shape, generator=gen) - 0.5) * 2 * gmax).float()
    into = g0.clone().cuda()
    tr.folding_penalty_grad(fl.cuda(), jr.EPS, into=into)
    assert torch.equal(into.cpu()[zero], g0[zero])
    assert (into.cpu().double() - (g0.double() + g64)).abs().max().item() <= b


def test_threshold_moves_the_active_set(tr):
    """A threshold below every determinant: P = 0, a zero gradient, and an accumulating call changes no bit; above every determinant: every voxel is active."""
    case = jr.FIELD_CASES[2]
    fl, d = jr.field(case).cuda(), jr.reference(case)["det64"]
    p, g = tr.folding_penalty_grad(fl, float(d.min()) - 1.0)
    assert float(p) == 0.0 and not bool(g.any())
    g0 = jr.field(jr.FIELD_CASES[2]).cuda() * 3.0
    into = g0.clone()
    tr.folding_penalty_grad(fl, float(d.min()) - 1.0, weight=5.0, into=into)
    assert torch.equal(into, g0)
    hi = float(d.max()) + 1.0
    p64, g64 = jr.penalty_grad(jr.field(case), hi)
    p, g = tr.folding_penalty_grad(fl, hi)
    assert abs(float(p) - float(p64)) <= 1e-5 * float(p64) and (g.cpu().double() - g64).abs().max().item() <= 1e-4 * g64.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. determinism
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [jr.FIELD_CASES[1], jr.FIELD_CASES[6]], ids=jr.case_id)
def test_same_bits_on_every_call_and_in_every_batch(tr, case):
    fl = jr.field(case).cuda()
    d1, d2 = tr.jacobian_determinant(fl), tr.jacobian_determinant(fl)
    (p1, g1), (p2, g2) = tr.folding_penalty_grad(fl), tr.folding_penalty_grad(fl)
    assert torch.equal(d1, d2) and torch.equal(p1, p2) and torch.equal(g1, g2)
    for b in range(2):
        pa, ga = tr.folding_penalty_grad(fl[b:b + 1])
        assert torch.equal(tr.jacobian_determinant(fl[b:b + 1]), d1[b:b + 1]) and torch.equal(pa, p1[b:b + 1]) and torch.equal(ga, g1[b:b + 1])
    bad = fl.clone()
    bad[0, 0].view(-1)[7] = float("nan")
    bad[0, 1].view(-1)[bad[0, 1].numel() // 2] = float("inf")
    db, (pb, gb) = tr.jacobian_determinant(bad), tr.folding_penalty_grad(bad)
    assert torch.equal(db[1], d1[1]) and torch.equal(pb[1], p1[1]) and torch.equal(gb[1], g1[1])
    assert bool(torch.isfinite(db[1]).all()) and bool(torch.isfinite(gb[1]).all()) and bool(torch.isfinite(pb[1]))
    assert not bool(torch.isfinite(db[0]).all())


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the loops
# ---------------------------------------------------------------------------------------------------------------------------------------
def _solver(tr, row, weight, capacity=jr.ITERS):
    kw = dict(capacity=capacity, folding_weight=weight, folding_threshold=jr.EPS)
    if row == "ncc":
        r = jr.NCC_ROW
        mov, tgt, ctrl0 = jr.ncc_setup()
        return tr.BSplineSolver(mov.cuda(), tgt.cuda(), r["spacing"], loss=tr.LossSpec(w_ncc=1.0), optimizer=r["optimizer"], lr=r["lr"], init=ctrl0, **kw)
    name = row[3:]
    _, _, spacing, optimizer, lr, _, lam = fr.LOOPS[name]
    mov, tgt, theta, mask, rng, ctrl0 = jr.mi_setup(name)
    return tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, optimizer=optimizer, lr=lr, init=ctrl0, bending_weight=lam, mi=dict(bins=32),
                            mask=None if mask is None else mask.cuda(), initial=theta, **kw)


def _row_geometry(row):
    return (jr.NCC_ROW["shape"], jr.NCC_ROW["spacing"]) if row == "ncc" else fr.LOOPS[row[3:]][0:3:2]


@pytest.mark.parametrize("row", list(jr.loop_rows()))
def test_penalised_loop_vs_torch_autograd(tr, row):
    """trx_bspline_run_fold / trx_bspline_mi_run_fold, 10 iterations, against the arbiter in fp64 with the bars of the other loops."""
    fn, w = jr.loop_rows()[row], jr.row_weight(row)
    r64, r32 = fn(w, torch.float64), fn(w, torch.float32)
    assert np.all(np.diff(r64[0]) < 0) and r64[1][0] > 0
    s = _solver(tr, row, w)
    s.run(jr.ITERS)
    torch.cuda.synchronize()
    assert int(s.step[0]) == jr.ITERS
    _loop_bars(s.losses[0].cpu().numpy(), s.ctrl.cpu().numpy(), (r64[0], r64[3]), (r32[0], r32[3]), f"penalised {row}")
    shape, spacing = _row_geometry(row)
    assert torch.equal(s.flow, tr.bspline_expand(s.ctrl, shape, spacing))


@pytest.mark.parametrize("row", ["ncc", "mi-adam"])
def test_weight_zero_is_the_existing_entry_point(tr, row):
    """The *_fold entry point with fold->weight == 0 (the solver's struct, its weight set to 0 after construction) against the existing one."""
    plain, fold = _solver(tr, row, 0.0), _solver(tr, row, 1.0)
    assert plain.fold is None and fold.fold is not None and fold.ws_bytes > plain.ws_bytes
    fold.fold.weight = 0.0
    plain.run(jr.ITERS)
    fold.run(jr.ITERS)
    torch.cuda.synchronize()
    assert torch.equal(plain.losses, fold.losses) and torch.equal(plain.ctrl, fold.ctrl) and torch.equal(plain.flow, fold.flow)


@pytest.mark.parametrize("row", ["ncc", "mi-bending"])
def test_split_runs_give_the_bits_of_one_run(tr, row):
    one, two = _solver(tr, row, jr.row_weight(row)), _solver(tr, row, jr.row_weight(row))
    one.run(10)
    two.run(4)
    two.run(6)
    torch.cuda.synchronize()
    assert torch.equal(one.losses, two.losses) and torch.equal(one.ctrl, two.ctrl) and torch.equal(one.flow, two.flow) and torch.equal(one.adam_v, two.adam_v)


def test_penalised_loop_with_the_overlap_rule_and_a_batch(tr):
    """overlap=True and B = 2 through trx_bspline_mi_run_fold: it runs, the loss holds the total (above the unpenalised run's first loss by weight * P of
    the starting flow), and a pair has the bits of the same pair alone."""
    mov, tgt, theta, _, _, ctrl0 = jr.mi_setup("adam")
    mov2, tgt2, c2, th2 = torch.cat([mov, mov.flip(2)]).cuda(), torch.cat([tgt, tgt.flip(2)]).cuda(), torch.cat([ctrl0, 0.5 * ctrl0]), theta.expand(2, -1, -1)
    kw = dict(optimizer="adam", lr=0.1, capacity=4, mi=dict(bins=32), overlap=True)
    both = tr.BSplineSolver(mov2, tgt2, 4, init=c2, initial=th2, folding_weight=jr.MI_WEIGHT, **kw)
    free = tr.BSplineSolver(mov2, tgt2, 4, init=c2, initial=th2, **kw)
    p0 = tr.folding_penalty(both.flow, jr.EPS)
    both.run(4)
    free.run(4)
    alone = tr.BSplineSolver(mov2[1:], tgt2[1:], 4, init=c2[1:], initial=th2[1:], folding_weight=jr.MI_WEIGHT, **kw)
    alone.run(4)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(both.losses).all()) and float(p0[0]) > 0
    want = free.losses[:, 0].double() + jr.MI_WEIGHT * p0.double()
    assert (both.losses[:, 0].double() - want).abs().max().item() <= 2e-5 * want.abs().max().item()
    assert torch.equal(alone.losses[0], both.losses[1]) and torch.equal(alone.ctrl[0], both.ctrl[1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. memory contract
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [jr.FIELD_CASES[1], jr.FIELD_CASES[5], jr.BLOCK_CASES[0]], ids=jr.case_id)
def test_kernels_stay_inside_their_buffers(tr, case):
    """det, penalty, dflow and an exact workspace between canaries; the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    fl = jr.field(case).cuda()
    B, nd, sp = fl.shape[0], fl.shape[1], tuple(fl.shape[2:])
    geom = (nd, B) + tr._engine._dhw(sp)
    n = math.prod(sp)
    gfl = _Guarded(fl.numel() * 4, 0x69)
    gfl.region.copy_(fl.view(torch.uint8).reshape(-1))
    det, pen, dflow = _Guarded(B * n * 4, 0x96), _Guarded(B * 4, 0x3C), _Guarded(B * nd * n * 4, 0xC3)
    ws_bytes = lib.trx_flow_folding_workspace_bytes(*geom)
    ws = _Guarded(ws_bytes, 0x5A)
    stream = _lib.current_stream(torch.device("cuda"))
    _lib.check(lib.trx_flow_jacobian(_lib.ptr(gfl.region), *geom, _lib.ptr(det.region), stream), "trx_flow_jacobian")
    run = lambda nbytes: lib.trx_flow_folding(_lib.ptr(gfl.region), *geom, jr.EPS, 1.0, _lib.ptr(pen.region), _lib.ptr(dflow.region), 0,  # noqa: E731
                                              _lib.ptr(ws.region), nbytes, stream)
    assert run(ws_bytes - 1) == -3
    _lib.check(run(ws_bytes), "trx_flow_folding")
    torch.cuda.synchronize()
    for buf, what in ((gfl, "flow"), (det, "det"), (pen, "penalty"), (dflow, "dflow"), (ws, "the workspace")):
        buf.check(what)
    p, g = tr.folding_penalty_grad(fl, jr.EPS)
    assert torch.equal(det.floats((B, 1) + sp), tr.jacobian_determinant(fl)) and torch.equal(pen.floats((B,)), p) and torch.equal(dflow.floats(tuple(fl.shape)), g)
    assert torch.equal(gfl.floats(tuple(fl.shape)), fl)


def test_penalised_loop_stays_inside_its_buffers(tr):
    """trx_bspline_run_fold with the workspace at exactly trx_bspline_fold_workspace_bytes - one byte less is TRX_ERR_WORKSPACE - and the state
    between canaries; the bits of the solver."""
    from torchregister_amd import _lib
    lib = _lib.load()
    iters, r = 3, jr.NCC_ROW
    shape, d = r["shape"], r["spacing"]
    want = _solver(tr, "ncc", r["weight"], capacity=iters)
    mov, tgt, _ = jr.ncc_setup()
    mov, tgt = mov.cuda(), tgt.cuda()
    G = want.grid
    nctrl, nflow = 3 * math.prod(G) * 4, 3 * math.prod(shape) * 4
    g = dict(ctrl=_Guarded(nctrl, 0x3C), adam_m=_Guarded(nctrl, 0x3C), adam_v=_Guarded(nctrl, 0x3C), flow=_Guarded(nflow, 0xA5), dflow=_Guarded(nflow, 0xC3),
             losses=_Guarded(iters * 4, 0x96), step=_Guarded(4, 0x96))
    for k in ("ctrl", "adam_m", "adam_v", "losses", "step"):
        g[k].region.copy_(getattr(want, k).contiguous().view(torch.uint8).reshape(-1))
    st = _lib.BSplineState()
    for k in g:
        setattr(st, k, g[k].region.data_ptr())
    st.losses_capacity, st.bending_weight = iters, 0.0
    vol = tr._engine._Batch(mov, tgt, tables=False).vol()
    ws_bytes = lib.trx_bspline_fold_workspace_bytes(3, 1, *shape, *d)
    assert ws_bytes == want.ws_bytes > 0
    ws = _Guarded(ws_bytes, 0x5A)
    d3, fold = (ctypes.c_int * 3)(*d), _lib.FoldCfg(r["weight"], jr.EPS)
    run = lambda n: lib.trx_bspline_run_fold(ctypes.byref(vol), ctypes.byref(want.loss_c), ctypes.byref(want.opt), ctypes.byref(st), d3, ctypes.byref(fold),  # noqa: E731
                                             iters, _lib.ptr(ws.region), n, _lib.current_stream(torch.device("cuda")))
    assert run(ws_bytes - 1) == -3
    _lib.check(run(ws_bytes), "trx_bspline_run_fold")
    torch.cuda.synchronize()
    for k in g:
        g[k].check(k)
    ws.check("the workspace")
    want.run(iters)
    torch.cuda.synchronize()
    for k in ("ctrl", "adam_m", "adam_v", "losses", "step"):
        assert torch.equal(g[k].region, getattr(want, k).contiguous().view(torch.uint8).reshape(-1)), k


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. what it is for, through Register
# ---------------------------------------------------------------------------------------------------------------------------------------
def _fold_stats(reg):
    d = reg.jacobian()
    return d.amin().item(), (d <= 0).float().mean().item()


def test_register_ncc_unfolds_with_the_penalty(tr):
    """NCC B-spline, (16, 18, 20), spacing 3, Adam 0.3, 40 iterations from zero.  Unpenalised the deformation folds (the fp64 arbiter: 27 % of the voxels,
    minimum -4.2); with folding_weight=1e4 the minimum determinant stays positive (arbiter +0.22, never below +0.17 during the run) and the data term
    costs at most 1.25 x (arbiter 1.09 x).  Without the feature: TypeError on the keyword."""
    u = jr.USE_NCC
    a0, a1 = jr.use_run("ncc", 0.0), jr.use_run("ncc", u["weight"])
    print(f"arbiter: unpenalised {a0}, penalised {a1}")
    assert a0["folded"] > 0.2 and a0["min_det"] < -2 and a1["min_det_run"] > 0.1 and a1["data"] <= 1.15 * a0["data"]
    mov, tgt = (t.cuda() for t in jr.use_ncc_pair())
    kw = dict(flow_model="bspline", criterion=[tr.NCCLoss()], weight=[1.0], optimizer="adam", spacing=u["spacing"])
    free, pen = tr.Register("flow", **kw), tr.Register("flow", folding_weight=u["weight"], **kw)
    free.optim(mov, tgt, lr=jr.USE_LR, max_epochs=jr.USE_ITERS)
    pen.optim(mov, tgt, lr=jr.USE_LR, max_epochs=jr.USE_ITERS)
    (m0, s0), (m1, s1) = _fold_stats(free), _fold_stats(pen)
    data0, data1 = tr.NCCLoss()(tgt, free(mov)).item(), tr.NCCLoss()(tgt, pen(mov)).item()
    print(f"unpenalised: min det {m0:.3f}, {100 * s0:.1f} % folded, NCC loss {data0:.4f}; folding_weight={u['weight']:g}: min det {m1:.3f}, {100 * s1:.1f} % folded, "
          f"NCC loss {data1:.4f} ({data1 / data0:.3f} x)")
    assert s0 > 0.1 and m0 < -1
    assert m1 > 0 and s1 == 0
    assert data1 <= 1.25 * data0
    assert pen.losses.shape == (1, jr.USE_ITERS) and pen.losses[0, -1].item() >= data1 - 1e-3      # .losses hold the total: data + weight P >= data
    assert torch.equal(pen.jacobian(), tr.jacobian_determinant(pen.theta)) and pen.jacobian().shape == (1, 1) + u["shape"]


def test_register_mi_through_an_initial_affine_unfolds_with_the_penalty(tr):
    """MILoss through initial= at spacing 2: unpenalised minimum < -0.3 and more than 2 % folded (arbiter -1.30, 7.4 %); folding_weight=100: minimum > 0
    (arbiter +0.29)."""
    u = jr.USE_MI
    a0, a1 = jr.use_run("mi", 0.0), jr.use_run("mi", u["weight"])
    print(f"arbiter: unpenalised {a0}, penalised {a1}")
    assert a0["folded"] > 0.05 and a0["min_det"] < -1 and a1["min_det_run"] > 0.1
    mov, tgt = (t.cuda() for t in jr.use_mi_pair())
    theta = fr.loop_theta(3)
    kw = dict(flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=u["spacing"])
    free, pen = tr.Register("flow", **kw), tr.Register("flow", folding_weight=u["weight"], **kw)
    free.optim(mov, tgt, lr=jr.USE_LR, max_epochs=jr.USE_ITERS, initial=theta)
    pen.optim(mov, tgt, lr=jr.USE_LR, max_epochs=jr.USE_ITERS, initial=theta)
    (m0, s0), (m1, s1) = _fold_stats(free), _fold_stats(pen)
    print(f"unpenalised: min det {m0:.3f}, {100 * s0:.1f} % folded, loss {free.losses[0, -1].item():.5f}; folding_weight={u['weight']:g}: min det {m1:.3f}, "
          f"loss {pen.losses[0, -1].item():.5f}")
    assert m0 < -0.3 and s0 > 0.02
    assert m1 > 0 and s1 == 0
    assert torch.equal(pen.jacobian(), tr.jacobian_determinant(pen.theta))


def test_register_two_levels_with_the_penalty(tr):
    """levels=2 applies the same weight at every level: the run finishes without a fold on the NCC pair."""
    u = jr.USE_NCC
    mov, tgt = (t.cuda() for t in jr.use_ncc_pair())
    reg = tr.Register("flow", flow_model="bspline", criterion=[tr.NCCLoss()], weight=[1.0], optimizer="adam", spacing=u["spacing"], levels=2,
                      folding_weight=u["weight"])
    reg.optim(mov, tgt, lr=jr.USE_LR, max_epochs=[20, 20])
    m, s = _fold_stats(reg)
    print(f"levels=2, folding_weight={u['weight']:g}: min det {m:.3f}, {100 * s:.1f} % folded, level losses {[ls[0, -1].item() for ls in reg.level_losses]}")
    assert m > 0 and reg.jacobian().shape == (1, 1) + u["shape"] and len(reg.level_losses) == 2
    assert torch.equal(reg.jacobian(), tr.jacobian_determinant(reg.theta))


def test_jacobian_of_the_other_flow_models(tr):
    """reg.jacobian() is the map of reg.theta for mode='flow' with any flow model."""
    mov, tgt = (t.cuda() for t in jr.use_ncc_pair())
    reg = tr.Register("flow", flow_model="direct", criterion=[tr.NCCLoss()], weight=[1.0], optimizer="adam")
    reg.optim(mov, tgt, lr=0.05, max_epochs=3)
    assert torch.equal(reg.jacobian(), tr.jacobian_determinant(reg.theta)) and reg.jacobian().shape == (1, 1) + jr.USE_NCC["shape"]
