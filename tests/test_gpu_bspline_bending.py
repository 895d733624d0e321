"""GPU checks of the bending-energy regulariser of the B-spline free-form deformation (csrc/bspline.hip: trx_bspline_bending and
trx_bspline_state.bending_weight): energy and gradient against the fp64 restatement (tests/bspline_bending_ref.py) at the lattice sizes where
the tiling and the bands' edges can go wrong, accumulate semantics, affine lattices, determinism and batch independence, guard bytes,
bending_weight = 0, the device-side loop against torch autograd on the CPU, the early stop on the total, and the public surface."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

import bspline_bending_ref as bref
import bspline_ref as ref
from conftest import bar
from test_gpu_bspline import _Guarded, _ctrl0, _pair, _rand

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _geom(sp, d):
    nd = len(sp)
    return nd, (1,) * (3 - nd) + tuple(sp), (1,) * (3 - nd) + tuple(d)


def _bending(ctrl, sp, d, dctrl=None, weight=1.0, accumulate=0):
    """trx_bspline_bending through the C ABI on a fresh workspace: energy [B] (and whatever the call left in `dctrl`)."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd, dhw, d3 = _geom(sp, d)
    B = ctrl.shape[0]
    ws_bytes = lib.trx_bspline_workspace_bytes(nd, B, *dhw, *d3)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    energy = torch.full((B,), float("nan"), device="cuda")
    rc = lib.trx_bspline_bending(_lib.ptr(ctrl), _lib.ptr(energy), _lib.ptr(dctrl), weight, accumulate, nd, B, *dhw, *d3, _lib.ptr(ws), ws_bytes,
                                 _lib.current_stream(torch.device("cuda")))
    _lib.check(rc, "trx_bspline_bending")
    torch.cuda.synchronize()
    return energy


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. energy and gradient against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
def _cases(n=40, seed=1999):
    """(B, spatial, spacing): the fixed cases, then seeded random ones up to n, drawn as in test_gpu_bspline._cases."""
    cases = [(1, (13, 18, 23), (4, 5, 3)),      # general 3-D
             (1, (17, 17, 17), (4, 4, 4)),      # S - 1 divisible by the spacing
             (1, (5, 6, 7), (8, 8, 8)),         # the spacing is larger than the volume
             (1, (9, 10, 11), (1, 1, 1)),       # spacing 1
             (1, (1, 12, 20), (3, 3, 4)),       # an axis of one voxel
             (1, (19, 26), (4, 6)),             # 2-D
             (3, (13, 18, 23), (4, 5, 3)),      # batch
             (2, (1, 1, 9), (2, 2, 2)),         # two axes of one voxel
             (1, (40, 3), (9, 1)),              # 2-D, one very short axis
             (1, (40, 37, 33), (2, 1, 2)),      # lattice 23 x 40 x 20: several tiles per axis, none a multiple of a tile
             (2, (70, 90), (1, 2))]             # 2-D, lattice 73 x 48
    rng = random.Random(seed)
    pool = [1, 2, 3, 4, 5] + list(range(7, 41))
    while len(cases) < n:
        nd = rng.choice((2, 3))
        sp = tuple(rng.choice(pool) for _ in range(nd))
        if math.prod(sp) > 40000:
            continue
        cases.append((rng.randint(1, 3), sp, tuple(rng.randint(1, 9) for _ in range(nd))))
    return cases


CASES = _cases()
CASE_IDS = ["%dx%s-d%s" % (c[0], "x".join(map(str, c[1])), "x".join(map(str, c[2]))) for c in CASES]


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: CASE_IDS[i])
def test_energy_and_gradient_match_the_restatement(tr, case):
    """tr.bspline_bending on uniform noise in [-1, 3]: each pair's energy to bar(E32, E64, 1e-5 E64), the gradient to
    bar(g32, g64, 1e-5 max|g64|), fp32 figures from the restatement's Gram form."""
    B, sp, d = CASES[case]
    nd = len(sp)
    ctrl = _rand((B, nd) + ref.grid(sp, d), 40 + case)
    e64, g64 = bref.energy_gram(ctrl, sp, d)
    e32, g32 = bref.energy_gram(ctrl, sp, d, dtype=torch.float32)
    energy, grad = tr.bspline_bending(ctrl.cuda(), sp, d, grad=True)
    assert energy.shape == (B,) and grad.shape == ctrl.shape
    assert torch.equal(tr.bspline_bending(ctrl.cuda(), sp, d), energy)
    for b in range(B):
        err, tol = abs(energy[b].item() - e64[b].item()), bar(e32[b].numpy(), e64[b].numpy(), 1e-5 * e64[b].item())
        print(f"energy {CASE_IDS[case]} pair {b}: E {e64[b].item():.6e} err {err:.3e} bar {tol:.3e}")
        assert err <= tol, ("energy", b, err, tol)
    err, tol = (grad.double().cpu() - g64).abs().max().item(), bar(g32.numpy(), g64.numpy(), 1e-5 * g64.abs().max().item())
    print(f"gradient {CASE_IDS[case]}: max|g| {g64.abs().max().item():.3e} err {err:.3e} bar {tol:.3e}")
    assert err <= tol, ("gradient", err, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. accumulate semantics
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sp,d", [(2, (13, 18, 23), (4, 5, 3)), (1, (19, 26), (4, 6))])
def test_accumulate_weight_and_null_gradient(tr, B, sp, d):
    """accumulate = 0 overwrites (a NaN-filled dctrl comes back finite, = weight g); accumulate = 1 adds to what is there; dctrl = NULL gives
    the same energy bits.  `pre` is noise of the size of weight g, so that the rounding of pre + weight g (6e-8 of it) stays far inside the
    bar of test 1, 1e-5 weight max|g64|."""
    nd, w = len(sp), 0.75
    ctrl = _rand((B, nd) + ref.grid(sp, d), 3)
    e64, g64 = bref.energy_gram(ctrl, sp, d)
    _, g32 = bref.energy_gram(ctrl, sp, d, dtype=torch.float32)
    gmax = g64.abs().max().item()
    c = ctrl.cuda()
    e_null = _bending(c, sp, d)
    out = torch.full_like(c, float("nan"))
    e_over = _bending(c, sp, d, dctrl=out, weight=w, accumulate=0)
    assert torch.equal(e_null, e_over) and torch.isfinite(out).all()
    err, tol = (out.double().cpu() - w * g64).abs().max().item(), bar(w * g32.numpy(), w * g64.numpy(), 1e-5 * w * gmax)
    assert err <= tol, ("overwrite", err, tol)
    assert abs(e_over[0].item() - e64[0].item()) <= 1e-5 * e64[0].item()          # the energy is unweighted
    pre = (_rand(ctrl.shape, 4, -1.0, 1.0) * w * gmax).float()
    acc = pre.cuda().clone()
    e_acc = _bending(c, sp, d, dctrl=acc, weight=w, accumulate=1)
    assert torch.equal(e_acc, e_null)
    err, tol = (acc.double().cpu() - (pre.double() + w * g64)).abs().max().item(), bar((pre + w * g32).numpy(), (pre.double() + w * g64).numpy(), 1e-5 * w * gmax)
    print(f"accumulate: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, ("accumulate", err, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. affine lattices
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp,d", [((13, 18, 23), (4, 5, 3)), ((40, 37, 33), (2, 1, 2)), ((70, 90), (1, 2))])
def test_an_affine_lattice_has_no_energy(tr, sp, d):
    """ctrl_c linear in the lattice indices: |E| <= 1e-7 K_E with K_E = nd max|ctrl|^2 (sum_a 4 / d_a^2)^2, the scale of the energy of a
    lattice of that amplitude (noise lattices have about 1e-4 K_E; the fp32 restatement gives at most 3e-10 K_E here).  E is not clamped:
    a slightly negative value is in order."""
    nd = len(sp)
    G = ref.grid(sp, d)
    idx = torch.meshgrid(*[torch.arange(g, dtype=torch.float64) for g in G], indexing="ij")
    a = [0.31, -0.17, 0.23]
    ctrl = torch.stack([(c + 1) * (sum(a[i] * idx[i] for i in range(nd)) + 0.4) for c in range(nd)])[None].float()
    K = nd * ctrl.abs().max().item() ** 2 * sum(4.0 / v ** 2 for v in d) ** 2
    energy, grad = tr.bspline_bending(ctrl.cuda(), sp, d, grad=True)
    print(f"affine {sp} / {d}: E {energy[0].item():.3e}, K_E {K:.3e}, ratio {abs(energy[0].item()) / K:.3e}")
    assert abs(energy[0].item()) <= 1e-7 * K and torch.isfinite(grad).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch independence
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_pairs_do_not_see_each_other(tr):
    for sp, d in (((13, 18, 23), (4, 5, 3)), ((40, 37, 33), (2, 1, 2)), ((70, 90), (1, 2))):
        c = _rand((2, len(sp)) + ref.grid(sp, d), 3).cuda()
        (e1, g1), (e2, g2) = tr.bspline_bending(c, sp, d, grad=True), tr.bspline_bending(c, sp, d, grad=True)
        assert torch.equal(e1, e2) and torch.equal(g1, g2)
        es, gs = tr.bspline_bending(c[1:], sp, d, grad=True)
        assert torch.equal(e1[1:], es) and torch.equal(g1[1:], gs)

    shape, spacing = (20, 24, 28), (5, 4, 6)
    mov, tgt = _pair(shape, B=2)
    c0 = _ctrl0(2, shape, spacing, 8)
    kw = dict(loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.025, capacity=6, bending_weight=4.5e4)
    runs = []
    for sl in (slice(0, 2), slice(0, 2), slice(1, 2)):
        s = tr.BSplineSolver(mov[sl].cuda(), tgt[sl].cuda(), spacing, init=c0[sl], **kw)
        s.run(6)
        runs.append(s)
    torch.cuda.synchronize()
    a, b, solo = runs
    assert torch.equal(a.ctrl, b.ctrl) and torch.equal(a.losses, b.losses) and torch.equal(a.flow, b.flow)
    assert torch.equal(a.ctrl[1:], solo.ctrl) and torch.equal(a.losses[1:], solo.losses) and torch.equal(a.flow[1:], solo.flow)
    assert not torch.equal(a.ctrl[1:].cpu(), c0[1:]) and torch.isfinite(a.losses).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. guard bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,sp,d", [(2, (13, 18, 23), (4, 5, 3)), (1, (5, 6, 7), (8, 8, 8)), (3, (19, 26), (4, 6))])
def test_calls_stay_inside_their_buffers(tr, B, sp, d):
    """trx_bspline_bending and a 3-iteration trx_bspline_run with bending_weight > 0, the workspace at exactly trx_bspline_workspace_bytes:
    canaries around energy, dctrl / ctrl, flow, dflow and the workspace are intact, and the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd, dhw, d3 = _geom(sp, d)
    G = ref.grid(sp, d)
    ws_bytes = lib.trx_bspline_workspace_bytes(nd, B, *dhw, *d3)
    assert ws_bytes > 0
    nflow, nctrl = B * nd * math.prod(sp) * 4, B * nd * math.prod(G) * 4
    ws, flow, dflow, dctrl, energy = _Guarded(ws_bytes, 0x5A), _Guarded(nflow, 0xA5), _Guarded(nflow, 0xC3), _Guarded(nctrl, 0x3C), _Guarded(B * 4, 0x96)
    stream = _lib.current_stream(torch.device("cuda"))
    ctrl = _rand((B, nd) + G, 6).cuda()
    rc = lib.trx_bspline_bending(_lib.ptr(ctrl), _lib.ptr(energy.region), _lib.ptr(dctrl.region), 1.0, 0, nd, B, *dhw, *d3, _lib.ptr(ws.region), ws_bytes,
                                 stream)
    _lib.check(rc, "trx_bspline_bending")
    torch.cuda.synchronize()
    e, g = tr.bspline_bending(ctrl, sp, d, grad=True)
    assert torch.equal(energy.floats((B,)), e) and torch.equal(dctrl.floats((B, nd) + G), g)
    for buf, what in ((ws, "the workspace"), (energy, "energy"), (dctrl, "dctrl")):
        buf.check(what)

    mov, tgt = _pair(sp, B=B)
    batch = tr._engine._Batch(mov.cuda(), tgt.cuda(), tables=False)
    vol = batch.vol()
    cg = dctrl.floats((B, nd) + G)
    c0 = _ctrl0(B, sp, d, 9).cuda()
    cg.copy_(c0)
    m, v = torch.zeros_like(c0), torch.zeros_like(c0)
    losses, step = torch.full((B, 3), float("nan"), device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    st = _lib.BSplineState()
    st.ctrl, st.adam_m, st.adam_v = cg.data_ptr(), m.data_ptr(), v.data_ptr()
    st.flow, st.dflow = flow.region.data_ptr(), dflow.region.data_ptr()
    st.losses, st.losses_capacity, st.step = losses.data_ptr(), 3, step.data_ptr()
    st.bending_weight = 20.0
    loss, opt = tr.LossSpec(w_mse=1.0, w_ncc=0.01).c(), tr._engine.opt_cfg("adam", 0.05)
    rc = lib.trx_bspline_run(ctypes.byref(vol), ctypes.byref(loss), ctypes.byref(opt), ctypes.byref(st), (ctypes.c_int * 3)(*d3), 3,
                             _lib.ptr(ws.region), ws_bytes, stream)
    _lib.check(rc, "trx_bspline_run")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (flow, "flow"), (dflow, "dflow"), (dctrl, "ctrl")):
        buf.check(what)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), d, loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01), optimizer="adam", lr=0.05, init=c0, capacity=3,
                         bending_weight=20.0)
    s.run(3)
    torch.cuda.synchronize()
    assert step.tolist() == [3] * B and torch.equal(cg, s.ctrl) and torch.equal(losses, s.losses)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. bending_weight = 0
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_weight_zero_gives_the_bits_of_a_solver_without_the_keyword(tr):
    shape, spacing = (20, 24, 28), (5, 4, 6)
    mov, tgt = (t.cuda() for t in _pair(shape, B=2))
    kw = dict(loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01), optimizer="adam", lr=0.05, init=_ctrl0(2, shape, spacing, 7), capacity=8)
    plain, zero = tr.BSplineSolver(mov, tgt, spacing, **kw), tr.BSplineSolver(mov, tgt, spacing, bending_weight=0.0, **kw)
    plain.run(8)
    zero.run(8)
    torch.cuda.synchronize()
    assert torch.equal(plain.losses, zero.losses) and torch.equal(plain.ctrl, zero.ctrl) and torch.equal(plain.flow, zero.flow)
    assert torch.isfinite(plain.losses).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. the loop against torch autograd on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def _arbiter(mov, tgt, spacing, ctrl0, lr, iters, optimizer, dtype, lam, **loss_kw):
    """test_gpu_bspline._arbiter with the penalty: expand -> flow_warp -> weighted_loss, + lam * E (the restatement's squares form), under torch
    autograd + torch.optim on the CPU.  Returns the totals, the final ctrl and the bending energy of the final ctrl."""
    from oracle import compose
    sp = tuple(mov.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    c = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([c], lr) if optimizer == "sgd" else torch.optim.Adam([c], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = compose.weighted_loss(tgt, compose.flow_warp(mov, ref.expand(c, sp, spacing, dtype=dtype)), **loss_kw)
        if lam:
            e = e + lam * bref.energy_squares(c, sp, spacing, dtype=dtype).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), c.detach().numpy(), bref.energy_squares(c.detach(), sp, spacing).sum().item()


CASE_A = ((20, 24, 28), (5, 4, 6), "adam", 0.025, 4.5e4, dict(w_ncc=1.0))
LOOP_CASES = [CASE_A,
              ((20, 24, 28), (5, 4, 6), "sgd", 250.0, 19.3, dict(w_mse=1.0)),
              ((40, 44), (5, 6), "adam", 0.0125, 653.0, dict(w_mse=1.0, w_ncc=0.01))]


@pytest.mark.parametrize("shape,spacing,optimizer,lr,lam,loss_kw", LOOP_CASES)
def test_bspline_loop_with_bending_vs_torch_autograd(tr, shape, spacing, optimizer, lr, lam, loss_kw):
    """trx_bspline_run with bending_weight = lam against the same objective (data term + lam E) under torch autograd in fp64, 12 iterations
    from a random control tensor of amplitude 0.4; bars as in test_bspline_loop_vs_torch_autograd.  lam and lr were chosen on the CPU so that
    the arbiter's total falls in every iteration (NCC + Adam 148.706 -> 102.681, MSE + SGD 0.0318819 -> 0.0115101, 2-D 0.803229 -> 0.603203);
    in the first case lam E is a third of the total at the start."""
    iters = 12
    mov, tgt = _pair(shape)
    c0 = _ctrl0(1, shape, spacing, 7)
    l64, c64, _ = _arbiter(mov, tgt, spacing, c0, lr, iters, optimizer, torch.float64, lam, **loss_kw)
    l32, c32, _ = _arbiter(mov, tgt, spacing, c0, lr, iters, optimizer, torch.float32, lam, **loss_kw)
    print(f"arbiter: total {l64[0]:.6g} -> {l64[-1]:.6g}")
    assert np.all(np.diff(l64) < 0)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, loss=tr.LossSpec(**loss_kw), optimizer=optimizer, lr=lr, init=c0, capacity=iters,
                         bending_weight=lam)
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
# 8. early stop on the total
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", ["one", "split", "single"])
def test_bspline_loop_with_bending_stops_on_the_total(tr, calls):
    """stop_crit halfway between totals 4 and 5 of a probe run: the solver stops at the total that falls below it (a data term alone is a
    third smaller and would stop at once), bit for bit against un-stopped solvers run k + 1 and k iterations."""
    shape, spacing, optimizer, lr, lam, loss_kw = CASE_A
    mov, tgt = (t.cuda() for t in _pair(shape))
    N, k = 12, 5
    kw = dict(loss=tr.LossSpec(**loss_kw), optimizer=optimizer, lr=lr, init=_ctrl0(1, shape, spacing, 7), capacity=N, bending_weight=lam)
    free = tr.BSplineSolver(mov, tgt, spacing, **kw)
    free.run(N)
    L = free.losses[0].cpu().numpy().astype(np.float64)
    assert np.all(np.diff(L[: k + 2]) < 0), "the probe run must descend so that a threshold between two totals is well defined"
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
    assert torch.equal(s.flow_last, before.flow) and not torch.equal(s.flow_last, s.flow)
    assert torch.equal(s.adam_m, after.adam_m) and torch.equal(s.adam_v, after.adam_v)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. public surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_flow_register_and_register_take_the_bending_weight(tr):
    """Case 7a through flow_register (from the test's random start) and Register (spacing 5, from zero): the bending energy of the final
    lattice is below that of the same run with bending_weight = 0 (CPU arbiter from the random start: 7.1e-5 against 2.3e-3)."""
    shape, spacing, optimizer, lr, lam, _ = CASE_A
    mov, tgt = (t.cuda() for t in _pair(shape))
    energies = {}
    for w in (lam, 0.0):
        fr = tr.flow_register(shape, criterions=[tr.NCCLoss()], weights=[1.0], lr=lr, max_epochs=12, flow_model="bspline", spacing=spacing, optimizer=optimizer,
                              bending_weight=w)
        fr.init_control = _ctrl0(1, shape, spacing, 7)
        fr.optimize(mov, tgt, debug=False)
        assert fr.losses.shape == (1, 12) and torch.isfinite(fr.losses).all() and torch.isfinite(fr.control).all()
        energies[w] = tr.bspline_bending(fr.control, shape, spacing)[0].item()
    print(f"flow_register: E {energies[lam]:.3e} with the penalty, {energies[0.0]:.3e} without")
    assert energies[lam] < energies[0.0]
    for w in (lam, 0.0):
        reg = tr.Register("flow", criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=5, optimizer=optimizer, bending_weight=w)
        reg.optim(mov, tgt, lr=lr, max_epochs=12)
        assert reg.control.shape == (1, 3) + tr.bspline_grid(shape, 5) and torch.isfinite(reg.control).all() and torch.isfinite(reg(mov)).all()
        energies[w] = tr.bspline_bending(reg.control, shape, 5)[0].item()
    print(f"Register: E {energies[lam]:.3e} with the penalty, {energies[0.0]:.3e} without")
    assert energies[lam] < energies[0.0]


def test_register_levels_apply_the_weight_to_each_level(tr):
    """levels=2: the coarse level is the single-level run on the coarse images with the same lambda, and the fine level is a BSplineSolver on
    base = upsample_flow(coarse flow) with the same lambda (its lattice from zero, the base not penalised): equal loss curves, bit for bit.
    The fine level's recorded losses are totals: entry t = data term at the lattice before update t + lambda E of that lattice, checked at
    the last entry against bspline_bending and a one-iteration solver without the penalty, to 1e-5 of the total (fp32 sums of two terms)."""
    from torchregister_amd.warpings import loss_spec_from
    shape, lam, lr = (20, 24, 28), 4.5e4, 0.025
    mov, tgt = (t.cuda() for t in _pair(shape))
    kw = dict(criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=5, optimizer="adam", bending_weight=lam)
    reg = tr.Register("flow", levels=2, **kw)
    reg.optim(mov, tgt, lr=lr, max_epochs=[8, 6])
    l0, l1 = reg.level_losses
    assert l0.shape == (1, 8) and l1.shape == (1, 6) and torch.isfinite(l0).all() and torch.isfinite(l1).all()
    movs, tgts = tr.pyramid(mov, 2, align_corners=True), tr.pyramid(tgt, 2, align_corners=True)
    coarse = tr.Register("flow", **kw)
    coarse.optim(movs[0], tgts[0], lr=lr, max_epochs=8)
    assert torch.equal(coarse.losses, l0)
    base = tr.upsample_flow(coarse.final_theta, shape)
    spec = loss_spec_from([tr.NCCLoss()], [1.0])
    skw = dict(loss=spec, optimizer="adam", lr=lr, base=base, capacity=6)
    fine = tr.BSplineSolver(movs[1], tgts[1], 5, bending_weight=lam, **skw)
    fine.run(5)
    ctrl5 = fine.ctrl.clone()
    fine.run(1)
    torch.cuda.synchronize()
    assert torch.equal(fine.losses, l1) and torch.equal(fine.ctrl, reg.control)
    data = tr.BSplineSolver(movs[1], tgts[1], 5, init=ctrl5, **skw)
    data.run(1)
    torch.cuda.synchronize()
    e5 = tr.bspline_bending(ctrl5, shape, 5)[0].item()
    total = data.losses[0, 0].item() + lam * e5
    print(f"fine level, entry 5: recorded {l1[0, 5].item():.6f}, data {data.losses[0, 0].item():.6f} + lambda E {lam * e5:.6f}")
    assert lam * e5 > 1e-3 * total, "the penalty must be visible in the total for this check to mean anything"
    assert abs(l1[0, 5].item() - total) <= 1e-5 * abs(total)
