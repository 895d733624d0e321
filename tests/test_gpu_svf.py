"""GPU checks of the stationary-velocity-field model (csrc/svf.hip, trx_bspline_svf_run in csrc/bspline.hip): trx_svf_exp and its adjoint against
the fp64 restatement (tests/svf_ref.py) at shapes where the edge handling can go wrong, the directional identity of the adjoint, determinism,
batch independence and guard bytes, the fold test in closed form, the device-side loop against torch autograd on the CPU, the early stop, and
the public surface (svf_exp, BSplineSolver(squarings=), flow_register / Register(diffeomorphic=True))."""
import numpy as np
import pytest
import torch

import bspline_ref as bref
import phantoms as ph
import svf_ref as ref
from conftest import bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


CASE_IDS = ["%dx%s-K%d" % (c[0], "x".join(map(str, c[1])), c[2]) for c in ref.CASES]
_CACHE = {}


def _case(case, inverse):
    """Inputs and the restatement's results of a case, computed once: v, dflow (fp32), exp and the adjoint in fp64 and fp32."""
    key = (case, inverse)
    if key not in _CACHE:
        K = ref.CASES[case][2]
        v, g = ref.case_inputs(case, inverse)
        _CACHE[key] = dict(v=v, g=g, K=K, f64=ref.exp(v, K, inverse), f32=ref.exp(v, K, inverse, dtype=torch.float32),
                           b64=ref.exp_backward(v, g, K, inverse), b32=ref.exp_backward(v, g, K, inverse, dtype=torch.float32))
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1, 2. exp and its adjoint against the fp64 restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("case", range(len(ref.CASES)), ids=lambda i: CASE_IDS[i])
def test_exp_matches_the_restatement(tr, case, inverse):
    """max |svf_exp - ref64| <= bar(ref32, ref64, 1e-5 max|ref64|): the forward is continuous across lattice planes, so there are no outliers."""
    c = _case(case, inverse)
    got = tr.svf_exp(c["v"].cuda(), c["K"], inverse=inverse).double().cpu()
    assert got.shape == c["v"].shape
    err, tol = (got - c["f64"]).abs().max().item(), bar(c["f32"].numpy(), c["f64"].numpy(), 1e-5 * c["f64"].abs().max().item())
    print(f"exp {CASE_IDS[case]} inverse={inverse}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)
    if c["K"] == 0:
        assert torch.equal(got.float(), -c["v"] if inverse else c["v"])


@pytest.mark.parametrize("inverse", [False, True], ids=["fwd", "inv"])
@pytest.mark.parametrize("case", range(len(ref.CASES)), ids=lambda i: CASE_IDS[i])
def test_exp_backward_matches_the_restatement(tr, case, inverse):
    """Every element finite; all but at most max(4, 0.1 %) of them within bar(ref32, ref64, 1e-5 max|dvel_ref64|) (the gradient of a trilinear
    sample jumps where a position crosses a lattice plane: single elements may differ between any two precisions; the seeds are those at
    which the restatement's own fp32 shows none, tests/test_svf_host.py).  So that the allowance hides no real error, the directional
    identity: for 8 smooth directions d, <dvel_gpu, d> = <dflow, (exp64(v + e d) - exp64(v - e d)) / 2e>, e = 1e-4, to 1e-4 relative (the
    directions are those of svf_ref.directions: small, and with no kink of exp inside the difference quotient)."""
    c = _case(case, inverse)
    got = tr.svf_exp_backward(c["v"].cuda(), c["g"].cuda(), c["K"], inverse=inverse).double().cpu()
    assert bool(torch.isfinite(got).all())
    tol = bar(c["b32"].numpy(), c["b64"].numpy(), 1e-5 * c["b64"].abs().max().item())
    err = (got - c["b64"]).abs()
    left_out, allowed = int((err > tol).sum()), max(4, got.numel() // 1000)
    print(f"backward {CASE_IDS[case]} inverse={inverse}: max err {err.max().item():.3e} bar {tol:.3e}, {left_out} of {got.numel()} elements beyond the bar (allowed {allowed})")
    assert left_out <= allowed, (left_out, allowed, err.max().item(), tol)
    dirs = ref.directions(case, inverse)
    assert len(dirs) == 8
    for d, rhs in dirs:
        lhs = (got * d).sum().item()
        assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (lhs, rhs)


def test_autograd_through_svf_exp_gives_the_bits_of_svf_exp_backward(tr):
    c = _case(1, False)
    v = c["v"].cuda().requires_grad_()
    flow = tr.svf_exp(v, c["K"])
    assert flow.requires_grad and torch.equal(flow.detach(), tr.svf_exp(c["v"].cuda(), c["K"]))
    flow.backward(c["g"].cuda())
    assert torch.equal(v.grad, tr.svf_exp_backward(c["v"].cuda(), c["g"].cuda(), c["K"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. determinism, batch independence, guard bytes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bits_and_pairs_do_not_see_each_other(tr):
    c = _case(1, False)        # (2, (9, 10, 11), K = 4)
    v, g = c["v"].cuda(), c["g"].cuda()
    assert torch.equal(tr.svf_exp_backward(v, g, 4), tr.svf_exp_backward(v, g, 4))
    v3, g3 = ref.smooth_field(3, (9, 10, 11), 6.0, 77).cuda(), ref.smooth_field(3, (9, 10, 11), 1.0, 78, noise=0.5).cuda()
    g3[2] *= 1000.0            # the other pairs' gradients are of another magnitude: a pair's fixed-point scale is its own
    for inverse in (False, True):
        assert torch.equal(tr.svf_exp(v3, 4, inverse=inverse)[1:2], tr.svf_exp(v3[1:2], 4, inverse=inverse))
        assert torch.equal(tr.svf_exp_backward(v3, g3, 4, inverse=inverse)[1:2], tr.svf_exp_backward(v3[1:2], g3[1:2], 4, inverse=inverse))


def test_a_non_finite_dflow_stays_in_its_pair(tr):
    v, g = ref.smooth_field(2, (9, 10, 11), 3.0, 5).cuda(), ref.smooth_field(2, (9, 10, 11), 1.0, 6, noise=0.5).cuda()
    want = tr.svf_exp_backward(v[1:], g[1:], 4)
    g[0, 1, 3, 4, 5] = float("inf")
    got = tr.svf_exp_backward(v, g, 4)
    assert torch.equal(got[1:], want) and not bool(torch.isfinite(got[0]).all())
    zero = tr.svf_exp_backward(v, torch.zeros_like(g), 4)
    assert torch.count_nonzero(zero).item() == 0


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


@pytest.mark.parametrize("case", [0, 1, 2, 6], ids=lambda i: CASE_IDS[i])
def test_calls_stay_inside_their_buffers(tr, case):
    """trx_svf_exp and trx_svf_exp_backward with the workspace at exactly trx_svf_workspace_bytes: canaries around flow, dvel and the
    workspace are intact, and the guarded calls give the bits of the wrappers."""
    from torchregister_amd import _lib
    lib = _lib.load()
    B, sp, K, _ = ref.CASES[case]
    nd = len(sp)
    c = _case(case, False)
    v, g = c["v"].cuda(), c["g"].cuda()
    geom = (nd, B) + (1,) * (3 - nd) + sp + (K, 0)
    ws_bytes = lib.trx_svf_workspace_bytes(*geom[:-1])
    assert ws_bytes > 0
    ws, flow, dvel = _Guarded(ws_bytes, 0x5A), _Guarded(v.numel() * 4, 0xA5), _Guarded(v.numel() * 4, 0xC3)
    stream = _lib.current_stream(torch.device("cuda"))
    _lib.check(lib.trx_svf_exp(_lib.ptr(v), _lib.ptr(flow.region), *geom, _lib.ptr(ws.region), ws_bytes, stream), "trx_svf_exp")
    _lib.check(lib.trx_svf_exp_backward(_lib.ptr(v), _lib.ptr(g), _lib.ptr(dvel.region), *geom, _lib.ptr(ws.region), ws_bytes, stream), "trx_svf_exp_backward")
    torch.cuda.synchronize()
    for buf, what in ((ws, "the workspace"), (flow, "flow"), (dvel, "dvel")):
        buf.check(what)
    assert torch.equal(flow.floats(v.shape), tr.svf_exp(v, K)) and torch.equal(dvel.floats(v.shape), tr.svf_exp_backward(v, g, K))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the fold test (closed form)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spatial,det_plain,det_exp", [((32, 40), -0.38, 0.284), ((16, 18, 20), -0.30, 0.304)])
def test_exp_unfolds_what_the_displacement_folds(tr, spatial, det_plain, det_exp):
    """id + v folds (minimum central-difference determinant -0.38 / -0.30 in fp64), id + exp(v) with 6 squarings does not (+0.284 / +0.304):
    the GPU's minimum is positive and within 1e-3 of the restatement's; exp(-v) meets the bar of the exp test."""
    v = ref.fold_field(spatial)
    assert abs(ref.jacobian_det(v).min().item() - det_plain) < 0.01
    f64 = ref.exp(v, 6)
    want = ref.jacobian_det(f64).min().item()
    assert abs(want - det_exp) < 1e-3
    got = ref.jacobian_det(tr.svf_exp(v.float().cuda(), 6).double().cpu()).min().item()
    print(f"fold {spatial}: min det id + v {ref.jacobian_det(v).min().item():.4f}, id + exp(v) restatement {want:.4f}, GPU {got:.4f}")
    assert got > 0 and abs(got - want) <= 1e-3
    i64, i32 = ref.exp(v.float(), 6, inverse=True), ref.exp(v.float(), 6, inverse=True, dtype=torch.float32)
    inv = tr.svf_exp(v.float().cuda(), 6, inverse=True).double().cpu()
    err, tol = (inv - i64).abs().max().item(), bar(i32.numpy(), i64.numpy(), 1e-5 * i64.abs().max().item())
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. squarings = 0 is trx_bspline_run
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair(shape, seed=0, B=1):
    """Targets and movings of the B-spline loop tests: two different blob phantoms plus a ripple."""
    tgt = torch.cat([ph.blobs(shape, 61 + 10 * b + seed) + 0.05 * ph.vol(shape, 0.031, "sin") for b in range(B)])
    mov = torch.cat([ph.blobs(shape, 62 + 10 * b + seed) + 0.05 * ph.vol(shape, 0.027, "cos") for b in range(B)])
    return mov, tgt


def _ctrl0(B, shape, spacing, seed, amp=0.4):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, len(shape)) + bref.grid(shape, spacing), generator=g) * 2 * amp - amp


@pytest.mark.parametrize("shape,spacing", [((20, 24, 28), (5, 4, 6)), ((40, 44), (5, 6))])
def test_zero_squarings_is_the_displacement_loop_bit_for_bit(tr, shape, spacing):
    mov, tgt = (t.cuda() for t in _pair(shape))
    kw = dict(loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01), optimizer="adam", lr=0.1, init=_ctrl0(1, shape, spacing, 7), capacity=6, keep_last=True)
    plain, svf = tr.BSplineSolver(mov, tgt, spacing, **kw), tr.BSplineSolver(mov, tgt, spacing, squarings=0, **kw)
    plain.run(6)
    svf.run(6)
    torch.cuda.synchronize()
    assert torch.isfinite(plain.losses).all() and not torch.equal(plain.ctrl.cpu(), kw["init"])
    assert torch.equal(plain.ctrl, svf.ctrl) and torch.equal(plain.losses, svf.losses)
    assert torch.equal(plain.flow_last, svf.velocity_last) and torch.equal(plain.flow_last, svf.flow_last) and torch.equal(plain.flow, svf.flow)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. the loop against torch autograd on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def _arbiter(mov, tgt, spacing, ctrl0, K, lr, iters, optimizer, dtype, bending_weight=0.0, **loss_kw):
    """bspline_ref.expand -> svf_ref.exp -> oracle/compose.py flow_warp -> weighted_loss (+ lambda bending energy) under torch autograd +
    torch.optim, on the CPU."""
    from oracle import compose
    sp = tuple(mov.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    c = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([c], lr) if optimizer == "sgd" else torch.optim.Adam([c], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = compose.weighted_loss(tgt, compose.flow_warp(mov, ref.exp(bref.expand(c, sp, spacing, dtype=dtype), K, dtype=dtype)), **loss_kw)
        if bending_weight:
            import bspline_bending_ref as bend
            e = e + bending_weight * bend.energy_squares(c, sp, spacing, dtype=dtype).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), c.detach().numpy()


LOOP_CASES = [((20, 24, 28), (5, 4, 6), "adam", 0.1, 0.0, dict(w_ncc=1.0)),
              ((20, 24, 28), (5, 4, 6), "sgd", 1000.0, 0.0, dict(w_mse=1.0)),
              ((40, 44), (5, 6), "adam", 0.05, 0.0, dict(w_mse=1.0, w_ncc=0.01)),
              ((20, 24, 28), (5, 4, 6), "adam", 0.025, 4.5e4, dict(w_ncc=1.0))]


@pytest.mark.parametrize("shape,spacing,optimizer,lr,bending,loss_kw", LOOP_CASES, ids=["ncc-adam", "mse-sgd", "2d", "bending"])
def test_svf_loop_vs_torch_autograd(tr, shape, spacing, optimizer, lr, bending, loss_kw):
    """trx_bspline_svf_run (expand -> exp -> fused loss and dL/dphi -> the adjoint of exp -> reduce -> SGD / Adam, all on the device), K = 4,
    against the same objective under torch autograd in fp64, 12 iterations from a random control tensor of amplitude 0.4; bars = max(floor,
    2 x the arbiter's own fp32-vs-fp64 gap) with the floors of test_bspline_loop_vs_torch_autograd.  Each lr was chosen on the CPU so that
    the arbiter's loss falls in every iteration (NCC + Adam 99.1661 -> 90.6135, MSE + SGD 0.0106422 -> 0.00896352, 2-D 0.535492 -> 0.463125,
    NCC + Adam with bending_weight 4.5e4 - a third of the total at the start - 148.706 -> 102.681)."""
    iters, K = 12, 4
    mov, tgt = _pair(shape)
    c0 = _ctrl0(1, shape, spacing, 7)
    l64, c64 = _arbiter(mov, tgt, spacing, c0, K, lr, iters, optimizer, torch.float64, bending, **loss_kw)
    l32, c32 = _arbiter(mov, tgt, spacing, c0, K, lr, iters, optimizer, torch.float32, bending, **loss_kw)
    assert np.all(np.diff(l64) < 0)
    s = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, loss=tr.LossSpec(**loss_kw), optimizer=optimizer, lr=lr, init=c0, capacity=iters, squarings=K,
                         bending_weight=bending)
    s.run(iters)
    torch.cuda.synchronize()
    e, b = np.max(np.abs(s.losses[0].cpu().numpy() - l64)), bar(l32, l64, 2e-5 * np.max(np.abs(l64)))
    print(f"loss curve {l64[0]:.6g} -> {l64[-1]:.6g}: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {np.max(np.abs(l32 - l64)):.3e})")
    assert e <= b, ("loss curve", e, b)
    e, b = np.max(np.abs(s.ctrl.cpu().numpy() - c64)), bar(c32, c64, 2e-4)
    print(f"ctrl: err {e:.3e} bar {b:.3e} (arbiter fp32-fp64 {np.max(np.abs(c32 - c64)):.3e})")
    assert e <= b, ("ctrl", e, b)
    assert int(s.step[0]) == iters
    assert torch.equal(s.velocity, tr.bspline_expand(s.ctrl, shape, spacing)) and torch.equal(s.flow, tr.svf_exp(s.velocity, K))
    assert torch.equal(s.inverse_flow(), tr.svf_exp(s.velocity, K, inverse=True))


def test_svf_loop_stops_exactly(tr):
    """stop_crit between two recorded losses of a probe run: step = index + 1, that iteration's update has been applied, velocity_last is the
    velocity of that forward and flow_last its exponential, nothing is recorded or changed afterwards - bit for bit against un-stopped
    solvers run k + 1 and k iterations."""
    shape, spacing, K, N, k = (20, 24, 28), (5, 4, 6), 4, 12, 5
    mov, tgt = (t.cuda() for t in _pair(shape))
    kw = dict(loss=tr.LossSpec(w_mse=1.0, w_ncc=0.01), optimizer="adam", lr=0.1, init=_ctrl0(1, shape, spacing, 7), capacity=N, squarings=K)
    free = tr.BSplineSolver(mov, tgt, spacing, **kw)
    free.run(N)
    L = free.losses[0].cpu().numpy().astype(np.float64)
    assert np.all(np.diff(L[: k + 2]) < 0), "the probe run must descend so that a threshold between two losses is well defined"
    s = tr.BSplineSolver(mov, tgt, spacing, stop_crit=0.5 * (L[k] + L[k - 1]), **kw)
    s.run(4)
    s.run(N - 4)
    torch.cuda.synchronize()
    assert int(s.step[0]) == k + 1 and int(s.stopped[0]) != 0
    got = s.losses[0].cpu().numpy()
    assert np.array_equal(got[: k + 1], free.losses[0, : k + 1].cpu().numpy()) and np.all(np.isnan(got[k + 1:]))
    after, before = tr.BSplineSolver(mov, tgt, spacing, **kw), tr.BSplineSolver(mov, tgt, spacing, **kw)
    after.run(k + 1)
    before.run(k)
    torch.cuda.synchronize()
    assert torch.equal(s.ctrl, after.ctrl) and torch.equal(s.velocity, after.velocity) and torch.equal(s.flow, after.flow)
    assert torch.equal(s.velocity_last, before.velocity) and torch.equal(s.flow_last, before.flow) and not torch.equal(s.flow_last, s.flow)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. public surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _interior_mse(a, b):
    inner = (slice(None), slice(None)) + tuple(slice(3, -3) for _ in range(a.dim() - 2))
    return ((a[inner] - b[inner]) ** 2).mean().item()


def test_register_diffeomorphic_single_level(tr):
    """Blobs warped by ph.flow_field, NCC + Adam, spacing 6, 6 squarings, 15 iterations (CPU arbiter, _arbiter from a zero lattice: 3.537 -> 0.823)."""
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, ph.flow_field(shape)).cuda()
    tgt = tgt.cuda()
    reg = tr.Register("flow", criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, diffeomorphic=True, optimizer="adam")
    reg.optim(mov, tgt, lr=0.1, max_epochs=15)
    losses = reg.losses[0].cpu().numpy()
    print(f"register diffeomorphic: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses.shape == (15,) and losses[-1] < losses[0]
    assert reg.theta.shape == (1, 3) + shape and reg.velocity.shape == (1, 3) + shape and reg.control.shape == (1, 3) + tr.bspline_grid(shape, 6)
    assert torch.equal(reg.theta, tr.svf_exp(reg.velocity, 6)) and torch.equal(reg.inverse_flow, tr.svf_exp(reg.velocity, 6, inverse=True))
    assert torch.equal(reg.final_theta, tr.svf_exp(tr.bspline_expand(reg.control, shape, 6), 6))
    warped = reg(mov)
    assert torch.equal(warped, tr._engine.flow_warp(mov, reg.theta)) and torch.equal(reg.inverse(warped), tr._engine.flow_warp(warped, reg.inverse_flow))
    there, back = _interior_mse(warped, mov), _interior_mse(reg.inverse(warped), mov)
    print(f"interior MSE to moving: warped {there:.3e}, warped and back {back:.3e}")
    assert back < there
    assert float(ref.jacobian_det(reg.theta.double().cpu()).min()) > 0


def test_register_diffeomorphic_levels_hand_over_the_velocity(tr):
    """levels=2, max_epochs=[15, 0]: the fine level's lattice stays zero, so its velocity is its base, upsample_flow of the coarse level's
    final VELOCITY, bit for bit, and the deformation is the exponential of that."""
    from oracle import compose
    shape = (24, 28, 32)
    tgt = ph.blobs(shape, 5)
    mov = compose.flow_warp(tgt, ph.flow_field(shape)).cuda()
    tgt = tgt.cuda()
    kw = dict(criterion=[tr.NCCLoss()], weight=[1.0], flow_model="bspline", spacing=6, diffeomorphic=True, squarings=5, optimizer="adam")
    reg = tr.Register("flow", levels=2, **kw)
    reg.optim(mov, tgt, lr=0.1, max_epochs=[15, 0])
    assert [ls.shape[-1] for ls in reg.level_losses] == [15, 0]
    coarse = tr.Register("flow", **kw)
    coarse.optim(tr.pyramid(mov, 2, align_corners=True)[0], tr.pyramid(tgt, 2, align_corners=True)[0], lr=0.1, max_epochs=15)
    assert torch.equal(coarse.losses, reg.level_losses[0])
    coarse_final_velocity = tr.bspline_expand(coarse.control, tr.pyramid_shapes(shape, 2)[0], 6)
    assert torch.equal(reg.velocity, tr.upsample_flow(coarse_final_velocity, shape))
    assert torch.equal(reg.theta, tr.svf_exp(reg.velocity, 5)) and torch.count_nonzero(reg.control).item() == 0
    assert torch.equal(reg.inverse_flow, tr.svf_exp(reg.velocity, 5, inverse=True))
