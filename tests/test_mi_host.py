"""CPU checks of the mutual-information restatement (tests/mi_ref.py) on its own: the properties the definition in include/trx.h promises, so
that the GPU tests (tests/test_gpu_mi.py) only have to assert parity with it."""
import pytest
import torch

import bspline_ref
import mi_ref
import phantoms as ph


def _pair(shape=(12, 14, 16), seed=3):
    """The multimodal pair: a blob phantom as target; the same phantom warped by a small flow, then sent through the non-monotone map 4x(1 - x)."""
    from oracle import compose
    tgt = ph.blobs(shape, seed)
    warped = compose.flow_warp(tgt, ph.flow_field(shape, amp=1.2, f=0.013))
    return tgt, warped, 4.0 * warped * (1.0 - warped)


def test_weights_partition_unity_and_their_derivatives_sum_to_zero():
    r = torch.linspace(0.0, 1.0, 1001, dtype=torch.float64)
    w, d = mi_ref.weights(r), mi_ref.dweights(r)
    assert (w >= 0).all() and (w.sum(-1) - 1.0).abs().max().item() < 1e-15
    assert d.sum(-1).abs().max().item() < 1e-15
    rr = r.clone().requires_grad_()
    for j in range(4):
        (g,) = torch.autograd.grad(mi_ref.weights(rr)[:, j].sum(), rr)
        assert (g - d[:, j]).abs().max().item() < 1e-14


@pytest.mark.parametrize("bins", [8, 32, 64])
def test_joint_table_sums_to_one_and_every_index_is_inside(bins):
    g = torch.Generator().manual_seed(bins)
    t, w = torch.rand(2, 500, generator=g) * 3 - 1, torch.rand(2, 500, generator=g) * 3 - 1
    rng = torch.tensor([[-1.0, 2.0, -1.0, 2.0], [0.0, 1.0, 0.0, 1.0]])       # the second pair has values outside its range on both sides
    a, c, u, _ = mi_ref.coords(t, w, bins, rng)
    assert a.min() >= 0 and a.max() <= bins - 1 and c.min() >= 1 and c.max() <= bins - 3
    r = u - c
    assert r.min() >= 0 and r.max() <= 1
    P = mi_ref.joint(t, w, bins, rng)
    assert (P >= 0).all() and (P.sum((1, 2)) - 1.0).abs().max().item() < 1e-14


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("bins", [8, 32])
def test_loss_is_not_negative(bins, normalized):
    tgt, _, mov = _pair()
    g = torch.Generator().manual_seed(1)
    noise = torch.rand(tgt.shape, generator=g)
    for t, w in ((tgt, mov), (tgt, tgt), (tgt, noise), (noise, mov)):
        v = mi_ref.loss(t, w, bins, 1.0, normalized).item()
        assert v >= -1e-12, v
        if normalized:
            assert v <= 1.0 + 1e-12, v


@pytest.mark.parametrize("normalized", [False, True])
def test_interior_finite_differences_match_autograd(normalized):
    """Central differences (h = 1e-6, fp64 throughout) at 40 voxels whose coordinate x lies strictly inside (0, K - 3) and away from it by more
    than h: 1e-7 relative to the largest gradient.  A voxel exactly on an end of the range is only one-sidedly differentiable and is left out."""
    tgt, _, mov = _pair()
    bins = 16
    rng = mi_ref.fit_range(tgt, mov)
    w = mov.double().clone().requires_grad_()
    (grad,) = torch.autograd.grad(mi_ref.loss(tgt, w, bins, 1.0, normalized, rng).sum(), w)
    _, _, u, _ = mi_ref.coords(tgt.reshape(1, -1), mov.double().reshape(1, -1), bins, rng)
    x = (u - 1.0).flatten()
    interior = ((x > 1e-3) & (x < bins - 3 - 1e-3)).nonzero().flatten()
    pick = interior[torch.linspace(0, len(interior) - 1, 40).long()]
    h, flat = 1e-6, mov.double().flatten()
    worst = 0.0
    for i in pick.tolist():
        up, dn = flat.clone(), flat.clone()
        up[i] += h
        dn[i] -= h
        fd = (mi_ref.loss(tgt, up.view_as(mov), bins, 1.0, normalized, rng) - mi_ref.loss(tgt, dn.view_as(mov), bins, 1.0, normalized, rng)).item() / (2 * h)
        worst = max(worst, abs(fd - grad.flatten()[i].item()))
    assert worst <= 1e-7 * grad.abs().max().item(), (worst, grad.abs().max().item())


@pytest.mark.parametrize("normalized", [False, True])
def test_gradient_is_the_table_formula(normalized):
    """autograd through index_add equals (s_w / N) [0 <= x <= K - 3] sum_j G[a][c - 1 + j] beta'_j(r) with G = d loss / d P."""
    tgt, _, mov = _pair()
    bins = 32
    rng = torch.tensor([[0.1, 0.8, 0.05, 0.9]])                # narrower than the data: clamped voxels on both sides
    w = mov.double().clone().requires_grad_()
    (grad,) = torch.autograd.grad(mi_ref.loss(tgt, w, bins, 2.0, normalized, rng).sum(), w)
    G = mi_ref.grad_table(mi_ref.joint(tgt, mov.double(), bins, rng), 2.0, normalized)[0]
    a, c, u, s_w = mi_ref.coords(tgt.reshape(1, -1), mov.double().reshape(1, -1), bins, rng)
    x, r = (u - 1.0)[0], (u - c)[0]
    inside = (mov.double().flatten() - rng[0, 2].double()) * s_w
    mask = ((inside >= 0) & (inside <= bins - 3)).double()
    rows = G[a[0][:, None], (c[0] - 1)[:, None] + torch.arange(4)]
    want = s_w / x.numel() * mask * (rows * mi_ref.dweights(r)).sum(-1)
    assert (mask == 0).any() and (mask == 1).any()
    assert (grad.flatten() - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("normalized", [False, True])
def test_intensity_remaps_leave_the_loss_unchanged(normalized):
    """With ranges fitted to the data, loss(t, w) = loss(t, -2.5 w + 7) (a negative slope mirrors the bins) and = loss(2 t, w), to 1e-8.  Images, ranges
    and coordinates are fp64 here: in fp32 the two runs round their coordinates differently."""
    tgt, _, mov = _pair()
    w = mov.double()
    lo, hi = w.min().item(), w.max().item()
    t_lo, t_hi = tgt.min().item(), tgt.max().item()
    f64 = dict(dtype=torch.float64)
    base = mi_ref.loss(tgt, w, 32, 1.0, normalized, torch.tensor([[t_lo, t_hi, lo, hi]], **f64)).item()
    flipped = mi_ref.loss(tgt, -2.5 * w + 7.0, 32, 1.0, normalized, torch.tensor([[t_lo, t_hi, -2.5 * hi + 7.0, -2.5 * lo + 7.0]], **f64)).item()
    assert abs(base - flipped) <= 1e-8, (base, flipped)
    scaled = mi_ref.loss(2.0 * tgt, w, 32, 1.0, normalized, torch.tensor([[2.0 * t_lo, 2.0 * t_hi, lo, hi]], **f64)).item()
    assert abs(base - scaled) <= 1e-8, (base, scaled)


def test_degenerate_tables_and_constant_images():
    """H_TW = 0 (a table with one cell): loss 0 and gradient 0 in both modes.  A constant target has H_T = 0 and H_TW = H_W: the plain loss
    is 0 and its gradient vanishes.  A constant warped image carries no mutual information: the plain loss is alpha H_T, and the gradient
    vanishes in both modes (every voxel sees the same four table entries per target bin, in ratios that the derivative weights, which sum to
    0, cancel).  The cubic window never puts a real image into a single cell, so H_TW = 0 is reached only by the table itself."""
    P = torch.zeros(1, 8, 8, dtype=torch.float64)
    P[0, 3, 4] = 1.0
    for normalized in (False, True):
        assert mi_ref.loss_from_table(P, 1.0, normalized).item() == 0.0
        assert mi_ref.grad_table(P, 1.0, normalized).abs().max().item() == 0.0
    tgt, _, mov = _pair()
    const = torch.full_like(tgt, 0.37)
    w = mov.double().clone().requires_grad_()
    v = mi_ref.loss(const, w, 32, 1.0, False)
    (g,) = torch.autograd.grad(v.sum(), w)
    assert abs(v.item()) <= 1e-12 and g.abs().max().item() <= 1e-12
    for normalized in (False, True):
        w = const.double().clone().requires_grad_()
        v = mi_ref.loss(tgt, w, 32, 1.5, normalized)
        (g,) = torch.autograd.grad(v.sum(), w)
        assert g.abs().max().item() <= 1e-12 and torch.isfinite(v).all()
        if not normalized:
            P = mi_ref.joint(tgt, const.double(), 32)
            h_t = -(P.sum(2)[P.sum(2) > 0] * torch.log(P.sum(2)[P.sum(2) > 0])).sum().item()
            assert abs(v.item() - 1.5 * h_t) <= 1e-12


def _register(tgt, mov, criterion, iters=40, spacing=4, lr=0.1):
    from oracle import compose
    sp = tuple(tgt.shape[2:])
    t64, m64 = tgt.double(), mov.double()
    c = torch.zeros((1, 3) + bspline_ref.grid(sp, spacing), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([c], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = criterion(t64, compose.flow_warp(m64, bspline_ref.expand(c, sp, spacing, dtype=torch.float64)))
        e.backward()
        opt.step()
        losses.append(e.item())
    return losses, bspline_ref.expand(c.detach(), sp, spacing, dtype=torch.float64)


def test_mutual_information_registers_a_multimodal_pair():
    """B-spline FFD (spacing 4, Adam lr 0.1, 40 iterations, fp64) of the remapped moving image onto the target.  The arbiter is the MSE between
    the target and the UN-remapped moving image warped by the flow the criterion found: the objective falls 0.3878 -> 0.2383 and that MSE
    2.54e-3 -> 0.97e-3 (ratio 0.38; asserted < 0.5, the bar the criterion was proposed with).  The prototype behind that bar recorded 0.3965 -> 0.2438 and
    0.98e-3: its objective differs by 2 % already at iteration 0, where the MSE agrees, so the difference is in how it formed its bins (its code is not
    kept; fitting the range per call or once, widened to 0 or not, all give 0.3878 here), not in the loop."""
    from oracle import compose
    tgt, plain, mov = _pair()
    rng = mi_ref.fit_range(tgt, mov)
    mse = lambda flow: ((tgt.double() - compose.flow_warp(plain.double(), flow)) ** 2).mean().item()  # noqa: E731
    before = mse(torch.zeros(1, 3, *tgt.shape[2:], dtype=torch.float64))
    losses, flow = _register(tgt, mov, lambda t, w: mi_ref.loss(t, w, 32, 1.0, False, rng).sum())
    ratio = mse(flow) / before
    print(f"MI: objective {losses[0]:.4f} -> {losses[-1]:.4f}, MSE {before:.3e} -> {mse(flow):.3e} (ratio {ratio:.3f})")
    assert losses[-1] < losses[0] and ratio < 0.5, (losses[0], losses[-1], ratio)
