"""Parzen joint-histogram mutual information (Mattes-style) - the definition behind trx_mi_loss_grad (include/trx.h), restated in torch.

Per pair: target t, warped w (N voxels), K bins, range (lo_t, hi_t, lo_w, hi_w) in fp32.
  target bin   a = clamp(floor((t - lo_t) s_t), 0, K - 1),  s_t = K / (hi_t - lo_t)  (0 for an empty range) - a box window.  Always formed with
               the kernel's fp32 operations (one subtract, one multiply), whatever `dtype` says.
  warped       x = (w - lo_w) s_w,  s_w = (K - 3) / (hi_w - lo_w)  (0 for an empty range),  u = 1 + clamp(x, 0, K - 3),  c = min(floor(u), K - 3),
               r = u - c; bins c - 1 .. c + 2 receive the cubic B-spline weights of r.  s_w and x are formed in w's own dtype (fp32 input: the
               kernel's fp32 divide, subtract and multiply; fp64 input: fp64, for finite differences and invariance checks), everything behind
               them in `dtype`.
  P[a][k] = (1 / N) sum_v [a_v = a] beta_k(u_v) by index_add into K^2 cells; entropies with the natural logarithm, 0 log 0 = 0.
  loss = alpha (H_TW - H_W)  or, normalized,  alpha (2 - (H_T + H_W) / H_TW)  (0 when H_TW = 0).
Differentiable with respect to w (torch autograd; clamp's backward is inclusive at both ends)."""
import torch


def weights(r):
    """The four cubic B-spline weights of r in [0, 1], stacked on a new last axis: they sum to 1."""
    r2 = r * r
    r3 = r2 * r
    u = 1.0 - r
    return torch.stack([u * u * u, 3.0 * r3 - 6.0 * r2 + 4.0, -3.0 * r3 + 3.0 * r2 + 3.0 * r + 1.0, r3], dim=-1) / 6.0


def dweights(r):
    """d weights / d r: they sum to 0."""
    r2 = r * r
    u = 1.0 - r
    return torch.stack([-u * u, 3.0 * r2 - 4.0 * r, -3.0 * r2 + 2.0 * r + 1.0, r2], dim=-1) / 2.0


def fit_range(target, moving):
    """[B][4] fp32 (lo_t, hi_t, lo_w, hi_w): the target's min / max, the moving image's min / max widened to contain 0."""
    t, m = target.detach().float().flatten(1), moving.detach().float().flatten(1)
    return torch.stack([t.amin(1), t.amax(1), m.amin(1).clamp(max=0.0), m.amax(1).clamp(min=0.0)], dim=1)


def scales(rng, bins, dtype=torch.float32):
    """(s_t, s_w) [B] in `dtype`, by one subtraction and one division in it; 0 where the range is empty."""
    rng = rng.to(dtype)
    dt, dw = rng[:, 1] - rng[:, 0], rng[:, 3] - rng[:, 2]
    one, zero = torch.ones_like(dt), torch.zeros_like(dt)
    # a tensor divided by a tensor: `number / tensor` is reciprocal-then-multiply in torch, one rounding more than the kernel's division
    s_t = torch.where(rng[:, 1] > rng[:, 0], torch.full_like(dt, bins) / torch.where(dt != 0, dt, one), zero)
    s_w = torch.where(rng[:, 3] > rng[:, 2], torch.full_like(dw, bins - 3) / torch.where(dw != 0, dw, one), zero)
    return s_t, s_w


def coords(t, w, bins, rng):
    """t, w [B][N] -> a [B][N] (long), c [B][N] (long), u [B][N] (w's dtype, differentiable), s_w [B] (w's dtype).  The target bin is always formed
    in fp32; the warped coordinate in w's dtype (range and scale converted to it first: an fp32 range is exact in fp64)."""
    s_t, _ = scales(rng, bins)
    a = torch.floor((t.float() - rng[:, 0:1].float()) * s_t[:, None]).clamp(0, bins - 1).long()
    _, s_w = scales(rng, bins, w.dtype)
    x = (w - rng[:, 2:3].to(w.dtype)) * s_w[:, None]
    u = 1.0 + x.clamp(0.0, float(bins - 3))
    c = torch.floor(u.detach()).clamp(max=bins - 3).long()
    return a, c, u, s_w


def joint(target, warped, bins=32, rng=None, dtype=torch.float64):
    """P [B][K][K] (target bin, warped bin)."""
    B = target.shape[0]
    t, w = target.reshape(B, -1), warped.reshape(B, -1)
    if rng is None:
        rng = fit_range(t, w)
    N = t.shape[1]
    a, c, u, _ = coords(t, w, bins, rng)
    r = (u - c.to(u.dtype)).to(dtype)
    wt = weights(r)                                                            # [B][N][4]
    cell = (a * bins + c - 1)[:, :, None] + torch.arange(4)                    # [B][N][4]
    cell = cell + (torch.arange(B) * bins * bins)[:, None, None]
    P = torch.zeros(B * bins * bins, dtype=dtype).index_add(0, cell.reshape(-1), wt.reshape(-1))
    return P.reshape(B, bins, bins) / N


def _entropy(p, dim):
    safe = torch.where(p > 0, p, torch.ones_like(p))
    return -(p * torch.log(safe)).sum(dim=dim)


def loss_from_table(P, alpha=1.0, normalized=False):
    """[B] from P [B][K][K]."""
    h_tw, h_t, h_w = _entropy(P, (1, 2)), _entropy(P.sum(2), 1), _entropy(P.sum(1), 1)
    if not normalized:
        return alpha * (h_tw - h_w)
    ok = h_tw > 0
    return torch.where(ok, alpha * (2.0 - (h_t + h_w) / torch.where(ok, h_tw, torch.ones_like(h_tw))), torch.zeros_like(h_tw))


def loss(target, warped, bins=32, alpha=1.0, normalized=False, rng=None, dtype=torch.float64):
    """[B] losses of target / warped [B, ...] (any trailing shape)."""
    return loss_from_table(joint(target, warped, bins, rng, dtype), alpha, normalized)


def grad_table(P, alpha=1.0, normalized=False):
    """G [B][K][K] = d loss / d P (0 where P = 0), by autograd on loss_from_table."""
    Pv = P.detach().clone().requires_grad_()
    (g,) = torch.autograd.grad(loss_from_table(Pv, alpha, normalized).sum(), Pv)
    return torch.where(P > 0, g, torch.zeros_like(g))
