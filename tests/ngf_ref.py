"""CPU restatement of the normalised gradient field criterion (include/trx.h: trx_ngf_loss_grad).

`loss` is the definition in torch ops with clamped indices, differentiable, with its per-voxel arithmetic in `dtype` (fp64: the arbiter; fp32: what fp32
arithmetic in another order gives - the yardstick of the GPU tests' bars) and its sum over the voxels in fp64, as the definition has it.  `adjoint_gather` is the closed-form D^T q of the header written out in
numpy, voxel by voxel: what the backward kernel must reproduce, checked against autograd in tests/test_ngf_host.py."""
import numpy as np
import torch


def differences(x, voxel=None, dtype=torch.float64):
    """[B,nd,*spatial]: (D_a x)(n) = sc / h_a (x(n + (ip - n_a) e_a) - x(n - (n_a - im) e_a)), ip = min(n_a + 1, S_a - 1), im = max(n_a - 1, 0),
    sc = 1/2 where ip - im == 2 else 1, of x [B,1,*spatial]."""
    x = x.to(dtype)
    nd = x.dim() - 2
    out = []
    for a in range(nd):
        S = x.shape[2 + a]
        n = torch.arange(S)
        ip, im = torch.clamp(n + 1, max=S - 1), torch.clamp(n - 1, min=0)
        sc = torch.where(ip - im == 2, torch.tensor(0.5, dtype=dtype), torch.tensor(1.0, dtype=dtype))
        h = 1.0 if voxel is None else float(voxel[a])
        shape = [1] * x.dim()
        shape[2 + a] = S
        out.append((sc * torch.tensor(1.0 / h, dtype=dtype)).reshape(shape) * (x.index_select(2 + a, ip) - x.index_select(2 + a, im)))
    return torch.cat(out, dim=1)


def _mask(mask, like):
    B = like.shape[0]
    if mask is None:
        return torch.ones((B, 1) + tuple(like.shape[2:]), dtype=torch.bool)
    return (torch.as_tensor(mask).reshape((B, 1) + tuple(like.shape[2:])) != 0)


def ratio(target, warped, eps, voxel=None, dtype=torch.float64):
    """(r [B,1,*spatial], gT, gW, s, a, b) with r = s^2 / (a b), 0 where a b == 0."""
    B = target.shape[0]
    gT, gW = differences(target, voxel, dtype), differences(warped, voxel, dtype)
    e = torch.as_tensor(eps).to(dtype).reshape(B, 2, *([1] * (target.dim() - 2)))
    s = (gW * gT).sum(1, keepdim=True)
    a = (gW * gW).sum(1, keepdim=True) + e[:, 1:2] ** 2
    b = (gT * gT).sum(1, keepdim=True) + e[:, 0:1] ** 2
    ab = a * b
    zero = ab == 0
    r = torch.where(zero, torch.zeros_like(ab), s * s / torch.where(zero, torch.ones_like(ab), ab))
    return r, gT, gW, s, a, b


def loss(target, warped, eps, voxel=None, mask=None, alpha=1.0, dtype=torch.float64):
    """[B] in `dtype`: alpha (1 - (1 / N_m) sum over the mask of r); 0 for a pair whose mask is empty.  Differentiable with respect to `warped`.
    The per-voxel arithmetic runs in `dtype`; the sum over the voxels runs in fp64 whatever `dtype` is, as the definition has it (the kernel adds r
    in fp64) - so the fp32 figure does not depend on the order in which a host's torch build adds a long fp32 vector - and is rounded to `dtype` once."""
    B = target.shape[0]
    r = ratio(target, warped, eps, voxel, dtype)[0]
    m = _mask(mask, target)
    n = m.reshape(B, -1).sum(1).double()
    mean = (r * m.to(dtype)).reshape(B, -1).double().sum(1) / torch.clamp(n, min=1.0)
    return torch.where(n > 0, alpha * (1.0 - mean), torch.zeros_like(mean)).to(dtype)


def fit_eps(target, moving, eta=1.0, voxel=None, mask=None):
    """[B,2] fp32: eta times the (masked) mean of |D I| of the target and of the moving image (fp32 arithmetic, as ngf_edge_parameters); a pair
    whose mask is empty, and an image of another shape than the mask, use the whole image."""
    B = target.shape[0]
    cols = []
    for x in (target, moving):
        mag = differences(x.float(), voxel, torch.float32).square().sum(1).sqrt().reshape(B, -1)
        mean = mag.mean(1)
        if mask is not None and tuple(x.shape[2:]) == tuple(target.shape[2:]):
            m = _mask(mask, target).reshape(B, -1).float()
            n = m.sum(1)
            mean = torch.where(n > 0, (mag * m).sum(1) / n.clamp(min=1.0), mean)
        cols.append(float(eta) * mean)
    return torch.stack(cols, dim=1)


def q_tilde(target, warped, eps, voxel=None, mask=None):
    """numpy fp64 [B,nd,*spatial]: q = dr / dgW = 2 s gT / (a b) - 2 s^2 gW / (a^2 b), 0 outside the mask and where a b == 0."""
    r, gT, gW, s, a, b = (t.numpy() for t in ratio(target, warped, eps, voxel, torch.float64))
    ab = a * b
    ok = (ab != 0) & _mask(mask, target).numpy()
    safe_ab, safe_a = np.where(ab != 0, ab, 1.0), np.where(a != 0, a, 1.0)
    q = 2.0 * s * gT / safe_ab - 2.0 * s * s * gW / (safe_a * safe_ab)
    return np.where(ok, q, 0.0)


def adjoint_gather(q, voxel=None):
    """numpy [B,*spatial]: (D^T q)(y) = sum_a (1 / h_a) [ [y_a >= 1] sc_a(y - e_a) q_a(y - e_a) + [y_a = S_a - 1] sc_a(y) q_a(y)
    - [y_a <= S_a - 2] sc_a(y + e_a) q_a(y + e_a) - [y_a = 0] sc_a(y) q_a(y) ], one voxel at a time, with sc from the definition of the difference."""
    B, nd = q.shape[:2]
    sp = q.shape[2:]
    out = np.zeros((B,) + sp)

    def sc(n, S):
        return 0.5 if min(n + 1, S - 1) - max(n - 1, 0) == 2 else 1.0

    for b in range(B):
        for y in np.ndindex(*sp):
            acc = 0.0
            for a in range(nd):
                S, h = sp[a], 1.0 if voxel is None else float(voxel[a])
                lo, hi = list(y), list(y)
                lo[a] -= 1
                hi[a] += 1
                t = 0.0
                if y[a] >= 1:
                    t += sc(y[a] - 1, S) * q[(b, a) + tuple(lo)]
                if y[a] == S - 1:
                    t += sc(y[a], S) * q[(b, a) + y]
                if y[a] <= S - 2:
                    t -= sc(y[a] + 1, S) * q[(b, a) + tuple(hi)]
                if y[a] == 0:
                    t -= sc(y[a], S) * q[(b, a) + y]
                acc += t / h
            out[(b,) + y] = acc
    return out


def grad_closed_form(target, warped, eps, voxel=None, mask=None, alpha=1.0):
    """numpy fp64 [B,1,*spatial]: grad_warped = -(alpha / N_m) D^T q (0 for a pair whose mask is empty)."""
    B = target.shape[0]
    n = _mask(mask, target).reshape(B, -1).sum(1).numpy().astype(np.float64)
    scale = np.where(n > 0, -alpha / np.maximum(n, 1.0), 0.0)
    g = adjoint_gather(q_tilde(target, warped, eps, voxel, mask), voxel)
    return (g * scale.reshape((B,) + (1,) * (g.ndim - 1)))[:, None]
