"""The arbiter of the fused rigid / affine mutual-information entry points (trx_affine_mi_loss_grad, trx_affine_mi_run): oracle/compose.py::affine_warp
(with pose_to_theta for rigid) composed with tests/mi_ref.py::loss under torch autograd and torch.optim on the CPU, in fp32 and fp64.  A single
evaluation returns the loss, d loss / d theta and the joint table P; a loop returns the loss curve and the final parameter.  Nothing here touches
the GPU; tests/test_affine_mi_host.py asserts the conditions the GPU tests rely on (the loss falls, the two precisions stay together)."""
import functools

import numpy as np
import torch

import mi_ref
import phantoms as ph

# starts off the identity: there every sample sits on a voxel centre and the interpolant is only one-sidedly differentiable
THETA0_3 = [[1.01, 0.013, -0.007, 0.011], [-0.009, 0.99, 0.012, -0.013], [0.006, -0.011, 1.008, 0.009]]
THETA0_2 = [[1.01, 0.013, 0.011], [-0.009, 0.99, -0.013]]
POSE0_3 = (0.03, -0.02, 0.025, 0.05, -0.04, 0.03)
POSE0_2 = (0.04, 0.03, -0.02)


@functools.lru_cache(maxsize=None)
def pair(shape, seed=5):
    """(moving, target) [1,1,*shape] fp32: a blob phantom as target; the phantom warped by THETA_STAR and sent through the non-monotone map 4w(1 - w)."""
    from oracle import compose
    t = ph.blobs(shape, seed)
    w = compose.affine_warp(torch.tensor(ph.THETA_STAR3 if len(shape) == 3 else ph.THETA_STAR2), t)
    return (4.0 * w * (1.0 - w)).float(), t


def theta0(nd):
    return torch.tensor(THETA0_3 if nd == 3 else THETA0_2)


def pose0(nd):
    return torch.tensor(POSE0_3 if nd == 3 else POSE0_2)


def evaluate(mov, tgt, theta, rng, bins=32, alpha=1.0, normalized=False, dtype=torch.float64):
    """One evaluation for B pairs: (loss [B], dtheta [B,nd,nd+1], P [B,K,K]) as fp64 tensors; the warp, the weights and the sums in `dtype`."""
    from oracle import compose
    th = theta.detach().to(dtype).clone().requires_grad_()
    warped = compose.affine_warp(th, mov.to(dtype))
    loss = mi_ref.loss(tgt, warped, bins, alpha, normalized, rng, dtype)
    (g,) = torch.autograd.grad(loss.sum(), th)
    P = mi_ref.joint(tgt, warped.detach(), bins, rng, dtype)
    return loss.detach().double(), g.double(), P.double()


def loop(mov, tgt, rng, mode, optimizer, lr, iters, start, mi, dtype):
    """`iters` iterations for one pair: (losses [iters], final parameter) as numpy arrays.  mode 'affine': start = theta [nd,nd+1], the parameter;
    'rigid': start = the pose vector, theta = pose_to_theta(pose).  mi: dict(bins, alpha, normalized)."""
    from oracle import compose
    nd = mov.dim() - 2
    mov = mov.to(dtype)
    p = start.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        theta = compose.pose_to_theta(p) if mode == "rigid" else p.reshape(1, nd, nd + 1)
        e = mi_ref.loss(tgt, compose.affine_warp(theta, mov), rng=rng, dtype=dtype, **mi).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), p.detach().numpy().copy()


ITERS = 10
# id -> (shape, mode, optimiser, lr, normalized).  The rates are as high as the arbiter allows: at affine sgd 0.02, 2-D affine adam 0.005 or 2-D rigid
# sgd 0.03 it crosses interpolation kinks - its two precisions part by 1e-4 .. 7e-2 and the loss stops falling.  The SGD rows see the gradient's
# magnitude; Adam hides it.
LOOPS = {
    "affine-adam": ((12, 14, 16), "affine", "adam", 0.005, False),
    "affine-sgd": ((12, 14, 16), "affine", "sgd", 0.01, False),
    "rigid-adam": ((12, 14, 16), "rigid", "adam", 0.01, False),
    "rigid-sgd": ((12, 14, 16), "rigid", "sgd", 0.03, False),
    "rigid-normalized": ((12, 14, 16), "rigid", "adam", 0.005, True),
    "2d-affine": ((24, 28), "affine", "adam", 0.002, False),
    "2d-affine-sgd": ((24, 28), "affine", "sgd", 0.005, False),
    "2d-rigid": ((24, 28), "rigid", "adam", 0.005, False),
}


def start_of(shape, mode):
    return pose0(len(shape)) if mode == "rigid" else theta0(len(shape))


@functools.lru_cache(maxsize=None)
def loop_pair(name):
    """(r64, r32) of one LOOPS configuration - each (losses, final parameter) - computed once per process."""
    shape, mode, optimizer, lr, normalized = LOOPS[name]
    mov, tgt = pair(shape)
    rng = mi_ref.fit_range(tgt, mov)
    mi = dict(bins=32, alpha=1.0, normalized=normalized)
    return tuple(loop(mov, tgt, rng, mode, optimizer, lr, ITERS, start_of(shape, mode), mi, dt) for dt in (torch.float64, torch.float32))
