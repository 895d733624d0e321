"""The CPU arbiters that more than one test module uses: the objectives of the device-side loops composed from oracle/compose.py and the
restatements (tests/bspline_ref.py) under torch autograd + torch.optim, the local-NCC reference, the inputs they are fed, and the inputs
and references of the 2-D second-trip flow case of tests/launch_geometry.py.  Not a test."""
import numpy as np
import torch

import bspline_ref
import launch_geometry as lg
import phantoms as ph
from conftest import bar
from oracle import compose


def rand(shape, seed, lo=-1.0, hi=3.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


# ---------------------------------------------------------------------------------------------------------------------------------------
# dense flow + NCC (+ smoothness): the extensions of tests/test_gpu_flow.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def torch_flow_loop(mov, tgt, lr, iters, optimizer, smooth, dtype, flow0=None):
    """NCC (+ lambda / nd * sum_d mean(forward difference along d)^2) on the flow itself, SGD or Adam, from `flow0` (zeros if None)."""
    nd = mov.dim() - 2
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    fl = (torch.zeros(1, nd, *mov.shape[2:], dtype=dtype) if flow0 is None else flow0.to(dtype).clone()).requires_grad_()
    opt = torch.optim.SGD([fl], lr) if optimizer == "sgd" else torch.optim.Adam([fl], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = compose.ncc_loss(tgt, compose.flow_warp(mov, fl))
        if smooth:
            reg = 0.0
            for d in range(nd):
                df = fl.diff(dim=2 + d)
                reg = reg + (df * df).mean()
            e = e + smooth * reg / nd
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), fl.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# local NCC: tests/test_gpu_lncc.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def lncc_ref(tgt, wrp, window, alpha, dtype):
    """(loss [B], dloss/dwarped) of oracle/compose.py::local_ncc_loss, per pair: the kernel returns one loss per pair."""
    y = tgt.to(dtype)
    w = wrp.to(dtype).clone().requires_grad_()
    losses, grads = [], []
    for b in range(y.shape[0]):
        l = compose.local_ncc_loss(y[b:b + 1], w[b:b + 1], window, alpha)
        (g,) = torch.autograd.grad(l, w)
        losses.append(l.item())
        grads.append(g[b:b + 1].numpy())
    return np.asarray(losses), np.concatenate(grads)


def lncc_pair(shape, B=1):
    nd = len(shape)
    tgt = torch.cat([ph.blobs(shape, 300 + b) + 0.05 * ph.vol(shape, 0.37 + 0.01 * b, "sin") for b in range(B)])
    if nd == 3:
        wrp = torch.cat([compose.affine_warp(torch.tensor(ph.THETA_STAR3)[None], tgt[b:b + 1]) for b in range(B)])
    else:
        wrp = torch.cat([compose.affine_warp(torch.tensor(ph.THETA_STAR2)[None], tgt[b:b + 1]) for b in range(B)])
    return tgt, wrp + 0.02 * ph.vol(tuple(wrp.shape[2:]), 0.23, "cos")


def torch_lncc_flow_loop(mov, tgt, lr, iters, optimizer, smooth, window, flow0, dtype):
    """local_ncc_loss of flow_warp (+ smooth_regulariser) under torch autograd + torch.optim"""
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    fl = flow0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([fl], lr) if optimizer == "sgd" else torch.optim.Adam([fl], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = compose.local_ncc_loss(tgt, compose.flow_warp(mov, fl), window=window)
        if smooth:
            e = e + compose.smooth_regulariser(fl, smooth)
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), fl.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# B-spline loop: tests/test_gpu_bspline.py
# ---------------------------------------------------------------------------------------------------------------------------------------
def loop_pair(shape, seed=0, B=1):
    """Targets and movings of the loop tests: two different blob phantoms plus a ripple."""
    tgt = torch.cat([ph.blobs(shape, 61 + 10 * b + seed) + 0.05 * ph.vol(shape, 0.031, "sin") for b in range(B)])
    mov = torch.cat([ph.blobs(shape, 62 + 10 * b + seed) + 0.05 * ph.vol(shape, 0.027, "cos") for b in range(B)])
    return mov, tgt


def bspline_ctrl0(B, shape, spacing, seed, amp=0.4):
    return rand((B, len(shape)) + bspline_ref.grid(shape, spacing), seed, -amp, amp)


def bspline_arbiter(mov, tgt, spacing, ctrl0, lr, iters, optimizer, dtype, base=None, **loss_kw):
    """tests/bspline_ref.py::expand -> oracle/compose.py flow_warp -> weighted_loss under torch autograd + torch.optim, on the CPU."""
    sp = tuple(mov.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    c = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([c], lr) if optimizer == "sgd" else torch.optim.Adam([c], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        e = compose.weighted_loss(tgt, compose.flow_warp(mov, bspline_ref.expand(c, sp, spacing, base=base, dtype=dtype)), **loss_kw)
        e.backward()
        opt.step()
        losses.append(e.item())
    return np.asarray(losses), c.detach().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# The 2-D second-trip flow case (launch_geometry.FLOW2_CASES["big"]).
#
# What a check at a million voxels can see is set by its inputs.  The derivative of a bilinear sample jumps where x + flow crosses a
# lattice line, and at coordinates of ~1000 a position is rounded to 6e-5 voxels in fp32: with a flow that passes through integers, a few
# dozen of a million samples take the other one-sided derivative in fp32 than in fp64, the arbiter's own fp32-vs-fp64 gap becomes the size
# of the gradient itself and the bar (twice that gap) lets every gradient pass.  Adam adds its own form of it: it normalises the step, so
# where a gradient is ~0 its sign, and with it a step of lr, differs between any two precisions.  So here
#   * the flows stay off the lattice: every component is 0.5 +- 0.2 at most, through the whole run (asserted), so no sample has a kink
#     within reach and the gap stays at fp32 rounding;
#   * the images carry a smooth ripple that reaches the last rows, so that the voxels of the second trip (the last 4099 of the image) have
#     gradients as large as the rest, and the target a band along its last rows, so that the loss depends on their moments;
#   * the runs against the arbiter are SGD, with lr = 500 so that the second-trip voxels move by up to 0.15 voxel (the NCC gradient is ~1e-5
#     per voxel at a million voxels), and the start flow carries a fine ripple so that the smoothness term moves it by more than the bar.
# flow2_big_check_teeth asserts the resulting bar-to-signal ratios; it runs on the CPU (tests/test_launch_geometry_host.py).
# ---------------------------------------------------------------------------------------------------------------------------------------
FLOW2_TAIL = lg.FLOW_2D_BLOCKS * lg.TRX_BLOCK        # first voxel of the second trip at B = 1
FLOW2_RUNS = {"sgd": dict(optimizer="sgd", lr=500.0, smooth=0.0, iters=4), "sgd-smooth": dict(optimizer="sgd", lr=500.0, smooth=500.0, iters=4)}
_FLOW2 = {}


def _yx(shape):
    return torch.arange(shape[0], dtype=torch.float64)[:, None], torch.arange(shape[1], dtype=torch.float64)[None, :]


def flow2_big_flow(amp, fine=0.0):
    """fp32 [1, 2, H, W] in 0.5 +- (amp + fine): two slow sinusoids per channel, plus a fine ripple of amplitude `fine`."""
    shape = lg.FLOW2_CASES["big"]["shape"]
    y, x = _yx(shape)
    rip = fine * torch.sin(1.3 * y + 0.2) * torch.cos(1.1 * x)
    f0 = 0.5 + amp * (torch.sin(0.021 * y + 0.4) + torch.cos(0.017 * x)) / 2 + rip
    f1 = 0.5 + amp * (torch.cos(0.011 * y) + torch.sin(0.023 * x + 0.4)) / 2 - rip
    return torch.stack([f0, f1]).float()[None]


def flow2_big():
    """dict(shape, mov, tgt, fl; ncc32, ncc64, mse32, mse64 = oracle.c_flow_loss_grad results at fl), computed once."""
    import oracle
    if "mov" not in _FLOW2:
        shape = lg.FLOW2_CASES["big"]["shape"]
        y, x = _yx(shape)
        img = lambda seed, py, px: (ph.blobs(shape, seed).double()[0, 0] + 0.3 * torch.sin(0.043 * y + py) * torch.cos(0.051 * x + px)).float()[None, None]   # noqa: E731
        mov, tgt, fl = img(62, 0.3, 0.0), img(61, 0.55, 0.3), flow2_big_flow(0.2)
        # a band along the last rows of the target alone: the five moments of the second trip's voxels weigh in the loss
        tgt = (tgt.double() + 0.5 * torch.exp(-((shape[0] - 1 - y) / 3.0) ** 2) * torch.cos(0.08 * x + 0.2)).float()
        _FLOW2.update(shape=shape, mov=mov, tgt=tgt, fl=fl)
        for dt, tag in ((np.float32, "32"), (np.float64, "64")):
            m, t, f = mov[0, 0].numpy().astype(dt), tgt[0, 0].numpy().astype(dt), fl[0].numpy().astype(dt)
            _FLOW2["ncc" + tag] = oracle.c_flow_loss_grad(m, t, f, oracle.wts(w_ncc=1.0))
            _FLOW2["mse" + tag] = oracle.c_flow_loss_grad(m, t, f, oracle.wts(w_mse=1.0))
    return _FLOW2


def tail(a):
    """[..., H, W] -> the second-trip voxels [..., H W - FLOW2_TAIL]"""
    return np.asarray(a).reshape(a.shape[:-2] + (-1,))[..., FLOW2_TAIL:]


def flow2_big_gradient_bars(lname):
    """(d64, bar over the image, bar over the second-trip voxels) of the gradient of `lname` (ncc / mse): each bar from its own voxels."""
    c = flow2_big()
    d32, d64 = c[lname + "32"][2], c[lname + "64"][2]
    return d64, bar(d32, d64, 1e-4 * np.max(np.abs(d64))), bar(tail(d32), tail(d64), 1e-4 * np.max(np.abs(tail(d64))))


def flow2_big_run(variant):
    """dict(f0, l32, l64, f32, f64) of a FLOW2_RUNS variant under torch_flow_loop, computed once."""
    key = "run-" + variant
    if key not in _FLOW2:
        c, v = flow2_big(), FLOW2_RUNS[variant]
        f0 = flow2_big_flow(0.05, fine=0.03)
        l32, f32 = torch_flow_loop(c["mov"], c["tgt"], v["lr"], v["iters"], v["optimizer"], v["smooth"], torch.float32, f0)
        l64, f64 = torch_flow_loop(c["mov"], c["tgt"], v["lr"], v["iters"], v["optimizer"], v["smooth"], torch.float64, f0)
        _FLOW2[key] = dict(f0=f0, l32=l32, l64=l64, f32=f32, f64=f64)
    return _FLOW2[key]


def flow2_big_check_teeth():
    """The bars of the 2-D second-trip tests against the signal of the second-trip voxels (see above); returns the figures as text lines."""
    out = []
    for lname in ("ncc", "mse"):
        d64, b_all, b_tail = flow2_big_gradient_bars(lname)
        m_all, m_tail = np.max(np.abs(d64)), np.max(np.abs(tail(d64)))
        out.append(f"flow2 big {lname} gradient: max {m_all:.3e} bar {b_all:.3e}; second trip: max {m_tail:.3e} bar {b_tail:.3e} (bar / signal {b_tail / m_tail:.1e})")
        assert b_all <= 1e-3 * m_all and b_tail <= 1e-3 * m_tail and m_tail >= 0.3 * m_all, out[-1]
    # a moments pass that skipped the second trip: the five sums without those voxels, n of the whole image (flow_coef_kernel's form of the NCC)
    c = flow2_big()
    yv, wv = c["tgt"][0, 0].numpy().astype(np.float64).reshape(-1), c["ncc64"][3].reshape(-1)

    def ncc(yv, wv, n=yv.size):
        Sy, Sw = yv.sum(), wv.sum()
        Saa, Sbb, Sab = (yv * yv).sum() - Sy * Sy / n, (wv * wv).sum() - Sw * Sw / n, (yv * wv).sum() - Sy * Sw / n
        return 100.0 * (1.0 - Sab / np.sqrt(Saa * Sbb + 1e-10))
    t64, cut = c["ncc64"][0], ncc(yv[:FLOW2_TAIL], wv[:FLOW2_TAIL])
    assert abs(ncc(yv, wv) - t64) <= 1e-9 * abs(t64)
    out.append(f"flow2 big ncc loss {t64:.6f}; without the second trip's voxels {cut:.6f}: off by {abs(cut - t64):.3e}, bar {2e-5 * max(1.0, abs(t64)):.3e}")
    assert abs(cut - t64) >= 20 * 2e-5 * max(1.0, abs(t64)), out[-1]
    fl = c["fl"].numpy()
    assert np.min(fl - np.floor(fl)) >= 0.25 and np.max(fl - np.floor(fl)) <= 0.75
    runs = {k: flow2_big_run(k) for k in FLOW2_RUNS}
    for k, r in runs.items():
        b = bar(r["f32"], r["f64"], 2e-4)
        move = np.abs(tail(r["f64"]) - tail(r["f0"].numpy()))
        frac = r["f64"] - np.floor(r["f64"])
        out.append(f"flow2 big run {k}: flow bar {b:.3e}; second trip moves by up to {move.max():.3e}, median {np.median(move):.3e} (bar / largest move {b / move.max():.1e}); "
                   f"fractional parts in [{frac.min():.3f}, {frac.max():.3f}]")
        assert b <= 2e-2 * move.max() and np.median(move) >= 2.0 * b and frac.min() >= 0.2 and frac.max() <= 0.8, out[-1]
    d = np.abs(tail(runs["sgd-smooth"]["f64"]) - tail(runs["sgd"]["f64"])).max()
    b = bar(runs["sgd-smooth"]["f32"], runs["sgd-smooth"]["f64"], 2e-4)
    out.append(f"flow2 big: the smoothness term moves the second-trip voxels by up to {d:.3e} (bar / that {b / d:.1e})")
    assert b <= 0.1 * d, out[-1]
    return out
