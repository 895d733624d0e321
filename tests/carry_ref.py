"""The loop of trx_affine_run restated for ONE pair on the CPU, and the observable that says which form of the loop ran.  Not a test.

`loop`: N iterations built only from oracle.c_affine_loss_grad (loss and dL/dtheta of one forward), oracle.c_theta_fwd and oracle.c_theta_vjp (rigid:
theta of the pose and the chain rule), in the dtype of its inputs - fp64 as the reference, fp32 as the second leg of the arbiter.  It shares nothing
with the kernels' epilogue (fin_load / fin_apply / fin_update of csrc/affine_finalize.h), which both forms of trx_affine_run run: a test that compares
the one-launch form with the two-launch form cannot see a mistake there, a test against this file can.
  affine: the 12 theta entries are the parameters;  rigid: the 6 pose entries, theta = Theta(pose)
  SGD:    p -= lr g
  Adam:   m = m + (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;  p -= lr / (1 - beta1^(t+1)) * m / (sqrt(v) / sqrt(1 - beta2^(t+1)) + eps)
          (torch.optim.Adam; t counts the iterations of every call so far)
  loss:   rounded to fp32 before the strict-< test of the best record (what the device stores and compares, and what error.item() of the reference
          gives);  best = the first strict minimum, with the theta of that forward.
tests/test_carry_ref_host.py pins the SGD legs on oracle.c_affine_loop and the Adam leg on torch.optim.Adam.

`fill_sentinel` / `carry_ran`: the carry buffers of the workspace (AffineSolver.carry_state) are written by launches of the carry form and by nothing
else.  Filled with a bit pattern that no arithmetic produces before run(n), they tell afterwards whether that call ran as one launch per iteration."""
import numpy as np
import torch

import oracle

SENTINEL = 0x7FA5C3D2   # a NaN with a payload: no kernel computes these bits, and isfinite() tells it from every value the record may hold
FIELDS = dict(theta=(0, 12), param=(12, 24), m=(24, 36), v=(36, 48))   # csrc/affine_finalize.h: kCarryTheta / Param / M / V; the step (int) at 48
STEP, RECORD = 48, 49                                                    # floats 49 .. 63 of a pair's 64 belong to nobody


def loop(mov, tgt, w, lr, iters, optimizer="sgd", theta0=None, pose0=None, betas=(0.9, 0.999), eps=1e-8, tables=None, state=None):
    """`iters` iterations on one pair (mov, tgt: ndarrays [*spatial] of one dtype, which is the dtype of everything).  From theta0 (affine) or pose0
    (rigid), or from `state`: the dict an earlier call returned (the optimiser's moments, t and the best record carry on).  Returns dict(losses [iters],
    thetas [iters]: theta of every forward, grads [iters]: dL/dparam of every forward, theta, param, m, v: the final state, t, best_idx, best_theta,
    best_loss, grad: the last gradient, mode)."""
    dt = mov.dtype
    nd = mov.ndim
    if state is not None:
        mode, p, m, v, t = state["mode"], state["param"].copy(), state["m"].copy(), state["v"].copy(), state["t"]
        best_loss, best_idx, best_theta = state["best_loss"], state["best_idx"], state["best_theta"]
    else:
        mode = "rigid" if pose0 is not None else "affine"
        p = np.array(pose0, dtype=dt).reshape(-1) if mode == "rigid" else np.array(np.eye(nd, nd + 1) if theta0 is None else theta0, dtype=dt).reshape(nd, nd + 1)
        m, v, t = np.zeros_like(p), np.zeros_like(p), 0
        best_loss, best_idx, best_theta = None, -1, None
    rigid = mode == "rigid"
    lr, b1, b2, eps = dt.type(lr), dt.type(betas[0]), dt.type(betas[1]), dt.type(eps)
    one = dt.type(1.0)
    losses, thetas, grads = [], [], []
    for _ in range(iters):
        th = oracle.c_theta_fwd(p) if rigid else p
        thetas.append(np.array(th, copy=True))
        total, _, dth, _ = oracle.c_affine_loss_grad(mov, tgt, th, w, tables)
        losses.append(dt.type(total))
        lossf = float(np.float32(total))
        if best_loss is None or lossf < best_loss:
            best_loss, best_idx, best_theta = lossf, t, thetas[-1]
        g = (oracle.c_theta_vjp(p, dth) if rigid else dth).astype(dt)
        grads.append(g)
        if optimizer == "adam":
            m = (m + (g - m) * (one - b1)).astype(dt)
            v = (b2 * v + (one - b2) * g * g).astype(dt)
            bc1, bc2 = one - b1 ** (t + 1), one - b2 ** (t + 1)
            p = (p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))).astype(dt)
        elif optimizer == "sgd":
            p = (p - lr * g).astype(dt)
        else:
            raise ValueError(optimizer)
        t += 1
    theta = np.array(oracle.c_theta_fwd(p) if rigid else p, copy=True)
    return dict(losses=np.asarray(losses), thetas=np.asarray(thetas), grads=np.asarray(grads), theta=theta, param=p, m=m, v=v, t=t, best_idx=best_idx,
                best_theta=best_theta, best_loss=best_loss, grad=grads[-1] if grads else None, mode=mode)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the observable
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bits(buf):
    return buf.view(torch.int32)


def _has_buffers(solver):
    import ctypes
    if solver.nd == 3:
        return True
    assert solver.lib.trx_affine_workspace_carry_offset(ctypes.byref(solver.vol)) == 0   # 2-D: the workspace has no carry buffers
    return False


def fill_sentinel(solver):
    """every float of the solver's two carry buffers = SENTINEL (call it in front of every run() whose form is asked about)"""
    if _has_buffers(solver):
        for buf in solver.carry_state():
            _bits(buf).fill_(SENTINEL)


def carry_ran(solver, start, n, not_finite=()):
    """Did the run(n) behind the last fill_sentinel(solver), which started at step `start`, run in the carry form?  False: the whole region still
    holds the sentinel (nothing of that call wrote a carry buffer).  True: it holds exactly what the loop of trx_affine_run leaves - launch k of n
    writes the buffer of parity (n - 1 - k) & 1, the first seeds its buffer with the caller's state (step `start`), launch k > 0 the state behind
    iteration k - 1 - asserted here:
      * n >= 2; the record of every pair in buffer 0 is at step start + n - 1, in buffer 1 at step start + n - 2;
      * theta, the parameters (12 affine, 6 pose entries) and, under Adam, both moments are finite in both buffers;
      * the fields this mode does not write (pose entries 6 .. 11, the moments under SGD) are the zeros of the seeding launch or still the sentinel;
      * floats 49 .. 63 of every pair keep the sentinel: nothing writes past the record.
    Anything else (one buffer written, a wrong step, a NaN state, a write past the record) fails the assertion.  not_finite: pairs whose state the
    test made NaN on purpose (a NaN image).  2-D: the workspace has no carry buffers (asserted), False.  Host sync."""
    from torchregister_amd import _lib
    if not _has_buffers(solver):
        return False
    torch.cuda.synchronize()
    bufs = [_bits(b).cpu() for b in solver.carry_state()]
    if all(bool((b == SENTINEL).all()) for b in bufs):
        return False
    assert n >= 2, f"a run of {n} iteration(s) wrote a carry buffer"
    adam, npar = solver.opt.kind == _lib.OPT_ADAM, 6 if solver.mode == "rigid" else 12
    for k, b in enumerate(bufs):
        assert b[:, STEP].tolist() == [start + n - 1 - k] * b.shape[0], (k, b[:, STEP].tolist(), start, n)
        assert bool((b[:, RECORD:] == SENTINEL).all()), f"buffer {k}: floats {RECORD} .. 63 of a record were written"
        f = b.view(torch.float32)
        written = [f[:, 0:12], f[:, 12:12 + npar]] + ([f[:, 24:24 + npar], f[:, 36:36 + npar]] if adam else [])
        keep = [p for p in range(b.shape[0]) if p not in not_finite]
        assert all(bool(torch.isfinite(x[keep]).all()) for x in written), (k, f[:, :STEP])
        idle = [b[:, 12 + npar:24]] + ([b[:, 24 + npar:36], b[:, 36 + npar:48]] if adam else [b[:, 24:48]])
        assert all(bool(((x == SENTINEL) | (x == 0)).all()) for x in idle), (k, f[:, :STEP])
    return True
