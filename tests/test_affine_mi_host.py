"""Host-side checks of the fused rigid / affine mutual-information loop (csrc/affine_mi.hip): the workspace query and the refusals of the two entry
points - every call here must be rejected before any HIP call, so it needs no GPU -, the dispatch of device_loop=True, and the conditions the
GPU tests (tests/test_gpu_affine_mi.py) rely on in their arbiter (tests/affine_mi_ref.py): for every loop configuration the fp64 loss falls in
every iteration and the fp32 and fp64 runs stay together."""
import ctypes

import numpy as np
import pytest
import torch

import affine_mi_ref as aref

OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5


def _vol(_lib, ndim=3, B=2, dhw=(12, 14, 16), ptr=True):
    v = _lib.Volumes()
    v.ndim, v.B, (v.D, v.H, v.W) = ndim, B, dhw
    v.moving = v.target = 4096 if ptr else None          # never dereferenced: every call below is refused first
    v.moving_stride = v.target_stride = dhw[0] * dhw[1] * dhw[2]
    return v


def _cfg(_lib, bins=32, alpha=1.0, rng=4096):
    c = _lib.MICfg()
    c.bins, c.alpha, c.normalized, c.range = bins, alpha, 0, rng
    return c


def test_workspace_query_is_host_arithmetic():
    from torchregister_amd import _lib
    lib = _lib.load()
    q = lambda v, k: lib.trx_affine_mi_workspace_bytes(ctypes.byref(v), k)  # noqa: E731
    assert q(_vol(_lib), 32) > 0 and q(_vol(_lib, ptr=False), 8) > 0 and q(_vol(_lib), 64) > 0
    assert q(_vol(_lib, 2, 3, (1, 13, 17)), 8) > 0
    assert q(_vol(_lib), 7) == 0 and q(_vol(_lib), 65) == 0
    assert q(_vol(_lib, ndim=4), 32) == 0 and q(_vol(_lib, 2, 1, (2, 13, 17)), 32) == 0
    assert q(_vol(_lib, B=0), 32) == 0 and q(_vol(_lib, B=65536), 32) == 0 and q(_vol(_lib, dhw=(2048, 1024, 1024)), 32) == 0
    assert lib.trx_affine_mi_workspace_bytes(None, 32) == 0
    # counts, G, one partial row of nd (nd + 1) floats per 16384 voxels, the loop's losses: each region rounded up to 256 bytes
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for ndim, B, dhw, K in ((3, 2, (12, 14, 16), 32), (3, 1, (40, 40, 40), 64), (2, 3, (1, 13, 17), 8)):
        rows = -(-dhw[0] * dhw[1] * dhw[2] // 16384)
        assert q(_vol(_lib, ndim, B, dhw), K) == up(B * K * K * 8) + up(B * K * K * 4) + up(B * rows * ndim * (ndim + 1) * 4) + up(B * 4)
    # the rows of a pair do not depend on the batch: the partial region grows linearly in B
    assert q(_vol(_lib, B=4, dhw=(64, 64, 64)), 32) - q(_vol(_lib, B=2, dhw=(64, 64, 64)), 32) == 2 * (32 * 32 * 12 + 16 * 12 * 4)


def test_entry_points_refuse_before_any_launch():
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    vol = _vol(_lib)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), 32)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731

    def grad(v=vol, c=_cfg(_lib), theta=4096, loss=4096, ws=4096, nbytes=n):
        return lib.trx_affine_mi_loss_grad(ref(v), ref(c), P(theta) if theta else None, P(loss) if loss else None, P(4096), P(ws) if ws else None, nbytes, None)

    assert grad(v=None) == ARG and grad(c=None) == ARG and grad(theta=None) == ARG and grad(loss=None) == ARG and grad(ws=None) == ARG
    assert grad(v=_vol(_lib, ptr=False)) == ARG and grad(c=_cfg(_lib, rng=None)) == ARG
    assert grad(c=_cfg(_lib, bins=7)) == ARG and grad(c=_cfg(_lib, bins=65)) == ARG
    assert grad(c=_cfg(_lib, alpha=float("nan"))) == ARG and grad(c=_cfg(_lib, alpha=float("inf"))) == ARG
    assert grad(v=_vol(_lib, B=0)) == ARG and grad(v=_vol(_lib, dhw=(0, 14, 16))) == ARG
    assert grad(v=_vol(_lib, ndim=4)) == NDIM and grad(v=_vol(_lib, ndim=2)) == NDIM
    assert grad(nbytes=n - 1) == WS and grad(nbytes=0) == WS

    opt = _lib.OptCfg(_lib.OPT_ADAM, 0.01, 0.9, 0.999, 1e-8)

    def state(**kw):
        st = _lib.AffineState()
        st.mode = _lib.PARAM_AFFINE
        for f in ("param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "losses", "step"):
            setattr(st, f, 4096)
        st.losses_capacity = 5
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def run(v=vol, c=_cfg(_lib), o=opt, st=state(), iters=1, ws=4096, nbytes=n):
        return lib.trx_affine_mi_run(ref(v), ref(c), ref(o), ref(st), iters, P(ws) if ws else None, nbytes, None)

    assert run(v=None) == ARG and run(c=None) == ARG and run(o=None) == ARG and run(st=None) == ARG and run(ws=None) == ARG and run(iters=-1) == ARG
    assert run(c=_cfg(_lib, rng=None)) == ARG and run(c=_cfg(_lib, bins=7)) == ARG and run(c=_cfg(_lib, bins=65)) == ARG
    assert run(c=_cfg(_lib, alpha=float("nan"))) == ARG
    assert run(v=_vol(_lib, ndim=4)) == NDIM and run(v=_vol(_lib, ndim=2)) == NDIM
    assert run(nbytes=n - 1) == WS
    assert run(iters=6) == CAP                                    # as trx_affine_run: more iterations than the loss curve holds
    assert run(st=state(param=None)) == ARG and run(st=state(step=None)) == ARG and run(st=state(best_idx=None)) == ARG
    assert run(st=state(adam_m=None)) == ARG and run(st=state(mode=2)) == ARG
    assert run(o=_lib.OptCfg(7, 0.01, 0.9, 0.999, 1e-8)) == ARG
    assert run(iters=0) == OK                                     # nothing to enqueue: no HIP call either


def test_device_loop_dispatch_raises_before_any_tensor():
    """device_loop=True takes exactly [MILoss] with a non-zero weight, rigid or affine: every other request raises ValueError while the images are
    still untouched (they are CPU tensors here, which the GPU path itself would refuse with another exception type)."""
    import torch.nn as nn
    import torchregister_amd as tr
    assert tr.AffineMISolver is tr._engine.AffineMISolver and tr.affine_mi_loss_grad is tr._engine.affine_mi_loss_grad
    import TorchRegister
    assert TorchRegister.AffineMISolver is tr.AffineMISolver and TorchRegister.affine_mi_loss_grad is tr.affine_mi_loss_grad
    bad = [([nn.MSELoss()], [1.0]), ([tr.MILoss(), tr.NCCLoss()], [1.0, 1.0]), ([tr.MILoss()], [0.0]), (None, None), ([tr.MILoss()], None)]
    m = t = torch.zeros(1, 1, 8, 8, 8)
    for crit, w in bad:
        for mode in ("rigid", "affine"):
            with pytest.raises(ValueError, match="device_loop"):
                tr.Register(mode, criterion=crit, weight=w, device_loop=True)
        for fn in (tr.affine_register, tr.rigid_register):
            with pytest.raises(ValueError, match="device_loop"):
                fn(m, t, criterions=crit, weights=w, grad_edges=False, device_loop=True)
    with pytest.raises(ValueError, match="device_loop"):
        tr.Register("flow", criterion=[tr.MILoss()], weight=[1.0], flow_model="direct", device_loop=True)
    reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True)
    assert reg.device_loop is True and tr.Register("rigid").device_loop is False
    assert tr.warpings.device_loop_settings([tr.MILoss(bins=16, alpha=2.0, normalized=True)], [0.5]) == dict(
        bins=16, alpha=1.0, normalized=True, target_range=None, moving_range=None)


@pytest.mark.parametrize("name", list(aref.LOOPS))
def test_arbiter_descends_and_its_precisions_stay_together(name):
    """What test_gpu_affine_mi.py's loop test relies on: the fp64 loss falls in every one of the 10 iterations, and the fp32 run stays within
    1e-5 (loss curve) and 2e-5 (final parameter) of it - so the loop bars are the floors 2e-5 |loss| and 2e-4, not the arbiter's own noise."""
    (l64, p64), (l32, p32) = aref.loop_pair(name)
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    print(f"{name}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, lgap {lgap:.1e}, pgap {pgap:.1e}")
    assert len(l64) == aref.ITERS and np.all(np.isfinite(l64)) and np.all(np.diff(l64) < 0), l64
    assert lgap <= 1e-5 and pgap <= 2e-5, (lgap, pgap)


def test_arbiter_single_evaluation_is_consistent():
    """The arbiter's dtheta against central differences of its own loss (fp64, h = 1e-6) at the 3-D start, and its table sums to one."""
    import mi_ref
    mov, tgt = aref.pair((12, 14, 16))
    rng = mi_ref.fit_range(tgt, mov)
    th = aref.theta0(3)[None]
    loss, g, P = aref.evaluate(mov, tgt, th, rng, 32, 1.0, False)
    assert abs(P.sum().item() - 1.0) < 1e-12 and loss.shape == (1,) and g.shape == (1, 3, 4)
    h = 1e-6
    for i, j in ((0, 0), (1, 3), (2, 1)):
        d = torch.zeros(1, 3, 4, dtype=torch.float64)
        d[0, i, j] = h
        fd = (aref.evaluate(mov, tgt, th.double() + d, rng)[0] - aref.evaluate(mov, tgt, th.double() - d, rng)[0]).item() / (2 * h)
        assert abs(fd - g[0, i, j].item()) <= 1e-5 * g.abs().max().item(), (i, j, fd, g[0, i, j].item())
