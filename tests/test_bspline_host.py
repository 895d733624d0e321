"""CPU-only checks of the cubic B-spline free-form deformation: the grid rule, the restatement's own properties (tests/bspline_ref.py, fp64),
the argument checks of every trx_bspline_* entry point before any HIP call, and the validation of Register / flow_register."""
import ctypes

import pytest
import torch
import torch.nn as nn

import bspline_ref as ref

GRID_RULE = [(17, 4, 8), (16, 4, 7), (5, 8, 4), (1, 3, 4), (9, 1, 12)]   # (S, spacing, G)


@pytest.mark.parametrize("S,d,G", GRID_RULE)
def test_grid_rule(S, d, G):
    """G = (S - 1) // d + 4 from the C ABI, the Python wrapper and the restatement, on every axis of a 3-D and a 2-D geometry."""
    import torchregister_amd as tr
    from torchregister_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 3)(-1, -1, -1)
    assert lib.trx_bspline_grid(3, S, 7, 9, d, 2, 3, out) == 0 and tuple(out) == (G, 7, 6)
    assert lib.trx_bspline_grid(3, 7, S, 9, 2, d, 3, out) == 0 and tuple(out) == (7, G, 6)
    assert lib.trx_bspline_grid(3, 7, 9, S, 2, 3, d, out) == 0 and tuple(out) == (7, 6, G)
    assert lib.trx_bspline_grid(2, 1, 9, S, 0, 3, d, out) == 0 and tuple(out) == (1, 6, G)          # 2-D: sz is ignored, Gz = 1
    assert tr.bspline_grid((S, 7, 9), (d, 2, 3)) == (G, 7, 6) == ref.grid((S, 7, 9), (d, 2, 3))
    assert tr.bspline_grid((S, S, S), d) == (G, G, G)
    assert tr.bspline_grid((9, S), (3, d)) == (6, G)


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 2 - 1


CASES = [((13, 18, 23), (4, 5, 3)), ((17, 17, 17), 4), ((5, 6, 7), 8), ((9, 10, 11), 1), ((1, 12, 20), (3, 3, 4)), ((19, 26), (4, 6))]


@pytest.mark.parametrize("spatial,spacing", CASES)
def test_restatement_partition_of_unity(spatial, spacing):
    nd = len(spatial)
    ctrl = torch.full((2, nd) + ref.grid(spatial, spacing), 0.7321, dtype=torch.float64)
    assert (ref.expand(ctrl, spatial, spacing) - 0.7321).abs().max().item() <= 1e-14


@pytest.mark.parametrize("spatial,spacing", CASES)
def test_restatement_reproduces_linear_functions(spatial, spacing):
    """ctrl_i = a . (i - 1) d + b on the lattice gives flow(x) = a . x + b on the voxels."""
    nd = len(spatial)
    sp = ref.per_axis(spacing, nd)
    a, b = [0.31, -0.17, 0.23][:nd], 0.4
    pts = torch.meshgrid(*[(torch.arange(g, dtype=torch.float64) - 1) * d for g, d in zip(ref.grid(spatial, sp), sp)], indexing="ij")
    vox = torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in spatial], indexing="ij")
    ctrl = (sum(a[i] * pts[i] for i in range(nd)) + b)[None, None].expand(1, nd, *pts[0].shape)
    want = sum(a[i] * vox[i] for i in range(nd)) + b
    assert (ref.expand(ctrl, spatial, spacing)[0] - want).abs().max().item() <= 1e-12


@pytest.mark.parametrize("spatial,spacing", CASES)
def test_restatement_reduce_is_the_adjoint(spatial, spacing):
    nd = len(spatial)
    c, g = _rand((2, nd) + ref.grid(spatial, spacing), 1), _rand((2, nd) + tuple(spatial), 2)
    lhs, rhs = (ref.expand(c, spatial, spacing) * g).sum().item(), (c * ref.reduce(g, spacing)).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    base = _rand((2, nd) + tuple(spatial), 3)
    assert torch.equal(ref.expand(torch.zeros_like(c), spatial, spacing, base), base)


P = ctypes.c_void_p


def test_operator_argument_checks_without_gpu():
    """trx_bspline_grid / _workspace_bytes / _expand / _reduce return their status before any HIP call."""
    from torchregister_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 3)()
    ok = (3, 2, 16, 16, 16, 4, 4, 4)                              # ndim, B, D, H, W, sz, sy, sx
    n = lib.trx_bspline_workspace_bytes(*ok)
    assert n >= 2 * 3 * (16 * 16 * 7 + 16 * 7 * 7) * 4                # the two intermediates of six volumes
    assert lib.trx_bspline_workspace_bytes(2, 1, 1, 16, 16, 0, 4, 4) > 0                           # 2-D: sz is ignored
    assert lib.trx_bspline_grid(3, 16, 16, 16, 4, 4, 4, None) == -1
    for bad, code in (((4, 2, 16, 16, 16, 4, 4, 4), -2), ((1, 2, 16, 16, 16, 4, 4, 4), -2),       # ndim
                      ((2, 2, 3, 16, 16, 4, 4, 4), -2),                                              # D != 1 with ndim 2
                      ((3, 0, 16, 16, 16, 4, 4, 4), -1), ((3, 2, 0, 16, 16, 4, 4, 4), -1), ((3, 2, 16, -1, 16, 4, 4, 4), -1),
                      ((3, 2, 16, 16, 16, 0, 4, 4), -1), ((3, 2, 16, 16, 16, 4, 0, 4), -1), ((3, 2, 16, 16, 16, 4, 4, 0), -1),   # spacing 0
                      ((2, 2, 1, 16, 16, 1, 4, -2), -1), ((3, 2, 16, 16, 16, 4, 4, 1025), -1),
                      ((3, 1, 2048, 1024, 1024, 8, 8, 8), -1)):                                      # 2^31 voxels
        assert lib.trx_bspline_workspace_bytes(*bad) == 0, bad
        assert lib.trx_bspline_grid(bad[0], *bad[2:], out) == (code if bad[1] > 0 else 0), bad      # (the grid takes no batch size)
        assert lib.trx_bspline_expand(P(16), None, P(16), *bad, P(16), 1 << 40, None) == code, bad
        assert lib.trx_bspline_reduce(P(16), P(16), *bad, P(16), 1 << 40, None) == code, bad
    assert lib.trx_bspline_expand(None, None, P(16), *ok, P(16), n, None) == -1                    # null ctrl
    assert lib.trx_bspline_expand(P(16), None, None, *ok, P(16), n, None) == -1                    # null flow
    assert lib.trx_bspline_expand(P(16), None, P(16), *ok, None, n, None) == -1                    # null workspace
    assert lib.trx_bspline_reduce(None, P(16), *ok, P(16), n, None) == -1                          # null dflow
    assert lib.trx_bspline_reduce(P(16), None, *ok, P(16), n, None) == -1                          # null dctrl
    assert lib.trx_bspline_reduce(P(16), P(16), *ok, None, n, None) == -1                          # null workspace
    assert lib.trx_bspline_expand(P(16), None, P(16), *ok, P(16), n - 1, None) == -3               # workspace one byte short
    assert lib.trx_bspline_expand(P(16), P(16), P(16), *ok, P(16), n - 1, None) == -3
    assert lib.trx_bspline_reduce(P(16), P(16), *ok, P(16), n - 1, None) == -3


def _loop_args(B=2, D=16, H=16, W=16, ndim=3, adam=False, capacity=8):
    from torchregister_amd import _lib
    vol = _lib.Volumes()
    vol.moving, vol.target, vol.moving_stride, vol.target_stride = 16, 16, D * H * W, D * H * W
    vol.ndim, vol.B, vol.D, vol.H, vol.W = ndim, B, D, H, W
    st = _lib.BSplineState()
    st.ctrl, st.flow, st.dflow, st.losses, st.step, st.losses_capacity = 16, 16, 16, 16, 16, capacity
    if adam:
        st.adam_m, st.adam_v = 16, 16
    return vol, _lib.LossCfg(1.0, 0.0, 100.0, 0.0, 3.0), _lib.OptCfg(_lib.OPT_ADAM if adam else _lib.OPT_SGD, 0.1, 0.9, 0.999, 1e-8), st


def test_loop_argument_checks_without_gpu():
    """trx_bspline_run / trx_bspline_step return their status before any HIP call."""
    from torchregister_amd import _lib
    lib = _lib.load()
    sp = (ctypes.c_int * 3)(4, 4, 4)
    n = lib.trx_bspline_workspace_bytes(3, 2, 16, 16, 16, 4, 4, 4)
    by = ctypes.byref

    def run(vol, loss, opt, st, spacing=sp, iters=3, ws=P(16), nbytes=n):
        a = [by(x) if x is not None else None for x in (vol, loss, opt, st)]
        rc = lib.trx_bspline_run(*a, spacing, iters, ws, nbytes, None)
        if iters == 1:
            assert lib.trx_bspline_step(*a, spacing, ws, nbytes, None) == rc
        return rc

    vol, loss, opt, st = _loop_args()
    assert run(None, loss, opt, st) == -1 and run(vol, None, opt, st) == -1 and run(vol, loss, None, st) == -1 and run(vol, loss, opt, None) == -1
    assert run(vol, loss, opt, st, spacing=None) == -1 and run(vol, loss, opt, st, ws=None) == -1
    for field in ("ctrl", "flow", "dflow", "step"):
        v2, l2, o2, s2 = _loop_args()
        setattr(s2, field, None)
        assert run(v2, l2, o2, s2) == -1, field
    for field in ("moving", "target"):
        v2, l2, o2, s2 = _loop_args()
        setattr(v2, field, None)
        assert run(v2, l2, o2, s2) == -1, field
    v2, l2, o2, s2 = _loop_args(adam=True)
    s2.adam_m = None
    assert run(v2, l2, o2, s2) == -1                                                               # Adam without its moments
    o2.kind = 7
    assert run(v2, l2, o2, s2) == -1                                                               # unknown optimiser
    v2, l2, o2, s2 = _loop_args(ndim=4)
    assert run(v2, l2, o2, s2) == -2
    v2, l2, o2, s2 = _loop_args(ndim=2, D=3)
    assert run(v2, l2, o2, s2) == -2                                                               # D != 1 in 2-D
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert run(vol, loss, opt, st, spacing=(ctypes.c_int * 3)(*bad)) == -1, bad                # spacing 0
    v2, l2, o2, s2 = _loop_args(ndim=2, D=1)
    assert run(v2, l2, o2, s2, spacing=(ctypes.c_int * 3)(0, 4, 4), iters=-1, nbytes=1 << 40) == -1     # sz ignored in 2-D; iters < 0
    assert run(v2, l2, o2, s2, spacing=(ctypes.c_int * 3)(0, 4, 4), nbytes=lib.trx_bspline_workspace_bytes(2, 2, 1, 16, 16, 0, 4, 4) - 1) == -3
    v2, l2, o2, s2 = _loop_args(B=1, D=2048, H=1024, W=1024)
    assert run(v2, l2, o2, s2, nbytes=1 << 40) == -1                                               # 2^31 voxels
    assert run(vol, loss, opt, st, nbytes=n - 1) == -3                                             # workspace one byte short
    assert run(vol, loss, opt, st, iters=1, nbytes=n - 1) == -3
    assert run(vol, loss, opt, st, iters=9) == -5                                                  # iters beyond losses_capacity
    assert run(vol, loss, opt, st, iters=0) == 0                                                   # nothing to enqueue


def test_register_and_flow_register_validation_before_the_gpu():
    """Bad B-spline settings are refused before any tensor reaches the GPU (CPU tensors would otherwise raise 'no CPU fallback')."""
    import torchregister_amd as tr
    fused = dict(criterion=[tr.NCCLoss()], weight=[1.0])
    with pytest.raises(ValueError, match="spacing"):
        tr.Register("flow", flow_model="direct", spacing=6, **fused)
    with pytest.raises(ValueError, match="spacing"):
        tr.Register("flow", spacing=6, **fused)                    # flow_model='unet'
    with pytest.raises(ValueError, match="spacing"):
        tr.Register("affine", spacing=6)
    for bad in (0, -3, (4, 0, 4), 2.5, True):
        with pytest.raises(ValueError, match="spacing"):
            tr.Register("flow", flow_model="bspline", spacing=bad, **fused)
    with pytest.raises(ValueError, match="smooth_weight"):
        tr.Register("flow", flow_model="bspline", spacing=6, smooth_weight=0.5, **fused)
    with pytest.raises(ValueError, match="direct"):
        tr.Register("flow", flow_model="unet", levels=2)           # unchanged: the U-Net is tied to one image size
    tr.Register("flow", flow_model="bspline", spacing=6, levels=2, **fused)          # levels > 1 is accepted
    tr.Register("flow", flow_model="bspline", levels=2, **fused)                     # spacing defaults to 8

    shape = (16, 20, 24)
    with pytest.raises(ValueError, match="spacing"):
        tr.flow_register(shape, criterions=[nn.MSELoss()], weights=[1.0], flow_model="direct", spacing=4)
    with pytest.raises(ValueError, match="spacing"):
        tr.flow_register(shape, criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=0)
    with pytest.raises(ValueError, match="spacing"):
        tr.flow_register(shape, criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=(4, 4))     # one per axis
    with pytest.raises(ValueError, match="smooth_weight"):
        tr.flow_register(shape, criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=4, smooth_weight=1.0)
    for crit in ([nn.L1Loss()], [nn.MSELoss(), tr.LocalNCCLoss()], [tr.NMILoss()]):
        with pytest.raises(ValueError, match="MSELoss.*NCCLoss.*SSDLoss"):
            tr.flow_register(shape, criterions=crit, weights=[1.0, 1.0], flow_model="bspline", spacing=4)
    with pytest.raises(ValueError, match="MSELoss.*NCCLoss.*SSDLoss"):
        tr.flow_register(shape, flow_model="bspline")              # the default list carries the NMI loss
    fr = tr.flow_register(shape, criterions=[nn.MSELoss(), tr.NCCLoss(), tr.SSDLoss()], weights=[1.0, 0.5, 0.1], flow_model="bspline", spacing=(4, 5, 6))
    assert fr.spacing == (4, 5, 6) and tr.flow_register(shape, criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline").spacing == (8, 8, 8)

    mov, tgt = torch.rand(1, 1, 32, 32, 32), torch.rand(1, 1, 32, 32, 32)
    with pytest.raises(ValueError, match="MSELoss.*NCCLoss.*SSDLoss"):
        tr.Register("flow", criterion=[nn.L1Loss()], weight=[1.0], flow_model="bspline", spacing=6).optim(mov, tgt, max_epochs=3)
    with pytest.raises(ValueError, match="spacing"):
        tr.Register("flow", flow_model="bspline", spacing=(4, 4), **fused).optim(mov, tgt, max_epochs=3)      # two spacings, three axes
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.Register("flow", flow_model="bspline", spacing=6, levels=2, **fused).optim(mov, tgt, max_epochs=[3, 3])   # a valid schedule reaches the GPU check
