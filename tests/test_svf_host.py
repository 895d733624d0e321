"""CPU-only checks of the stationary-velocity-field model: the restatement's own properties (tests/svf_ref.py: its sampler against
oracle/compose.py::flow_warp, the explicit adjoint against torch autograd, K = 0, the sign, the fold test), the conditions on the inputs the
GPU tests use, the status codes of the five entry points, and the validation of the Python keywords - all before any GPU is touched."""
import ctypes

import pytest
import torch
import torch.nn as nn

import svf_ref as ref
from oracle import compose

P = ctypes.c_void_p


@pytest.mark.parametrize("B,spatial", [(2, (7, 9, 11)), (1, (2, 5, 3)), (2, (12, 15)), (1, (2, 2))])
def test_exp_is_repeated_squaring_with_the_reference_warp(B, spatial):
    """One squaring of the restatement = u + compose.flow_warp(u, u) (grid_sample, align_corners=True, zeros) on shapes whose axes are all >= 2,
    and exp = K of them from u_0 = 2^-K v (fp64, 1e-12).  A third of the positions leave the volume."""
    v = ref.smooth_field(B, spatial, 4.0, 3).double()
    u = v / 8
    for _ in range(3):
        a, b = u + ref.sample(u, u), u + compose.flow_warp(u, u)
        assert (a - b).abs().max().item() <= 1e-12
        u = a
    assert torch.equal(u, ref.exp(v, 3))
    assert ref.share_outside(u) > 0.15


@pytest.mark.parametrize("B,spatial,K,amp", [(2, (7, 9, 11), 3, 4.0), (1, (12, 15), 4, 5.0), (1, (1, 8, 9), 2, 2.0)])
@pytest.mark.parametrize("inverse", [False, True])
def test_the_explicit_adjoint_equals_autograd(B, spatial, K, amp, inverse):
    """exp_backward (g + splat + position derivative over the in-bounds corners, level by level) against autograd through exp: fp64, 1e-12
    relative, with about a third of the voxels leaving the volume."""
    v, g = ref.smooth_field(B, spatial, amp, 11).double(), ref.smooth_field(B, spatial, 1.0, 12, noise=0.5).double()
    if min(spatial) > 1:
        assert ref.share_outside(ref.exp(v, K, inverse)) > 0.2
    a, b = ref.exp_backward(v, g, K, inverse), ref.exp_backward_autograd(v, g, K, inverse)
    assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()


def test_zero_squarings_is_the_identity_and_inverse_negates():
    v, g = ref.smooth_field(1, (5, 6, 7), 1.0, 1), ref.smooth_field(1, (5, 6, 7), 1.0, 2)
    assert torch.equal(ref.exp(v, 0, dtype=torch.float32), v) and torch.equal(ref.exp(v, 0, inverse=True, dtype=torch.float32), -v)
    assert torch.equal(ref.exp_backward(v, g, 0, dtype=torch.float32), g) and torch.equal(ref.exp_backward(v, g, 0, True, dtype=torch.float32), -g)
    assert torch.equal(ref.exp(v, 3, inverse=True), ref.exp(-v, 3))


@pytest.mark.parametrize("spatial,det_plain,det_exp", [((32, 40), -0.38, 0.284), ((16, 18, 20), -0.30, 0.304)])
def test_exp_unfolds_what_the_displacement_folds(spatial, det_plain, det_exp):
    """The closed-form field of the fold test: id + v has a negative determinant, id + exp(v) with 6 squarings a positive one (fp64)."""
    v = ref.fold_field(spatial)
    assert abs(ref.jacobian_det(v).min().item() - det_plain) < 0.005
    assert abs(ref.jacobian_det(ref.exp(v, 6)).min().item() - det_exp) < 5e-4
    lin = torch.stack([0.1 * ref.identity(spatial)[0, a] * (a + 1) for a in range(len(spatial))])[None]     # flow_a = 0.1 (a + 1) x_a
    want = 1.0
    for a in range(len(spatial)):
        want *= 1 + 0.1 * (a + 1)
    assert (ref.jacobian_det(lin) - want).abs().max().item() < 1e-12


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("case", range(len(ref.CASES)))
def test_the_gpu_tests_inputs_meet_their_conditions(case, inverse):
    """At the seeds of SEEDS the adjoint in fp32 and in fp64 agree at EVERY element to 1e-5 max|dvel| (so an element the GPU leaves beyond the
    bar is the GPU's), exp agrees to 1e-5 max|flow|, the cases meant to leave the volume do, and the first 32 candidate directions hold
    eight for which the restatement itself meets the directional identity to 1e-6."""
    B, spatial, K, amp = ref.CASES[case]
    v, g = ref.case_inputs(case, inverse)
    assert v.dtype == torch.float32 and v.shape == (B, len(spatial)) + spatial
    f64, f32 = ref.exp(v, K, inverse), ref.exp(v, K, inverse, dtype=torch.float32)
    assert (f32.double() - f64).abs().max().item() <= 1e-5 * f64.abs().max().item()
    b64, b32 = ref.exp_backward(v, g, K, inverse), ref.exp_backward(v, g, K, inverse, dtype=torch.float32)
    assert int(((b32.double() - b64).abs() > 1e-5 * b64.abs().max()).sum()) == 0
    if case in ref.MIN_OUTSIDE:
        assert ref.share_outside(f64) >= ref.MIN_OUTSIDE[case]
    dirs = ref.directions(case, inverse)          # eight directions whose difference quotient holds no kink of exp
    assert len(dirs) == 8 and all(abs(rhs) > 0 for _, rhs in dirs)


def test_operator_argument_checks_without_gpu():
    """trx_svf_workspace_bytes / trx_svf_exp / trx_svf_exp_backward return their status before any HIP call: null pointers -1, ndim -2,
    squarings outside 0 .. 12 -1, more than 2^31 voxels -1, a workspace one byte short -3."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ok = (3, 2, 16, 16, 16, 4)                     # ndim, B, D, H, W, squarings
    n = lib.trx_svf_workspace_bytes(*ok)
    field = 2 * 3 * 16 ** 3 * 4
    assert n >= 4 * field + 2 * field + 2 * field          # levels, two gradients, the int64 accumulator
    assert lib.trx_svf_workspace_bytes(3, 2, 16, 16, 16, 0) > 0
    assert lib.trx_svf_workspace_bytes(3, 1, 256, 256, 256, 6) == 6 * 201326592 + 2 * 201326592 + 402653184 + 256

    def fwd(vel=P(16), flow=P(16), geom=ok, inverse=0, ws=P(16), nbytes=n):
        return lib.trx_svf_exp(vel, flow, *geom, inverse, ws, nbytes, None)

    def bwd(vel=P(16), dflow=P(16), dvel=P(16), geom=ok, inverse=0, ws=P(16), nbytes=n):
        return lib.trx_svf_exp_backward(vel, dflow, dvel, *geom, inverse, ws, nbytes, None)

    assert fwd(vel=None) == -1 and fwd(flow=None) == -1 and fwd(ws=None) == -1 and fwd(nbytes=n - 1) == -3
    assert bwd(vel=None) == -1 and bwd(dflow=None) == -1 and bwd(dvel=None) == -1 and bwd(ws=None) == -1 and bwd(nbytes=n - 1) == -3
    for bad, code in (((4, 2, 16, 16, 16, 4), -2), ((1, 2, 16, 16, 16, 4), -2), ((2, 2, 3, 16, 16, 4), -2), ((3, 0, 16, 16, 16, 4), -1),
                      ((3, 65536, 16, 16, 16, 4), -1), ((3, 2, 16, 0, 16, 4), -1), ((3, 2, 16, 16, 16, -1), -1), ((3, 2, 16, 16, 16, 13), -1),
                      ((3, 1, 2048, 1024, 1025, 1), -1)):
        assert lib.trx_svf_workspace_bytes(*bad) == 0, bad
        assert fwd(geom=bad, nbytes=1 << 62) == code and bwd(geom=bad, nbytes=1 << 62) == code, bad
    assert lib.trx_svf_workspace_bytes(3, 1, 2048, 1024, 1024, 1) > 0                                     # exactly 2^31 voxels


def test_loop_argument_checks_without_gpu():
    """trx_bspline_svf_run returns trx_bspline_run's status codes, and its own for squarings and the larger workspace, before any HIP call."""
    from torchregister_amd import _lib
    from test_bspline_host import _loop_args
    lib = _lib.load()
    sp = (ctypes.c_int * 3)(4, 4, 4)
    geom = (3, 2, 16, 16, 16, 4, 4, 4)
    n = lib.trx_bspline_svf_workspace_bytes(*geom, 4)
    field = 2 * 3 * 16 ** 3 * 4
    assert n >= lib.trx_bspline_workspace_bytes(*geom) + 2 * field + lib.trx_svf_workspace_bytes(3, 2, 16, 16, 16, 4)
    assert lib.trx_bspline_svf_workspace_bytes(*geom, 13) == 0 and lib.trx_bspline_svf_workspace_bytes(*geom, -1) == 0
    assert lib.trx_bspline_svf_workspace_bytes(3, 2, 16, 16, 16, 4, 0, 4, 4) == 0 and lib.trx_bspline_svf_workspace_bytes(4, 2, 16, 16, 16, 4, 4, 4, 4) == 0
    by = ctypes.byref

    def run(vol, loss, opt, st, spacing=sp, squarings=4, iters=3, ws=P(16), nbytes=n):
        a = [by(x) if x is not None else None for x in (vol, loss, opt, st)]
        return lib.trx_bspline_svf_run(*a, spacing, squarings, iters, ws, nbytes, None)

    vol, loss, opt, st = _loop_args()
    assert run(None, loss, opt, st) == -1 and run(vol, None, opt, st) == -1 and run(vol, loss, None, st) == -1 and run(vol, loss, opt, None) == -1
    assert run(vol, loss, opt, st, spacing=None) == -1 and run(vol, loss, opt, st, ws=None) == -1
    for f in ("ctrl", "flow", "dflow", "step"):
        v2, l2, o2, s2 = _loop_args()
        setattr(s2, f, None)
        assert run(v2, l2, o2, s2) == -1, f
    assert run(vol, loss, opt, st, squarings=13) == -1 and run(vol, loss, opt, st, squarings=-1) == -1
    assert run(vol, loss, opt, st, nbytes=n - 1) == -3 and run(vol, loss, opt, st, iters=9) == -5 and run(vol, loss, opt, st, iters=-1) == -1
    assert run(vol, loss, opt, st, iters=0) == 0                                                           # nothing to enqueue
    v2, l2, o2, s2 = _loop_args(ndim=4)
    assert run(v2, l2, o2, s2) == -2
    v2, l2, o2, s2 = _loop_args()
    s2.bending_weight = -1.0
    assert run(v2, l2, o2, s2) == -1


def test_keyword_validation_before_the_gpu():
    """diffeomorphic / squarings: mode='flow' with flow_model='bspline' and the fused criteria only."""
    import torchregister_amd as tr
    fused = dict(criterion=[tr.NCCLoss()], weight=[1.0])
    for args, kw in ((("flow",), dict(flow_model="direct")), (("flow",), dict(flow_model="unet")), (("flow",), dict()), (("affine",), dict()), (("rigid",), dict())):
        with pytest.raises(ValueError, match="diffeomorphic"):
            tr.Register(*args, diffeomorphic=True, **kw, **fused)
    with pytest.raises(ValueError, match="diffeomorphic"):
        tr.Register("flow", flow_model="bspline", diffeomorphic=True, criterion=[tr.MILoss()], weight=[1.0])
    for bad in (-1, 13, 2.0, True, None, "6"):
        with pytest.raises(ValueError, match="squarings"):
            tr.Register("flow", flow_model="bspline", spacing=6, diffeomorphic=True, squarings=bad, **fused)
    reg = tr.Register("flow", flow_model="bspline", spacing=6, diffeomorphic=True, optimizer="adam", levels=2, **fused)
    assert reg.diffeomorphic and reg.squarings == 6 and reg.velocity is None and reg.inverse_flow is None
    with pytest.raises(RuntimeError, match="diffeomorphic"):
        reg.inverse(torch.zeros(1, 1, 8, 8, 8))
    assert not tr.Register("flow", flow_model="bspline", spacing=6, **fused).diffeomorphic

    shape = (16, 20, 24)
    mse = dict(criterions=[nn.MSELoss()], weights=[1.0])
    for fm in ("direct", "unet"):
        with pytest.raises(ValueError, match="diffeomorphic"):
            tr.flow_register(shape, flow_model=fm, diffeomorphic=True, **mse)
    with pytest.raises(ValueError, match="diffeomorphic"):
        tr.flow_register(shape, flow_model="bspline", spacing=4, diffeomorphic=True, criterions=[tr.MILoss()], weights=[1.0])
    with pytest.raises(ValueError, match="squarings"):
        tr.flow_register(shape, flow_model="bspline", spacing=4, diffeomorphic=True, squarings=13, **mse)
    fr = tr.flow_register(shape, flow_model="bspline", spacing=4, diffeomorphic=True, squarings=3, **mse)
    assert fr.diffeomorphic and fr.squarings == 3
    with pytest.raises(RuntimeError, match="diffeomorphic"):
        fr.inverse(torch.zeros(1, 1, *shape))

    mov, tgt = torch.rand(1, 1, 16, 16, 16), torch.rand(1, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="squarings"):
        tr.BSplineSolver(mov, tgt, 4, squarings=13)
    with pytest.raises(ValueError, match="squarings"):
        tr.BSplineSolver(mov, tgt, 4, squarings=4, mi=dict(bins=16))
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.BSplineSolver(mov, tgt, 4, squarings=4)
    with pytest.raises(ValueError, match="squarings"):
        tr.svf_exp(torch.zeros(1, 3, 4, 4, 4), squarings=13)
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.svf_exp(torch.zeros(1, 3, 4, 4, 4))
