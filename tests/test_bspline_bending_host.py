"""CPU-only checks of the bending energy of the B-spline free-form deformation: the restatement's own properties (tests/bspline_bending_ref.py,
fp64), the argument checks of trx_bspline_bending and of trx_bspline_state.bending_weight before any HIP call, and the validation of
Register / flow_register / BSplineSolver."""
import ctypes

import pytest
import torch
import torch.nn as nn

import bspline_bending_ref as bref
import bspline_ref as ref

CASES = [((13, 18, 23), (4, 5, 3)), ((17, 17, 17), 4), ((5, 6, 7), 8), ((9, 10, 11), 1), ((1, 12, 20), (3, 3, 4)), ((19, 26), (4, 6)),
         ((1, 1, 9), 2), ((40, 3), (9, 1))]


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 4 - 1


@pytest.mark.parametrize("spatial,spacing", CASES)
def test_squares_form_under_autograd_equals_the_gram_form(spatial, spacing):
    """E and dE/dctrl: the definition (sums of squared second derivatives, differentiated by torch autograd) against the Gram form, rtol 1e-9
    in fp64 (of E, and of max|g| for the gradient)."""
    nd = len(spatial)
    c = _rand((2, nd) + ref.grid(spatial, spacing), 1).requires_grad_()
    e_sq = bref.energy_squares(c, spatial, spacing)
    g_sq, = torch.autograd.grad(e_sq.sum(), c)
    e_gr, g_gr = bref.energy_gram(c.detach(), spatial, spacing)
    assert (e_sq.detach() > 0).all()
    assert torch.allclose(e_sq.detach(), e_gr, rtol=1e-9, atol=0.0), (e_sq, e_gr)
    assert (g_sq - g_gr).abs().max().item() <= 1e-9 * g_gr.abs().max().item()


def test_derivative_matrices_differentiate_the_spline():
    """M^(1) and M^(2) against central differences of the B-spline itself, evaluated between the voxels with a finer lattice position: a
    displacement ctrl x M^(0) sampled at spacing d is the same spline as the one a lattice of spacing d * f samples at f times the voxels.
    The spline's third derivative is piecewise constant and bounded by T = 8 max|c| / d^3, so a central first difference of step h is off by
    at most h^2 T / 6 and a central second difference (at a knot, where the third derivative jumps) by at most h T."""
    S, d, f = 9, 3, 64
    c = _rand((1, 1, ref.grid((S,) * 2, d)[0], 1), 3)[0, 0, :, 0]
    fine = ref.axis_matrix((S - 1) * f + 1, d * f) @ c          # the spline at x = j / f
    h = 1.0 / f
    T = 8 * c.abs().max().item() / d ** 3
    for x in range(1, S - 1):
        j = x * f
        d1 = (fine[j + 1] - fine[j - 1]) / (2 * h)
        d2 = (fine[j + 1] - 2 * fine[j] + fine[j - 1]) / (h * h)
        assert abs((bref.deriv_matrix(S, d, 1) @ c)[x] - d1) <= h * h * T
        assert abs((bref.deriv_matrix(S, d, 2) @ c)[x] - d2) <= h * T


@pytest.mark.parametrize("spatial,spacing", CASES)
def test_an_affine_lattice_has_no_bending_energy(spatial, spacing):
    """ctrl_c linear in the lattice indices: E = 0 in fp64.  The squares form squares its rounding (second derivatives of 1e-12 max|ctrl| at
    the most: 1e-24 max|ctrl|^2); the Gram form is linear in it: |g| <= 1e-13 max|ctrl|, hence |E| <= 1/2 numel max|ctrl| max|g|."""
    nd = len(spatial)
    G = ref.grid(spatial, spacing)
    idx = torch.meshgrid(*[torch.arange(g, dtype=torch.float64) for g in G], indexing="ij")
    a = [0.31, -0.17, 0.23]
    ctrl = torch.stack([(c + 1) * (sum(a[i] * idx[i] for i in range(nd)) + 0.4) for c in range(nd)])[None]
    scale = ctrl.abs().max().item() ** 2
    e_gr, g = bref.energy_gram(ctrl, spatial, spacing)
    assert bref.energy_squares(ctrl, spatial, spacing).abs().max().item() <= 1e-24 * scale
    assert g.abs().max().item() <= 1e-13 * ctrl.abs().max().item() and e_gr.abs().max().item() <= 0.5 * ctrl.numel() * 1e-13 * scale


def test_gram_matrices_are_banded():
    for S, d in ((23, 3), (5, 8), (1, 4), (12, 1)):
        for k in range(3):
            R = bref.gram_matrix(S, d, k)
            i, j = torch.meshgrid(torch.arange(R.shape[0]), torch.arange(R.shape[1]), indexing="ij")
            assert torch.count_nonzero(R[(i - j).abs() > 3]).item() == 0 and torch.equal(R, R.t())


P = ctypes.c_void_p


def test_bending_argument_checks_without_gpu():
    """trx_bspline_bending returns its status before any HIP call: null pointers -1, ndim -2, a workspace one byte short -3."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ok = (3, 2, 16, 16, 16, 4, 4, 4)                              # ndim, B, D, H, W, sz, sy, sx
    n = lib.trx_bspline_workspace_bytes(*ok)
    assert n > 0

    def call(ctrl=P(16), energy=P(16), dctrl=P(16), geom=ok, ws=P(16), nbytes=n):
        return lib.trx_bspline_bending(ctrl, energy, dctrl, 1.0, 0, *geom, ws, nbytes, None)

    assert call(ctrl=None) == -1 and call(energy=None) == -1 and call(ws=None) == -1
    assert call(nbytes=n - 1) == -3 and call(dctrl=None, nbytes=n - 1) == -3       # dctrl is optional: the call gets as far as the workspace check
    for bad, code in (((4, 2, 16, 16, 16, 4, 4, 4), -2), ((1, 2, 16, 16, 16, 4, 4, 4), -2), ((2, 2, 3, 16, 16, 4, 4, 4), -2),
                      ((3, 0, 16, 16, 16, 4, 4, 4), -1), ((3, 2, 16, 16, 16, 4, 0, 4), -1), ((3, 2, 16, 16, 16, 4, 4, 1025), -1)):
        assert call(geom=bad, nbytes=1 << 40) == code, bad
    # the workspace holds the bands (21 floats per control point of every axis) and one partial per 8 x 8 x 8 lattice tile and volume
    assert n >= 21 * 3 * 7 * 4 + 2 * 3 * 1 * 4


def test_bending_weight_of_the_loop_is_checked_without_gpu():
    """trx_bspline_run / _step: a negative or non-finite bending_weight is -1 before any HIP call; the field is the struct's last."""
    from torchregister_amd import _lib
    from test_bspline_host import _loop_args
    lib = _lib.load()
    assert _lib.BSplineState._fields_[-1][0] == "bending_weight"
    sp = (ctypes.c_int * 3)(4, 4, 4)
    n = lib.trx_bspline_workspace_bytes(3, 2, 16, 16, 16, 4, 4, 4)
    by = ctypes.byref
    for bad in (-1.0, -1e-30, float("inf"), float("nan")):
        vol, loss, opt, st = _loop_args()
        st.bending_weight = bad
        assert lib.trx_bspline_run(by(vol), by(loss), by(opt), by(st), sp, 3, P(16), n, None) == -1, bad
        assert lib.trx_bspline_step(by(vol), by(loss), by(opt), by(st), sp, P(16), n, None) == -1, bad
    vol, loss, opt, st = _loop_args()
    st.bending_weight = 2.5
    assert lib.trx_bspline_run(by(vol), by(loss), by(opt), by(st), sp, 0, P(16), n, None) == 0          # nothing to enqueue
    assert lib.trx_bspline_run(by(vol), by(loss), by(opt), by(st), sp, 3, P(16), n - 1, None) == -3


def test_bending_weight_validation_before_the_gpu():
    """Register / flow_register take bending_weight only with flow_model='bspline'; smooth_weight keeps raising there."""
    import torchregister_amd as tr
    fused = dict(criterion=[tr.NCCLoss()], weight=[1.0])
    for kw in (dict(flow_model="direct"), dict(flow_model="unet"), dict()):
        with pytest.raises(ValueError, match="bending_weight"):
            tr.Register("flow", bending_weight=0.5, **kw, **fused)
    with pytest.raises(ValueError, match="bending_weight"):
        tr.Register("affine", bending_weight=0.5)
    for bad in (-1.0, float("inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="bending_weight"):
            tr.Register("flow", flow_model="bspline", spacing=6, bending_weight=bad, **fused)
    assert tr.Register("flow", flow_model="bspline", spacing=6, bending_weight=3, levels=2, **fused).bending_weight == 3.0
    tr.Register("flow", flow_model="direct", bending_weight=0.0, **fused)                # the default value is accepted everywhere
    with pytest.raises(ValueError, match="smooth_weight.*bending_weight"):
        tr.Register("flow", flow_model="bspline", spacing=6, smooth_weight=0.5, **fused)

    shape = (16, 20, 24)
    mse = dict(criterions=[nn.MSELoss()], weights=[1.0])
    for fm in ("direct", "unet"):
        with pytest.raises(ValueError, match="bending_weight"):
            tr.flow_register(shape, flow_model=fm, bending_weight=1.0, **mse)
    with pytest.raises(ValueError, match="bending_weight"):
        tr.flow_register(shape, flow_model="bspline", spacing=4, bending_weight=-2.0, **mse)
    with pytest.raises(ValueError, match="smooth_weight.*bending_weight"):
        tr.flow_register(shape, flow_model="bspline", spacing=4, smooth_weight=1.0, **mse)
    assert tr.flow_register(shape, flow_model="bspline", spacing=4, bending_weight=7.5, **mse).bending_weight == 7.5
    assert tr.flow_register(shape, flow_model="direct", **mse).bending_weight == 0.0

    mov, tgt = torch.rand(1, 1, 16, 16, 16), torch.rand(1, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="bending_weight"):
        tr.BSplineSolver(mov, tgt, 4, bending_weight=-1.0)
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.bspline_bending(torch.zeros((1, 3) + ref.grid((16, 16, 16), 4)), (16, 16, 16), 4)
