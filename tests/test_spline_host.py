"""Host-side checks of the nearest-neighbour and cubic B-spline resampling: the reference of record (tests/spline_ref.py)
against scipy and torch, the conditions on the inputs that tests/test_gpu_spline.py relies on, and every refusal of the C ABI and of the Python
layer - none of which needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spline_ref as sr
import test_affine_mi_grids_host as ghost

OK, ARG, NDIM, WS = 0, -1, -2, -3
REJECTED = ctypes.c_size_t(-1).value


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.COEF_SHAPES))
def test_coefficients_are_scipys_mirror_spline_filter(name):
    ndi = pytest.importorskip("scipy.ndimage")
    x = sr.volume(sr.COEF_SHAPES[name]).double()
    got = sr.coefficients(x)
    for b in range(2):
        for c in range(2):
            want = ndi.spline_filter(x[b, c].numpy(), order=3, mode="mirror", output=np.float64)
            assert np.abs(got[b, c].numpy() - want).max() <= 1e-12
    # the form the kernels evaluate, truncated at 16 taps a side: 4.5e-9 of the range (the range is 1)
    assert (sr.coefficients_fir(x) - got).abs().max().item() <= 1e-8
    assert (sr.coefficients_fir(x, reach=40) - got).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(sr.CASES))
def test_cubic_sample_is_scipys_map_coordinates_inside_the_field_of_view(name):
    ndi = pytest.importorskip("scipy.ndimage")
    x = sr.case(name)[0].double()
    pos = sr.case_positions(name)
    got = sr.sample_cubic(sr.coefficients(x), pos)
    inside = ~sr.outside(pos, x.shape[2:])
    for b in range(2):
        coords = pos[b].flip(-1).reshape(-1, pos.shape[-1]).T.numpy()                  # [nd, M] in the tensor's axis order
        for c in range(2):
            want = torch.from_numpy(ndi.map_coordinates(x[b, c].numpy(), coords, order=3, mode="mirror")).reshape(pos.shape[1:-1])
            assert (got[b, c] - want)[inside[b]].abs().max().item() <= 1e-12
    assert bool((got[~inside[:, None].expand_as(got)] == 0).all())


@pytest.mark.parametrize("name", list(sr.COEF_SHAPES))
def test_the_spline_interpolates(name):
    x = sr.volume(sr.COEF_SHAPES[name]).double()
    nd = x.dim() - 2
    pos = sr.positions(x.shape[2:], None, torch.zeros((2, nd) + tuple(x.shape[2:]), dtype=torch.float64))
    assert (sr.sample_cubic(sr.coefficients(x), pos) - x).abs().max().item() <= 1e-12


@pytest.mark.parametrize("name", list(sr.CASES))
def test_nearest_is_grid_samples_nearest_mode(name):
    x = sr.labels(sr.CASES[name][1]).double()
    pos = sr.case_positions(name)
    S = torch.tensor(tuple(x.shape[2:])[::-1], dtype=torch.float64)
    want = F.grid_sample(x, (2.0 * pos + 1.0) / S - 1.0, mode="nearest", padding_mode="zeros", align_corners=False)
    keep = sr.kept(pos, x.shape[2:], nearest=True)[:, None].expand_as(want)
    assert torch.equal(sr.sample_nearest(x, pos)[keep], want[keep])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the conditions the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sr.CASES))
def test_cases_meet_their_conditions(name):
    x, theta, flow = sr.case(name)
    pos = sr.case_positions(name)
    assert tuple(pos.shape[1:-1]) == sr.CASES[name][0] and pos.shape[0] == 2 and x.shape[:2] == (2, 2)
    share = sr.outside(pos, x.shape[2:]).double().mean().item()
    dropped = [1.0 - sr.kept(pos, x.shape[2:], nearest).double().mean().item() for nearest in (False, True)]
    print(f"{name}: {100 * share:.1f} % outside the field of view, kept leaves out {100 * dropped[0]:.3f} % (cubic) {100 * dropped[1]:.3f} % (nearest)")
    assert 0.05 <= share <= 0.50
    assert max(dropped) <= 0.01
    # every voxel outside the field of view that is kept is also outside in fp32, and the other way round
    keep = sr.kept(pos, x.shape[2:])
    assert torch.equal(sr.outside(pos, x.shape[2:])[keep], sr.outside(sr.case_positions(name, torch.float32), x.shape[2:])[keep])


def test_cubic_beats_linear_on_the_analytic_volume():
    """Reference cubic rms <= 0.25 x reference linear rms on interior voxels (measured: 0.054; nearest 0.103, linear 0.0172, cubic 0.00093)."""
    from oracle import compose
    img, flow, truth, interior = sr.analytic()
    pos = sr.positions(img.shape[2:], None, flow)
    cubic = sr.rms(sr.sample_cubic(sr.coefficients(img), pos)[0, 0] - truth, interior)
    linear = sr.rms(compose.flow_warp(img.double(), flow.double())[0, 0] - truth, interior)
    nearest = sr.rms(sr.sample_nearest(img.double(), pos)[0, 0] - truth, interior)
    print(f"rms against the analytic value: nearest {nearest:.4g} linear {linear:.4g} cubic {cubic:.4g} ({cubic / linear:.3f} of linear)")
    assert interior.double().mean().item() > 0.4
    assert cubic <= 0.25 * linear and linear < nearest


# ---------------------------------------------------------------------------------------------------------------------------------------
# refusals, before any HIP call
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ptr = lambda p: P(p) if p else None  # noqa: E731
    _vol, _grid = ghost._vol, ghost._grid
    inf, nan = float("inf"), float("nan")

    q = lib.trx_spline_workspace_bytes
    assert q(3, 4, 12, 14, 16) == 4 * 12 * 14 * 16 * 4 and q(2, 1, 1, 5, 13) == 5 * 13 * 4
    assert q(3, 1, 1, 1, 9) == 0 and q(2, 3, 1, 1, 9) == 0                    # one pass: no intermediate, and 0 is a valid answer
    for bad in ((1, 1, 1, 5, 13), (4, 1, 2, 5, 13), (0, 1, 1, 5, 13), (3, 0, 12, 14, 16), (3, -1, 12, 14, 16), (3, 65536, 12, 14, 16), (3, 1, 0, 14, 16),
                (3, 1, 12, 0, 16), (3, 1, 12, 14, -3), (2, 1, 2, 5, 13), (3, 1, 2048, 1024, 1024)):
        assert q(*bad) == REJECTED, bad

    def coef(src=4096, dst=8192, ndim=3, N=4, dhw=(12, 14, 16), ws=4096, nbytes=None):
        need = q(ndim, N, *dhw)
        return lib.trx_spline_coefficients(ptr(src), ptr(dst), ndim, N, *dhw, ptr(ws), (0 if need == REJECTED else need) if nbytes is None else nbytes, None)

    n = q(3, 4, 12, 14, 16)
    assert coef(src=None) == ARG and coef(dst=None) == ARG and coef(src=4096, dst=4096) == ARG
    assert coef(ndim=1) == NDIM and coef(ndim=4) == NDIM and coef(ndim=2) == NDIM and coef(ndim=2, dhw=(2, 5, 13)) == NDIM
    assert coef(N=0) == ARG and coef(N=65536) == ARG and coef(dhw=(0, 14, 16)) == ARG and coef(dhw=(12, -1, 16)) == ARG and coef(dhw=(12, 14, 0)) == ARG
    assert coef(dhw=(2048, 1024, 1024)) == ARG
    assert coef(nbytes=n - 1) == WS and coef(nbytes=0) == WS and coef(ws=None) == WS

    vol = _vol(_lib, B=1)

    def rs(v=vol, g=None, theta=4096, flow=4096, channels=2, order=3, out=4096):
        return lib.trx_transform_resample(ref(v), ref(g), ptr(theta), ptr(flow), channels, order, ptr(out), None)

    assert rs(v=None) == ARG and rs(out=None) == ARG and rs(v=_vol(_lib, B=1, ptr=False)) == ARG
    assert rs(theta=None, flow=None) == ARG and rs(g=_grid(_lib), theta=None) == ARG
    assert rs(channels=0) == ARG and rs(channels=-2) == ARG
    for order in (1, 2, -1, 4):
        assert rs(order=order) == ARG and rs(order=order, g=_grid(_lib)) == ARG
    assert rs(v=_vol(_lib, ndim=4)) == NDIM and rs(v=_vol(_lib, ndim=1)) == NDIM and rs(v=_vol(_lib, 2, 1, (2, 17, 19))) == NDIM
    assert rs(v=_vol(_lib, B=0)) == ARG and rs(v=_vol(_lib, B=70000)) == ARG and rs(v=_vol(_lib, dhw=(2048, 1024, 1024))) == ARG
    assert rs(v=_vol(_lib, dhw=(12, 0, 16))) == ARG
    # trx_moving_grid's own refusals
    for g in (_grid(_lib, (0, 13, 18)), _grid(_lib, (15, -1, 18)), _grid(_lib, (15, 13, 0)), _grid(_lib, (2048, 1024, 1024)), _grid(_lib, s0=nan),
              _grid(_lib, s5=inf), _grid(_lib, s3=nan), _grid(_lib, s11=-inf), _grid(_lib, s0=0.0), _grid(_lib, s6=-1.0), _grid(_lib, s10=0.0)):
        for order in (0, 3):
            assert rs(g=g, order=order) == ARG, (g.D, g.H, g.W, list(g.scale))
    assert rs(v=_vol(_lib, 2, 1, (1, 17, 19)), g=_grid(_lib, (2, 14, 23))) == NDIM
    # a good request passes every check but the one asked about: the call gets as far as the next refusal
    for g in (None, _grid(_lib), _grid(_lib, s3=0.0, s7=-2.0, s11=0.0), _grid(_lib, (1, 1, 1))):
        for order in (0, 3):
            assert rs(g=g, order=order, out=None) == ARG and rs(g=g, order=order, flow=None, channels=0) == ARG
    assert rs(theta=None, out=None) == ARG                                      # flow alone is a transform


def test_entry_points_refuse_before_any_launch():
    check_refusals()


def test_signatures_list_the_three_symbols():
    from torchregister_amd import _lib
    lib = _lib.load()
    for name in ("trx_spline_coefficients", "trx_transform_resample"):
        assert name in _lib.SIGNATURES and getattr(lib, name).restype is ctypes.c_int
    assert "trx_spline_workspace_bytes" in _lib.SIGNATURES and lib.trx_spline_workspace_bytes.restype is ctypes.c_size_t
    assert lib.trx_version() == 240


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python layer: ValueError before any device work (CPU tensors are the proof that nothing touched a device first)
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_python_refusals(x):
    import torch.nn as nn
    import torchregister_amd as tr
    nd, B = x.dim() - 2, x.shape[0]
    eye = torch.eye(nd, nd + 1)[None]
    flow = torch.zeros((B, nd) + tuple(x.shape[2:]))
    # unknown interpolation, on resample and on all four methods - finished or not
    ffd = tr.flow_register(x.shape[2:], criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=4)
    finished = tr.flow_register(x.shape[2:], criterions=[nn.MSELoss()], weights=[1.0], flow_model="bspline", spacing=4)
    finished.flow = finished.inverse_flow = flow
    reg, reg_done = tr.Register("rigid"), tr.Register("rigid")
    reg_done.theta = eye
    flow_reg = tr.Register("flow", flow_model="bspline", criterion=[nn.MSELoss()], weight=[1.0], spacing=4, diffeomorphic=True)
    flow_reg.theta, flow_reg.warp, flow_reg.inverse_flow, flow_reg._inverse_warp = flow, finished.deform, flow, finished.inverse
    for bad in ("bicubic", "bilinear", "Cubic", 3, None):
        for call in (lambda: tr.resample(x, theta=eye, interpolation=bad), lambda: tr.resample(x, flow=flow, interpolation=bad),
                     lambda: reg(x, interpolation=bad), lambda: reg_done(x, interpolation=bad), lambda: reg.inverse(x, interpolation=bad),
                     lambda: flow_reg(x, interpolation=bad), lambda: flow_reg.inverse(x, interpolation=bad),
                     lambda: ffd.deform(x, interpolation=bad), lambda: ffd.inverse(x, interpolation=bad),
                     lambda: finished.deform(x, interpolation=bad), lambda: finished.inverse(x, interpolation=bad)):
            with pytest.raises(ValueError, match="interpolation"):
                call()
    # no transform, and shapes that do not fit
    for interpolation in tr._engine.INTERPOLATIONS:
        kw = dict(interpolation=interpolation)
        with pytest.raises(ValueError, match="theta, flow or both"):
            tr.resample(x, **kw)
        for bad in (dict(theta=torch.zeros(B + 2, nd, nd + 1)), dict(theta=torch.zeros(1, nd, nd)), dict(theta=torch.zeros(nd, nd + 1)), dict(theta="theta"),
                    dict(flow=torch.zeros((B + 2, nd) + tuple(x.shape[2:]))), dict(flow=torch.zeros((B, nd + 1) + tuple(x.shape[2:]))),
                    dict(flow=torch.zeros((B, nd) + tuple(x.shape[3:]))), dict(flow=torch.zeros((B, nd) + tuple(s + 1 for s in x.shape[2:]))),
                    dict(flow=flow, size=tuple(s + 1 for s in x.shape[2:])), dict(flow=flow, scale=torch.ones(nd, nd + 1)),
                    dict(theta=eye, size=(4,) * (nd + 1)), dict(theta=eye, size=(0,) + (4,) * (nd - 1)), dict(theta=eye, scale=torch.ones(nd, nd)),
                    dict(theta=eye, flow=torch.zeros((B, nd, 5) + (4,) * (nd - 1)), size=(4,) * nd)):
            with pytest.raises(ValueError):
                tr.resample(x, **bad, **kw)
        with pytest.raises(ValueError):
            tr.resample(x[0], theta=eye, **kw)
        # a valid request passes the validation and is refused by the device check, as today's calls are
        for good in (dict(theta=eye), dict(flow=flow), dict(flow=flow[:1]), dict(theta=eye, flow=torch.zeros((B, nd, 5) + (4,) * (nd - 1))),
                     dict(theta=eye, size=(5,) + (4,) * (nd - 1), scale=torch.ones(nd, nd + 1))):
            with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
                tr.resample(x, **good, **kw)
    with pytest.raises(ValueError):
        tr.spline_coefficients(x[0, 0])
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.spline_coefficients(x)
    # interpolation='linear' raises what today's call raises
    for today, now in ((lambda: tr._engine.affine_warp(eye.expand(B, -1, -1), x), lambda: tr.resample(x, theta=eye, interpolation="linear")),
                       (lambda: tr._engine.flow_warp(x, flow), lambda: tr.resample(x, flow=flow, interpolation="linear")),
                       (lambda: tr.affine_flow_warp(x, eye, flow), lambda: tr.resample(x, theta=eye, flow=flow, interpolation="linear")),
                       (lambda: reg_done(x), lambda: reg_done(x, interpolation="linear")),
                       (lambda: finished.deform(x), lambda: finished.deform(x, interpolation="linear")),
                       (lambda: finished.inverse(x), lambda: finished.inverse(x, interpolation="linear")),
                       (lambda: flow_reg(x), lambda: flow_reg(x, interpolation="linear")),
                       (lambda: flow_reg.inverse(x), lambda: flow_reg.inverse(x, interpolation="linear"))):
        with pytest.raises(Exception) as before:
            today()
        with pytest.raises(type(before.value)) as after:
            now()
        assert str(after.value) == str(before.value)
    # the refusals of before stand
    with pytest.raises(RuntimeError, match="optim"):
        reg(x)
    with pytest.raises(RuntimeError, match="optim"):
        reg(x, interpolation="cubic")
    with pytest.raises(RuntimeError, match="diffeomorphic"):
        reg.inverse(x, interpolation="nearest")
    with pytest.raises(RuntimeError, match="diffeomorphic"):
        ffd.inverse(x, interpolation="nearest")
    with pytest.raises(NotImplementedError):
        tr.SpatialTransformer(x.shape[2:], mode="bicubic")


def test_python_refuses_before_any_device_work():
    import torchregister_amd as tr
    import TorchRegister
    assert TorchRegister.resample is tr.resample and tr.resample is tr._engine.resample
    assert TorchRegister.spline_coefficients is tr.spline_coefficients and tr.spline_coefficients is tr._engine.spline_coefficients
    check_python_refusals(torch.zeros(2, 2, 5, 6, 7))
    check_python_refusals(torch.zeros(1, 3, 9, 8))
