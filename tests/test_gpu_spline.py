"""GPU checks of the nearest-neighbour and cubic B-spline resampling (trx_spline_coefficients, trx_transform_resample, resample and interpolation= of
the public interface) against tests/spline_ref.py.  The shapes are the smallest at which the kernels can still go wrong: axes
shorter than the filter's reach, W below a wave, odd sizes, 2-D, more than one tile per line and block per volume, N = B C = 4 volumes, an axis of one
voxel inside a 3-D call.  tests/test_spline_host.py asserts the conditions on the inputs (how many samples leave the field of view, which voxels the
comparisons leave out).
The bar of every comparison against fp64: max(1e-5 x the input's range - what the project holds trx_affine_warp_grids to -, 4 x the gap between the
reference run in fp32 and in fp64)."""
import functools

import pytest
import torch
import torch.nn as nn

import affine_mi_grids_ref as gref
import spline_ref as sr
from test_spline_host import check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _bar(x, gap):
    return max(1e-5 * (x.max() - x.min()).item(), 4.0 * gap)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. coefficients
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _coef_reference(name):
    """(x, fp64 coefficients, gap of the fp32 restatement): computed once, shared, never written to."""
    x = sr.volume(sr.COEF_SHAPES[name])
    c64 = sr.coefficients(x)
    return x, c64, (sr.coefficients(x, torch.float32).double() - c64).abs().max().item()


@pytest.mark.parametrize("name", list(sr.COEF_SHAPES))
def test_coefficients_against_the_fp64_reference(tr, name):
    x, want, gap = _coef_reference(name)
    got = tr.spline_coefficients(x.cuda())
    assert got.shape == x.shape and got.dtype == torch.float32
    err, bar = (got.cpu().double() - want).abs().max().item(), _bar(x, gap)
    print(f"{name}: coefficients err {err:.3e} bar {bar:.3e} (fp32 restatement {gap:.3e}, max |c| {want.abs().max().item():.2f})")
    assert err <= bar
    assert torch.equal(got, tr.spline_coefficients(x.cuda()))                                   # the same bits on two calls
    assert torch.equal(got[1:, 1:], tr.spline_coefficients(x[1:, 1:].cuda()))                   # a volume alone and inside a batch
    if name == "1x6x8":                                                                         # an axis of one voxel is left alone:
        assert torch.equal(got[:, :, 0], tr.spline_coefficients(x[:, :, 0].cuda()))             # the 2-D call of the same planes


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. cubic resample, one case per position chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def _call(tr, name, x, interpolation, **kw):
    _, theta, flow = sr.case(name)
    scale = sr.case_scale(name)
    return tr.resample(x.cuda(), theta=None if theta is None else theta.cuda(), flow=None if flow is None else flow.cuda(),
                       size=sr.CASES[name][0] if flow is None else None, scale=None if scale is None else scale.float(), interpolation=interpolation, **kw)


@functools.lru_cache(maxsize=None)
def _cubic_reference(name):
    """(fp64 result, kept voxels [2,1,*S_t], outside [2,1,*S_t], gap of the fp32 restatement on the kept voxels)."""
    x = sr.case(name)[0]
    pos = sr.case_positions(name)
    want = sr.sample_cubic(sr.coefficients(x), pos)
    keep = sr.kept(pos, x.shape[2:])[:, None]
    r32 = sr.sample_cubic(sr.coefficients(x, torch.float32), sr.case_positions(name, torch.float32), torch.float32).double()
    return want, keep, sr.outside(pos, x.shape[2:])[:, None], (r32 - want)[keep.expand_as(want)].abs().max().item()


@pytest.mark.parametrize("name", list(sr.CASES))
def test_cubic_resample_against_the_fp64_reference(tr, name):
    x = sr.case(name)[0]
    want, keep, out, gap = _cubic_reference(name)
    got = _call(tr, name, x, "cubic")
    assert got.shape == want.shape and got.dtype == torch.float32
    k = keep.expand_as(want)
    err, bar = (got.cpu().double() - want)[k].abs().max().item(), _bar(x, gap)
    print(f"{name}: cubic err {err:.3e} bar {bar:.3e} (fp32 restatement {gap:.3e}; {100 * out.double().mean().item():.1f} % outside)")
    assert err <= bar
    assert bool((got.cpu()[(keep & out).expand_as(want)] == 0).all())                            # outside the field of view: exactly 0
    assert torch.equal(got, _call(tr, name, x, "cubic"))
    assert torch.equal(got[:, 1:], _call(tr, name, x[:, 1:], "cubic"))                           # channels share coordinates and weights
    assert torch.equal(got[:1], _call_pair0(tr, name, x))                                        # a pair does not depend on its batch


def _call_pair0(tr, name, x):
    """Pair 0 alone: a pair does not depend on its batch."""
    _, theta, flow = sr.case(name)
    scale = sr.case_scale(name)
    return tr.resample(x[:1].cuda(), theta=None if theta is None else theta[:1].cuda(), flow=None if flow is None else flow[:1].cuda(),
                       size=sr.CASES[name][0] if flow is None else None, scale=None if scale is None else scale.float())


@pytest.mark.parametrize("name", ["2x3x33", "7x9x11", "5x13", "12x14x70", "1x6x8"])
def test_cubic_at_integer_positions_returns_the_input(tr, name):
    """theta = I and zero flow, through both position chains: the spline interpolates."""
    x, _, gap = _coef_reference(name)
    nd = x.dim() - 2
    bar = _bar(x, gap)
    eye = torch.eye(nd, nd + 1)[None].cuda()
    zero = torch.zeros((2, nd) + tuple(x.shape[2:])).cuda()
    for label, kw in (("flow", dict(flow=zero)), ("theta", dict(theta=eye)), ("theta + flow", dict(theta=eye, flow=zero))):
        err = (tr.resample(x.cuda(), **kw).cpu().double() - x.double()).abs().max().item()
        print(f"{name}: {label} at the lattice points: err {err:.3e} bar {bar:.3e}")
        assert err <= bar


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. nearest resample
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sr.CASES if not sr.CASES[n][2]])
def test_nearest_through_a_flow_is_the_existing_kernel(tr, name):
    x, _, flow = sr.case(name)
    assert torch.equal(_call(tr, name, x, "nearest"), tr._engine.flow_warp(x.cuda(), flow.cuda(), nearest=True))
    lab = sr.labels(sr.CASES[name][1])
    assert torch.equal(_call(tr, name, lab, "nearest"), tr._engine.flow_warp(lab.cuda(), flow.cuda(), nearest=True))


@pytest.mark.parametrize("name", [n for n in sr.CASES if sr.CASES[n][2]])
def test_nearest_through_theta_carries_labels_exactly(tr, name):
    lab = sr.labels(sr.CASES[name][1])
    pos = sr.case_positions(name)
    want = sr.sample_nearest(lab.double(), pos)
    keep = sr.kept(pos, lab.shape[2:], nearest=True)[:, None].expand_as(want)
    got = _call(tr, name, lab, "nearest")
    assert got.shape == want.shape
    wrong = (got.cpu().double() != want)[keep].sum().item()
    print(f"{name}: nearest, {wrong} of {int(keep.sum())} kept voxels differ; values {sorted(set(got.cpu().flatten().tolist()))}")
    assert wrong == 0
    assert set(got.cpu().flatten().tolist()) <= set(float(v) for v in range(8))                  # no label is invented anywhere
    assert torch.equal(got, _call(tr, name, lab, "nearest")) and torch.equal(got[:, 1:], _call(tr, name, lab[:, 1:], "nearest"))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. what it is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_cubic_on_the_analytic_volume(tr):
    """GPU cubic rms <= 1.05 x the reference's cubic rms against the analytic value on the interior voxels."""
    img, flow, truth, interior = sr.analytic()
    ref = sr.rms(sr.sample_cubic(sr.coefficients(img), sr.positions(img.shape[2:], None, flow))[0, 0] - truth, interior)
    rms = {k: sr.rms(tr.resample(img.cuda(), flow=flow.cuda(), interpolation=k)[0, 0].cpu().double() - truth, interior) for k in ("nearest", "linear", "cubic")}
    print(f"rms against the analytic value: nearest {rms['nearest']:.4g} linear {rms['linear']:.4g} cubic {rms['cubic']:.4g} (reference cubic {ref:.4g})")
    assert rms["cubic"] <= 1.05 * ref
    assert rms["cubic"] < rms["linear"] < rms["nearest"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. public interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_linear_is_the_existing_warps_bit_for_bit(tr):
    x, theta, flow = sr.case("composed")
    xc, th, fl = x.cuda(), theta.cuda(), flow.cuda()
    assert torch.equal(tr.resample(xc, theta=th, flow=fl, interpolation="linear"), tr.affine_flow_warp(xc, th, fl))
    assert torch.equal(tr.resample(xc, theta=th, size=flow.shape[2:], interpolation="linear"), tr._engine.affine_warp(th, xc, size=flow.shape[2:]))
    assert torch.equal(tr.resample(xc, theta=th, interpolation="linear"), tr._engine.affine_warp(th, xc))
    x, _, flow = sr.case("flow")
    assert torch.equal(tr.resample(x.cuda(), flow=flow.cuda(), interpolation="linear"), tr._engine.flow_warp(x.cuda(), flow.cuda()))
    x, theta, _ = sr.case("grids-world")
    scale = sr.case_scale("grids-world").float()
    got = tr.resample(x.cuda(), theta=theta.cuda(), size=(10, 12, 14), scale=scale, interpolation="linear")
    assert torch.equal(got, tr._engine.affine_warp(theta.cuda() * scale.cuda(), x.cuda(), size=(10, 12, 14)))


def test_register_interpolation_through_both_stages(tr):
    """The test that fails without the feature: a rigid stage on two lattices (10 x 12 x 14 from 20 x 18 x 16, in millimetres), the B-spline stage composed
    with it, and a label map and an image carried through each with the interpolation of the caller's choice."""
    tshape, mshape = (10, 12, 14), (20, 18, 16)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, mshape))
    rigid = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6))
    rigid.optim(mov, tgt, lr=0.01, max_epochs=3, moving_voxel=gref.VOXEL_M3, target_voxel=gref.VOXEL_T3)
    ffd = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4)
    ffd.optim(mov, tgt, lr=0.05, max_epochs=3, initial=rigid)
    x = torch.cat([mov, sr.labels(mshape)[:1, :1].cuda()], dim=1)
    for reg in (rigid, ffd):
        assert torch.equal(reg(x), reg(x, interpolation="linear")) and reg(x).shape == (1, 2) + tshape
    for k in ("nearest", "cubic"):
        assert torch.equal(rigid(x, interpolation=k), tr.resample(x, theta=rigid.theta, size=tshape, interpolation=k))
        assert torch.equal(ffd(x, interpolation=k), tr.resample(x, theta=ffd.initial, flow=ffd.theta, interpolation=k))
        assert ffd(x, interpolation=k).shape == (1, 2) + tshape
    assert torch.equal(tr.resample(x, theta=ffd.initial, flow=ffd.theta, interpolation="linear"), ffd(x))
    lab = ffd(x, interpolation="nearest")[:, 1]
    assert set(lab.cpu().flatten().tolist()) <= set(float(v) for v in range(8))
    # the three interpolations are three different answers to the same transform
    assert not torch.equal(ffd(x, interpolation="cubic"), ffd(x)) and not torch.equal(ffd(x, interpolation="nearest"), ffd(x))


def test_diffeomorphic_inverse_takes_an_interpolation(tr):
    tshape = (10, 12, 14)
    mov, tgt = (x.cuda() for x in gref.pair(tshape, tshape))
    reg = tr.Register("flow", flow_model="bspline", criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", spacing=4, diffeomorphic=True, squarings=4)
    reg.optim(mov, tgt, lr=0.05, max_epochs=3)
    x = torch.cat([mov, mov * mov], dim=1)
    assert torch.equal(reg.inverse(x), reg.inverse(x, interpolation="linear"))
    for k in ("nearest", "cubic"):
        assert torch.equal(reg.inverse(x, interpolation=k), tr.resample(x, flow=reg.inverse_flow, interpolation=k))
        assert torch.equal(reg(x, interpolation=k), tr.resample(x, flow=reg.theta, interpolation=k))


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()
    x = sr.case("flow")[0].cuda()
    with pytest.raises(ValueError, match="interpolation"):
        tr.resample(x, flow=sr.case("flow")[2].cuda(), interpolation="bicubic")
    with pytest.raises(ValueError, match="theta, flow or both"):
        tr.resample(x)
