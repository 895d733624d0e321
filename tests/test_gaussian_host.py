"""Host checks of the Gaussian operator and the voxel-aware pyramid schedule (no GPU): the restatement against its two outside yardsticks, the
schedule's arithmetic, the refusals of Register's new keywords and of the C ABI."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gaussian_ref as gr

ARG, NDIM, WS = -1, -2, -3


def volume():
    return np.random.default_rng(20240).standard_normal((9, 13, 70))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement against scipy (same size) and F.interpolate (sigma = 0)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("padding,mode", [("border", "nearest"), ("zeros", "constant")])
@pytest.mark.parametrize("sigma", [(0.6, 1.7, 3.2), (4.0, 0, 0.5)])
def test_restatement_against_scipy(sigma, padding, mode):
    import scipy.ndimage as ndi
    x = volume()
    for truncate in (4.0, 2.5):
        got = gr.gaussian_resample(x, x.shape, sigma, truncate=truncate, padding=padding)
        want = ndi.gaussian_filter(x, sigma, mode=mode, truncate=truncate)
        err = float(np.abs(got - want).max())
        print(f"sigma {sigma} {padding} truncate {truncate}: max |restatement - scipy| = {err:.3g}")
        assert err <= 2e-14


@pytest.mark.parametrize("align_corners", [False, True])
@pytest.mark.parametrize("size", [(5, 7, 33), (12, 13, 100)])
def test_restatement_against_interpolate(size, align_corners):
    x = volume()
    got = gr.gaussian_resample(x, size, 0.0, align_corners=align_corners)
    want = F.interpolate(torch.from_numpy(x)[None, None], size=size, mode="trilinear", align_corners=align_corners)[0, 0].numpy()
    err = float(np.abs(got - want).max())
    print(f"{size} align_corners={align_corners}: max |restatement - F.interpolate| = {err:.3g}")
    assert err <= 2e-14


def test_fp32_switch_runs_in_fp32_and_stays_close():
    x = volume().astype(np.float32)
    r64 = gr.gaussian_resample(x, (9, 13, 35), (0.6, 1.7, 3.2))
    r32 = gr.gaussian_resample(x, (9, 13, 35), (0.6, 1.7, 3.2), fp32=True)
    assert r64.dtype == np.float64 and r32.dtype == np.float32
    assert 0 < np.abs(r32 - r64).max() < 1e-5


def test_radius():
    assert [gr.radius(s) for s in (0.1, 0.5, 3.2)] == [0, 2, 13]
    x = volume()
    assert np.array_equal(gr.gaussian_resample(x, x.shape, 0.1), x)      # R = 0: the identity
    R, g = gr.taps(3.2)
    assert len(g) == 2 * R + 1 and abs(g.sum() - 1) < 1e-15 and np.array_equal(g, g[::-1])


# ---------------------------------------------------------------------------------------------------------------------------------------
# pyramid_schedule
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_schedule_worked_values():
    import torchregister_amd as tr
    shrink, sigma = tr.pyramid_schedule((120, 512, 512), 3, voxel=(3.0, 0.7, 0.7))
    assert [tuple(f) for f in shrink] == [(1, 4, 4), (1, 2, 2), (1, 1, 1)]
    assert [tuple(s) for s in sigma] == [(0.0, 2.0, 2.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.0)]
    shrink, sigma = tr.pyramid_schedule((100, 256, 256), 3, voxel=(1.2, 0.9, 0.9))
    assert [tuple(f) for f in shrink] == [(3, 4, 4), (1, 2, 2), (1, 1, 1)]
    assert [tuple(s) for s in sigma] == [(1.5, 2.0, 2.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.0)]
    shrink, sigma = tr.pyramid_schedule((64, 64, 64), 3)      # no voxel sizes: the halving factors
    assert [tuple(f) for f in shrink] == [(4, 4, 4), (2, 2, 2), (1, 1, 1)]
    assert [tuple(s) for s in sigma] == [(2.0, 2.0, 2.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)]


def test_schedule_2d_and_one_level():
    import torchregister_amd as tr
    shrink, sigma = tr.pyramid_schedule((33, 130), 3, voxel=(2.0, 0.5))
    assert [tuple(f) for f in shrink] == [(1, 4), (1, 2), (1, 1)]
    assert [tuple(s) for s in sigma] == [(0.0, 2.0), (0.0, 1.0), (0.0, 0.0)]
    assert tr.pyramid_schedule((5, 5), 1) == ([(1, 1)], [(0.0, 0.0)])


def test_schedule_min_size_back_off():
    import torchregister_amd as tr
    from torchregister_amd.gaussian import schedule_shapes
    shrink, sigma = tr.pyramid_schedule((20, 64, 64), 4)
    assert [tuple(f) for f in shrink] == [(2, 8, 8), (2, 4, 4), (2, 2, 2), (1, 1, 1)]      # ceil(20 / 3) = 7 < 8: the first axis stops at 2
    assert [tuple(s) for s in sigma] == [(1.0, 4.0, 4.0), (1.0, 2.0, 2.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)]
    assert schedule_shapes((20, 64, 64), shrink) == [(10, 8, 8), (10, 16, 16), (10, 32, 32), (20, 64, 64)]
    # the showcase pair of the GPU test
    assert schedule_shapes((12, 40, 44), tr.pyramid_schedule((12, 40, 44), 3, (3.0, 0.7, 0.7))[0]) == [(12, 10, 11), (12, 20, 22), (12, 40, 44)]
    assert schedule_shapes((24, 30, 32), tr.pyramid_schedule((24, 30, 32), 3, (1.2, 0.9, 0.9))[0]) == [(8, 8, 8), (24, 15, 16), (24, 30, 32)]


def test_schedule_refusals():
    import torchregister_amd as tr
    with pytest.raises(ValueError, match=r"levels=3: no axis of \(10, 10, 10\) can be halved without going below 8 voxels; the largest levels that works for "
                                         r"\(20, 20, 20\) is 2"):
        tr.pyramid_schedule((20, 20, 20), 3)
    with pytest.raises(ValueError, match="levels=3"):
        tr.pyramid_shapes((20, 20, 20), 3)      # the wording is pyramid_shapes'
    with pytest.raises(ValueError):
        tr.pyramid_schedule((20, 20, 20), 0)
    for bad in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0)):
        with pytest.raises(ValueError):
            tr.pyramid_schedule((64, 64, 64), 2, voxel=bad)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Register's keywords
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_register_init_refusals():
    import torchregister_amd as tr
    mi = dict(criterion=[tr.MILoss()], weight=[1.0])
    good = [(1, 2, 2), (1, 1, 1)]
    for kw in (dict(shrink=good), dict(shrink='voxel'), dict(smoothing=[(0, 1, 1), (0, 0, 0)]), dict(moving_shrink=good), dict(moving_smoothing=[1.0, 0.0])):
        with pytest.raises(ValueError, match="levels > 1"):
            tr.Register(mode='rigid', levels=1, **kw)
    for kw in (dict(smoothing=[1.0, 0.0]), dict(moving_shrink=good), dict(moving_smoothing=[1.0, 0.0])):
        with pytest.raises(ValueError, match="go with shrink"):
            tr.Register(mode='rigid', levels=2, device_loop=True, **mi, **kw)
    for bad in (good[:1], good + good[-1:], [(1, 2.0, 2), (1, 1, 1)], [(0, 2, 2), (1, 1, 1)], [(True, 2, 2), (1, 1, 1)], [(1, 2, 2), (1, 1, 2)], 'mm', 3,
                [(), ()]):
        with pytest.raises(ValueError):
            tr.Register(mode='affine', levels=2, shrink=bad)
        if not isinstance(bad, (str, int)):
            with pytest.raises(ValueError):
                tr.Register(mode='rigid', levels=2, device_loop=True, shrink=good, moving_shrink=bad, **mi)
    for bad in ([1.0], [1.0, 0.0, 0.0], [(-1.0, 0, 0), 0.0], [float("inf"), 0.0], 1.0):
        with pytest.raises(ValueError):
            tr.Register(mode='affine', levels=2, shrink=good, smoothing=bad)
    with pytest.raises(ValueError, match="'voxel'"):
        tr.Register(mode='rigid', levels=2, device_loop=True, shrink='voxel', smoothing=[1.0, 0.0], **mi)
    # a schedule of its own for the moving image: only where the two images may lie on lattices of their own
    for kw in (dict(mode='affine'), dict(mode='rigid'), dict(mode='flow', flow_model='direct'), dict(mode='flow', flow_model='bspline'),
               dict(mode='flow', flow_model='bspline', diffeomorphic=True), dict(mode='flow', flow_model='direct', **mi)):
        with pytest.raises(ValueError, match="lattices of their own"):
            tr.Register(levels=2, shrink=good, moving_shrink=good, **kw)
    # ... and what is accepted
    tr.Register(mode='affine', levels=2, shrink=good)
    tr.Register(mode='flow', flow_model='direct', levels=2, shrink=[2, 1], smoothing=[1.0, 0.0])
    tr.Register(mode='affine', levels=2, shrink=[2, 1], smoothing=[(1.0, 1.0, 1.0), (0, 0, 0)])      # bare factors: the sigmas' length waits for optim
    with pytest.raises(ValueError):
        tr.Register(mode='affine', levels=2, shrink=[(2, 2, 2), (1, 1, 1)], smoothing=[(1.0, 1.0), (0, 0)])
    tr.Register(mode='rigid', levels=2, device_loop=True, shrink=good, moving_shrink=[(2, 2, 2), (1, 1, 1)], **mi)
    tr.Register(mode='flow', flow_model='bspline', levels=2, shrink=good, moving_smoothing=[0.5, 0.0], **mi)
    reg = tr.Register(mode='rigid', levels=3, device_loop=True, shrink='voxel', **mi)
    assert reg.level_schedule is None and reg.shrink == 'voxel'
    assert tr.Register().shrink is None


def test_register_optim_refusals_before_any_device_work():
    """shrink='voxel' without voxel sizes for both images, and a moving schedule in flow mode without initial=: ValueError on CPU tensors, i.e. before the
    first call that would need the GPU."""
    import torchregister_amd as tr
    mi = dict(criterion=[tr.MILoss()], weight=[1.0])
    x = torch.zeros(1, 1, 16, 16, 16)
    with pytest.raises(ValueError, match="shrink='voxel'"):
        tr.Register(mode='rigid', levels=2, device_loop=True, shrink='voxel', **mi).optim(x, x)
    with pytest.raises(ValueError, match=r"initial="):
        tr.Register(mode='flow', flow_model='bspline', levels=2, shrink=[(1, 2, 2), (1, 1, 1)], moving_shrink=[(2, 2, 2), (1, 1, 1)], **mi).optim(x, x)
    with pytest.raises(ValueError):      # the factors against the images' number of axes
        tr.Register(mode='affine', levels=2, shrink=[(2, 2), (1, 1)]).optim(x, x)
    with pytest.raises(ValueError):      # ... and the sigmas that came with bare factors
        tr.Register(mode='affine', levels=2, shrink=[2, 1], smoothing=[(1.0, 1.0), (0, 0)]).optim(x, x)
    bad = torch.eye(4, dtype=torch.float64)[:3]      # a malformed header under shrink='voxel': the headers' own ValueError, not a reshape error
    with pytest.raises(ValueError):
        tr.Register(mode='rigid', levels=2, device_loop=True, shrink='voxel', **mi).optim(x, x, moving_affine=bad, target_affine=torch.eye(4, dtype=torch.float64))


def test_python_refusals_on_cpu_tensors():
    import torchregister_amd as tr
    from torchregister_amd import _lib
    x = torch.zeros(1, 1, 4, 5, 6)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        tr.gaussian_smooth(x, 1.0)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        tr.gaussian_resample(x, (2, 3, 4), 1.0)
    for bad in (-1.0, float("nan"), (1.0, 1.0)):
        with pytest.raises(ValueError):
            tr.gaussian_smooth(x, bad)
    with pytest.raises(ValueError):
        tr.gaussian_smooth(x, 1.0, voxel=(1.0, 0.0, 1.0))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ptr = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
    inf, nan = float("inf"), float("nan")
    q = lib.trx_gaussian_workspace_bytes
    n = q(3, 2, 9, 13, 70, 9, 13, 70)
    assert n == (16384 + 16380) * 4      # two volumes, two same-size intermediates of 8190 floats each; the second pair starts on a 256-byte boundary
    assert q(2, 3, 1, 33, 130, 1, 33, 130) == -(-3 * 33 * 130 // 64) * 64 * 4      # 2-D: one intermediate
    assert q(3, 1, 5, 6, 7, 5, 6, 7) >= lib.trx_resample_workspace_bytes(3, 1, 5, 6, 7, 5, 6, 7)

    def call(src=4096, dst=8192, ndim=3, N=2, dhw=(9, 13, 70), out=(9, 13, 70), sigma=(1.0, 1.0, 1.0), truncate=4.0, align=0, padding=1, ws=4096, nbytes=n):
        s = None if sigma is None else (ctypes.c_float * len(sigma))(*sigma)
        return lib.trx_gaussian_resample(ptr(src), ptr(dst), ndim, N, *dhw, *out, s, truncate, align, padding, ptr(ws), nbytes, None)

    assert call(src=None) == ARG and call(dst=None) == ARG and call(ws=None) == ARG and call(sigma=None) == ARG
    for bad, want in ((dict(ndim=1), NDIM), (dict(ndim=4), NDIM), (dict(ndim=2), NDIM), (dict(N=0), ARG), (dict(dhw=(0, 13, 70)), ARG),
                      (dict(out=(9, 0, 70)), ARG), (dict(out=(9, 13, -1)), ARG), (dict(dhw=(2048, 1024, 1024)), ARG), (dict(out=(2048, 1024, 1024)), ARG)):
        assert call(**bad) == want, bad
        assert q(bad.get("ndim", 3), bad.get("N", 2), *bad.get("dhw", (9, 13, 70)), *bad.get("out", (9, 13, 70))) == 0
    for bad in ((-1.0, 1.0, 1.0), (1.0, nan, 1.0), (1.0, 1.0, inf), (1.0, -inf, 1.0)):
        assert call(sigma=bad) == ARG, bad
    for bad in (0.0, -4.0, nan, inf):
        assert call(truncate=bad) == ARG, bad
    assert call(align=2) == ARG and call(align=-1) == ARG and call(padding=2) == ARG and call(padding=-1) == ARG
    # the cap: R = 128 (sigma 32 at truncate 4) is taken - the call goes on to the workspace check -, R = 129 is not
    assert call(sigma=(32.0, 0.0, 0.0), nbytes=n - 1) == WS
    assert call(sigma=(0.0, 32.2, 0.0)) == ARG and call(sigma=(0.0, 0.0, 1000.0)) == ARG and call(sigma=(1.0, 1.0, 16.0), truncate=8.1) == ARG
    # one byte short is refused whatever the sigmas (even where no pass would run)
    assert call(nbytes=n - 1) == WS and call(nbytes=0) == WS and call(sigma=(0.0, 0.0, 0.0), nbytes=n - 1) == WS
    assert call(ndim=2, N=3, dhw=(1, 33, 130), out=(1, 33, 130), sigma=(1.0, -1.0), nbytes=n) == ARG      # only ndim sigmas are read ...
    assert call(ndim=2, N=3, dhw=(1, 33, 130), out=(1, 33, 130), sigma=(1.0, 1.0), nbytes=q(2, 3, 1, 33, 130, 1, 33, 130) - 1) == WS


def test_c_abi_refusals_without_a_device():
    check_refusals()
