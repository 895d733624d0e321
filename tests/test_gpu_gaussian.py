"""trx_gaussian_resample on the GPU against its fp64 restatement (tests/gaussian_ref.py), and the Python layer on top of it: gaussian_smooth in
millimetres and under autograd, pyramid / pyramid_masks under a schedule.  The bar of every comparison is conftest.bar(ref32, ref64, floor) with
floor = 2^-22 max|x|; each case prints its error and its bar."""
import functools

import numpy as np
import pytest
import torch

import gaussian_ref as gr
from conftest import bar
from test_gaussian_host import check_refusals

pytestmark = pytest.mark.gpu

# (name, tensor shape, output size or None = same size, sigma per spatial axis, align_corners)
CASES = {
    "row_crosses_a_wave": ((1, 1, 9, 13, 70), None, (0.6, 1.7, 3.2), False),            # R = 13 on x
    "radius_beyond_the_axis": ((1, 1, 9, 13, 70), None, (4.0, 0.0, 0.0), False),        # R = 16 > 9: every tap clamps; two axes without a pass
    "axis_of_one_voxel": ((1, 1, 1, 17, 66), None, (2.0, 1.0, 1.0), False),             # border: identity along it; zeros: the centre weight
    "two_d_six_volumes": ((2, 3, 33, 130), None, (1.5, 2.5), False),                    # more than two waves per row
    "shrink_false": ((1, 1, 20, 45, 67), (20, 15, 17), (0.0, 1.5, 2.0), False),         # integer and non-integer ratios, a shrink with smoothing
    "shrink_true": ((1, 1, 20, 45, 67), (20, 15, 17), (0.0, 1.5, 2.0), True),
    "grow_keep_shrink": ((1, 1, 9, 13, 70), (12, 13, 35), (0.0, 0.0, 1.0), False),
    "halo_longer_than_a_wave": ((1, 1, 8, 8, 300), None, (0.0, 0.0, 20.0), False),      # R = 80, several staged runs per row
    "ring_beyond_48_kib": ((1, 1, 300, 8, 64), None, (24.0, 0.0, 0.0), False),          # R = 96 along z: a ring of 202 rows, 51 712 bytes of LDS per wave
    "largest_radius": ((1, 1, 8, 300, 70), None, (0.0, 32.0, 0.0), False),              # R = 128 along y, the cap: 266 rows, 68 096 bytes
}


@functools.lru_cache(maxsize=None)
def volume(shape, seed=7):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, padding):
    """(ref64, bar) of a case: computed once, shared, never written to."""
    shape, size, sigma, align = CASES[name]
    x = volume(shape)
    size = tuple(shape[2:]) if size is None else size
    sig = [float(np.float32(s)) for s in sigma]      # what the C ABI receives
    r64 = gr.gaussian_resample(x, size, sig, align_corners=align, padding=padding)
    r32 = gr.gaussian_resample(x, size, sig, align_corners=align, padding=padding, fp32=True)
    r64.setflags(write=False)
    return r64, bar(r32, r64, gr.floor(x))


@pytest.mark.parametrize("padding", ["border", "zeros"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_restatement(name, padding):
    import torchregister_amd as tr
    shape, size, sigma, align = CASES[name]
    x = torch.from_numpy(volume(shape)).cuda()
    size = tuple(shape[2:]) if size is None else size
    want, tol = reference(name, padding)
    got = tr.gaussian_resample(x, size, sigma, align_corners=align, padding=padding)
    again = tr.gaussian_resample(x, size, sigma, align_corners=align, padding=padding)
    assert tuple(got.shape) == tuple(shape[:2]) + size and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"{name} {padding}: max |kernel - restatement| = {err:.3e}, bar {tol:.3e}")
    assert err <= tol
    assert torch.equal(got, again)      # the same bits on every call


def test_axis_of_one_voxel_border_is_the_identity_along_it():
    """Along an axis of one voxel every tap clamps onto that voxel: border padding gives x sum(g) - the identity up to the rounding of the fp32 taps' sum,
    inside the bar -, zeros padding leaves the centre tap alone: x g_R, one rounding."""
    import torchregister_amd as tr
    xn = volume((1, 1, 1, 17, 66))
    x = torch.from_numpy(xn).cuda()
    r32 = gr.gaussian_resample(xn, xn.shape[2:], (2.0, 0.0, 0.0), fp32=True)
    tol = bar(r32, xn, gr.floor(xn))
    err = float((tr.gaussian_smooth(x, (2.0, 0.0, 0.0)) - x).abs().max())
    print(f"axis of one voxel, border: max |G x - x| = {err:.3e}, bar {tol:.3e}")
    assert err <= tol
    R, g = gr.taps(2.0)
    got = tr.gaussian_smooth(x, (2.0, 0.0, 0.0), padding='zeros')
    assert torch.equal(got, x * float(np.float32(g[R])))      # one in-range tap: the centre weight, one rounding


def test_a_volume_does_not_depend_on_its_batch_2d():
    import torchregister_amd as tr
    x = torch.from_numpy(volume((2, 3, 33, 130))).cuda()
    for padding in ("border", "zeros"):
        full = tr.gaussian_smooth(x, (1.5, 2.5), padding=padding)
        alone = tr.gaussian_smooth(x[1:2, 2:3].contiguous(), (1.5, 2.5), padding=padding)
        assert torch.equal(full[1:2, 2:3], alone)


def test_several_rounds_of_chunks_give_each_volume_its_own_bits():
    """Eight volumes of 160^3: two same-size intermediates of 16 MB each per volume against a chunk of 96 MiB - the call runs in three rounds."""
    import torchregister_amd as tr
    x = torch.randn((8, 1, 160, 160, 160), device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    full = tr.gaussian_smooth(x, 0.5)
    assert not torch.equal(full, x)
    for v in range(8):
        assert torch.equal(full[v:v + 1], tr.gaussian_smooth(x[v:v + 1], 0.5)), v


def test_no_pass_is_a_copy_and_small_sigma_is_the_identity():
    import torchregister_amd as tr
    x = torch.from_numpy(volume((1, 1, 9, 13, 70))).cuda()
    for sigma in (0.0, 0.1):      # R = (int)(0.4 + 0.5) = 0
        got = tr.gaussian_smooth(x, sigma)
        assert torch.equal(got, x) and got.data_ptr() != x.data_ptr()


def test_sigma_in_millimetres():
    import torchregister_amd as tr
    x = torch.from_numpy(volume((1, 1, 9, 13, 70))).cuda()
    assert torch.equal(tr.gaussian_smooth(x, 2.1, voxel=(3.0, 0.7, 0.7)), tr.gaussian_smooth(x, (0.7, 3.0, 3.0)))
    assert torch.equal(tr.gaussian_smooth(x, (3.0, 1.4, 0.7), voxel=(3.0, 0.7, 0.7)), tr.gaussian_smooth(x, (1.0, 2.0, 1.0)))


def test_zeros_padding_is_its_own_adjoint():
    """<G x, y> = <x, G y> in fp64 sums.  Each element of G x and G y is within its bar e of the exact value, and the exact operator is symmetric, so the
    two sums differ by at most e_x sum|y| + e_y sum|x|."""
    import torchregister_amd as tr
    shape, sigma = (1, 1, 9, 13, 70), (0.6, 1.7, 3.2)
    xn, yn = volume(shape), volume(shape, seed=8)
    x, y = torch.from_numpy(xn).cuda(), torch.from_numpy(yn).cuda()
    gx, gy = tr.gaussian_smooth(x, sigma, padding='zeros'), tr.gaussian_smooth(y, sigma, padding='zeros')
    sig = [float(np.float32(s)) for s in sigma]
    tol = 0.0
    for a, b in ((xn, yn), (yn, xn)):
        r64 = gr.gaussian_resample(a, shape[2:], sig, padding='zeros')
        r32 = gr.gaussian_resample(a, shape[2:], sig, padding='zeros', fp32=True)
        tol += bar(r32, r64, gr.floor(a)) * float(np.abs(b.astype(np.float64)).sum())
    lhs, rhs = float((gx.double() * y.double()).sum()), float((x.double() * gy.double()).sum())
    print(f"<Gx, y> = {lhs:.9f}, <x, Gy> = {rhs:.9f}, difference {abs(lhs - rhs):.3e}, bar {tol:.3e}")
    assert abs(lhs - rhs) <= tol


def test_autograd_through_zeros_padding_and_border_refusal():
    import torchregister_amd as tr
    shape, sigma = (1, 1, 9, 13, 70), (0.6, 1.7, 3.2)
    x = torch.from_numpy(volume(shape)).cuda().requires_grad_(True)
    w = torch.from_numpy(volume(shape, seed=9)).cuda()
    out = tr.gaussian_smooth(x, sigma, padding='zeros')
    assert out.requires_grad and torch.equal(out.detach(), tr.gaussian_smooth(x.detach(), sigma, padding='zeros'))
    grad, = torch.autograd.grad(out, x, grad_outputs=w)
    assert torch.equal(grad, tr.gaussian_smooth(w, sigma, padding='zeros'))
    with pytest.raises(ValueError, match="padding='zeros'"):
        tr.gaussian_smooth(x, sigma)
    assert not tr.gaussian_smooth(x.detach(), sigma).requires_grad


def test_pyramid_under_a_schedule():
    import torchregister_amd as tr
    from torchregister_amd.pyramid import resample
    x = torch.from_numpy(volume((1, 2, 12, 40, 46))).cuda()
    shrink = [(1, 4, 4), (1, 2, 2), (1, 1, 1)]
    sigma = [(0.0, 2.0, 2.0), (0.0, 0.7, 1.3), (0.0, 0.0, 0.0)]
    for align in (False, True):
        levels = tr.pyramid(x, 3, align_corners=align, shrink=shrink, sigma=sigma)
        assert [tuple(l.shape[2:]) for l in levels] == [(12, 10, 12), (12, 20, 23), (12, 40, 46)]      # ceil(S / f)
        for lvl, sg in zip(levels[:2], sigma):
            assert torch.equal(lvl, tr.gaussian_resample(x, lvl.shape[2:], sg, align_corners=align))      # of x, not of the level above
        assert levels[2].data_ptr() == x.data_ptr()
    default = tr.pyramid(x, 3, shrink=shrink)      # sigma None: f / 2 where f > 1
    assert torch.equal(default[0], tr.gaussian_resample(x, (12, 10, 12), (0.0, 2.0, 2.0)))
    assert torch.equal(default[1], tr.gaussian_resample(x, (12, 20, 23), (0.0, 1.0, 1.0)))
    smoothed_finest = tr.pyramid(x, 2, shrink=[(1, 2, 2), (1, 1, 1)], sigma=[(0, 1, 1), (0, 0.5, 0.5)])[1]
    assert torch.equal(smoothed_finest, tr.gaussian_smooth(x, (0, 0.5, 0.5))) and not torch.equal(smoothed_finest, x)
    # without a schedule: today's statements
    today = [x]
    for s in tr.pyramid_shapes(x.shape[2:], 3)[-2::-1]:
        today.append(resample(today[-1], s, False))
    for a, b in zip(tr.pyramid(x, 3), today[::-1]):
        assert torch.equal(a, b)
    for bad in (dict(sigma=[1.0, 0.0, 0.0]), dict(shrink=shrink[:2]), dict(shrink=[(1, 4, 4), (1, 2, 2), (1, 1, 2)]), dict(shrink=[(1, 4), (1, 2), (1, 1)])):
        with pytest.raises(ValueError):
            tr.pyramid(x, 3, **bad)


def test_pyramid_masks_under_a_schedule():
    import torchregister_amd as tr
    shape, shrink = (12, 40, 44), [(1, 4, 4), (1, 2, 2), (1, 1, 1)]
    m = np.zeros((1, 1) + shape, dtype=np.float32)
    m[0, 0, 2:10, 8:32, 8:32] = 1      # the box's faces lie two input voxels from the nearest sample of either level
    sigma = [(0.0, 2.0, 2.0), (0.0, 1.0, 1.0), (0.0, 0.0, 0.0)]
    sizes = [(12, 10, 11), (12, 20, 22), shape]
    want = []
    for size, sg in zip(sizes, sigma):
        r64 = gr.gaussian_resample(m, size, sg)
        r32 = gr.gaussian_resample(m, size, sg, fp32=True)
        tol = bar(r32, r64, gr.floor(m))
        gap = float(np.abs(r64 - 0.5).min())
        print(f"level {size}: nearest value to 0.5 is {gap:.3f} away, bar {tol:.3e}")
        assert gap > tol      # the threshold cannot flip within the kernel's error
        want.append(r64 >= 0.5)
    got = tr.pyramid_masks(torch.from_numpy(m).cuda() * 3, 3, shrink=shrink)      # any non-zero value counts
    for g, w in zip(got, want):
        assert g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy().astype(bool), w)
    assert 0 < int(got[0].sum()) < got[0].numel()
    with pytest.raises(ValueError, match="no voxel left at level 1"):
        tiny = torch.zeros((1, 1) + shape, device="cuda")
        tiny[0, 0, 5, 20, 20] = 1
        tr.pyramid_masks(tiny, 3, shrink=shrink)


def test_c_abi_refusals_on_the_gpu_box():
    check_refusals()
