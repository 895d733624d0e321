"""Randomised parity sweeps of the operators that came after the first fuzz suite (tests/fuzz_ops.py): one test per family runs the family's pinned
(cases, seed) of tests/fuzz_ops_cases.py::PINNED - tests/test_fuzz_ops_host.py asserts that these draws select every class that matters (2-D, an axis of
one voxel, rows of one and of two waves, a strided axis beyond 256, a sub-box beyond 256, chunk seams, batches with and without an empty pair, every
interpolation order, padding and chain order) - through the public wrappers against the restatements under tests/, with the bars of the fixed-shape
tests.  The full sweeps (300 cases per family, `python tests/fuzz_ops.py all 300 <seed>`) are recorded in profiles/fuzz_ops.txt.
The times are those of one run on the MI355X, arbiter included."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _run(family):
    import fuzz_ops
    import fuzz_ops_cases as fc
    n, seed = fc.PINNED[family]
    fails, worst = fuzz_ops.RUN[family](n, seed, verbose=True)
    assert fails == 0, worst


def test_sweep_distance_transform():
    """32 cases: squared distance and nearest feature, with and without voxel sizes; masks of one voxel, 0.2 / 5 / 50 % and sub-boxes (a quarter beyond index 256 of an axis of 260 .. 330), different kinds per pair, empty pairs.  0.7 - 2.2 s."""
    _run("distance")


def test_sweep_mask_surface():
    """24 cases, equality with distance_ref.surface.  0.01 s."""
    _run("surface")


def test_sweep_label_overlap():
    """24 cases: L from {1, 2, 5, 255, 256, 257, 4096}, uint8 and int32, values >= L and negative ones, maps of long runs; equality with numpy's counts.  0.2 s."""
    _run("overlap")


def test_sweep_moments():
    """24 cases: the raw order-2 sums with and without offset, masked and not, their order-1 columns against trx_image_moments bit for bit, image_covariance and image_moments.  0.3 - 0.4 s."""
    _run("moments")


def test_sweep_compose_flows():
    """24 cases, both paddings.  0.6 s."""
    _run("compose")


def test_sweep_invert_flow():
    """24 cases at the fixed count of 12 updates, fields scaled to a Lipschitz bound of 0.8.  1.2 - 1.5 s."""
    _run("invert")


def test_sweep_jacobian_and_folding_penalty():
    """24 cases: the map, the penalty per pair, its gradient against autograd on every voxel.  0.4 s."""
    _run("jacobian")


def test_sweep_prefilter_and_resample():
    """24 cases: spline_coefficients, and resample nearest / linear / cubic through theta, a flow, both, unequal lattices, a world scale.  0.9 - 1.2 s."""
    _run("spline")


def test_sweep_points_and_images_through_the_chain():
    """24 cases: transform_points (the drawn chain order, both paddings) and resample_affine_then_flow (the drawn order and padding).  0.7 - 1.7 s."""
    _run("chain")


def test_sweep_svf_exp_and_adjoint():
    """12 cases: svf_exp forward or inverse with 1 .. 7 squarings, the adjoint's elements and two directions (of twelve candidates) of the directional identity.  1.4 - 2.6 s."""
    _run("svf")


def test_sweep_bspline_expand_reduce_bending():
    """24 cases: expand with and without base, reduce, bending energy and gradient; spacings 1 .. 9 per axis, also larger than the axis.  0.6 s."""
    _run("bspline")


def test_sweep_pyramid_resampler():
    """24 cases: resample to sizes that shrink, keep or grow each axis on its own, the levels of pyramid(), upsample_flow.  0.1 s."""
    _run("pyramid")


# ---------------------------------------------------------------------------------------------------------------------------------------
# cases the 300-case sweeps (profiles/fuzz_ops.txt) found above the fixed-shape bars, pinned with their analysis and the multiple of the restatement's own
# fp32 - fp64 gap that they stand at
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_pinned_chain_seed2025_case278():
    """`python tests/fuzz_ops.py chain 300 2025`, case 278: a linear image from a (14, 5, 270) source onto (18, 4, 30), zeros padding.  The GPU image is
    1.504e-5 from the fp64 restatement against the sweep's bar of 1.390e-5 = twice the restatement's own fp32 - fp64 gap (6.95e-6): 2.16 x that gap, the
    one case of 188 interpolated ones over the bar.  Analysis in fp64 on the CPU (tests/test_fuzz_ops_host.py holds it): along the axis of 270 voxels an
    fp32 coordinate has a spacing of 3.05e-5, the restatement's own fp32 positions are up to 4.6e-5 voxels from the fp64 ones, and the steepest neighbour
    difference of the image is 0.30 - 1.4e-5 of value from the position's rounding alone, whatever samples at it; the kernel's coordinate arithmetic
    rounds in another order than the restatement's.  The sweep keeps its bar and reports the case; this test holds it to 2.5 x the restatement's own
    gap (the factor tests/test_gpu_fuzz_pinned.py gives a kernel that sums in another order than its specification), and everything else of the case
    to the sweep's bars."""
    import fuzz_ops
    det = []
    fuzz_ops.run_chain(279, 2025, verbose=True, only=278, details=det)
    assert len(det) == 1 and det[0]["rec"]["src_shape"] == (14, 5, 270) and det[0]["rec"]["order"] == 1, det
    f = det[0]["figures"]
    print(f, det[0]["messages"])
    assert all(m.startswith("image order 1") and "bar" in m for m in det[0]["messages"]), det      # points, the field of view: the sweep's bars
    assert f["image_err"] <= 2.5 * f["image_fp32_gap"], f


def test_pinned_svf_seed2025_case29():
    """`python tests/fuzz_ops.py svf 300 2025`, case 29 (the worst of five: 7, 29, 73, 102, 290): a (65, 2) field, 7 squarings, the inverse.  The
    directional identity <dvel, d> = <dflow, d exp / d eps> missed 1e-4 relative by 2.06e-4 while not one element of the adjoint was beyond its bar.
    Analysis in fp64 on the CPU: the sum <dvel, d> = -1.7e-5 cancels, and the restatement's own fp32 adjoint misses the same identity by 1.07e-4 (1.21e-4,
    1.45e-4, 1.63e-4, 1.21e-4 in the other four, where the GPU's miss equals the restatement's to three digits) while its fp64 adjoint meets it to 1e-7:
    the miss is what fp32 makes of the sum, not the adjoint's formula.  The sweep's bar since: 1e-4 or twice the restatement's own fp32 - fp64 gap of the
    sum.  The case holds it at 1.9 x that gap."""
    import fuzz_ops
    det = []
    fails, _ = fuzz_ops.run_svf(30, 2025, verbose=True, only=29, details=det)
    assert len(det) == 1 and det[0]["rec"]["shape"] == (65, 2) and det[0]["rec"]["K"] == 7, det
    dirs = det[0]["figures"]["directional"]
    print(dirs)
    assert fails == 0, det
    assert max(d["restatement_fp32_miss"] for d in dirs) > 1e-4, dirs      # the restatement in fp32 does not meet 1e-4 either
    assert all(d["miss"] <= max(1e-4, 2.0 * d["restatement_fp32_miss"]) for d in dirs), dirs
