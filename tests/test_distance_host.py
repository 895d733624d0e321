"""CPU-only checks of the distance transform, the mask surface and the overlap counts: the restatement tests/distance_ref.py
against a brute force and, where it is installed, scipy.ndimage; what the GPU tests of tests/test_gpu_distance.py rest on; every refusal of the C ABI
without a device; the Python interface's ValueErrors on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import distance_ref as dr

OK, ARG, NDIM, WS = 0, -1, -2, -3


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES[:dr.BRUTE], ids=dr.case_id)
def test_restatement_is_the_brute_force(case):
    """Separable min-plus == the minimum over every feature: equal integers without voxel sizes, within 1e-12 relative in fp64 with them; an empty pair is
    'no feature' everywhere."""
    r, voxel = dr.reference(case), case[3]
    for b in range(case[1]):
        want = dr.brute(r["mask"][b], voxel)
        if voxel is None:
            assert np.array_equal(r["int"][b], want)
        elif not r["mask"][b].any():
            assert np.isinf(r["f64"][b]).all() and np.isinf(want).all()
        else:
            assert np.abs(r["f64"][b] - want).max() <= 1e-12 * want.max()


@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_restatement_against_scipy(case):
    """distance_transform_edt of the complement (it measures to the nearest ZERO) and mask & ~binary_erosion(border_value=0) on every case; scipy defines
    nothing for a mask without a feature, that pair is left to the brute force."""
    ndi = pytest.importorskip("scipy.ndimage")
    r, voxel = dr.reference(case), case[3]
    nd = len(case[2])
    for b in range(case[1]):
        m = r["mask"][b] != 0
        eroded = ndi.binary_erosion(m, structure=ndi.generate_binary_structure(nd, 1), border_value=0)
        assert np.array_equal(r["surface"][b] != 0, m & ~eroded)
        if not m.any():
            continue
        want = ndi.distance_transform_edt(~m, sampling=None if voxel is None else [float(np.float32(v)) for v in voxel]) ** 2
        got = (r["int"] if voxel is None else r["f64"])[b].astype(np.float64)
        assert np.abs(got - want).max() <= 1e-9 * max(1.0, want.max())


def test_cases_hold_what_the_gpu_tests_need():
    """The properties the shapes were chosen for: a row that crosses a wave, an axis of one voxel, a reach of 129 on a strided axis, more than one block per
    pass, every voxel a candidate, integers below 2^24, the shell of the full mask, and a dilation radius no rounding decides."""
    by = {c[0]: c for c in dr.CASES}
    assert by["one-voxel-axis"][2][1] == 1 and by["one-voxel-axis"][2][2] > 64 and by["row-ends"][2][2] > 128
    far = dr.reference(by["far-on-z"])["int"]
    assert far.max() >= 129 ** 2 and len(np.unique(far[0, :, 0, 0])) == 130      # every z of a column leaves the search at another step
    assert all(dr.reference(c)["int"].max() < 2 ** 24 for c in dr.CASES if c[3] is None)
    assert dr.reference(by["checkerboard"])["int"].max() == 1
    s = dr.reference(by["full"])["surface"][0]
    shell = np.ones_like(s)
    shell[1:-1, 1:-1, 1:-1] = 0
    assert np.array_equal(s, shell)
    ball = dr.reference(by["ball"])
    assert dr.between_attainable(ball["int"], 2.5) and dr.between_attainable(dr.dist2(1 - ball["mask"]), 2.5)
    aniso = dr.reference(by["aniso-and-empty"])
    assert not aniso["mask"][1].any() and 10 <= aniso["mask"][0].sum() <= 100


def test_overlap_and_surface_metrics_of_the_restatement():
    a, b = dr.label_maps(2, (9, 10, 11), 5, np.int32, 3)
    c = dr.overlap_counts(a, b, 5)
    assert (a < 0).any() and (a >= 5).any() and c[:, 4].sum() == 0 and np.isnan(dr.dice(c)[:, 4]).all()
    assert c[0, 2, 0] == (a[0] == 2).sum() and c[1, 3, 2] == ((a[1] == 3) & (b[1] == 3)).sum()
    assert np.array_equal(dr.dice(dr.overlap_counts(a, a, 5))[:, :4], np.ones((2, 4)))
    m = dr.ball((9, 10, 11), radius=3.0)
    same = dr.surface_metrics(m, m)
    assert same["hausdorff"] == 0 and same["assd"] == 0 and same["n_a"] == same["n_b"] > 0
    shifted = dr.surface_metrics(m, np.roll(m, 2, axis=2))
    assert shifted["hausdorff"] == 2.0 and 0 < shifted["assd"] < 2.0 and shifted["hd_percentile"] <= 2.0
    assert np.isnan(dr.surface_metrics(m, np.zeros_like(m))["hausdorff"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ptr = lambda p: P(p) if p else None  # noqa: E731
    inf, nan = float("inf"), float("nan")
    assert lib.trx_version() == 240

    q = lib.trx_distance_workspace_bytes
    n = q(3, 2, 5, 6, 7)
    # 2 x 210 voxels: 1680 bytes of values, two int16 maps of 840 bytes, 60 row bytes and 10 plane bytes, each part rounded up to 256
    assert n == 1792 + 2 * 1024 + 256 + 256
    assert q(2, 1, 1, 19, 26) == 2048 + 1024 + 256 + 256      # 494 voxels: 1976 bytes of values, ONE int16 map of 988 bytes, 19 row bytes, 1 plane byte
    assert q(3, 1, 33, 65, 70) == -(-150150 * 4 // 256) * 256 + 2 * (-(-150150 * 2 // 256) * 256) + -(-33 * 65 // 256) * 256 + 256

    def dt(mask=4096, ndim=3, B=2, dhw=(5, 6, 7), voxel=None, dist2=4096, nearest=4096, ws=4096, nbytes=n):
        v = None if voxel is None else (ctypes.c_float * len(voxel))(*voxel)
        return lib.trx_distance_transform(ptr(mask), ndim, B, *dhw, v, ptr(dist2), ptr(nearest), ptr(ws), nbytes, None)

    def surf(mask=4096, ndim=3, B=2, dhw=(5, 6, 7), surface=4096):
        return lib.trx_mask_surface(ptr(mask), ndim, B, *dhw, ptr(surface), None)

    def over(a=4096, b=4096, label_bytes=1, ndim=3, B=2, dhw=(5, 6, 7), L=5, counts=4096):
        return lib.trx_label_overlap(ptr(a), ptr(b), label_bytes, ndim, B, *dhw, L, ptr(counts), None)

    assert dt(mask=None) == ARG and dt(dist2=None) == ARG and dt(ws=None) == ARG
    assert surf(mask=None) == ARG and surf(surface=None) == ARG
    assert over(a=None) == ARG and over(b=None) == ARG and over(counts=None) == ARG
    for bad, want in ((dict(ndim=1), NDIM), (dict(ndim=4), NDIM), (dict(ndim=2), NDIM), (dict(B=0), ARG), (dict(B=65536), ARG), (dict(dhw=(0, 6, 7)), ARG),
                      (dict(dhw=(5, -1, 7)), ARG), (dict(dhw=(5, 6, 0)), ARG), (dict(dhw=(16385, 1, 1)), ARG), (dict(dhw=(1, 16385, 1)), ARG),
                      (dict(dhw=(1, 1, 16385)), ARG), (dict(dhw=(2048, 1024, 1024)), ARG), (dict(dhw=(8, 16384, 16384)), ARG)):
        assert dt(**bad) == want and surf(**bad) == want and over(**bad) == want, bad
        assert q(bad.get("ndim", 3), bad.get("B", 2), *bad.get("dhw", (5, 6, 7))) == 0
    assert q(3, 1, 7, 16384, 16384) > 0      # the largest sizes and just under 2^31 voxels are no refusal
    for bad in ((nan, 1.0, 1.0), (1.0, inf, 1.0), (1.0, 1.0, -inf), (0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, -0.0)):
        assert dt(voxel=bad) == ARG, bad
    assert dt(ndim=2, B=1, dhw=(1, 19, 26), voxel=(1.0, 0.0), nbytes=q(2, 1, 1, 19, 26)) == ARG
    assert dt(ndim=2, B=1, dhw=(1, 19, 26), voxel=(1.0, 2.0), nbytes=q(2, 1, 1, 19, 26) - 1) == WS      # only ndim sizes are read
    assert dt(nbytes=n - 1) == WS and dt(nbytes=0) == WS and dt(voxel=(3.0, 0.7, 0.9), nbytes=n - 1) == WS
    assert dt(nearest=None, nbytes=n - 1) == WS      # a nullable nearest is no refusal, and it does not shrink the workspace
    for bad in (dict(L=0), dict(L=-1), dict(L=4097), dict(label_bytes=0), dict(label_bytes=2), dict(label_bytes=8)):
        assert over(**bad) == ARG, bad


def test_c_abi_refusals_without_a_device():
    check_refusals()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python interface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_on_cpu_tensors():
    import torchregister_amd as tr
    from torchregister_amd import _lib
    good = torch.zeros(1, 1, 4, 5, 6)
    good[0, 0, 1, 2, 3] = 1
    masks = (tr.distance_transform, tr.signed_distance, tr.mask_surface, lambda m: tr.dilate_mask(m, 1.0), lambda m: tr.erode_mask(m, 1.0),
             lambda m: tr.surface_distances(m, m), lambda m: tr.label_overlap(m, m, 2))
    for fn in masks:
        for shape in ((4,), (4, 5), (1, 2, 3, 4, 5, 6), (1, 2, 4, 5, 6), (0, 1, 4, 5), (1, 1, 0, 5)):
            with pytest.raises(ValueError):
                fn(torch.zeros(shape))
        with pytest.raises(ValueError):
            fn(None)
    for voxel in ((1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0), "abc", 2.0):
        for fn in (tr.distance_transform, tr.signed_distance, lambda m, voxel: tr.dilate_mask(m, 1.0, voxel), lambda m, voxel: tr.erode_mask(m, 1.0, voxel),
                   lambda m, voxel: tr.surface_distances(m, m, voxel)):
            with pytest.raises(ValueError, match="voxel"):
                fn(good, voxel=voxel)
    for radius in (-1.0, -1e-9, float("nan"), float("inf"), "x", None, True):
        for fn in (tr.dilate_mask, tr.erode_mask):
            with pytest.raises(ValueError, match="radius"):
                fn(good, radius)
    for empty_or_full in (torch.zeros(1, 1, 4, 5, 6), torch.ones(1, 4, 5, 6), torch.cat([good, torch.zeros_like(good)])):
        with pytest.raises(ValueError, match="empty|full"):
            tr.signed_distance(empty_or_full)
    labels = torch.zeros(1, 4, 5, 6, dtype=torch.int32)
    for bad in (labels.float(), labels.double(), labels.half(), labels.bool()):
        with pytest.raises(ValueError, match="integer label map"):
            tr.label_overlap(bad, labels, 3)
        with pytest.raises(ValueError, match="integer label map"):
            tr.label_overlap(labels, bad, 3)
    with pytest.raises(ValueError, match="different shapes"):
        tr.label_overlap(labels, torch.zeros(1, 4, 5, 7, dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="different shapes"):
        tr.surface_distances(good, torch.zeros(1, 1, 4, 5, 7))
    for L in (0, 4097, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="labels"):
            tr.label_overlap(labels, labels, L)
    for pct in (-1.0, 100.5, "x", None):
        with pytest.raises(ValueError, match="percentile"):
            tr.surface_distances(good, good, percentile=pct)
    # with every argument in order the functions ask for GPU tensors: there is no CPU path
    for fn in (tr.distance_transform, tr.signed_distance, tr.mask_surface, lambda m: tr.dilate_mask(m, 1.0), lambda m: tr.erode_mask(m, 1.0),
               lambda m: tr.surface_distances(m, m), lambda m: tr.label_overlap(m.int(), m.int(), 2), lambda m: tr.distance_transform(m[:, 0], (1.0, 2.0, 3.0))):
        with pytest.raises(_lib.TrxError, match="no CPU fallback"):
            fn(good)
