"""The Euclidean distance transform, the mask surface, the overlap counts and what the host layer builds on them, on the GPU (trx_distance_transform,
trx_mask_surface, trx_label_overlap) against tests/distance_ref.py; tests/test_distance_host.py asserts what these tests rest
on.  The shapes are the smallest at which the passes can go wrong: a corner, an empty pair in a batch, a plane, an axis of one voxel, a row that crosses a
wave, several blocks per pass, the farthest reach on a strided axis."""
import numpy as np
import pytest
import torch

import distance_ref as dr
from conftest import bar
from test_distance_host import check_refusals

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _gpu(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the references are read-only


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the transform
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_squared_distance_and_nearest_feature(tr, case):
    """Without voxel sizes the squared distance is the int64 restatement cast to fp32, bit for bit; with them it is within the bar of the fp64 one.  0 on
    every feature.  A pair without a feature is +inf with nearest == -1.  nearest, without assuming a tie rule: in range, on a feature, and the distance
    recomputed from it is dist2 (equal integers / within the bar).  Two calls give equal bits; distance_transform(m) is the sqrt of the squared call."""
    name, B, sp, voxel = case
    r = dr.reference(case)
    m = _gpu(r["mask"])
    d2, idx = tr.distance_transform(m, voxel, squared=True, return_indices=True)
    assert d2.shape == (B, 1) + sp and d2.dtype == torch.float32 and idx.shape == (B, len(sp)) + sp and idx.dtype == torch.int32
    msgs = dr.check_transform(d2[:, 0].cpu().numpy(), idx.cpu().numpy(), r["mask"], voxel, r, report=lambda line: print(f"{name} {line}"))
    assert not msgs, msgs
    again, idx2 = tr.distance_transform(m, voxel, squared=True, return_indices=True)
    assert torch.equal(again, d2) and torch.equal(idx2, idx)
    assert torch.equal(tr.distance_transform(m, voxel, squared=True), d2)      # the bits do not depend on whether nearest is asked for
    assert torch.equal(tr.distance_transform(m[:, None].float() * 3.0, voxel), d2.sqrt())      # [B,1,*sp], any numeric dtype, non-zero = set


def test_a_pair_has_the_bits_of_the_pair_alone(tr):
    """The batch of an anisotropic random pair and an empty one: pair 0 has the bits of the same mask run alone, on both paths."""
    case = dr.CASES[1]
    m = _gpu(dr.reference(case)["mask"])
    for voxel in (case[3], None):
        both, ib = tr.distance_transform(m, voxel, squared=True, return_indices=True)
        alone, ia = tr.distance_transform(m[:1], voxel, squared=True, return_indices=True)
        assert torch.equal(both[:1], alone) and torch.equal(ib[:1], ia)
        assert bool(torch.isposinf(both[1]).all()) and bool((ib[1] == -1).all())
        flipped, _ = tr.distance_transform(m.flip(0), voxel, squared=True, return_indices=True)
        assert torch.equal(flipped[1:], alone) and bool(torch.isposinf(flipped[0]).all())


def test_workspace_is_exact_and_buffers_are_kept(tr):
    """The C entry point with dist2, nearest and a workspace of exactly trx_distance_workspace_bytes between canaries; one byte less is refused."""
    from test_gpu_bspline import _Guarded
    from torchregister_amd import _lib
    lib = _lib.load()
    case = dr.CASES[4]
    sp, n = case[2], int(np.prod(case[2]))
    m = _gpu(dr.reference(case)["mask"])
    want, want_idx = tr.distance_transform(m, squared=True, return_indices=True)
    nbytes = lib.trx_distance_workspace_bytes(3, 1, *sp)
    d2, idx, ws, surf = _Guarded(n * 4, 0x96), _Guarded(3 * n * 4, 0x3C), _Guarded(nbytes, 0x5A), _Guarded(n, 0xC3)
    stream = _lib.current_stream(torch.device("cuda"))
    run = lambda k: lib.trx_distance_transform(_lib.ptr(m), 3, 1, *sp, None, _lib.ptr(d2.region), _lib.ptr(idx.region), _lib.ptr(ws.region), k, stream)  # noqa: E731
    assert run(nbytes - 1) == -3
    _lib.check(run(nbytes), "trx_distance_transform")
    _lib.check(lib.trx_mask_surface(_lib.ptr(m), 3, 1, *sp, _lib.ptr(surf.region), stream), "trx_mask_surface")
    torch.cuda.synchronize()
    for buf, what in ((d2, "dist2"), (idx, "nearest"), (ws, "the workspace"), (surf, "surface")):
        buf.check(what)
    assert torch.equal(d2.floats((1, 1) + sp), want) and torch.equal(idx.region.view(torch.int32).reshape(want_idx.shape), want_idx)
    assert torch.equal(surf.region.reshape((1, 1) + sp), tr.mask_surface(m))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. the surface and the overlap counts
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dr.CASES, ids=dr.case_id)
def test_mask_surface(tr, case):
    """Equal to the restatement on every case (the full mask's surface is its outer shell: tests/test_distance_host.py)."""
    r = dr.reference(case)
    s = tr.mask_surface(_gpu(r["mask"]))
    assert s.dtype == torch.uint8 and s.shape == (case[1], 1) + case[2]
    assert torch.equal(s[:, 0].cpu(), torch.from_numpy(r["surface"].copy()))


@pytest.mark.parametrize("dtype", [np.uint8, np.int32], ids=["uint8", "int32"])
def test_label_overlap_counts(tr, dtype):
    """(2, 9, 10, 11), L = 5, values >= L and (int32) negative ones: counts equal numpy's, Dice = 2 |a and b| / (|a| + |b|), NaN for the label absent from
    both; int64 maps are cast and give the same counts."""
    a, b = dr.label_maps(2, (9, 10, 11), 5, dtype, 3)
    want = dr.overlap_counts(a, b, 5)
    assert (a >= 5).any() and (dtype == np.uint8 or (a < 0).any()) and want[:, 4].sum() == 0
    dice, counts = tr.label_overlap(_gpu(a), _gpu(b), 5)
    assert counts.dtype == torch.int64 and dice.dtype == torch.float64 and counts.shape == (2, 5, 3) and dice.shape == (2, 5)
    assert torch.equal(counts.cpu(), torch.from_numpy(want))
    d = dice.cpu().numpy()
    assert np.isnan(d[:, 4]).all() and np.array_equal(d[:, :4], dr.dice(want)[:, :4]) and (d[:, :4] > 0).all()
    _, c64 = tr.label_overlap(_gpu(a.astype(np.int64))[:, None], _gpu(b.astype(np.int64))[:, None], 5)
    _, again = tr.label_overlap(_gpu(a), _gpu(b), 5)
    assert torch.equal(c64, counts) and torch.equal(again, counts)


def test_label_overlap_with_the_largest_table(tr):
    """(1, 33, 65, 70), L = 4096: ten blocks add into one table of the largest LDS size."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 4200, size=(1, 33, 65, 70)).astype(np.int32)
    b = np.where(rng.random(a.shape) < 0.5, a, rng.integers(-5, 4200, size=a.shape)).astype(np.int32)
    want = dr.overlap_counts(a, b, 4096)
    _, counts = tr.label_overlap(_gpu(a), _gpu(b), 4096)
    assert torch.equal(counts.cpu(), torch.from_numpy(want)) and want[..., 2].sum() > 50000


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. what the host layer builds on them
# ---------------------------------------------------------------------------------------------------------------------------------------
def _check_metrics(got, p, w64, w32, what):
    for k in ("hausdorff", "hd_percentile", "assd"):
        g, bb = getattr(got, k)[p].item(), bar(w32[k], w64[k], 1e-6 * abs(w64[k]))
        print(f"{what} {k}: {g:.6f} against {w64[k]:.6f}, err {abs(g - w64[k]):.3e} bar {bb:.3e}")
        assert abs(g - w64[k]) <= bb
    assert got.n_a[p].item() == w64["n_a"] and got.n_b[p].item() == w64["n_b"]


def test_surface_distances(tr):
    """Two offset balls in (33, 65, 70) with voxel (2, 1, 1) and two random blobs in (9, 10, 11), in voxels: every field within 1e-6 relative of the
    restatement (bar() over the fp32 run of it); a mask against itself gives zeros; an empty mask gives NaN, also inside a batch."""
    sp, voxel = (33, 65, 70), (2.0, 1.0, 1.0)
    a, b = dr.ball(sp, (14, 30, 30), 9.0), dr.ball(sp, (17, 34, 37), 11.0)
    got = tr.surface_distances(_gpu(a[None].astype(np.uint8)), _gpu(b[None].astype(np.uint8)), voxel)
    assert all(t.dtype == torch.float64 and t.shape == (1,) for t in got[:3]) and got.n_a.dtype == torch.int64
    _check_metrics(got, 0, dr.surface_metrics(a, b, voxel), dr.surface_metrics(a, b, voxel, dtype=np.float32), "balls")
    sp = (9, 10, 11)
    c, d = dr.blobs(sp, 1), dr.blobs(sp, 2)
    batch_a = _gpu(np.stack([c, c, c]).astype(np.uint8))[:, None]
    batch_b = _gpu(np.stack([d, c, np.zeros_like(c)]).astype(np.uint8))[:, None]
    got = tr.surface_distances(batch_a, batch_b, percentile=95.0)
    _check_metrics(got, 0, dr.surface_metrics(c, d), dr.surface_metrics(c, d, dtype=np.float32), "blobs")
    assert got.hausdorff[1].item() == 0 and got.hd_percentile[1].item() == 0 and got.assd[1].item() == 0 and got.n_a[1].item() == got.n_b[1].item() > 0
    assert all(bool(torch.isnan(t[2])) for t in got[:3]) and got.n_b[2].item() == 0 and got.n_a[2].item() > 0
    med = tr.surface_distances(batch_a[:1], batch_b[:1], percentile=50.0)
    w = dr.surface_metrics(c, d, percentile=50.0)
    assert abs(med.hd_percentile[0].item() - w["hd_percentile"]) <= 1e-6 * w["hd_percentile"] and med.hausdorff[0].item() == got.hausdorff[0].item()


def test_dilate_and_erode(tr):
    """The ball grown and shrunk by 2.5 voxels, and by 2.5 mm at voxel (2, 1, 1): the thresholded restatement.  2.5 lies strictly between two attainable
    distances (asserted here and in tests/test_distance_host.py), so rounding decides nothing."""
    case = next(c for c in dr.CASES if c[0] == "ball")
    mask = dr.reference(case)["mask"]
    m = _gpu(mask)
    out2, in2 = dr.dist2(mask), dr.dist2(1 - mask)
    assert dr.between_attainable(out2, 2.5) and dr.between_attainable(in2, 2.5)
    grown, shrunk = tr.dilate_mask(m, 2.5), tr.erode_mask(m, 2.5)
    assert grown.dtype == torch.uint8 and grown.shape == (1, 1) + case[2]
    assert torch.equal(grown[:, 0].cpu(), torch.from_numpy((out2 <= 6.25).astype(np.uint8)))
    assert torch.equal(shrunk[:, 0].cpu(), torch.from_numpy((in2 > 6.25).astype(np.uint8)))
    assert mask.sum() < grown.sum().item() and 0 < shrunk.sum().item() < mask.sum()
    assert torch.equal(tr.dilate_mask(m, 0.0)[:, 0], m) and torch.equal(tr.erode_mask(m, 0.0)[:, 0], m)
    voxel = (2.0, 1.0, 1.0)
    out_mm, in_mm = dr.dist2(mask, voxel), dr.dist2(1 - mask, voxel)
    assert dr.between_attainable(out_mm, 2.5) and dr.between_attainable(in_mm, 2.5)
    assert torch.equal(tr.dilate_mask(m, 2.5, voxel)[:, 0].cpu(), torch.from_numpy((out_mm <= 6.25).astype(np.uint8)))
    assert torch.equal(tr.erode_mask(m, 2.5, voxel)[:, 0].cpu(), torch.from_numpy((in_mm > 6.25).astype(np.uint8)))


def test_signed_distance_of_a_ball(tr):
    """Positive outside, negative inside, never closer to zero than one voxel size, and the values of the two restated transforms; an empty or a full
    pair in the batch is a ValueError."""
    case = next(c for c in dr.CASES if c[0] == "ball")
    mask = dr.reference(case)["mask"]
    m = _gpu(mask)
    for voxel, least in ((None, 1.0), ((2.0, 0.5, 1.5), 0.5)):
        s = tr.signed_distance(m, voxel)
        assert s.shape == (1, 1) + case[2] and s.dtype == torch.float32
        got = s[:, 0].cpu().numpy().astype(np.float64)
        inside = mask != 0
        assert (got[inside] <= -least).all() and (got[~inside] >= least).all()
        if voxel is None:
            want = np.sqrt(dr.dist2(mask).astype(np.float64)) - np.sqrt(dr.dist2(1 - mask).astype(np.float64))
            floor = 1e-6 * np.abs(want).max()
        else:
            want = np.sqrt(dr.dist2(mask, voxel)) - np.sqrt(dr.dist2(1 - mask, voxel))
            w32 = np.sqrt(dr.dist2(mask, voxel, np.float32)) - np.sqrt(dr.dist2(1 - mask, voxel, np.float32))
            floor = bar(w32, want, 1e-6 * np.abs(want).max())
        e = np.abs(got - want).max()
        print(f"signed distance, voxel {voxel}: range {want.min():.3f} .. {want.max():.3f}, err {e:.3e} bar {floor:.3e}")
        assert e <= floor
    for bad in (torch.zeros_like(m), torch.ones_like(m), torch.cat([m, torch.zeros_like(m)])):
        with pytest.raises(ValueError, match="empty|full"):
            tr.signed_distance(bad)


def test_refusals_hold_next_to_a_device(tr):
    check_refusals()
