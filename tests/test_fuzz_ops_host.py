"""What the randomised operator sweeps (tests/fuzz_ops.py, tests/test_gpu_fuzz_ops.py) rest on, on the CPU: over the exact (cases, seed) pairs of the
GPU tests the generator selects every class that matters; a case is a function of (seed, index) alone; the distance arbiter agrees with the brute force
at the small drawn shapes; every exclusion cap holds for the restatements alone; the arbiters are quick.  No GPU, and nothing of the package."""
import collections
import math
import time

import numpy as np
import pytest
import torch

import chain_ref as cr
import distance_ref as dr
import flowops_ref as fr
import fuzz_ops_cases as fc
import spline_ref as sr

SHAPES = ("2d", "axis-of-1", "W-63..66", "W>=128", "y>=257", "z>=257", ">=2-chunks", "k*16384+-1")
# the classes a family's pinned sweep must hold at least one case of (tests/fuzz_ops_cases.py::classes)
BASE = ("2d", "axis-of-1", "W-63..66", "W>=128", ">=2-chunks")      # of every family: the shape rule is shared
SEAM = ("k*16384+-1",)                                               # of the families whose kernels work in chunks or blocks of voxels
REQUIRED = {
    "distance": SHAPES + ("sub-box", "sub-box-beyond-256", "empty-pair", "B3-all-non-empty", "two-non-empty-pairs", "voxel", "voxel-2d"),
    "surface": BASE + ("empty-pair",),
    "overlap": BASE + SEAM,
    "moments": BASE + SEAM,
    "compose": BASE + ("padding-border", "padding-zeros"),
    "invert": BASE,
    "jacobian": BASE + SEAM,
    "spline": BASE + ("order-0", "order-1", "order-3", "world-scale", "unequal-lattices", "unequal-2d", "axis>=257"),
    "chain": BASE + ("order-0", "order-1", "order-3", "padding-border", "padding-zeros", "chain-0", "chain-1", "unequal-lattices", "unequal-2d", "axis>=257"),
    "svf": BASE + SEAM,
    "bspline": BASE + ("spacing>axis",),
    "pyramid": BASE,
}
COUNTS = {f: fc.PINNED[f][0] for f in fc.FAMILIES}


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_the_pinned_sweeps_select_every_class(family):
    n, seed = fc.PINNED[family]
    count = collections.Counter()
    for rec in fc.cases(family, n, seed):
        count.update(fc.classes(rec))
    print(family, {k: count[k] for k in REQUIRED[family]})
    missing = [k for k in REQUIRED[family] if count[k] < 1]
    assert not missing, (family, missing)


def test_the_shape_rule():
    """Over 2000 draws: every axis comes from the groups (or a halving of one) or the voxel count is an aimed one; at most one axis is 257 or longer unless
    the count is aimed; at most 60 000 voxels; about 65 % are 3-D and about one in eight is aimed."""
    rng = np.random.default_rng(5)
    nd3 = aimed = 0
    for _ in range(2000):
        shape, aim = fc.draw_shape(rng)
        assert 2 <= len(shape) <= 3 and min(shape) >= 1 and math.prod(shape) <= fc.MAX_VOXELS
        nd3 += len(shape) == 3
        if aim is not None:
            aimed += 1
            assert math.prod(shape) == aim[0] * fc.CHUNK + aim[1] and max(shape) <= fc.AIM_CAP
        else:
            assert sum(s >= 257 for s in shape) <= 1 and max(shape) <= 330
    assert 0.60 < nd3 / 2000 < 0.70 and 0.08 < aimed / 2000 < 0.16


@pytest.mark.parametrize("family", fc.FAMILIES)
def test_a_case_is_a_function_of_seed_and_index(family):
    n, seed = fc.PINNED[family]
    first, again = fc.cases(family, n, seed), fc.cases(family, n, seed)
    assert first == again
    for k in (0, n // 2, n - 1):      # what only=k evaluates: the case drawn on its own
        assert fc.draw(family, fc.case_rng(family, seed, k)) == first[k]
    assert fc.cases(family, n, seed + 1) != first


def test_inputs_are_a_function_of_the_record():
    for family, build in (("distance", fc.mask_inputs), ("overlap", fc.overlap_inputs), ("moments", fc.moments_inputs), ("invert", fc.field_inputs),
                          ("chain", fc.chain_inputs), ("spline", fc.spline_inputs), ("svf", fc.svf_inputs), ("bspline", fc.bspline_inputs)):
        rec = fc.cases(family, 3, fc.PINNED[family][1])[2]
        a, b = build(rec), build(rec)
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y))


def test_distance_masks_are_what_the_record_says():
    """A pair is empty exactly where its kind says so; the features of a sub-box pair lie inside the box, which touches neither end of an axis; a box beyond
    256 lies beyond index 256 of an axis of stride > 1 or of the row."""
    n, seed = fc.PINNED["distance"]
    beyond = 0
    for rec in fc.cases("distance", n, seed):
        m = fc.mask_inputs(rec)
        assert m.shape == (rec["B"],) + rec["shape"] and m.dtype == np.uint8
        for b, kind in enumerate(rec["kinds"]):
            assert bool(m[b].any()) == (kind != "empty")
            assert kind == "empty" or rec["kinds"].count(kind) == 1      # different kinds per pair
            if kind == "single":
                assert m[b].sum() == 1
            if kind == "subbox":
                box = rec["boxes"][b]
                idx = np.argwhere(m[b])
                assert all(lo <= idx[:, a].min() and idx[:, a].max() <= hi for a, (lo, hi) in enumerate(box))
                assert any(lo >= 1 and hi <= s - 2 for (lo, hi), s in zip(box, rec["shape"]))
                if rec["beyond256"] and b == 0:
                    beyond += 1
                    assert any(lo > 256 for lo, _ in box)
    assert beyond >= 1


def test_dist2_is_the_brute_force_on_the_small_draws():
    """The arbiter at shapes it has not been used at: every pair of the first 400 draws with at most 400 voxels, with and without voxel sizes."""
    seed = fc.PINNED["distance"][1]
    done = 0
    for rec in fc.cases("distance", 400, seed):
        if math.prod(rec["shape"]) > 400:
            continue
        m = fc.mask_inputs(rec)
        voxel = rec["voxel"]
        g = dr.dist2(m, voxel)
        for b in range(rec["B"]):
            want = dr.brute(m[b], voxel)
            if voxel is None:
                assert np.array_equal(g[b], want), rec
            else:
                finite = np.isfinite(want)
                assert np.array_equal(np.isfinite(g[b]), finite) and np.allclose(g[b][finite], want[finite], rtol=1e-12, atol=0), rec
        done += 1
    print(f"{done} draws of at most 400 voxels")
    assert done >= 40


def test_overlap_maps_hold_what_the_kernel_must_ignore():
    """Over the pinned sweep: values >= L wherever the dtype can hold one, negative values in every int32 case, every L of the list within 200 draws."""
    n, seed = fc.PINNED["overlap"]
    for rec in fc.cases("overlap", n, seed):
        a, b = fc.overlap_inputs(rec)
        assert a.dtype == np.dtype(rec["dtype"]) and a.shape == (rec["B"],) + rec["shape"]
        for m in (a, b):
            if rec["dtype"] == "int32":
                assert ((m < 0).any() and (m >= rec["L"]).any()) or m.size < 500
            elif rec["L"] < 255:
                assert (m >= rec["L"]).any() or m.size < 500
    assert {rec["L"] for rec in fc.cases("overlap", 200, seed)} == set(fc.OVERLAP_L)


def test_the_invert_fields_are_contractions():
    n, seed = fc.PINNED["invert"]
    for rec in fc.cases("invert", n, seed):
        u, _ = fc.field_inputs(rec)
        assert fr.lipschitz_bound(u).max().item() <= fc.LIPSCHITZ * (1 + 1e-6), rec
    # the bound is one: a linear ramp of slope s along one axis has the constant s
    ramp = torch.zeros(1, 2, 4, 5)
    ramp[0, 1] = 0.25 * torch.arange(5.0)
    assert abs(fr.lipschitz_bound(ramp).item() - 0.25) < 1e-12


@pytest.mark.parametrize("family", ["chain", "spline"])
def test_kept_leaves_out_at_most_one_percent(family):
    """spline_ref.kept (a position within 1e-4 of a face of the field of view or, for nearest, of a rounding tie) removes at most 1 % of the voxels of
    every pinned case - the cap tests/test_spline_host.py and tests/test_chain_host.py hold the fixed cases to."""
    n, seed = fc.PINNED[family]
    worst = 0.0
    for rec in fc.cases(family, n, seed):
        if family == "chain":
            _, theta, flow, _ = fc.chain_inputs(rec)
            pos = cr.image_positions(theta, flow, rec["shape"], rec["src_shape"], rec["padding"])
        else:
            _, _, theta, flow, scale = fc.spline_inputs(rec)
            pos = sr.positions(rec["src_shape"], theta, flow, scale, size=rec["shape"])
        for nearest in (False, True):
            out = 1.0 - sr.kept(pos, rec["src_shape"], nearest=nearest).double().mean().item()
            worst = max(worst, out)
            assert out <= 0.01, (rec, nearest, out)
    print(f"{family}: kept() leaves out at most {100 * worst:.3f} % of a case")


def test_the_adjoint_allowance_covers_the_restatement_in_fp32():
    """The svf sweep counts the elements of the GPU adjoint beyond bar(fp32, fp64, 1e-5 max |dvel|) against max(4, 0.1 %).  On the pinned draws the
    restatement's own fp32 run stays within that allowance against the floor alone, so the allowance is not what absorbs a wide bar; and at least one clean
    direction of the directional identity exists for every case."""
    import fuzz_ops
    n, seed = fc.PINNED["svf"]
    for rec in fc.cases("svf", n, seed):
        v, g = fc.svf_inputs(rec)
        r = fuzz_ops.svf_reference(rec, v, g)
        beyond = int(((r["b32"].double() - r["b64"]).abs() > 1e-5 * r["b64"].abs().max().item()).sum())
        print(rec["shape"], "K", rec["K"], f"{beyond} fp32 elements beyond the floor, allowed {max(4, v.numel() // 1000)}, {len(r['dirs'])} directions")
        assert beyond <= max(4, v.numel() // 1000), rec
        assert len(r["dirs"]) >= 1, rec


def test_the_arbiters_are_quick():
    """The restatements of the costliest comparisons over their pinned sweeps (distance: three min-plus passes in up to three number formats; invert: 12
    updates in two): well under a minute in all - measured 1 s and 2 s."""
    import fuzz_ops
    t0 = time.perf_counter()
    for rec in fc.cases("distance", *fc.PINNED["distance"]):
        dr.run_reference(fc.mask_inputs(rec), rec["voxel"])
    for rec in fc.cases("invert", *fc.PINNED["invert"]):
        u, _ = fc.field_inputs(rec)
        fr.invert(u, fr.FIXED_K, 0.0)
        fr.invert(u.double(), fr.FIXED_K, 0.0)
    seconds = time.perf_counter() - t0
    print(f"{seconds:.1f} s")
    assert seconds < 30.0


def test_what_the_pinned_cases_rest_on():
    """The CPU side of tests/test_gpu_fuzz_ops.py's two pinned cases.  chain, seed 2025, case 278: the restatement's own fp32 positions are more than one
    fp32 ulp of a coordinate of 256 or more (3.05e-5 voxels) from the fp64 ones, and that distance times the steepest neighbour difference of the image
    is more than the restatement's own fp32 - fp64 gap of the image: the position's rounding alone accounts for an error of the size that was found.
    svf, seed 2025, case 29: the restatement's fp32 adjoint misses the directional identity by more than 1e-4 while its fp64 adjoint meets it to 1e-6."""
    import fuzz_ops
    rec = fc.draw("chain", fc.case_rng("chain", 2025, 278))
    assert rec["src_shape"] == (14, 5, 270) and rec["order"] == 1
    x, theta, flow, _ = fc.chain_inputs(rec)
    r64, r32, pos, keep, _ = fuzz_ops.chain_image_reference(rec, x, theta, flow)
    p32 = cr.image_positions(theta, flow, rec["shape"], rec["src_shape"], rec["padding"], torch.float32)
    moved = (p32.double() - pos)[keep].abs().max().item()
    gap = (r32.double() - r64)[keep[:, None].expand_as(r64)].abs().max().item()
    steepest = x.diff(dim=-1).abs().max().item()
    print(f"chain 278: fp32 positions {moved:.2e} voxels off, steepest neighbour difference {steepest:.3f}, the restatement's own image gap {gap:.3e}")
    assert 2.0 ** -15 < moved < 4 * 2.0 ** -15 and gap < moved * steepest < 2.5 * gap
    rec = fc.draw("svf", fc.case_rng("svf", 2025, 29))
    assert rec["shape"] == (65, 2) and rec["K"] == 7
    v, g = fc.svf_inputs(rec)
    r = fuzz_ops.svf_reference(rec, v, g)
    miss32 = max(abs((r["b32"].double() * d).sum().item() - rhs) / max(abs(rhs), 1e-300) for d, rhs in r["dirs"])
    miss64 = max(abs((r["b64"] * d).sum().item() - rhs) / max(abs(rhs), 1e-300) for d, rhs in r["dirs"])
    print(f"svf 29: the restatement's adjoint misses the identity by {miss32:.2e} in fp32, {miss64:.2e} in fp64")
    assert miss32 > 1e-4 and miss64 < 1e-6
