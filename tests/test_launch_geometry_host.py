"""CPU checks of tests/launch_geometry.py: (1) the restatement of the flow and local-NCC launch geometry predicts the library's workspace
sizes over a sweep of shapes - trx_flow_workspace_bytes carries nblk of the 3-D column walk and the 2-D block cap, trx_lncc_workspace_bytes the
finest z split; (2) every branch named in a family's table has a case, and every case selects the branches it claims; (3) the restatement's
own fp32 adjoint of the large SVF cases stays within the allowance of the GPU test at the committed seeds.

The B-spline plan (reduce_x_plan, bs_tw_log2, bs_grid) and the SVF caps (svf_stream_grid, the svf_max_kernel launch) are not visible
through any host-side call: launch_geometry.py restates them from the source lines it names, and that restatement can drift from the
library without this file noticing."""
import ctypes
import random

import pytest
import torch

import launch_geometry as lg
import svf_ref


def _vol(nd, B, D, H, W):
    from torchregister_amd import _lib
    v = _lib.Volumes()
    keep = ctypes.create_string_buffer(8)
    v.moving = ctypes.addressof(keep)     # the size query checks for NULL only
    v.ndim, v.B, v.D, v.H, v.W = nd, B, D, H, W
    return v, keep


def _sweep(n, seed):
    """Seeded shapes: 3-D with W over every block width and its edges, D around the segment thresholds; 2-D around the block cap."""
    rng = random.Random(seed)
    edges_w = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 449, 512, 513]
    edges_d = [1, 7, 8, 15, 16, 17, 31, 32, 63, 64, 65, 96, 97, 128, 200]
    out = []
    for _ in range(n):
        B = rng.choice([1, 1, 1, 2, 3, 8, 64, 65, 100])
        if rng.random() < 0.7:
            D = rng.choice(edges_d) if rng.random() < 0.5 else rng.randint(1, 220)
            W = rng.choice(edges_w) if rng.random() < 0.5 else rng.randint(1, 600)
            out.append((3, B, D, rng.randint(1, 70), W))
        else:
            out.append((2, B, 1, rng.randint(1, 1200), rng.randint(1, 1200)))
    return out


def test_flow_workspace_bytes_match_the_restatement():
    from torchregister_amd import _lib
    lib = _lib.load()
    seen = set()
    cases = _sweep(400, 7) + [(len(c["shape"]), c["B"]) + (1,) * (3 - len(c["shape"])) + tuple(c["shape"]) for f in ("flow3", "flow2") for c in lg.CASES[f].values()]
    for nd, B, D, H, W in cases:
        v, keep = _vol(nd, B, D, H, W)
        got, want = lib.trx_flow_workspace_bytes(ctypes.byref(v)), lg.flow_workspace_bytes(nd, B, D, H, W)
        assert got == want, ((nd, B, D, H, W), got, want)
        if nd == 3:
            g = lg.flow_col_geom(B, D, H, W)
            seen.add((g["colw_log2"], g["nzseg"] > 1, g["reorder"]))
        else:
            seen.add(("2d", lg.flow2_trips(B, H, W) >= 2))
    # the sweep itself reaches every block shape with and without seams and both block orders, and both sides of the 2-D cap
    assert {s[0] for s in seen} == {6, 7, 8, "2d"} and ("2d", True) in seen and ("2d", False) in seen
    for l2 in (6, 7, 8):
        assert {(l2, True, True), (l2, True, False), (l2, False, False)} <= seen, (l2, seen)


def test_lncc_workspace_bytes_match_the_restatement():
    from torchregister_amd import _lib
    lib = _lib.load()
    splits = set()
    cases = _sweep(400, 11) + [(len(c["shape"]), c["B"]) + (1,) * (3 - len(c["shape"])) + tuple(c["shape"]) for c in lg.LNCC_CASES.values()]
    for nd, B, D, H, W in cases:
        got, want = lib.trx_lncc_workspace_bytes(nd, B, D, H, W), lg.lncc_workspace_bytes(nd, B, D, H, W)
        assert got == want, ((nd, B, D, H, W), got, want)
        z = lg.lncc_zsplit(nd, B, D, H, W, lg.LNCC_SLOTS4)
        # the split is visible in the size only where it moves the partials across a 256-byte line: count those shapes
        if z > 1 and lg.cdiv(B * lg.cdiv(W, 32) * lg.cdiv(H, 16) * 4, 256) != lg.cdiv(B * lg.cdiv(W, 32) * lg.cdiv(H, 16) * z * 4, 256):
            splits.add(z)
    assert len(splits) >= 3, splits


@pytest.mark.parametrize("family", sorted(lg.BRANCHES))
def test_every_branch_has_a_case_and_every_case_selects_its_branches(family):
    """Keeps the GPU cases honest when a threshold is retuned: a case that no longer selects its branch fails here, on the CPU."""
    rules, cases = lg.BRANCHES[family], lg.CASES[family]
    covered = set()
    for name, case in cases.items():
        assert case["branches"], name
        for br in case["branches"]:
            assert br in rules, (family, name, br)
            assert rules[br][1](case), f"{family} case {name} {case['shape']} does not select {br}: {rules[br][0]}"
            covered.add(br)
    assert covered == set(rules), (family, sorted(set(rules) - covered))


def test_flow3_shapes_of_the_issue():
    """The two shapes derived on paper: (16, 4, 200) - 256 x 1, 2 segments, 8 blocks, reordered; (17, 3, 70) - 128 x 2, 9 + 8 planes, 4 blocks."""
    g = lg.flow_col_geom(1, 16, 4, 200)
    assert (g["colw"], g["rows"], g["nzseg"], g["nblk"], g["reorder"]) == (256, 1, 2, 8, True)
    g = lg.flow_col_geom(1, 17, 3, 70)
    assert (g["colw"], g["rows"], g["nzseg"], g["planes_per_seg"], g["nblk"], g["reorder"]) == (128, 2, 2, 9, 4, False)
    g = lg.flow_col_geom(1, 9, 5, 130)
    assert (g["colw"], g["ntx"], g["nty"], g["nzseg"]) == (64, 3, 2, 1)
    # the two slabs of the slab case are launches with seams of their own
    lo, mid, hi = lg.FLOW3_SLAB["bounds"]
    H, W = lg.FLOW3_SLAB["shape"][1:]
    assert all(lg.flow_col_geom(1, d, H, W)["nzseg"] > 1 and lg.flow_col_geom(1, d, H, W)["colw"] == 128 for d in (mid - lo, hi - mid))


def test_bspline_plan_of_the_segmented_cases():
    """The numbers the segmented cases were chosen for, and the LDS a block of the x pass of reduce asks for (below the 64 KB of a block)."""
    want = {"seg_d5": (816, 3, 0), "seg_d8": (509, 3, 1), "seg_d1024": (1, 8, 1)}
    for name, (Kc, nseg, pad) in want.items():
        p = lg.bs_geom(lg.BSPLINE_CASES[name])["plan"]
        assert (p["Kc"], p["nseg"], p["pad"]) == (Kc, nseg, pad), (name, p)
    for name, case in lg.BSPLINE_CASES.items():
        g = lg.bs_geom(case)
        lds = min(g["d"][2], g["S"][2]) * 16 + g["plan"]["R"] * g["plan"]["rowlen"] * 4
        assert lds <= 65536, (name, lds)
        assert all(1 <= q <= lg.BS_MAX_SPACING for q in g["d"])


def test_flow2_second_trip_bars_are_far_below_the_signal_of_the_second_trip():
    """The 2-D second-trip GPU tests can fail: on the CPU, from the arbiters alone - the gradient bars of the second-trip voxels are at most
    1e-3 of their largest gradient (which is at least 0.3 of the image's), the loss without those voxels misses its bar 20 times over, the
    flows of the SGD runs stay off the lattice, their bar is at most 2 % of the largest and half of the median movement of the second-trip
    voxels, and at most a tenth of what the smoothness term moves them by (tests/loop_arbiters.py: flow2_big_check_teeth)."""
    import loop_arbiters as arb
    for line in arb.flow2_big_check_teeth():
        print(line)


@pytest.mark.parametrize("name", [n for n, c in lg.SVF_CASES.items() if c["squarings"] > 0])
def test_svf_large_cases_fp32_adjoint_stays_within_the_allowance(name):
    """tests/test_svf_host.py's rule for the small cases - the restatement's own fp32 adjoint shows no element beyond 1e-5 max|dvel| - cannot
    hold at a quarter of a million voxels: some sampling position always lies within fp32 rounding of a lattice plane.  What the GPU test
    allows is max(4, 0.1 %) of the elements beyond its bar; the seed is one at which the restatement's fp32 run stays within that allowance
    against the FLOOR of the bar, and at which its largest deviation is below 1e-4 max|dvel| - no single jump sets the bar, which is then at
    most 2e-4 max|dvel|."""
    c = lg.SVF_CASES[name]
    v, g = lg.svf_case_inputs(name)
    b64 = svf_ref.exp_backward(v, g, c["squarings"])
    b32 = svf_ref.exp_backward(v, g, c["squarings"], dtype=torch.float32).double()
    assert bool(torch.isfinite(b64).all())
    err, m = (b32 - b64).abs(), b64.abs().max().item()
    beyond = int((err > 1e-5 * m).sum())
    print(f"svf {name}: {beyond} of {b64.numel()} fp32 elements beyond 1e-5 max|dvel| (allowed {max(4, b64.numel() // 1000)}), largest {err.max().item() / m:.2e} max|dvel|")
    assert beyond <= max(4, b64.numel() // 1000)
    assert err.max().item() <= 1e-4 * m
    assert svf_ref.share_outside(svf_ref.exp(v, c["squarings"])) > 0.01      # the out-of-bounds corners take part
