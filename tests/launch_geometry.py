"""Plain-Python restatement of the host-side launch geometry of the non-affine kernel families - which kernel variant, how many segments,
how many trips of a grid-stride loop a shape selects - and, per family, the table of shapes that the GPU tests run so that every such branch
is taken (tests/test_gpu_launch_geometry.py).  Not a test.

Each rule cites the function it restates.  trx_flow_workspace_bytes and trx_lncc_workspace_bytes expose the flow and local-NCC rules
without a GPU, and tests/test_launch_geometry_host.py compares them with this file over a sweep of shapes.  The B-spline plan and the SVF
caps have no such witness: they are pinned to the source lines named beside them and CAN DRIFT when those lines are retuned - the host test
then still passes, and only a reader of the diff can see that a table below has stopped selecting its branch.

A case is a dict: `shape` (spatial sizes), `B`, the family's parameters, and `branches`, the names of the branches the case exists for.
BRANCHES[family] maps each branch name to (condition in words, predicate over a case)."""
import math

TRX_BLOCK = 256


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------------------------------------------
# Dense flow (csrc/flow.hip)
# ------------------------------------------------------------------------------------------------------------------------------------
FLOW_BLOCKS = 2048          # TRX_FLOW_BLOCKS
FLOW_NP = 8                 # kFlowNP: floats per block partial
FLOW_COEF_BYTES = 44        # sizeof(FlowCoef): 10 floats + 1 int
FLOW_2D_BLOCKS = 4096       # flow_grid_x: `total`


def flow_col_geom(B, D, H, W):
    """flow_col_geom: the block shape (2^colw_log2 columns by 256 >> colw_log2 rows: the widest of 64, 128, 256 that pads W no further
    than 64 does), the tiles in x and y, the z segments (about FLOW_BLOCKS blocks, each segment at least 8 planes) and, ColWalk's rule, whether
    the block order is permuted for the XCDs (nblk a multiple of 8)."""
    l2 = 6
    best = cdiv(W, 64) * 64
    for cand in (7, 8):
        padded = cdiv(W, 1 << cand) * (1 << cand)
        if padded <= best:
            best, l2 = padded, cand
    colw, rows = 1 << l2, TRX_BLOCK >> l2
    ntx, nty = cdiv(W, colw), cdiv(H, rows)
    cols = ntx * nty * B
    want = max(1, min(cdiv(FLOW_BLOCKS, cols), D // 8))
    pps = cdiv(D, want)
    nzseg = cdiv(D, pps)
    nblk = ntx * nty * nzseg
    return dict(colw_log2=l2, colw=colw, rows=rows, ntx=ntx, nty=nty, planes_per_seg=pps, nzseg=nzseg, nblk=nblk, reorder=nblk % 8 == 0)


def flow_grid_x(ndim, B, D, H, W):
    """flow_grid_x: 3-D - the column walk's nblk; 2-D - one block per 256 voxels, capped at max(64, ceil(4096 / B))."""
    if ndim == 3:
        return flow_col_geom(B, D, H, W)["nblk"]
    return min(cdiv(D * H * W, TRX_BLOCK), max(64, cdiv(FLOW_2D_BLOCKS, B)))


def flow_workspace_bytes(ndim, B, D, H, W):
    """flow_workspace_size: the block partials, the pairs' coefficients and the fp64 stash of the lagged regulariser term."""
    return B * flow_grid_x(ndim, B, D, H, W) * FLOW_NP * 4 + B * FLOW_COEF_BYTES + 256 + B * 8 + 256


def flow2_trips(B, H, W):
    """Trips of the grid-stride loops of the 2-D kernels (flow_moments_kernel<2>, flow_update_kernel<2, ...>, the warps)."""
    return cdiv(H * W, flow_grid_x(2, B, 1, H, W) * TRX_BLOCK)


def _g3(case):
    return flow_col_geom(case["B"], *case["shape"])


BRANCHES = {}
BRANCHES["flow3"] = {
    "block_64x4": ("W <= 64 or 129..192 (mod 256)", lambda c: _g3(c)["colw_log2"] == 6),
    "block_128x2": ("W in 65..128 (mod 256)", lambda c: _g3(c)["colw_log2"] == 7),
    "block_256x1": ("W in 193..256 (mod 256)", lambda c: _g3(c)["colw_log2"] == 8),
    "wide_ragged_x": ("a 128- or 256-wide block with idle lanes: W no multiple of the block's width", lambda c: _g3(c)["colw_log2"] > 6 and c["shape"][2] % _g3(c)["colw"] != 0),
    "wide_idle_rows": ("a 128-wide block whose last rows lie outside the volume: H odd", lambda c: _g3(c)["colw_log2"] == 7 and c["shape"][1] % 2 != 0),
    "x_tiles_ragged": ("more than one tile in x, the last one ragged", lambda c: _g3(c)["ntx"] > 1 and c["shape"][2] % _g3(c)["colw"] != 0),
    "wide_seam": ("z segments (D >= 16) on a 128- or 256-wide block", lambda c: _g3(c)["colw_log2"] > 6 and _g3(c)["nzseg"] > 1),
    "seam_uneven": ("the last z segment shorter than the others", lambda c: _g3(c)["nzseg"] > 1 and c["shape"][0] % _g3(c)["planes_per_seg"] != 0),
    "reorder_on": ("nblk a multiple of 8: the XCD block order", lambda c: _g3(c)["reorder"]),
    "reorder_off": ("nblk no multiple of 8: blocks in launch order", lambda c: not _g3(c)["reorder"]),
}
FLOW3_CASES = {
    "w200": dict(shape=(16, 4, 200), B=1, branches=["block_256x1", "wide_ragged_x", "wide_seam", "reorder_on"]),
    "w70": dict(shape=(17, 3, 70), B=1, branches=["block_128x2", "wide_ragged_x", "wide_idle_rows", "wide_seam", "seam_uneven", "reorder_off"]),
    "w130": dict(shape=(9, 5, 130), B=1, branches=["block_64x4", "x_tiles_ragged", "reorder_off"]),
    "w450": dict(shape=(8, 3, 450), B=1, branches=["block_256x1", "x_tiles_ragged", "wide_ragged_x", "reorder_off"]),
}
# the whole volume of the slab test and its two slabs (each slab is a launch of its own depth)
FLOW3_SLAB = dict(shape=(40, 3, 70), B=1, bounds=(0, 17, 40), branches=["block_128x2", "wide_seam", "wide_idle_rows"])
# the local-NCC loop (MODE 2 of the update) behind a z-split criterion: the column walk's own geometry at that shape
FLOW3_LNCC_DEEP = dict(shape=(65, 8, 12), B=1, window=7, branches=["block_64x4", "seam_uneven", "reorder_on"])

BRANCHES["flow2"] = {
    "one_trip": ("H W <= 256 x grid: every thread has at most one voxel", lambda c: flow2_trips(c["B"], *c["shape"]) == 1),
    "second_trip": ("H W > 256 x max(64, 4096 / B): the grid-stride loops go round again", lambda c: flow2_trips(c["B"], *c["shape"]) >= 2),
}
FLOW2_CASES = {
    "small": dict(shape=(70, 90), B=1, branches=["one_trip"]),          # tests/test_gpu_flow.py runs it (the largest 2-D shape there)
    "big": dict(shape=(1025, 1027), B=1, branches=["second_trip"]),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# Local NCC (csrc/lncc.hip)
# ------------------------------------------------------------------------------------------------------------------------------------
LNCC_TX, LNCC_TY = 32, 16                  # kLX, kLY
LNCC_SLOTS4, LNCC_SLOTS3 = 1024, 768       # kLnccSlots4, kLnccSlots3


def lncc_zsplit(nd, B, D, H, W, want):
    """lncc_zsplit: z segments per column - enough blocks for `want` slots, each segment at least 32 planes; 2-D: 1."""
    if nd == 2:
        return 1
    cols = cdiv(W, LNCC_TX) * cdiv(H, LNCC_TY) * B
    return max(1, min(cdiv(want, cols), D // 32))


def lncc_instance(nd, B, D, H, W, window):
    """launch_lncc: (R, blocks per CU of the build, zsplit, form).  Windows 3, 5: <R, 4>, direct form; windows 7, 9: <R, 3> (tile form) when
    the 768-slot split is > 1, else <R, 1> (direct form) - lncc_direct<R, MW>()."""
    R = window // 2
    if R <= 2:
        return R, 4, lncc_zsplit(nd, B, D, H, W, LNCC_SLOTS4), "direct"
    z = lncc_zsplit(nd, B, D, H, W, LNCC_SLOTS3)
    return (R, 3, z, "tile") if z > 1 else (R, 1, z, "direct")


def lncc_workspace_bytes(nd, B, D, H, W):
    """trx_lncc_workspace_bytes: the block partials at the finest split any window uses (rounded up to 256 bytes) + the three fields."""
    nb = cdiv(W, LNCC_TX) * cdiv(H, LNCC_TY) * lncc_zsplit(nd, B, D, H, W, LNCC_SLOTS4)
    return cdiv(B * nb * 4, 256) * 256 + 3 * B * D * H * W * 4


def _li(case):
    s = case["shape"]
    return lncc_instance(len(s), case["B"], *((1,) * (3 - len(s)) + tuple(s)), case["window"])


def _zlen_uneven(case):
    D, z = case["shape"][0], _li(case)[2]
    return z > 1 and D % cdiv(D, z) != 0


BRANCHES["lncc"] = {
    "w3_split": ("window 3, D >= 64: <1, 4> with z segments", lambda c: _li(c)[0] == 1 and _li(c)[2] > 1),
    "w5_split": ("window 5, D >= 64: <2, 4> with z segments", lambda c: _li(c)[0] == 2 and _li(c)[2] > 1),
    "w7_tile": ("window 7, D >= 64 and fewer than 768 columns: <3, 3>, tile form", lambda c: _li(c)[:2] == (3, 3) and _li(c)[3] == "tile"),
    "w9_tile": ("window 9, D >= 64 and fewer than 768 columns: <4, 3>, tile form", lambda c: _li(c)[:2] == (4, 3) and _li(c)[3] == "tile"),
    "w7_direct": ("window 7, no split: <3, 1>, direct form", lambda c: _li(c)[:2] == (3, 1)),
    "w9_direct": ("window 9, no split: <4, 1>, direct form", lambda c: _li(c)[:2] == (4, 1)),
    "seam_uneven": ("zlen = ceil(D / zsplit) does not divide D", _zlen_uneven),
}
LNCC_CASES = {
    "w7_64": dict(shape=(64, 8, 12), B=1, window=7, branches=["w7_tile"]),
    "w7_65": dict(shape=(65, 8, 12), B=1, window=7, branches=["w7_tile", "seam_uneven"]),
    "w3_64": dict(shape=(64, 8, 12), B=1, window=3, branches=["w3_split"]),
    "w3_65": dict(shape=(65, 8, 12), B=1, window=3, branches=["w3_split", "seam_uneven"]),
    # already in tests/test_gpu_lncc.py::CASES (listed so that the table is whole; the host test checks that they still select these)
    "w9_70": dict(shape=(70, 20, 36), B=1, window=9, branches=["w9_tile"], existing=True),
    "w5_97": dict(shape=(97, 12, 33), B=2, window=5, branches=["w5_split", "seam_uneven"], existing=True),
    "w7_24": dict(shape=(24, 40, 33), B=1, window=7, branches=["w7_direct"], existing=True),
    "w9_20": dict(shape=(20, 18, 44), B=1, window=9, branches=["w9_direct"], existing=True),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# B-spline (csrc/bspline.hip) - no witness without a GPU: pinned to reduce_x_plan, bs_tw_log2, bs_grid and the launches in
# bspline_expand_impl / bspline_reduce_impl / launch_bs_axis
# ------------------------------------------------------------------------------------------------------------------------------------
BS_TILE_FLOATS = 4096       # kBsTileFloats
BS_MAX_SPACING = 1024       # TRX_BSPLINE_MAX_SPACING
BS_GRID_BLOCKS = 8192       # bs_grid
GRID_Y_MAX = 65535


def bs_tw_log2(W):
    """bs_tw_log2: the smallest power of two that covers min(W, 256)."""
    l2 = 0
    while (1 << l2) < min(W, TRX_BLOCK):
        l2 += 1
    return l2


def bs_grid(work_blocks, nvol):
    """bs_grid: (blocks in x, blocks in y) - the volumes along y (at most 65535), about 8192 blocks in all."""
    gy = min(nvol, GRID_Y_MAX)
    return max(1, min(work_blocks, max(1, BS_GRID_BLOCKS // gy))), gy


def reduce_x_plan(rows, W, G, d):
    """reduce_x_plan: rows of at most 4096 voxels are one segment (R rows per tile); longer rows are cut into segments of
    Kc = 4096 / d - 3 control points that re-read 3 d voxels each.  Even spacings pad every d-th float of the LDS row."""
    if W <= BS_TILE_FLOATS:
        Kc, nseg, n, R = G, 1, W, min(rows, max(1, BS_TILE_FLOATS // W))
    else:
        Kc = max(1, BS_TILE_FLOATS // d - 3)
        nseg, n, R = cdiv(G, Kc), (Kc + 3) * d, 1
    pad = 1 if d % 2 == 0 else 0
    return dict(R=R, Kc=Kc, nseg=nseg, n=n, pad=pad, rowlen=n + (n // d + 1 if pad else 0), ntile=cdiv(rows, R) * nseg)


def bs_geom(case):
    """The launches of one expand and one reduce of a case: per kernel (work blocks, grid x, grid y)."""
    sp, d, B = case["shape"], case["spacing"], case["B"]
    nd = len(sp)
    S, dd = (1,) * (3 - nd) + tuple(sp), (1,) * (3 - nd) + tuple(d)
    G = [(s - 1) // q + 4 for s, q in zip(S, dd)]
    if nd == 2:
        G[0] = 1
    nvol, rows, W = B * nd, S[0] * S[1], S[2]
    rpb = TRX_BLOCK >> bs_tw_log2(W)
    plan = reduce_x_plan(rows, W, G[2], dd[2])
    work = {"expand_y": cdiv(S[0] * S[1] * G[2], TRX_BLOCK), "expand_x": cdiv(rows, rpb), "reduce_x": plan["ntile"],
            "reduce_y": cdiv(S[0] * G[1] * G[2], TRX_BLOCK)}
    if nd == 3:
        work["expand_z"] = cdiv(S[0] * G[1] * G[2], TRX_BLOCK)
        work["reduce_z"] = cdiv(G[0] * G[1] * G[2], TRX_BLOCK)
    return dict(S=S, d=dd, G=G, nvol=nvol, plan=plan, work=work, grid={k: bs_grid(w, nvol) for k, w in work.items()})


def _second_trip(case, kernel):
    g = bs_geom(case)
    return g["work"][kernel] > g["grid"][kernel][0]


BRANCHES["bspline"] = {
    "expand_x_xc_loop": ("W > 256: bspline_expand_x_kernel's xc loop goes round again (TW = 256, one row per block)", lambda c: bs_geom(c)["S"][2] > 256),
    "reduce_x_segmented": ("W > 4096: nseg > 1", lambda c: bs_geom(c)["plan"]["nseg"] > 1),
    "reduce_x_inner_segment": ("nseg >= 3: a segment with c0 = k0 - 3 > 0 and a full Kc points", lambda c: bs_geom(c)["plan"]["nseg"] >= 3),
    "reduce_x_seg_odd_d": ("segmented, odd spacing: no padding", lambda c: bs_geom(c)["plan"]["nseg"] > 1 and bs_geom(c)["plan"]["pad"] == 0),
    "reduce_x_seg_even_d": ("segmented, even spacing: padding and the magic division", lambda c: bs_geom(c)["plan"]["nseg"] > 1 and bs_geom(c)["plan"]["pad"] == 1 and bs_geom(c)["plan"]["Kc"] > 1),
    "reduce_x_seg_kc1": ("segmented, spacing 1024: Kc = 1, one control point per segment", lambda c: bs_geom(c)["plan"]["nseg"] > 1 and bs_geom(c)["plan"]["Kc"] == 1),
    "x_d64_one_segment": ("spacing 64 along W on the one-segment path", lambda c: bs_geom(c)["plan"]["nseg"] == 1 and bs_geom(c)["d"][2] == 64),
    "x_d1024_one_segment": ("spacing 1024 along W <= 4096, W > d", lambda c: bs_geom(c)["plan"]["nseg"] == 1 and bs_geom(c)["d"][2] == 1024 and bs_geom(c)["S"][2] > 1024),
    "x_d_above_S": ("spacing > W: the weight table holds W < d entries", lambda c: bs_geom(c)["d"][2] > bs_geom(c)["S"][2]),
    "axis_d64": ("spacing 64 on an axis of bspline_axis_kernel, S > d", lambda c: any(q == 64 and s > q for s, q in zip(bs_geom(c)["S"][:2], bs_geom(c)["d"][:2]))),
    "axis_d1024_above_S": ("spacing 1024 > S on an axis of bspline_axis_kernel: table min(d, S) = S", lambda c: any(q == 1024 and s < q and s > 1 for s, q in zip(bs_geom(c)["S"][:2], bs_geom(c)["d"][:2]))),
    "grid2_axis_expand": ("bspline_axis_kernel<false>: more work blocks than 8192 / nvol", lambda c: _second_trip(c, "expand_y")),
    "grid2_axis_reduce": ("bspline_axis_kernel<true>: more work blocks than 8192 / nvol", lambda c: _second_trip(c, "reduce_y")),
    "grid2_expand_x": ("bspline_expand_x_kernel: more row blocks than 8192 / nvol", lambda c: _second_trip(c, "expand_x")),
    "grid2_reduce_x": ("bspline_reduce_x_kernel: more tiles than 8192 / nvol", lambda c: _second_trip(c, "reduce_x")),
    "nvol_above_grid_y": ("B ndim > 65535: the v += gridDim.y walk (B <= 65535 is checked, nvol = B ndim is not: B = 32769 in 2-D reaches it)", lambda c: bs_geom(c)["nvol"] > GRID_Y_MAX),
}
BSPLINE_CASES = {
    "xc": dict(shape=(3, 300), spacing=(2, 7), B=1, branches=["expand_x_xc_loop"]),
    "seg_d5": dict(shape=(2, 9000), spacing=(2, 5), B=1, branches=["reduce_x_segmented", "reduce_x_inner_segment", "reduce_x_seg_odd_d", "expand_x_xc_loop"]),
    "seg_d8": dict(shape=(2, 9000), spacing=(2, 8), B=1, branches=["reduce_x_segmented", "reduce_x_inner_segment", "reduce_x_seg_even_d"]),
    "seg_d1024": dict(shape=(3, 4200), spacing=(2, 1024), B=1, branches=["reduce_x_segmented", "reduce_x_seg_kc1", "reduce_x_inner_segment"]),
    "d64": dict(shape=(5, 3000), spacing=(2, 64), B=1, branches=["x_d64_one_segment"]),
    "d1024": dict(shape=(5, 3000), spacing=(2, 1024), B=1, branches=["x_d1024_one_segment"]),
    "d_above": dict(shape=(5, 700), spacing=(64, 1024), B=1, branches=["x_d_above_S"]),
    "axis_d64": dict(shape=(130, 3, 5), spacing=(64, 2, 2), B=1, branches=["axis_d64"]),
    "axis_d1024": dict(shape=(40, 70, 5), spacing=(1024, 64, 2), B=1, branches=["axis_d1024_above_S", "axis_d64"]),
    "grid2": dict(shape=(85, 85), spacing=(2, 2), B=512, branches=["grid2_axis_expand", "grid2_axis_reduce", "grid2_expand_x"]),
    "grid2_rx": dict(shape=(5, 4200), spacing=(2, 1024), B=128, branches=["grid2_reduce_x", "reduce_x_seg_kc1"]),
    "nvol": dict(shape=(2, 3), spacing=(2, 2), B=32769, branches=["nvol_above_grid_y"]),
}


# ------------------------------------------------------------------------------------------------------------------------------------
# SVF (csrc/svf.hip) - no witness without a GPU: pinned to svf_stream_grid (4096 blocks) and the svf_max_kernel launch in
# svf_backward_launch (1024 blocks per pair)
# ------------------------------------------------------------------------------------------------------------------------------------
SVF_SCALE_BLOCKS, SVF_MAX_BLOCKS = 4096, 1024


def svf_scale_trips(B, shape):
    """svf_scale_kernel over the whole field [B][nd][N] (trx_svf_exp always; trx_svf_exp_backward when squarings = 0)."""
    n = B * len(shape) * math.prod(shape)
    return cdiv(n, min(cdiv(n, TRX_BLOCK), SVF_SCALE_BLOCKS) * TRX_BLOCK)


def svf_max_trips(shape):
    """svf_max_kernel over one pair's nd N floats (trx_svf_exp_backward, squarings > 0)."""
    n = len(shape) * math.prod(shape)
    return cdiv(n, min(cdiv(n, TRX_BLOCK), SVF_MAX_BLOCKS) * TRX_BLOCK)


BRANCHES["svf"] = {
    "scale_second_trip": ("B nd N > 4096 x 256 floats", lambda c: svf_scale_trips(c["B"], c["shape"]) >= 2),
    "max_second_trip_2d": ("2-D, squarings > 0, 2 N > 1024 x 256 floats", lambda c: len(c["shape"]) == 2 and c["squarings"] > 0 and svf_max_trips(c["shape"]) >= 2),
    "max_second_trip_3d": ("3-D, squarings > 0, 3 N > 1024 x 256 floats: N > 87381", lambda c: len(c["shape"]) == 3 and c["squarings"] > 0 and svf_max_trips(c["shape"]) >= 2),
    "backward_k0_scale_second_trip": ("squarings = 0: the backward is the scale kernel, second trip", lambda c: c["squarings"] == 0 and svf_scale_trips(c["B"], c["shape"]) >= 2),
}
# amplitude, noise, seed: svf_ref.smooth_field's for the velocity.  The 2-D velocity carries no noise: at coordinates of ~500 voxels the fp32
# rounding of a position is 3e-5 voxels, a quarter of a million samples always hold some that fall on the other side of a lattice plane in
# fp32, and with noise in the field the gradient jumps there by a large amount - the bar (twice the restatement's own fp32-vs-fp64 gap)
# would then be set by one such element.  The seeds are those at which the restatement's own fp32 adjoint stays within the allowance and
# its largest deviation stays small (tests/test_launch_geometry_host.py; of seeds 1..8: 2-D seed 5 leaves 91 of 1 052 660 elements beyond
# 1e-5 max|dvel|, the largest 3.5e-5; 3-D seed 4 leaves none).
SVF_CASES = {
    "2d": dict(shape=(515, 511), B=2, squarings=3, amplitude=12.0, noise=0.0, seed=5, branches=["scale_second_trip", "max_second_trip_2d"]),
    "3d": dict(shape=(40, 48, 50), B=1, squarings=4, amplitude=3.0, noise=0.05, seed=4, branches=["max_second_trip_3d"]),
    "2d_k0": dict(shape=(515, 511), B=2, squarings=0, amplitude=12.0, noise=0.0, seed=5, branches=["scale_second_trip", "backward_k0_scale_second_trip"]),
}



def svf_case_inputs(name):
    """(velocity, dflow) of an SVF case, fp32: svf_ref.smooth_field, dflow with noise 0.5 as in svf_ref.case_inputs."""
    import svf_ref
    c = SVF_CASES[name]
    return (svf_ref.smooth_field(c["B"], c["shape"], c["amplitude"], 7000 + c["seed"], noise=c["noise"]),
            svf_ref.smooth_field(c["B"], c["shape"], 1.0, 8000 + c["seed"], noise=0.5))


CASES = {"flow3":dict(FLOW3_CASES, slab=FLOW3_SLAB, lncc_deep=FLOW3_LNCC_DEEP), "flow2": FLOW2_CASES, "lncc": LNCC_CASES, "bspline": BSPLINE_CASES,
         "svf": SVF_CASES}
