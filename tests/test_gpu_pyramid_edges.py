"""GPU checks of coarse-to-fine resampling where tests/test_gpu_pyramid.py does not look.

A. trx_resample against its fp64 restatement (tests/resample_ref.py) at the edges of the kernel: degenerate and far-off sizes with random
   (not smooth) inputs, batches that run in several chunks, more than 65535 volumes, and guard bytes around the output and the workspace.
B. The conventions themselves, against closed forms that do not use resample_ref: theta is one mapping at every level of the
   align_corners=False pyramid, and upsample_flow is a change of units (channel i along spatial dim i, scale (S-1)/(s-1)).
C. Register(levels > 1) on a batch of pairs, 2-D chains, and a level with no iterations.
"""
import ctypes
import math
import random

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import phantoms as ph
from resample_ref import resample_plan_ref, resample_ref, upsample_flow_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _rand(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 4 - 1).cuda()


def _close(got, want, x, scale=1.0):
    err = (got.double().cpu() - want).abs().max().item()
    bar = 1e-5 * x.abs().max().item() * scale
    assert err <= bar, (err, bar)


def _resample_args(shape, size):
    nd = len(size)
    sp = (1,) * (3 - nd) + tuple(shape[2:])
    so = (1,) * (3 - nd) + tuple(size)
    return (nd, shape[0] * shape[1]) + sp + so


# ---------------------------------------------------------------------------------------------------------------------------------------
# A1. randomised edge sweep
# ---------------------------------------------------------------------------------------------------------------------------------------
def _out_sizes(S):
    return sorted({1, 2, -(-S // 4), S // 2, -(-S // 2), S, S + 1, 2 * S, 3 * S + 1} - {0})


def _edge_cases(n=80, seed=2026):
    """(shape, size, align, channel_scale or None): the fixed cases below, then seeded random ones up to n."""
    cases = []
    for align in (0, 1):
        cases += [((2, 1, 2, 5, 4), (1, 5, 4), align, None),                # 2 -> 1 (D)
                  ((1, 2, 1, 6), (5, 6), align, [1.5, -0.5]),               # 1 -> 5 (H, 2-D)
                  ((1, 1, 3, 4, 64), (3, 4, 5), align, None),               # 64 -> 5 (W)
                  ((2, 1, 6, 5, 3), (6, 64, 3), align, [-2.0])]             # 5 -> 64 (H)
    cases += [((1, 2, 40, 21, 9), (13, 42, 7), 0, [0.75, 1.25]),            # three ratios: three passes, both intermediates
              ((1, 1, 40, 21, 9), (13, 42, 7), 1, None)]
    rng = random.Random(seed)
    pool = [1, 2, 3, 4, 5] + list(range(7, 71))
    while len(cases) < n:
        nd = rng.choice((2, 3))
        sp = tuple(rng.choice(pool) for _ in range(nd))
        size = tuple(rng.choice(_out_sizes(s)) for s in sp)
        if math.prod(sp) > 40000 or math.prod(size) > 40000:
            continue
        B, C = rng.randint(1, 3), rng.randint(1, 3)
        scale = [round(rng.uniform(-2.0, 2.0), 3) for _ in range(C)] if rng.random() < 0.5 else None
        cases.append(((B, C) + sp, size, rng.randint(0, 1), scale))
    return cases


EDGE_CASES = _edge_cases()


@pytest.mark.parametrize("case", range(len(EDGE_CASES)), ids=lambda i: "%s->%s-a%d-%s" % (EDGE_CASES[i][0], EDGE_CASES[i][1],
                                                                                        EDGE_CASES[i][2], "s" if EDGE_CASES[i][3] else "1"))
def test_resample_edge_sweep(tr, case):
    """80 seeded cases (_edge_cases, seed 2026), 2-D and 3-D: every axis on its own shrinks, grows or keeps its size; input sizes from
    {1, 2, 3, 4, 5, 7..70}, output sizes from {1, 2, ceil(S/4), floor(S/2), ceil(S/2), S, S+1, 2S, 3S+1} (at most 40000 voxels either
    side); align_corners 0 / 1; B, C in 1..3, a random channel_scale half of the time.  Fixed cases first, in both alignments:
    2 -> 1 along D, 1 -> 5 along H (2-D), 64 -> 5 along W, 5 -> 64 along H; then (40, 21, 9) -> (13, 42, 7), three ratios so that all
    three passes and both intermediates run.  Inputs are uniform noise, so each stencil weight is checked tap by tap."""
    from torchregister_amd.pyramid import resample
    shape, size, align, scale = EDGE_CASES[case]
    x = _rand(shape, 100 + case)
    y = resample(x, size, align_corners=align, channel_scale=scale)
    assert y.shape == shape[:2] + size
    _close(y, resample_ref(x, size, align, scale), x, max([1.0] + [abs(s) for s in scale or []]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# A4. guard bytes around the output and the workspace (trx_resample through ctypes, the workspace exactly what it reports)
# ---------------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096
OUT_FILL, WS_FILL = 0xA5, 0x5A


def _guarded_resample(x, size, align, channel_scale=None):
    """trx_resample of x with the output and the workspace inside larger buffers filled with a byte pattern; asserts that the bytes
    in front of and behind both regions are untouched.  Returns the output."""
    from torchregister_amd import _lib
    lib = _lib.load()
    args = _resample_args(tuple(x.shape), size)
    ws_bytes = lib.trx_resample_workspace_bytes(*args)
    assert ws_bytes > 0
    B, C = x.shape[:2]
    out_bytes = B * C * math.prod(size) * 4
    obuf = torch.full((GUARD + out_bytes + GUARD,), OUT_FILL, dtype=torch.uint8, device=x.device)
    wbuf = torch.full((GUARD + ws_bytes + GUARD,), WS_FILL, dtype=torch.uint8, device=x.device)
    out = obuf[GUARD:GUARD + out_bytes].view(torch.float32).view((B, C) + tuple(size))
    ws = wbuf[GUARD:GUARD + ws_bytes]
    scale = None if channel_scale is None else (ctypes.c_float * C)(*channel_scale)
    x = x.contiguous()
    rc = lib.trx_resample(_lib.ptr(x), _lib.ptr(out), *args, int(align), C, scale, _lib.ptr(ws), ws_bytes, _lib.current_stream(x.device))
    _lib.check(rc, "trx_resample")
    torch.cuda.synchronize()
    for buf, fill, n in ((obuf, OUT_FILL, out_bytes), (wbuf, WS_FILL, ws_bytes)):
        assert bool((buf[:GUARD] == fill).all()), "bytes written in front of the region"
        assert bool((buf[GUARD + n:] == fill).all()), "bytes written behind the region"
    return out


def test_resample_stays_inside_output_and_workspace_one_chunk(tr):
    """One chunk; chunk * t1 = 1782 floats is not a multiple of 64, so t2 starts after a rounding gap."""
    from torchregister_amd.pyramid import resample
    shape, size = (3, 1, 9, 11, 13), (5, 7, 6)
    chunk, t1, _, t2_off, _ = resample_plan_ref(3, shape[2:], size)
    assert chunk == 3 and (chunk * t1) % 64 != 0 and t2_off > chunk * t1
    x = _rand(shape, 21)
    for align in (0, 1):
        y = _guarded_resample(x, size, align, [0.5])
        _close(y, resample_ref(x, size, align, [0.5]), x)
        assert torch.equal(y, resample(x, size, align_corners=align, channel_scale=[0.5]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# A2. batches in several chunks (each through the guarded call of A4)
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_resample_chunked_batch(tr):
    """(5, 1, 256^3) -> 128^3: 48 MiB of intermediates per volume, chunks of 2 + 2 + 1.  Every output volume is, bit for bit, a call on that
    volume alone (a fixed summation order: no atomics, nothing that depends on the grid); the first volume of each chunk matches the fp64
    reference; the workspace is smaller than the un-chunked need (so a change of RESAMPLE_CHUNK_BYTES fails here rather than quietly
    dropping back to one chunk); nothing is written outside the output or the workspace."""
    from torchregister_amd import _lib
    from torchregister_amd.pyramid import resample
    shape, size = (5, 1, 256, 256, 256), (128, 128, 128)
    chunk, t1, t2, _, ws = resample_plan_ref(5, shape[2:], size)
    assert chunk == 2 and _lib.load().trx_resample_workspace_bytes(*_resample_args(shape, size)) == ws < 5 * (t1 + t2) * 4
    x = _rand(shape, 31)
    y = _guarded_resample(x, size, 0)
    for v in range(5):
        assert torch.equal(y[v:v + 1], resample(x[v:v + 1], size)), v
    for v in (0, 2, 4):
        _close(y[v:v + 1], resample_ref(x[v:v + 1], size), x[v:v + 1])


def test_upsample_flow_chunked(tr):
    """upsample_flow of (1, 3, 128^3) to 256^3: chunks of 2 + 1, the second starting at channel 2 (vol0 = 2 in the kernel's channel index).
    The same shape with three different channel scales, so that a channel index that forgets vol0 shows.  Each channel equals, bit for
    bit, a call on that channel alone with its own scale; channels 0 and 2 (the first of each chunk) match the fp64 reference."""
    from torchregister_amd import _lib
    from torchregister_amd.pyramid import resample
    shape, size = (1, 3, 128, 128, 128), (256, 256, 256)
    chunk, t1, t2, _, ws = resample_plan_ref(3, shape[2:], size)
    assert chunk == 2 and _lib.load().trx_resample_workspace_bytes(*_resample_args(shape, size)) == ws < 3 * (t1 + t2) * 4
    fl = _rand(shape, 41)
    up = tr.upsample_flow(fl, size)
    s = 255 / 127
    scales = [1.5, -2.0, 0.5]
    y = _guarded_resample(fl, size, 1, scales)
    for c in range(3):
        one = fl[:, c:c + 1]
        assert torch.equal(up[:, c:c + 1], resample(one, size, align_corners=True, channel_scale=[s])), c
        assert torch.equal(y[:, c:c + 1], resample(one, size, align_corners=True, channel_scale=[scales[c]])), c
    ref = upsample_flow_ref(fl, size)                                  # fp64, all three channels scaled by s
    for c in (0, 2):                                                   # the first channel of each chunk
        _close(up[:, c:c + 1], ref[:, c:c + 1], fl, s)
        _close(y[:, c:c + 1], ref[:, c:c + 1] * (scales[c] / s), fl, 2.0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# A3. more volumes than gridDim.y holds (65535): the kernel's volume loop
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_resample_more_than_65535_volumes(tr):
    from torchregister_amd.pyramid import resample
    x = _rand((1100, 64, 12, 10), 51)                                   # 70400 volumes at the kernel's 64 channels
    sc = [0.25 + 0.03 * c for c in range(64)]
    sc[63] = -1.75
    y = resample(x, (6, 5), channel_scale=sc)
    _close(y, resample_ref(x, (6, 5), False, sc), x, 1.75)
    x2 = _rand((70000, 1, 3, 4), 52)                                    # growth, one channel
    for align in (0, 1):
        _close(resample(x2, (7, 9), align_corners=align), resample_ref(x2, (7, 9), align), x2)


# ---------------------------------------------------------------------------------------------------------------------------------------
# B6. theta is one mapping at every level of the align_corners=False pyramid
# ---------------------------------------------------------------------------------------------------------------------------------------
def _norm_coord(S):
    """affine_grid's normalised coordinate (align_corners=False) of voxel i on an axis of S voxels, fp64."""
    return (2 * torch.arange(S, dtype=torch.float64) + 1) / S - 1


def _exact_masks(shapes):
    """Per level (coarsest first) and per axis: the voxels where the align_corners=False pyramid of a linear function is still exactly
    linear, i.e. every tap of the blur + interpolation stencil behind them, level by level, lies inside and on an exact voxel."""
    nd = len(shapes[-1])
    masks = [None] * len(shapes)
    masks[-1] = [torch.ones(s, dtype=torch.bool) for s in shapes[-1]]
    for k in range(len(shapes) - 2, -1, -1):
        masks[k] = []
        for d in range(nd):
            S, So, m = shapes[k + 1][d], shapes[k][d], masks[k + 1][d]
            if S == So:
                masks[k].append(m.clone())
                continue
            out = torch.zeros(So, dtype=torch.bool)
            for j in range(So):
                u = max((j + 0.5) * S / So - 0.5, 0.0)
                i0 = min(int(u), S - 1)
                out[j] = i0 - 2 >= 0 and i0 + 3 <= S - 1 and bool(m[i0 - 2:i0 + 4].all())
            masks[k].append(out)
    return masks


def _thetas(nd):
    a = math.radians(12.0)
    c, s = math.cos(a), math.sin(a)
    if nd == 2:
        out = [[[c, -s, 0.05], [s, c, -0.08]], [[0.85, 0.0, 0.0], [0.0, 1.15, 0.0]], [[1.0, 0.0, 0.12], [0.0, 1.0, -0.07]]]
    else:
        out = [[[c, -s, 0.0, 0.05], [s, c, 0.0, -0.08], [0.0, 0.0, 1.0, 0.03]],
               [[0.9, 0.0, 0.0, 0.0], [0.0, 1.12, 0.0, 0.0], [0.0, 0.0, 0.8, 0.0]],
               [[1.0, 0.0, 0.0, 0.1], [0.0, 1.0, 0.0, -0.05], [0.0, 0.0, 1.0, 0.08]]]
    return [torch.tensor(t, dtype=torch.float64)[None] for t in out]


@pytest.mark.parametrize("spatial,seed", [((45, 33, 70), 1), ((9, 130, 37), 2), ((61, 44), 3)])
def test_theta_is_one_mapping_at_every_level(tr, spatial, seed):
    """x = a . p + c with p affine_grid's normalised coordinates (align_corners=False).  The binomial blur and linear interpolation keep a
    linear function away from the border, and a coarse level of the align_corners=False pyramid covers the same extent, so every level of
    pyramid(x, 3) warped by get_affine_warp(theta) equals a . (theta . [p, 1]) + c wherever the sample point's taps lie on exact voxels
    (_exact_masks).  (9, 130, 37) keeps its 9 voxels under MIN_SIZE; (45, 33, 70) and (61, 44) have odd sizes, whose ceil(s/2) levels
    do not line up with the finer voxel centres.  Negative control: the align_corners=True pyramid misses by far more than the bar."""
    nd = len(spatial)
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(nd, generator=g, dtype=torch.float64) + 0.5) * torch.tensor([1.0, -1.0, 1.0][:nd], dtype=torch.float64)
    c0 = 0.3
    p = torch.meshgrid(*[_norm_coord(s) for s in spatial], indexing="ij")
    x = (sum(a[d] * p[d] for d in range(nd)) + c0)[None, None]
    xg = x.float().cuda()
    shapes = tr.pyramid_shapes(spatial, 3)
    masks = _exact_masks(shapes)
    lv, lv_ac = tr.pyramid(xg, 3), tr.pyramid(xg, 3, align_corners=True)
    xmax = x.abs().max().item()
    bar = 2e-5 * xmax
    worst, control = 0.0, 0.0
    for th in _thetas(nd):
        for k, s in enumerate(shapes):
            grid = F.affine_grid(th, (1, 1) + tuple(s), align_corners=False)[0]          # [*s, nd]: (x, y, z) = (W, H, D)
            want = sum(a[d] * grid[..., nd - 1 - d] for d in range(nd)) + c0
            inside = torch.ones(tuple(s), dtype=torch.bool)
            for d in range(nd):
                u = ((grid[..., nd - 1 - d] + 1) * s[d] - 1) / 2                     # the sample point in voxel units of level k
                f = torch.floor(u).long()
                ok = (f >= 0) & (f + 1 <= s[d] - 1)
                m = masks[k][d]
                inside &= ok & m[f.clamp(0, s[d] - 1)] & m[(f + 1).clamp(0, s[d] - 1)]
            assert inside.sum().item() >= 0.1 * inside.numel(), (s, inside.sum().item())
            got = tr.get_affine_warp(th.float().cuda(), lv[k]).double().cpu()[0, 0]
            worst = max(worst, (got - want)[inside].abs().max().item())
            if k < len(shapes) - 1:
                got_ac = tr.get_affine_warp(th.float().cuda(), lv_ac[k]).double().cpu()[0, 0]
                control = max(control, (got_ac - want)[inside].abs().max().item())
    # measured on the MI355X: worst 1.6e-7 .. 2.0e-7 of max|x| (fp32 rounding), the align_corners=True control 1.8e-2 .. 2.9e-2
    print(f"theta across levels {spatial}: worst {worst / xmax:.2e} of max|x|, align_corners=True control {control / xmax:.2e}")
    assert worst <= bar, (worst, bar)
    assert control > 100 * bar, (control, bar)


# ---------------------------------------------------------------------------------------------------------------------------------------
# B7. the flow hand-over is a change of units
# ---------------------------------------------------------------------------------------------------------------------------------------
def _voxel_grid(shape):
    return torch.meshgrid(*[torch.arange(s, dtype=torch.float64) for s in shape], indexing="ij")


@pytest.mark.parametrize("coarse,fine,seed", [((9, 33, 17), (9, 65, 33), 1), ((12, 20), (23, 40), 2)])
def test_upsample_flow_is_a_change_of_units(tr, coarse, fine, seed):
    """f(j) = A j + b per channel on the coarse grid (voxel units, different A and b per channel).  (a) upsample_flow(f, S) is the closed
    form scale * f(i / scale), scale_d = (S_d - 1) / (s_d - 1) (1 where the axis keeps its size): linear interpolation with
    align_corners=True is exact on it.  (b) With a linear image r on the fine grid and its restriction r(j * scale) on the coarse one
    (the align_corners=True pyramid, checked here too), SpatialTransformer of the fine image by the upsampled flow, the coarse warp
    interpolated to the fine grid, and the closed form r(i + up(i)) agree at interior voxels.  Channel order, scale and alignment of the
    hand-over are pinned without resample_ref."""
    nd = len(coarse)
    g = torch.Generator().manual_seed(seed)
    A = (torch.rand(nd, nd, generator=g, dtype=torch.float64) - 0.5) * 0.1       # [channel, spatial dim]
    b = (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) * 3.0
    scale = [1.0 if S == s else (S - 1) / (s - 1) for S, s in zip(fine, coarse)]
    assert len(set(scale)) > 1
    J = _voxel_grid(coarse)
    f = torch.stack([sum(A[c, d] * J[d] for d in range(nd)) + b[c] for c in range(nd)])[None]
    up = tr.upsample_flow(f.float().cuda(), fine).double().cpu()
    I = _voxel_grid(fine)
    want = torch.stack([scale[c] * (sum(A[c, d] * I[d] / scale[d] for d in range(nd)) + b[c]) for c in range(nd)])[None]
    err = (up - want).abs().max().item()
    assert err <= 1e-5 * f.abs().max().item() * max(scale), err

    # (b) semantics
    gr = torch.tensor([0.7, -0.4, 0.25][:nd], dtype=torch.float64)
    r = lambda pts: sum(gr[d] * pts[d] for d in range(nd)) + 1.5                 # noqa: E731
    r_fine = r(I)[None, None]
    r_coarse = r([J[d] * scale[d] for d in range(nd)])[None, None]
    pyr = tr.pyramid(r_fine.float().cuda(), 2, align_corners=True)             # the flow path's pyramid is this restriction
    assert tuple(pyr[0].shape[2:]) == tuple(coarse)
    cm = torch.ones(coarse, dtype=torch.bool)
    for d in range(nd):
        if coarse[d] != fine[d]:                                 # the 6-tap stencil behind coarse voxel j starts at floor(j * scale) - 2
            i0 = (J[d] * scale[d]).floor()
            cm &= (i0 >= 2) & (i0 + 3 <= fine[d] - 1)
    _close_masked(pyr[0].double().cpu()[0, 0], r_coarse[0, 0], cm, r_fine)

    warp_f = tr.SpatialTransformer(fine)(r_fine.float().cuda(), up.float().cuda()).double().cpu()[0, 0]
    warp_c = tr.SpatialTransformer(coarse)(r_coarse.float().cuda(), f.float().cuda()).double().cpu()
    warp_c_up = F.interpolate(warp_c, size=fine, mode="trilinear" if nd == 3 else "bilinear", align_corners=True)[0, 0]
    closed = r([I[d] + want[0, d] for d in range(nd)])
    # interior: the fine sample point strictly inside, and both coarse taps of the interpolation on coarse voxels whose sample is inside
    fm = torch.ones(fine, dtype=torch.bool)
    for d in range(nd):
        u = I[d] + want[0, d]
        fm &= (u >= 0) & (u < fine[d] - 1)
    cin = torch.ones(coarse, dtype=torch.bool)
    for d in range(nd):
        u = J[d] + f[0, d]
        cin &= (u >= 0) & (u < coarse[d] - 1)
    taps = [(I[d] / scale[d]).floor().long() for d in range(nd)]
    for corner in range(2 ** nd):
        t = [(taps[d] + ((corner >> d) & 1)).clamp(max=coarse[d] - 1) for d in range(nd)]
        fm &= cin[tuple(t)]
    assert fm.sum().item() >= 0.2 * fm.numel(), fm.sum().item()
    _close_masked(warp_f, closed, fm, r_fine)
    _close_masked(warp_c_up, closed, fm, r_fine)
    _close_masked(warp_f, warp_c_up, fm, r_fine)


def _close_masked(got, want, mask, x, rel=2e-5):
    err = (got - want)[mask].abs().max().item()
    bar = rel * x.abs().max().item()
    assert err <= bar, (err, bar)


# ---------------------------------------------------------------------------------------------------------------------------------------
# C8. Register(levels=3) on a batch of three pairs
# ---------------------------------------------------------------------------------------------------------------------------------------
POSES = [[[0.96, -0.17, 0.02, 0.06], [0.17, 0.96, 0.0, -0.04], [0.0, 0.03, 1.0, 0.03]],
         [[1.05, 0.0, 0.04, -0.05], [0.0, 0.95, 0.1, 0.02], [-0.03, 0.0, 1.0, 0.0]],
         [[0.98, 0.1, 0.0, 0.0], [-0.1, 0.98, 0.0, 0.07], [0.0, 0.0, 0.97, -0.06]]]


def _batch(shape=(36, 32, 40)):
    from oracle import compose
    movs = [ph.blobs(shape, 11 + i) for i in range(3)]
    tgts = [compose.affine_warp(torch.tensor(POSES[i])[None], movs[i]) for i in range(3)]
    return torch.cat(movs).cuda(), torch.cat(tgts).cuda()


def _affine_chain(tr, mov, tgt, mode, optimizer, lrs, eps, init):
    """The hand-written per-level chain: final parameters handed up unchanged.  Returns the last solver and per-level bodies."""
    movs, tgts = tr.pyramid(mov, len(eps)), tr.pyramid(tgt, len(eps))
    curves, bodies = [], []
    for k in range(len(eps)):
        s = tr.AffineSolver(movs[k], tgts[k], mode=mode, loss=tr.LossSpec(w_mse=1.0), optimizer=optimizer, lr=lrs[k], init=init,
                            capacity=max(1, eps[k]))
        s.run(eps[k])
        init = s.param[:, :6].clone() if mode == "rigid" else s.current_theta
        curves.append(s.losses[:, :eps[k]])
        bodies.append(s.bodies() if eps[k] else None)
    return s, curves, bodies


@pytest.mark.parametrize("mode,optimizer,lrs", [("affine", "sgd", [0.5, 0.2, 0.1]), ("rigid", "adam", [2e-2, 2e-2, 1e-2])])
def test_affine_family_levels_on_a_batch(tr, mode, optimizer, lrs):
    """B = 3 pairs with different poses over 3 levels: Register equals the hand-written chain on the batch bit for bit, and each pair's
    theta equals a Register run on that pair alone.  The latter is exact when B = 1 and B = 3 run the same kernel bodies at every level
    (asserted from AffineSolver.bodies()); pairs are independent, so the same body gives the same bits."""
    mov, tgt = _batch()
    eps = [30, 15, 8]
    init = None
    if mode == "rigid":
        init = torch.tensor([[0.02, -0.01, 0.03, 0.05, -0.02, 0.01], [0.0, 0.02, -0.02, -0.04, 0.03, 0.0],
                             [-0.03, 0.0, 0.01, 0.02, 0.0, -0.05]], device="cuda")
    reg = tr.Register(mode, criterion=[nn.MSELoss()], weight=[1.0], optimizer=optimizer, init=init, levels=3)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    s, curves, bodies = _affine_chain(tr, mov, tgt, mode, optimizer, lrs, eps, init)
    assert torch.equal(reg.theta, s.best) and torch.equal(reg.final_theta, s.current_theta)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))
    for i in range(3):
        one_init = None if init is None else init[i:i + 1]
        r1 = tr.Register(mode, criterion=[nn.MSELoss()], weight=[1.0], optimizer=optimizer, init=one_init, levels=3)
        r1.optim(mov[i:i + 1], tgt[i:i + 1], lr=lrs, max_epochs=eps)
        _, _, b1 = _affine_chain(tr, mov[i:i + 1], tgt[i:i + 1], mode, optimizer, lrs, eps, one_init)
        assert [b[i] for b in bodies] == [b[0] for b in b1], (bodies, b1)
        assert torch.equal(r1.theta, reg.theta[i:i + 1]), i
        assert torch.equal(r1.final_theta, reg.final_theta[i:i + 1]), i
        assert torch.equal(r1.losses, reg.losses[i:i + 1]), i


def _flow_chain(tr, mov, tgt, lrs, eps, sw):
    movs, tgts = tr.pyramid(mov, len(eps), align_corners=True), tr.pyramid(tgt, len(eps), align_corners=True)
    init, curves = None, []
    for k in range(len(eps)):
        s = tr.FlowSolver(movs[k], tgts[k], loss=tr.LossSpec(w_mse=1.0), optimizer="sgd", lr=lrs[k], capacity=max(1, eps[k]),
                          smooth_weight=sw, stop_crit=1e-4, keep_last=True,
                          init=None if init is None else tr.upsample_flow(init, movs[k].shape[2:]))
        s.run(eps[k])
        n = int(s.step.max()) if eps[k] else 0
        init = s.flow
        curves.append(s.losses[:, :n])
    return s, curves


def test_flow_levels_on_a_batch(tr):
    """Direct flow, B = 3, 3 levels: Register equals the hand-written chain on the batch bit for bit, and each pair's flow equals a
    Register run on that pair alone (the flow kernels treat pairs independently, per voxel and per pair)."""
    mov, tgt = _batch((32, 40, 36))
    lrs, eps, sw = [20.0, 10.0, 5.0], [20, 10, 6], 0.05
    reg = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=sw, levels=3)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    s, curves = _flow_chain(tr, mov, tgt, lrs, eps, sw)
    assert torch.equal(reg.final_theta, s.flow) and torch.equal(reg.theta, s.flow_last)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))
    for i in range(3):
        r1 = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=sw, levels=3)
        r1.optim(mov[i:i + 1], tgt[i:i + 1], lr=lrs, max_epochs=eps)
        assert torch.equal(r1.theta, reg.theta[i:i + 1]) and torch.equal(r1.final_theta, reg.final_theta[i:i + 1]), i


# ---------------------------------------------------------------------------------------------------------------------------------------
# C9. 2-D chains
# ---------------------------------------------------------------------------------------------------------------------------------------
def _pair2d(shape=(96, 80), seed=4):
    from oracle import compose
    mov = ph.blobs(shape, seed)
    th = torch.tensor([[0.97, -0.15, 0.05], [0.15, 0.97, -0.04]])[None]
    return mov.cuda(), compose.affine_warp(th, mov).cuda()


def test_rigid_levels_are_the_chain_of_solvers_2d(tr):
    mov, tgt = _pair2d()
    lrs, eps = [2e-2, 1e-2], [25, 12]
    torch.manual_seed(78)
    torch.cuda.manual_seed(78)
    reg = tr.Register("rigid", criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", levels=2)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    torch.manual_seed(78)
    torch.cuda.manual_seed(78)
    pose = torch.rand(3, device="cuda")[None]                     # 2-D rigid: 3 pose parameters, drawn once for the coarsest level
    movs, tgts = tr.pyramid(mov, 2), tr.pyramid(tgt, 2)
    curves = []
    for k in range(2):
        s = tr.AffineSolver(movs[k], tgts[k], mode="rigid", loss=tr.LossSpec(w_mse=1.0), optimizer="adam", lr=lrs[k], init=pose, capacity=eps[k])
        s.run(eps[k])
        pose = s.param[:, :3].clone()
        curves.append(s.losses[:, :eps[k]])
    assert reg.level_shapes == [(48, 40), (96, 80)]
    assert torch.equal(reg.theta, s.best) and torch.equal(reg.final_theta, s.current_theta)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))


def test_flow_levels_are_the_chain_of_solvers_2d(tr):
    mov, tgt = _pair2d((90, 77), 6)
    lrs, eps, sw = [20.0, 8.0], [20, 10], 0.05
    reg = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=sw, levels=2)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    s, curves = _flow_chain(tr, mov, tgt, lrs, eps, sw)
    assert reg.level_shapes == [(45, 39), (90, 77)]
    assert torch.equal(reg.final_theta, s.flow) and torch.equal(reg.theta, s.flow_last)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))
    assert reg(mov).shape == mov.shape


# ---------------------------------------------------------------------------------------------------------------------------------------
# C10. a level with max_epochs 0 passes its starting parameters through
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["affine", "rigid", "flow"])
def test_level_with_no_iterations_passes_through(tr, mode):
    """max_epochs=[0, 10, 10]: the coarsest level runs no iteration and hands its starting parameters up unchanged, so the result is the
    two-level chain on the finer levels started where the coarsest level would have started (affine: identity; rigid: the drawn pose;
    flow: zero)."""
    mov, tgt = _batch((32, 36, 40))
    mov, tgt = mov[:1], tgt[:1]
    eps = [0, 10, 10]
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    if mode == "flow":
        lrs = [20.0, 10.0, 5.0]
        reg = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=0.05, levels=3)
        reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
        s, curves = _flow_chain(tr, mov, tgt, lrs, eps, 0.05)
        assert torch.equal(reg.final_theta, s.flow) and torch.equal(reg.theta, s.flow_last)
    else:
        lrs = [0.5, 0.2, 0.1] if mode == "affine" else [2e-2] * 3
        opt = "sgd" if mode == "affine" else "adam"
        reg = tr.Register(mode, criterion=[nn.MSELoss()], weight=[1.0], optimizer=opt, levels=3)
        reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
        torch.manual_seed(5)
        torch.cuda.manual_seed(5)
        init = torch.rand(6, device="cuda")[None] if mode == "rigid" else None
        movs, tgts = tr.pyramid(mov, 3), tr.pyramid(tgt, 3)
        curves = [reg.level_losses[0]]
        for k in (1, 2):                                          # the coarsest level skipped: its start is the next level's start
            s = tr.AffineSolver(movs[k], tgts[k], mode=mode, loss=tr.LossSpec(w_mse=1.0), optimizer=opt, lr=lrs[k], init=init, capacity=eps[k])
            s.run(eps[k])
            init = s.param[:, :6].clone() if mode == "rigid" else s.current_theta
            curves.append(s.losses[:, :eps[k]])
        assert torch.equal(reg.theta, s.best) and torch.equal(reg.final_theta, s.current_theta)
    assert reg.level_losses[0].shape[-1] == 0
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))


@pytest.mark.parametrize("mode", ["affine", "rigid", "flow"])
def test_level_with_no_iterations_on_the_generic_path(tr, mode):
    """The same on the autograd path (a criterion with no fused form, honoured): levels=2 with max_epochs=[0, 5] is levels=1 with 5
    iterations, bit for bit (the coarsest level passes its start through, and the start is the same)."""
    mov, tgt = _pair2d((64, 48), 8)
    out = []
    for levels, eps in ((2, [0, 5]), (1, 5)):
        torch.manual_seed(9)
        torch.cuda.manual_seed(9)
        if mode == "flow":
            reg = tr.Register("flow", criterion=[nn.L1Loss()], weight=[1.0], flow_model="direct", levels=levels)
            reg.optim(mov, tgt, lr=5.0, max_epochs=eps)
        else:
            reg = tr.Register(mode, criterion=[nn.L1Loss()], weight=[1.0], honor_criterion=True, levels=levels)
            reg.optim(mov, tgt, lr=1e-2, max_epochs=eps)
        out.append(reg)
    assert out[0].level_losses[0].numel() == 0
    assert torch.equal(out[0].theta, out[1].theta) and torch.equal(out[0].final_theta, out[1].final_theta)
    assert torch.equal(out[0].losses.cpu(), out[1].losses.cpu())
