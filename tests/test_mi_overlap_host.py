"""Host-side checks of the overlap rule (trx_moving_grid.overlap / .mask), no GPU: what the rule is for (the crop phantom,
tests/mi_overlap_ref.py), the conditions tests/test_gpu_mi_overlap.py relies on (the border condition, the valid shares, the arbiter's two
precisions), and the interface - the struct against the ctypes mirror, every refusal of the C entry points through unmapped pointers, every
refusal of the Python layer with CPU tensors, and a valid request reaching "no CPU fallback"."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import affine_mi_grids_ref as gref
import mi_overlap_ref as oref
import mi_ref
from test_affine_mi_grids_host import _cfg, _grid, _vol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5      # trx_status (include/trx.h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. what it is for
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_what_it_is_for_in_the_arbiter():
    """phantoms.blobs((20,24,28), 5) as target; 1 + 4w(1 - w) of it (background 1, not 0) cropped to slices 3 .. 14 along z as moving image, so the true
    affine is diag(1, 1, 5/3) with a z translation of 1/6.  Affine, Adam 0.002, 150 iterations in fp64 from 0.04 off the truth on every entry (signs
    alternating); 60 % of the target samples overlap at the truth.  Measured: overlap only ends 0.0011 from the truth (z scale -0.006 %); with the
    zero padding counted and the range widened to 0 the run ends 0.051 away (z scale -3.1 %) - farther than it started."""
    err_o, z_o, share = oref.crop_run(True)
    err_z, z_z, _ = oref.crop_run(False)
    print(f"overlap at the truth {share:.3f}; final max|theta - truth|: overlap only {err_o:.4f} (z scale {100 * z_o:+.3f} %), zero padding {err_z:.4f} (z scale {100 * z_z:+.3f} %)")
    assert 0.4 < share < 0.95
    assert err_o <= 0.005
    assert err_z > 0.03


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. - 4. the conditions the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oref.CASES))
def test_cases_meet_the_border_condition_and_the_valid_share(name):
    """No sample of a GPU case lies within 1e-4 voxel of a decision (a border plane of the moving image, or a rounding boundary of the moving-mask
    lookup that changes the answer): the fp32 kernels and the fp64 restatement then agree on every validity bit.  40 % .. 95 % of a pair's samples
    are valid, and no moving size exceeds mi_overlap_ref.MAX_SIZE = 40, so a decision is taken at a coordinate of at most 39: the margin is 7 x the
    6 * 40 * 2^-24 = 1.4e-5 by which the six fp32 operations behind such a coordinate can round."""
    mov, tgt, theta, scale, tmask, mmask, _ = oref.case(name)
    mshape = tuple(mov.shape[2:])
    i = oref.affine_coords(theta, scale, mshape, tgt.shape[2:])
    valid = oref.valid_of(i, mshape, tmask, mmask)
    share = valid.double().flatten(1).mean(1)
    print(f"{name}: valid share {share.tolist()}, max |i| {i.abs().max().item():.1f}")
    assert oref.border_stable(i, mshape, tmask, mmask)
    assert bool((share > 0.40).all()) and bool((share < 0.95).all())
    assert max(mshape) <= oref.MAX_SIZE and i[valid[:, 0]].abs().max().item() <= oref.MAX_SIZE - 1 and oref.MARGIN / (6 * oref.MAX_SIZE * 2.0 ** -24) > 6.9
    v32 = oref.valid_of(oref.affine_coords(theta, scale, mshape, tgt.shape[2:], torch.float32), mshape, tmask, mmask)
    assert torch.equal(v32, valid)
    if name == "3chunks-mmask":      # three blocks per pair, each with valid and invalid voxels
        flat = valid.reshape(2, -1)
        for b in range(2):
            for k in range(3):
                part = flat[b, k * 16384:(k + 1) * 16384]
                assert 0 < int(part.sum()) < part.numel(), (b, k)


@pytest.mark.parametrize("name", list(oref.VALID_CASES))
def test_flow_valid_cases_meet_the_border_condition(name):
    """The cases on which tests/test_gpu_mi_overlap.py holds trx_affine_flow_valid to the restatement byte for byte: the border condition with and
    without the two masks, fp32 and fp64 coordinates deciding every voxel alike, a share of valid samples that exercises both answers."""
    mshape, theta, flow, scale, tmask, mmask = oref.valid_case(name)
    i = oref.flow_coords(theta, flow, mshape, scale)
    i32 = oref.flow_coords(theta, flow, mshape, scale, torch.float32)
    assert max(mshape) <= oref.MAX_SIZE
    for tm, mm in ((None, None), (tmask, mmask)):
        valid = oref.valid_of(i, mshape, tm, mm)
        share = valid.double().flatten(1).mean(1)
        print(f"{name}{' masked' if tm is not None else ''}: valid share {share.tolist()}")
        assert oref.border_stable(i, mshape, tm, mm)
        assert torch.equal(oref.valid_of(i32, mshape, tm, mm), valid)
        assert bool((share > 0.15).all()) and bool((share < 0.97).all())


def test_all_valid_and_none_valid_pairs():
    tshape, mshape = (12, 14, 16), (15, 13, 18)
    ones = gref.scale_of(mshape, tshape)
    for kind, want in (("all", 1.0), ("none", 0.0)):
        i = oref.affine_coords(oref.special_pair(kind), ones, mshape, tshape)
        assert oref.valid_of(i, mshape).double().mean().item() == want and oref.border_stable(i, mshape)


@pytest.mark.parametrize("name", list(oref.LOOPS) + list(oref.FLOW_LOOPS))
def test_loops_meet_the_border_condition_in_every_iteration(name):
    """Every iteration of the fp64 arbiter of every GPU loop: the border condition; the fp32 arbiter decides every validity bit the same way; the two
    loss curves stay within 1e-5 (measured 3e-7 .. 7e-7) although hundreds of samples change validity during a run.  The loss is NOT asserted to
    fall: it jumps when a sample crosses a border plane."""
    flow = name in oref.FLOW_LOOPS
    r64, r32 = oref.flow_loop_pair(name) if flow else oref.loop_pair(name)
    if flow:
        mov, _, _, mmask, *_ = oref.flow_loop_setup(name)
        tmask = None
    else:
        mov, _, _, tmask, mmask, _, _ = oref.loop_setup(name)
    mshape = tuple(mov.shape[2:])
    assert all(oref.border_stable(i, mshape, tmask, mmask) for i in r64[3])
    assert all(torch.equal(a, b) for a, b in zip(r64[2], r32[2]))
    shares = [v.double().mean().item() for v in r64[2]]
    flips = sum(int((r64[2][k] != r64[2][k + 1]).sum()) for k in range(oref.ITERS - 1))
    lgap = np.max(np.abs(r64[0] - r32[0]))
    print(f"{name}: valid share {min(shares):.3f} .. {max(shares):.3f}, {flips} validity changes, loss {r64[0][0]:.4f} -> {r64[0][-1]:.4f}, fp32-fp64 {lgap:.1e}")
    assert 0.40 < min(shares) and max(shares) < 0.95 and flips > 0
    assert np.all(np.isfinite(r64[0])) and lgap <= 1e-5


def test_rows_of_the_cross_lattice_table_as_they_stand():
    """Not a condition, a record: the six rows of affine_mi_grids_ref.LOOPS with the rule switched on and nothing else changed - how close a sample
    comes to a border plane in 10 iterations of the fp64 arbiter and whether the border condition holds.  Printed, and asserted only for the two
    rows the new table keeps unchanged or nearly so (2d-rigid, rigid-voxels): they meet it as they stand."""
    import affine_mi_ref as aref
    import mi_mask_ref as mref
    met = {}
    for name, (tshape, mshape, mode, optimizer, lr, voxels, masked) in gref.LOOPS.items():
        mov, tgt = gref.pair(tshape, mshape)
        scale = gref.scale_of(mshape, tshape, *(voxels or (None, None)))
        tmask = mref.loop_mask(tshape) if masked else None
        r = oref.loop(mov, tgt, oref.fit_range(tgt, mov, tmask), scale, mode, optimizer, lr, oref.ITERS, aref.start_of(tshape, mode),
                      dict(bins=32, alpha=1.0, normalized=False), torch.float64, tmask)
        S = torch.tensor(mshape[::-1], dtype=torch.float64) - 1
        dist = min(torch.minimum(i.abs(), (i - S).abs()).min().item() for i in r[3])
        met[name] = all(oref.border_stable(i, mshape, tmask) for i in r[3])
        print(f"{name}: minimum distance of a coordinate to a border plane {dist:.1e}, border condition {'met' if met[name] else 'missed'}")
    assert met["2d-rigid"] and met["rigid-voxels"]


def test_restatement_is_the_masked_criterion_on_the_validity():
    """evaluate() against its parts: the masked criterion of tests/mi_mask_ref.py on the validity; sum(P) = 1; the gradient is that of the masked chain
    (validity constant), checked by central differences that keep the validity set fixed."""
    mov, tgt, theta, scale, tmask, mmask, rng = oref.case("3d-voxels-mmask")
    loss, g, P, valid = oref.evaluate(mov, tgt, theta, scale, rng, tmask, mmask)
    l2, g2, P2 = gref.evaluate(mov, tgt, theta, scale, rng, mask=valid)
    assert torch.equal(loss, l2) and torch.equal(g, g2) and torch.allclose(P.sum((1, 2)), torch.ones(2, dtype=torch.float64), atol=1e-12)
    h = 1e-7
    d = torch.zeros(2, 3, 4, dtype=torch.float64)
    d[:, 1, 3] = h
    up, dn = (gref.evaluate(mov, tgt, theta.double() + s * d, scale, rng, mask=valid)[0] for s in (1.0, -1.0))
    fd = (up - dn) / (2 * h)
    assert torch.allclose(fd, g[:, 1, 3], rtol=1e-4, atol=1e-7), (fd, g[:, 1, 3])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_ctypes_mirror(tmp_path):
    """sizeof / offsetof of trx_moving_grid from a compiled C snippet against torchregister_amd._lib.MovingGrid; a zeroed struct means 'off'."""
    from torchregister_amd import _lib
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "trx.h"\nint main(void) { trx_moving_grid g = {0};\n'
                   'printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(trx_moving_grid), offsetof(trx_moving_grid, D), offsetof(trx_moving_grid, W),\n'
                   'offsetof(trx_moving_grid, scale), offsetof(trx_moving_grid, overlap), offsetof(trx_moving_grid, mask), g.overlap, g.mask == NULL);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(["which", c], capture_output=True).returncode == 0), None)
    assert cc is not None, "no C compiler"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    M = _lib.MovingGrid
    assert got == [ctypes.sizeof(M), M.D.offset, M.W.offset, M.scale.offset, M.overlap.offset, M.mask.offset, 0, 1]
    assert M.overlap.offset == 60 and M().overlap == 0 and M().mask is None      # the members of before keep their places: 3 ints and 12 floats


def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    vol = _vol(_lib)
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), 32)

    def grid(overlap=0, mask=None, **kw):
        g = _grid(_lib, **kw)
        g.overlap, g.mask = overlap, mask
        return g

    # a moving mask needs the rule; with the rule on the calls get as far as the workspace check, with the query of before
    for g, want in ((grid(0, 4096), ARG), (grid(1, 4096), WS), (grid(1), WS), (grid(7), WS)):
        assert lib.trx_affine_mi_loss_grad_grids(ref(vol), ref(g), ref(_cfg(_lib)), P(4096), P(4096), P(4096), P(4096), n - 1, None) == want
    opt = _lib.OptCfg(_lib.OPT_ADAM, 0.01, 0.9, 0.999, 1e-8)
    st = _lib.AffineState()
    st.mode = _lib.PARAM_AFFINE
    for f in ("param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "losses", "step"):
        setattr(st, f, 4096)
    st.losses_capacity = 5
    for g, want in ((grid(0, 4096), ARG), (grid(1, 4096), WS), (grid(1), WS)):
        assert lib.trx_affine_mi_run_grids(ref(vol), ref(g), ref(_cfg(_lib)), ref(opt), ref(st), 1, P(4096), n - 1, None) == want
    assert lib.trx_affine_mi_run_grids(ref(vol), ref(grid(1, 4096)), ref(_cfg(_lib)), ref(opt), ref(st), 6, P(4096), n, None) == CAP
    assert lib.trx_affine_mi_run_grids(ref(vol), ref(grid(1, 4096)), ref(_cfg(_lib)), ref(opt), ref(st), 0, P(4096), n, None) == OK

    # trx_affine_flow_valid: trx_affine_flow_warp's refusals, and the output
    def valid(v=vol, g=grid(1), theta=4096, flow=4096, out=4096):
        return lib.trx_affine_flow_valid(ref(v), ref(g), P(theta) if theta else None, P(flow) if flow else None, None, P(out) if out else None, None)
    assert valid(v=None) == ARG and valid(g=None) == ARG and valid(theta=None) == ARG and valid(flow=None) == ARG and valid(out=None) == ARG
    assert valid(v=_vol(_lib, ndim=4)) == NDIM and valid(v=_vol(_lib, B=0)) == ARG and valid(v=_vol(_lib, ptr=False)) == ARG
    assert valid(g=grid(1, dhw=(0, 13, 18))) == ARG and valid(g=grid(1, s0=float("nan"))) == ARG and valid(g=grid(1, s5=-1.0)) == ARG
    assert valid(v=_vol(_lib, 2, 1, (1, 13, 17)), g=grid(1, dhw=(2, 21, 15))) == NDIM

    # trx_bspline_mi_run_grids: the validity bytes lie behind the workspace of before
    sp = (ctypes.c_int * 3)(4, 4, 4)
    B, dhw = 2, (12, 14, 16)
    base = lib.trx_bspline_mi_workspace_bytes(3, B, *dhw, 4, 4, 4, 32)
    q = lambda g: lib.trx_bspline_mi_grids_workspace_bytes(3, B, *dhw, 4, 4, 4, 32, ref(g))  # noqa: E731
    assert base > 0 and q(None) == base and q(grid(0)) == base
    assert q(grid(1)) == q(grid(1, 4096)) == base + ((B * 12 * 14 * 16 + 255) // 256) * 256
    assert lib.trx_bspline_mi_grids_workspace_bytes(4, B, *dhw, 4, 4, 4, 32, ref(grid(1))) == 0
    assert lib.trx_bspline_mi_grids_workspace_bytes(3, B, *dhw, 4, 4, 4, 7, ref(grid(1))) == 0
    bs = _lib.BSplineState()
    for f in ("ctrl", "adam_m", "adam_v", "flow", "dflow", "losses", "step"):
        setattr(bs, f, 4096)
    bs.losses_capacity = 5

    def brun(g, nbytes, iters=1):
        return lib.trx_bspline_mi_run_grids(ref(vol), ref(g), P(4096), ref(_cfg(_lib)), ref(opt), ref(bs), sp, iters, P(4096), nbytes, None)
    assert brun(grid(0, 4096), q(grid(1))) == ARG
    assert brun(grid(1), q(grid(1)) - 1) == WS and brun(grid(1, 4096), base) == WS and brun(grid(0), base - 1) == WS
    assert brun(grid(1), q(grid(1)), iters=6) == CAP      # (the next refusal behind a sufficient workspace)
    assert brun(grid(0), base, iters=6) == CAP


def test_entry_points_refuse_before_any_launch():
    check_refusals()


def check_python_refusals(moving, target):
    """Every refusal of the Python layer, with CPU tensors: ValueError before anything touches a device (the GPU path refuses CPU tensors with another
    exception type).  Also run by the GPU suite with CUDA tensors."""
    import torch.nn as nn
    import torchregister_amd as tr
    mi = dict(criterion=[tr.MILoss()], weight=[1.0], optimizer="adam")
    mm = torch.ones((moving.shape[0], 1) + tuple(moving.shape[2:]), dtype=torch.bool)
    theta = torch.eye(3, 4)[None]
    unsupported = (tr.Register("rigid", **mi), tr.Register("affine", **mi, device_loop=False), tr.Register("rigid", criterion=[nn.MSELoss()], weight=[1.0]),
                   tr.Register("flow", **mi, flow_model="direct"), tr.Register("flow", **mi, flow_model="bspline", spacing=4),
                   tr.Register("flow", **mi, flow_model="bspline", spacing=4, levels=2),
                   tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", flow_model="bspline", spacing=4))
    for reg in unsupported:
        for kw in (dict(overlap=True), dict(moving_mask=mm), dict(overlap=True, moving_mask=mm)):
            with pytest.raises(ValueError, match="over the overlap only"):
                reg.optim(moving, target, max_epochs=2, **kw)
        assert reg.valid_fraction is None and reg.theta is None
    with pytest.raises(ValueError, match="over the overlap only"):      # diffeomorphic B-spline: no initial=, so no overlap either
        tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="bspline", spacing=4, diffeomorphic=True).optim(moving, target, max_epochs=2, overlap=True)
    for fn in (tr.affine_register, tr.rigid_register):
        with pytest.raises(ValueError, match="over the overlap only"):
            fn(moving, target, epochs=2, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, overlap=True)
        with pytest.raises(ValueError, match="over the overlap only"):
            fn(moving, target, epochs=2, criterions=[nn.MSELoss()], weights=[1.0], grad_edges=False, moving_mask=mm)
    fr = tr.flow_register(target.shape[2:], flow_model="bspline", spacing=4, criterions=[tr.MILoss()], weights=[1.0])
    with pytest.raises(ValueError, match="over the overlap only"):
        fr.optimize(moving, target, overlap=True)
    # supported loops: the moving mask's own refusals
    loop = tr.Register("rigid", **mi, device_loop=True)
    deform = tr.Register("flow", **mi, flow_model="bspline", spacing=4)
    for reg, kw in ((loop, {}), (deform, dict(initial=theta))):
        with pytest.raises(ValueError, match="overlap=False"):
            reg.optim(moving, target, max_epochs=2, overlap=False, moving_mask=mm, **kw)
        with pytest.raises(ValueError, match="does not match"):
            reg.optim(moving, target, max_epochs=2, moving_mask=torch.ones((moving.shape[0], 1) + tuple(s + 1 for s in moving.shape[2:])), **kw)
        with pytest.raises(ValueError, match="must be a tensor"):
            reg.optim(moving, target, max_epochs=2, moving_mask=[1, 2], **kw)
        assert reg.valid_fraction is None and reg.theta is None
    with pytest.raises(ValueError, match="overlap=False"):
        tr._engine.overlap_args(False, mm, moving)
    assert tr._engine.overlap_args(None, None, moving) == (False, None) and tr._engine.overlap_args(True, None, moving) == (True, None)
    on, m8 = tr._engine.overlap_args(None, mm[:, 0], moving)
    assert on and m8.dtype == torch.uint8 and m8.shape == mm.shape
    for cls_kw in (dict(overlap=True), dict(moving_mask=mm)):      # the B-spline solver itself: the rule needs the composed loop
        with pytest.raises(ValueError, match="initial"):
            tr.BSplineSolver(moving, target, 4, mi=dict(bins=32), **cls_kw)


def test_python_layer_refuses_before_any_device_work():
    check_python_refusals(torch.zeros(1, 1, 9, 7, 6), torch.zeros(1, 1, 5, 6, 7))


def test_a_valid_request_reaches_no_cpu_fallback():
    """CPU tensors and a supported request: every check passes and the call ends at the engine's own refusal of CPU tensors - there is no fallback."""
    import torchregister_amd as tr
    from torchregister_amd import _lib
    mov, tgt = torch.rand(1, 1, 9, 7, 6), torch.rand(1, 1, 5, 6, 7)
    mm = torch.ones(1, 9, 7, 6)
    mi = dict(criterion=[tr.MILoss()], weight=[1.0], optimizer="adam")
    for reg, kw in ((tr.Register("rigid", **mi, device_loop=True), {}), (tr.Register("affine", **mi, device_loop=True, levels=1), dict(mask=torch.ones(1, 5, 6, 7))),
                    (tr.Register("flow", **mi, flow_model="bspline", spacing=4), dict(initial=torch.eye(3, 4)[None]))):
        with pytest.raises(_lib.TrxError, match="no CPU fallback"):
            reg.optim(mov, tgt, max_epochs=2, overlap=True, moving_mask=mm, **kw)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        tr.affine_mi_loss_grad(mov, tgt, torch.eye(3, 4)[None], torch.zeros(1, 4), overlap=True, moving_mask=mm)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        tr.AffineMISolver(mov[:, :, :5, :6, :6].contiguous(), tgt[:, :, :, :, :6].contiguous(), overlap=True)      # one lattice: the rule still takes the cross-lattice path


def test_ranges_under_the_rule():
    """mi_range with the rule: the moving side is the image's own min / max (inside the moving mask), the target side as before."""
    import torchregister_amd as tr
    mov, tgt, _, _, _, mmask, rng = oref.case("3d-voxels-mmask")
    got = tr._engine.mi_range(tgt, mov, overlap=True, moving_mask=mmask)
    assert torch.equal(got, rng)
    assert torch.equal(tr._engine.mi_range(tgt, mov, overlap=True)[:, 2:], torch.stack([mov.flatten(1).amin(1), mov.flatten(1).amax(1)], 1))
    assert torch.equal(tr._engine.mi_range(tgt, mov), mi_ref.fit_range(tgt, mov)) and tr._engine.mi_range(tgt, mov)[1, 2].item() == 0.0      # off: widened to 0, as before
