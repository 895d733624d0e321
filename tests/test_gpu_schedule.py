"""Register(levels=L, shrink=..., smoothing=..., moving_shrink=..., moving_smoothing=...) on the GPU: a run under a schedule is the hand-written chain of
single-level runs on tr.pyramid(x, L, shrink=, sigma=) levels - the level voxel sizes v S / S_l, the pose / theta / flow handed up as _optim_levels
hands them up - bit for bit.  Every loop used here gives the same bits on every call (each test checks that first), so equality is the bar."""
import numpy as np
import pytest
import torch

import affine_mi_grids_ref as gref
import affine_mi_ref as aref
import mi_mask_ref as mref

pytestmark = pytest.mark.gpu

MSHAPE, TSHAPE = (12, 40, 44), (24, 30, 32)
MVOX, TVOX = (3.0, 0.7, 0.7), (1.2, 0.9, 0.9)      # a CT with thick slices against a nearly isotropic MR


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


@pytest.fixture(scope="module")
def ct_mr():
    return tuple(x.cuda() for x in gref.pair(TSHAPE, MSHAPE))


def _mi(tr, mode="rigid", **kw):
    return tr.Register(mode, criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, **kw)


def _level_voxel(voxel, full, level):
    return tuple(v * s / sl for v, s, sl in zip(voxel, full.shape[2:], level.shape[2:]))


def _chain_rigid(tr, mov, tgt, msched, tsched, pose, lr, epochs):
    """_optim_levels' statements for mode='rigid' with the device loop, on the schedule's levels; returns the last level's Register and the curves."""
    L = len(tsched[0])
    movs, tgts = tr.pyramid(mov, L, shrink=msched[0], sigma=msched[1]), tr.pyramid(tgt, L, shrink=tsched[0], sigma=tsched[1])
    curves = []
    for k in range(L):
        r = _mi(tr, init=pose)
        r.optim(movs[k], tgts[k], lr=lr, max_epochs=epochs, moving_voxel=_level_voxel(MVOX, mov, movs[k]), target_voxel=_level_voxel(TVOX, tgt, tgts[k]))
        pose = r.final_pose
        curves.append(r.losses)
    return r, curves


def _same(a, b):
    return torch.equal(a.theta, b.theta) and torch.equal(a.final_theta, b.final_theta) and torch.equal(a.losses, b.losses)


def test_rigid_mi_on_two_lattices_with_voxel_schedules(tr, ct_mr):
    from torchregister_amd.gaussian import schedule_shapes
    mov, tgt = ct_mr
    pose = aref.pose0(3)
    runs = []
    for _ in range(2):
        reg = _mi(tr, init=pose, levels=3, shrink='voxel')
        reg.optim(mov, tgt, lr=0.01, max_epochs=20, moving_voxel=MVOX, target_voxel=TVOX)
        runs.append(reg)
    assert _same(*runs)      # the fixed-point loop gives the same bits on every call
    reg = runs[0]
    tsched, msched = tr.pyramid_schedule(TSHAPE, 3, TVOX), tr.pyramid_schedule(MSHAPE, 3, MVOX)
    assert [tuple(f) for f in tsched[0]] == [(3, 4, 4), (1, 2, 2), (1, 1, 1)] and [tuple(f) for f in msched[0]] == [(1, 4, 4), (1, 2, 2), (1, 1, 1)]
    assert reg.level_schedule == (tsched, msched)
    assert reg.level_shapes == schedule_shapes(TSHAPE, tsched[0]) == [(8, 8, 8), (24, 15, 16), (24, 30, 32)]
    assert reg.target_shape == TSHAPE and reg(mov).shape == (1, 1) + TSHAPE
    ls = [c.cpu().numpy() for c in reg.level_losses]
    print("rigid + MILoss, shrink='voxel': " + ", ".join(f"{c[0, 0]:.5f} -> {c[0, -1]:.5f}" for c in ls))
    assert all(c.shape == (1, 20) and np.all(np.isfinite(c)) for c in ls)
    last, curves = _chain_rigid(tr, mov, tgt, msched, tsched, pose, 0.01, 20)
    assert torch.equal(reg.theta, last.theta) and torch.equal(reg.final_theta, last.final_theta) and torch.equal(reg.final_pose, last.final_pose)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))
    # the matrices' column norms carry the same voxel sizes
    hdr = _mi(tr, init=pose, levels=3, shrink='voxel')
    hdr.optim(mov, tgt, lr=0.01, max_epochs=[2, 0, 0], moving_affine=_axis_affine(MVOX), target_affine=_axis_affine(TVOX))
    assert [[tuple(f) for f in s[0]] for s in hdr.level_schedule] == [[tuple(f) for f in s[0]] for s in (tsched, msched)]


def _axis_affine(voxel):
    """A voxel-to-world matrix with axis-aligned columns in the tensor's axis order: column a has the norm voxel[a] (rows world x, y, z)."""
    A = torch.zeros(4, 4, dtype=torch.float64)
    for a, v in enumerate(voxel):
        A[2 - a, a] = v      # tensor axis 0 (z) runs along world z, axis 2 (x) along world x
    A[3, 3] = 1.0
    return A


def test_explicit_schedules_and_a_moving_schedule_of_its_own(tr, ct_mr):
    mov, tgt = ct_mr
    pose = aref.pose0(3)
    shrink, smoothing = [(2, 2, 2), (1, 1, 1)], [(0.5, 1.5, 1.5), (0.0, 0.6, 0.6)]
    mshrink = [(1, 3, 3), (1, 1, 1)]
    reg = _mi(tr, init=pose, levels=2, shrink=shrink, smoothing=smoothing, moving_shrink=mshrink)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[12, 8], moving_voxel=MVOX, target_voxel=TVOX)
    tsched = (shrink, [tuple(map(float, s)) for s in smoothing])
    msched = (mshrink, [(0.0, 1.5, 1.5), (0.0, 0.0, 0.0)])      # its own factors without sigmas: f / 2
    assert reg.level_schedule == (tsched, msched) and reg.level_shapes == [(12, 15, 16), TSHAPE]
    tgts, movs = tr.pyramid(tgt, 2, shrink=shrink, sigma=smoothing), tr.pyramid(mov, 2, shrink=mshrink)
    assert not torch.equal(tgts[1], tgt) and torch.equal(tgts[1], tr.gaussian_smooth(tgt, (0.0, 0.6, 0.6))) and movs[1].data_ptr() == mov.data_ptr()
    for k, e in enumerate((12, 8)):
        r = _mi(tr, init=pose)
        r.optim(movs[k], tgts[k], lr=0.01, max_epochs=e, moving_voxel=_level_voxel(MVOX, mov, movs[k]), target_voxel=_level_voxel(TVOX, tgt, tgts[k]))
        pose = r.final_pose
        assert torch.equal(r.losses, reg.level_losses[k])
    assert torch.equal(reg.theta, r.theta) and torch.equal(reg.final_theta, r.final_theta)


def test_affine_ncc_on_one_lattice_with_an_explicit_schedule(tr):
    mov, tgt = (x.cuda() for x in aref.pair((16, 24, 28)))
    shrink = [(1, 2, 2), (1, 1, 1)]
    new = lambda **kw: tr.Register("affine", criterion=[tr.NCCLoss()], weight=[1.0], honor_criterion=True, optimizer="adam", **kw)  # noqa: E731
    runs = []
    for _ in range(2):
        reg = new(init=aref.theta0(3), levels=2, shrink=shrink)
        reg.optim(mov, tgt, lr=2e-3, max_epochs=[20, 10])
        runs.append(reg)
    assert _same(*runs)      # the fused loop gives the same bits on every call
    reg = runs[0]
    assert reg.level_shapes == [(16, 12, 14), (16, 24, 28)] and reg.level_schedule[0] == reg.level_schedule[1] == (shrink, [(0.0, 1.0, 1.0), (0.0, 0.0, 0.0)])
    movs, tgts = tr.pyramid(mov, 2, shrink=shrink), tr.pyramid(tgt, 2, shrink=shrink)
    init = aref.theta0(3)
    for k, e in enumerate((20, 10)):
        r = new(init=init)
        r.optim(movs[k], tgts[k], lr=2e-3, max_epochs=e)
        init = r.final_theta
        assert torch.equal(r.losses, reg.level_losses[k])
    assert torch.equal(reg.theta, r.theta) and torch.equal(reg.final_theta, r.final_theta)
    ls = reg.level_losses[0].cpu().numpy()
    print(f"affine + NCC, shrink {shrink}: coarse {ls[0, 0]:.5f} -> {ls[0, -1]:.5f}")
    assert np.all(np.isfinite(ls)) and ls[0, -1] < ls[0, 0]


def test_bspline_mi_through_an_initial_theta_with_an_explicit_schedule(tr):
    from torchregister_amd.pyramid import level_theta
    shape = (16, 24, 28)
    mov, tgt = (x.cuda() for x in aref.pair(shape))
    theta = aref.theta0(3)[None].cuda()
    shrink, epochs = [(1, 2, 2), (1, 1, 1)], [10, 6]
    new = lambda: tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", spacing=4, levels=2, shrink=shrink)  # noqa: E731
    runs = []
    for _ in range(2):
        reg = new()
        reg.optim(mov, tgt, lr=0.05, max_epochs=epochs, initial=theta)
        runs.append(reg)
    assert _same(*runs) and torch.equal(runs[0].control, runs[1].control)      # the same bits on every call
    reg = runs[0]
    shapes = [(16, 12, 14), shape]
    assert reg.level_shapes == shapes and reg.target_shape == shape
    movs, tgts = tr.pyramid(mov, 2, align_corners=True, shrink=shrink), tr.pyramid(tgt, 2, align_corners=True, shrink=shrink)
    flow = None
    for k in range(2):
        lvl = tr.flow_register(shapes[k], **reg._flow_kw(32, 0.05, epochs[k])).to("cuda")
        lvl.base_flow = None if flow is None else tr.upsample_flow(flow, shapes[k])
        lvl.optimize(movs[k], tgts[k], "cpu", False, mask=None, initial=level_theta(theta, shape, shapes[k], shape, shapes[k]))
        flow = lvl.final_flow
        assert torch.equal(lvl.losses, reg.level_losses[k])
    assert torch.equal(reg.theta, lvl.flow) and torch.equal(reg.final_theta, lvl.final_flow) and torch.equal(reg.control, lvl.control)
    assert reg(mov).shape == (1, 1) + shape


def test_masks_and_overlap_follow_their_image_schedule(tr, ct_mr):
    mov, tgt = ct_mr
    pose = aref.pose0(3)
    mask, mmask = mref.ellipsoid(TSHAPE, 0.9).cuda(), mref.ellipsoid(MSHAPE, 0.95).cuda()
    reg = _mi(tr, init=pose, levels=3, shrink='voxel')
    reg.optim(mov, tgt, lr=0.01, max_epochs=[10, 6, 4], moving_voxel=MVOX, target_voxel=TVOX, mask=mask, moving_mask=mmask, overlap=True)
    assert all(bool(torch.isfinite(c).all()) for c in reg.level_losses) and 0 < float(reg.valid_fraction) <= 1
    tsched, msched = reg.level_schedule
    L = 3
    movs, tgts = tr.pyramid(mov, L, shrink=msched[0], sigma=msched[1]), tr.pyramid(tgt, L, shrink=tsched[0], sigma=tsched[1])
    masks, mmasks = tr.pyramid_masks(mask, L, shrink=tsched[0], sigma=tsched[1]), tr.pyramid_masks(mmask, L, shrink=msched[0], sigma=msched[1])
    assert [tuple(m.shape[2:]) for m in masks] == reg.level_shapes and [tuple(m.shape[2:]) for m in mmasks] == [tuple(x.shape[2:]) for x in movs]
    for k, e in enumerate((10, 6, 4)):
        r = _mi(tr, init=pose)
        r.optim(movs[k], tgts[k], lr=0.01, max_epochs=e, moving_voxel=_level_voxel(MVOX, mov, movs[k]), target_voxel=_level_voxel(TVOX, tgt, tgts[k]),
                mask=masks[k], moving_mask=mmasks[k], overlap=True)
        pose = r.final_pose
        assert torch.equal(r.losses, reg.level_losses[k])      # the level ran on pyramid_masks' masks under the same schedule
    assert torch.equal(reg.theta, r.theta) and torch.equal(reg.valid_fraction, r.valid_fraction)


def test_without_the_keywords_the_pyramid_is_todays(tr):
    mov, tgt = (x.cuda() for x in aref.pair((24, 28, 32)))
    pose = aref.pose0(3)
    reg = _mi(tr, init=pose, levels=3)
    reg.optim(mov, tgt, lr=0.01, max_epochs=[8, 6, 4])
    assert reg.level_schedule is None and reg.level_shapes == tr.pyramid_shapes((24, 28, 32), 3)
    movs, tgts = tr.pyramid(mov, 3, align_corners=False), tr.pyramid(tgt, 3, align_corners=False)
    for k, e in enumerate((8, 6, 4)):
        r = _mi(tr, init=pose)
        r.optim(movs[k], tgts[k], lr=0.01, max_epochs=e)
        pose = r.final_pose
        assert torch.equal(r.losses, reg.level_losses[k])
    assert torch.equal(reg.theta, r.theta) and torch.equal(reg.final_theta, r.final_theta)
