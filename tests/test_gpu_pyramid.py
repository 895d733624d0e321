"""GPU checks of coarse-to-fine registration: trx_resample against its fp64 torch restatement (tests/resample_ref.py), pyramid and
upsample_flow level by level, Register(levels=1) as the single-level path bit for bit, Register(levels=L) as the hand-written chain of
per-level solvers, and the capture range that is the reason for the feature."""
import math

import pytest
import torch
import torch.nn as nn

import phantoms as ph
from resample_ref import resample_ref, upsample_flow_ref

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


@pytest.mark.parametrize("align", [0, 1])
@pytest.mark.parametrize("shape,size", [((1, 1, 64, 64, 64), (32, 32, 32)), ((2, 3, 37, 50, 61), (19, 25, 31)),
                                        ((1, 1, 9, 130, 7), (9, 65, 7)), ((3, 2, 97, 128), (49, 64)),
                                        ((2, 2, 20, 9, 40), (10, 17, 40))])
def test_resample_matches_fp64_reference(tr, shape, size, align):
    from torchregister_amd.pyramid import resample
    x = _rand(shape, 11)
    y = resample(x, size, align_corners=align)
    assert y.shape == shape[:2] + size
    _close(y, resample_ref(x, size, align), x)
    assert torch.equal(y, resample(x, size, align_corners=align))          # deterministic: the same bits on every call


@pytest.mark.parametrize("align", [0, 1])
def test_resample_upsampling_with_channel_scale(tr, align):
    from torchregister_amd.pyramid import resample
    x = _rand((2, 3, 12, 17, 20), 5)
    sc = [1.5, -2.0, 0.5]
    y = resample(x, (23, 33, 40), align_corners=align, channel_scale=sc)
    _close(y, resample_ref(x, (23, 33, 40), align, sc), x, 2.0)
    same = resample(x, (12, 17, 20), align_corners=align, channel_scale=sc)   # no axis changes: only the scale
    _close(same, resample_ref(x, (12, 17, 20), align, sc), x, 2.0)


@pytest.mark.parametrize("align", [False, True])
def test_pyramid_levels_match_reference(tr, align):
    x = _rand((2, 1, 45, 64, 33), 3)
    lv = tr.pyramid(x, 3, align_corners=align)
    shapes = tr.pyramid_shapes(x.shape[2:], 3)
    assert lv[-1] is x and [tuple(t.shape[2:]) for t in lv] == shapes
    for k in range(2):                                           # each level from the level directly above it
        _close(lv[k], resample_ref(lv[k + 1], shapes[k], align), lv[k + 1])
    x2 = _rand((1, 2, 97, 128), 4)
    lv2 = tr.pyramid(x2, 3)
    for k in range(2):
        _close(lv2[k], resample_ref(lv2[k + 1], lv2[k].shape[2:], False), lv2[k + 1])


def test_upsample_flow_matches_reference(tr):
    fl = _rand((2, 3, 12, 16, 20), 6)
    up = tr.upsample_flow(fl, (23, 31, 40))
    _close(up, upsample_flow_ref(fl, (23, 31, 40)), fl, 2.0)
    fl2 = _rand((1, 2, 9, 32), 7)
    up2 = tr.upsample_flow(fl2, (9, 64))                          # an axis that keeps its size keeps its unit
    _close(up2, upsample_flow_ref(fl2, (9, 64)), fl2, 2.0)


def _pair(shape=(32, 32, 32), seed=3):
    mov = ph.blobs(shape, seed).cuda()
    th = torch.tensor([[0.96, -0.17, 0.02, 0.06], [0.17, 0.96, 0.0, -0.04], [0.0, 0.03, 1.0, 0.03]])[None]
    from oracle import compose
    return mov, compose.affine_warp(th, mov.cpu()).cuda()


@pytest.mark.parametrize("mode", ["affine", "rigid"])
def test_levels_one_is_the_single_level_path(tr, mode):
    mov, tgt = _pair()
    out = []
    for kw in ({}, {"levels": 1}):
        torch.manual_seed(1234)
        torch.cuda.manual_seed(1234)
        reg = tr.Register(mode, criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", **kw)
        reg.optim(mov, tgt, lr=1e-2, max_epochs=25)
        out.append(reg)
    assert torch.equal(out[0].theta, out[1].theta) and torch.equal(out[0].losses, out[1].losses)
    assert torch.equal(out[0].final_theta, out[1].final_theta)


def test_levels_one_is_the_single_level_path_flow(tr):
    mov, tgt = _pair()
    out = []
    for kw in ({}, {"levels": 1}):
        reg = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=0.05, **kw)
        reg.optim(mov, tgt, lr=5.0, max_epochs=20)
        out.append(reg)
    assert torch.equal(out[0].theta, out[1].theta) and torch.equal(out[0].losses, out[1].losses)


def test_affine_levels_are_the_chain_of_solvers(tr):
    mov, tgt = _pair((40, 36, 44))
    lrs, eps = [0.5, 0.2, 0.1], [30, 15, 8]
    reg = tr.Register("affine", criterion=[nn.MSELoss()], weight=[1.0], levels=3)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    movs, tgts = tr.pyramid(mov, 3), tr.pyramid(tgt, 3)
    init, curves = None, []
    for k in range(3):
        s = tr.AffineSolver(movs[k], tgts[k], mode="affine", loss=tr.LossSpec(w_mse=1.0), optimizer="sgd", lr=lrs[k], init=init, capacity=eps[k])
        s.run(eps[k])
        init = s.current_theta
        curves.append(s.losses[:, :eps[k]])
    assert reg.level_shapes == [(10, 9, 11), (20, 18, 22), (40, 36, 44)]
    assert torch.equal(reg.theta, s.best) and torch.equal(reg.final_theta, s.current_theta)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves)) and torch.equal(reg.losses, curves[-1])
    assert reg(mov).shape == mov.shape


def test_rigid_levels_are_the_chain_of_solvers(tr):
    mov, tgt = _pair((36, 36, 36), seed=5)
    lrs, eps = 2e-2, [25, 12, 6]
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    reg = tr.Register("rigid", criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", levels=3)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    torch.manual_seed(77)
    torch.cuda.manual_seed(77)
    pose = torch.rand(6, device="cuda")[None]                    # drawn once, for the coarsest level, as a single-level run draws it
    movs, tgts = tr.pyramid(mov, 3), tr.pyramid(tgt, 3)
    curves = []
    for k in range(3):
        s = tr.AffineSolver(movs[k], tgts[k], mode="rigid", loss=tr.LossSpec(w_mse=1.0), optimizer="adam", lr=lrs, init=pose, capacity=eps[k])
        s.run(eps[k])
        pose = s.param[:, :6].clone()
        curves.append(s.losses[:, :eps[k]])
    assert torch.equal(reg.theta, s.best) and torch.equal(reg.final_theta, s.current_theta)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))


def test_flow_levels_are_the_chain_of_solvers(tr):
    mov, tgt = _pair((32, 40, 36), seed=9)
    lrs, eps, sw = [20.0, 10.0, 5.0], [20, 10, 6], 0.05
    reg = tr.Register("flow", criterion=[nn.MSELoss()], weight=[1.0], flow_model="direct", smooth_weight=sw, levels=3)
    reg.optim(mov, tgt, lr=lrs, max_epochs=eps)
    movs, tgts = tr.pyramid(mov, 3, align_corners=True), tr.pyramid(tgt, 3, align_corners=True)
    init, curves = None, []
    for k in range(3):
        s = tr.FlowSolver(movs[k], tgts[k], loss=tr.LossSpec(w_mse=1.0), optimizer="sgd", lr=lrs[k], capacity=eps[k], smooth_weight=sw,
                          stop_crit=1e-4, keep_last=True, init=None if init is None else tr.upsample_flow(init, movs[k].shape[2:]))
        s.run(eps[k])
        n = int(s.step.max())
        init = s.flow
        curves.append(s.losses[:, :n])
    assert torch.equal(reg.final_theta, s.flow) and torch.equal(reg.theta, s.flow_last)
    assert all(torch.equal(a, b) for a, b in zip(reg.level_losses, curves))
    assert reg(mov).shape == mov.shape


def test_default_criterion_levels_2d(tr):
    """criterion=None (MSE + NCC + NMI through the dedicated NMI loop) on a small 2-D pair: both levels run and their curves fall."""
    mov = ph.blobs((96, 80), 4).cuda()
    from oracle import compose
    tgt = compose.affine_warp(torch.tensor(ph.THETA_STAR2)[None], mov.cpu()).cuda()
    reg = tr.Register("affine", levels=2)
    reg.optim(mov, tgt, lr=1e-4, max_epochs=[40, 20])
    assert len(reg.level_losses) == 2 and reg.level_shapes == [(48, 40), (96, 80)]
    for c in reg.level_losses:
        c = c.flatten().cpu()
        assert torch.isfinite(c).all() and c[-1] < c[0], c


# ---- capture range: a pose beyond the single-level basin (chosen with oracle/compose.py on the CPU at 64^3, same schedule) ----
CAPTURE_DEG, CAPTURE_T, CAPTURE_LR = 40.0, (0.1, -0.06, 0.04), 0.02
CAPTURE_ERR, CAPTURE_RATIO = 0.2, 0.0075


def _capture_case():
    a = math.radians(CAPTURE_DEG)
    th = torch.tensor([[math.cos(a), -math.sin(a), 0.0, CAPTURE_T[0]], [math.sin(a), math.cos(a), 0.0, CAPTURE_T[1]],
                       [0.0, 0.0, 1.0, CAPTURE_T[2]]])[None]
    mov = ph.blobs((64, 64, 64), 3)
    from oracle import compose
    return mov.cuda(), compose.affine_warp(th, mov).cuda(), th.cuda()


def test_levels_widen_the_capture_range(tr):
    mov, tgt, th = _capture_case()
    l0 = torch.mean((tr.get_affine_warp(torch.eye(3, 4, device="cuda")[None], mov) - tgt) ** 2).item()
    res = {}
    for levels, eps in ((3, [200, 100, 50]), (1, 350)):
        reg = tr.Register("affine", criterion=[nn.MSELoss()], weight=[1.0], optimizer="adam", levels=levels)
        reg.optim(mov, tgt, lr=CAPTURE_LR, max_epochs=eps)
        err = (reg.theta - th).abs().max().item()
        ratio = torch.mean((reg(mov) - tgt) ** 2).item() / l0
        res[levels] = (err, ratio)
    print("capture range: levels=3 err %.4f loss ratio %.5f | levels=1 err %.4f loss ratio %.5f" % (*res[3], *res[1]))
    assert res[3][0] <= CAPTURE_ERR and res[3][1] <= CAPTURE_RATIO, res
    assert res[1][0] > CAPTURE_ERR and res[1][1] > CAPTURE_RATIO, res
