"""GPU checks of the launch-geometry branches that the small shapes of the per-family tests never select (tests/launch_geometry.py holds the
selection rules and the table of cases; tests/test_launch_geometry_host.py checks on the CPU that each case selects its branch): the wide
blocks, seams and block orders of the 3-D flow column walk, the second trip of the 2-D flow kernels, the z-split instances of the local NCC,
the segmented x pass and the grid caps of the B-spline operators, and the block caps of the SVF kernels.

Every case runs through the public wrappers against the fp64 arbiter of its family, with that family's bars (no new tolerance):
  flow     oracle.c_flow_loss_grad / c_flow_warp and torch autograd loops over oracle/compose.py; loss 2e-5 rel, gradient bar(ref32, ref64,
           1e-4 max), loss curve bar(.., 1e-4 max), flow bar(.., 2e-4); the local-NCC loop 2e-5 / 2e-4 (tests/test_gpu_flow.py, test_gpu_lncc.py)
  lncc     oracle/compose.py::local_ncc_loss under autograd, floors 2e-5 / 2e-4 (tests/test_gpu_lncc.py)
  bspline  tests/bspline_ref.py, 1e-5 max|ctrl| and bar(r32, r64, 1e-5 prod(d) max|dflow|) (tests/test_gpu_bspline.py)
  svf      tests/svf_ref.py, bar(ref32, ref64, 1e-5 max), at most max(4, 0.1 %) elements of the adjoint beyond it, the directional identity to
           1e-4 relative (tests/test_gpu_svf.py)
bar(ref32, ref64, floor) = max(floor, 2 x the arbiter's own fp32-vs-fp64 gap).  Each test prints error and bar."""
import math

import numpy as np
import pytest
import torch

import bspline_ref as bref
import launch_geometry as lg
import loop_arbiters as arb
import oracle
import phantoms as ph
import svf_ref as sref
from conftest import bar

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torchregister_amd._engine as e
    assert torch.cuda.is_available()
    return e


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


def _flow0(shape, amp=0.4):
    """A smooth flow off the voxel lattice, fp32 [1, nd, *shape]: per channel a sum of one sinusoid per axis, plus 0.17."""
    nd = len(shape)
    ax = [torch.arange(n, dtype=torch.float64) for n in shape]
    freq = [[0.21, 0.17, 0.13], [0.11, 0.23, 0.19], [0.15, 0.12, 0.27]]
    chans = []
    for c in range(nd):
        f = torch.zeros(shape, dtype=torch.float64)
        for a in range(nd):
            view = [1] * nd
            view[a] = shape[a]
            f = f + (torch.sin if (a + c) % 2 == 0 else torch.cos)(freq[c][a] * ax[a] + 0.4 * a).view(view)
        chans.append(amp * (1.0 - 0.12 * c) * f)
    return torch.stack(chans).float()[None] + 0.17


# =====================================================================================================================================
# Dense flow, 3-D column walks
# =====================================================================================================================================
@pytest.mark.parametrize("name", sorted(lg.FLOW3_CASES))
def test_flow3_warp_loss_and_gradient_vs_oracle(eng, name):
    """trx_flow_warp, trx_flow_loss_grad (the moments pass and MODE 1 of the update) and trx_flow_warp_backward on the wide and ragged
    block shapes against the C oracle in fp64."""
    shape = lg.FLOW3_CASES[name]["shape"]
    mov, tgt = arb.loop_pair(shape)
    fl = _flow0(shape, 0.9)
    args = lambda dt, **kw: (mov[0, 0].numpy().astype(dt), tgt[0, 0].numpy().astype(dt), fl[0].numpy().astype(dt), oracle.wts(**kw))   # noqa: E731
    w = eng.flow_warp(mov.cuda(), fl.cuda())
    w32, w64 = (oracle.c_flow_warp(mov[0, 0].numpy().astype(dt), fl[0].numpy().astype(dt)) for dt in (np.float32, np.float64))
    e, b = np.max(np.abs(w[0, 0].cpu().numpy() - w64)), bar(w32, w64, 2e-6)
    print(f"flow3 {name} warp: err {e:.3e} bar {b:.3e}")
    assert e <= b, ("warp", e, b)
    refs = {}
    for lname, kw in (("ncc", dict(w_ncc=1.0)), ("mse", dict(w_mse=1.0))):
        terms, dfl = eng.flow_loss_grad(mov.cuda(), tgt.cuda(), fl.cuda(), eng.LossSpec(**kw))
        t64, _, d64, _ = oracle.c_flow_loss_grad(*args(np.float64, **kw))
        _, _, d32, _ = oracle.c_flow_loss_grad(*args(np.float32, **kw))
        refs[lname] = (d32, d64)
        e, b = abs(terms[0, 0].item() - t64), 2e-5 * max(1.0, abs(t64))
        print(f"flow3 {name} {lname} loss: err {e:.3e} bar {b:.3e}")
        assert e <= b, (lname, "loss", e, b)
        e, b = np.max(np.abs(dfl[0].cpu().numpy() - d64)), bar(d32, d64, 1e-4 * np.max(np.abs(d64)))
        print(f"flow3 {name} {lname} gradient: err {e:.3e} bar {b:.3e}")
        assert e <= b, (lname, "gradient", e, b)
    go = 2.0 * (w - tgt.cuda()) / w.numel()          # dMSE/dwarped: the generic backward must reproduce dMSE/dflow
    d32, d64 = refs["mse"]
    e, b = np.max(np.abs(eng.flow_warp_backward(mov.cuda(), fl.cuda(), go)[0].cpu().numpy() - d64)), bar(d32, d64, 1e-4 * np.max(np.abs(d64)))
    print(f"flow3 {name} warp backward: err {e:.3e} bar {b:.3e}")
    assert e <= b, ("warp backward", e, b)


def _run_three_ways(eng, mov, tgt, iters, **kw):
    """The fused run in calls of unequal length, single-iteration calls (which cannot fuse) and TRX_FLAG_TWO_PASS_FLOW: bit for bit equal
    (the assertion of test_fused_next_moments_are_bitwise_the_two_pass_steps).  Returns the fused solver."""
    from torchregister_amd import _lib
    a = eng.FlowSolver(mov, tgt, capacity=iters, **kw)
    a.run(iters - 3)
    a.run(2)
    a.run(1)
    b = eng.FlowSolver(mov, tgt, capacity=iters, **kw)
    for _ in range(iters):
        b.run(1)
    c = eng.FlowSolver(mov, tgt, capacity=iters, flags=_lib.FLAG_TWO_PASS_FLOW, **kw)
    c.run(iters)
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(a.losses, other.losses) and torch.equal(a.flow, other.flow)
        if a.adam_m is not None:
            assert torch.equal(a.adam_m, other.adam_m) and torch.equal(a.adam_v, other.adam_v)
    return a


@pytest.mark.parametrize("optimizer,lr,smooth", [("sgd", 1.0, 0.0), ("sgd", 1.0, 5.0), ("adam", 0.05, 0.0), ("adam", 0.05, 2.0)])
@pytest.mark.parametrize("name", sorted(lg.FLOW3_CASES))
def test_flow3_run_vs_torch_autograd_and_fused_equals_two_pass(eng, name, optimizer, lr, smooth):
    """trx_flow_run (SGD / Adam, with and without the smoothness term) from a flow off the lattice, 8 iterations, against torch autograd in
    fp64; the fused form, single-iteration calls and TRX_FLAG_TWO_PASS_FLOW agree bit for bit."""
    shape, iters = lg.FLOW3_CASES[name]["shape"], 8
    mov, tgt = arb.loop_pair(shape)
    f0 = _flow0(shape)
    l32, f32 = arb.torch_flow_loop(mov, tgt, lr, iters, optimizer, smooth, torch.float32, f0)
    l64, f64 = arb.torch_flow_loop(mov, tgt, lr, iters, optimizer, smooth, torch.float64, f0)
    s = _run_three_ways(eng, mov.cuda(), tgt.cuda(), iters, loss=eng.LossSpec(w_ncc=1.0), optimizer=optimizer, lr=lr, init=f0, smooth_weight=smooth)
    e, b = np.max(np.abs(s.losses[0].cpu().numpy() - l64)), bar(l32, l64, 1e-4 * np.max(np.abs(l64)))
    print(f"flow3 {name} {optimizer} smooth {smooth}: loss curve {l64[0]:.5g} -> {l64[-1]:.5g} err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss curve", e, b)
    e, b = np.max(np.abs(s.flow.cpu().numpy() - f64)), bar(f32, f64, 2e-4)
    print(f"flow3 {name} {optimizer} smooth {smooth}: flow err {e:.3e} bar {b:.3e}")
    assert e <= b, ("flow", e, b)
    assert np.max(np.abs(f64 - f0.numpy())) > 1e-3          # the run moved the flow


LNCC_LOOP = [("w70", 5, "sgd", 30.0, 0.0), ("w200", 9, "adam", 0.05, 2.0), ("lncc_deep", 7, "adam", 0.05, 2.0), ("lncc_deep", 3, "sgd", 20.0, 3.0)]


@pytest.mark.parametrize("name,window,optimizer,lr,smooth", LNCC_LOOP)
def test_flow3_lncc_loop_vs_torch_autograd(eng, name, window, optimizer, lr, smooth):
    """trx_flow_lncc_run - the warp written by the moments pass, MODE 2 of the update - on the wide blocks, and at D >= 64, where the
    criterion between them runs its z-split kernels; against the arbiter and the bars of test_gpu_lncc.py."""
    shape, iters = lg.CASES["flow3"][name]["shape"], 6
    mov, tgt = arb.loop_pair(shape)
    f0 = _flow0(shape)
    l32, f32 = arb.torch_lncc_flow_loop(mov, tgt, lr, iters, optimizer, smooth, window, f0, torch.float32)
    l64, f64 = arb.torch_lncc_flow_loop(mov, tgt, lr, iters, optimizer, smooth, window, f0, torch.float64)
    s = eng.FlowSolver(mov.cuda(), tgt.cuda(), optimizer=optimizer, lr=lr, init=f0, capacity=iters, smooth_weight=smooth, lncc=dict(window=window))
    s.run(iters)
    torch.cuda.synchronize()
    e, b = np.max(np.abs(s.losses[0].cpu().numpy() - l64)), bar(l32, l64, 2e-5 * np.max(np.abs(l64)))
    print(f"lncc loop {name} w{window} {optimizer}: loss curve {l64[0]:.5g} -> {l64[-1]:.5g} err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss curve", e, b)
    e, b = np.max(np.abs(s.flow.cpu().numpy() - f64)), bar(f32, f64, 2e-4)
    print(f"lncc loop {name} w{window} {optimizer}: flow err {e:.3e} bar {b:.3e}")
    assert e <= b, ("flow", e, b)
    assert l64[-1] < l64[0]


def test_flow3_slab_split_with_halos_on_the_wide_blocks(eng):
    """test_slab_partition_equals_whole_volume on 128 x 2 blocks: two slabs of 17 and 23 planes, each with a seam of its own, the smoothness
    term with the neighbours' boundary planes copied by hand; the tolerances of that test (loss curve 1e-5 rel, flow 1e-5)."""
    case = lg.FLOW3_SLAB
    shape, bounds, iters = case["shape"], case["bounds"], 6
    mov, tgt = (t.cuda() for t in arb.loop_pair(shape))
    kw = dict(loss=eng.LossSpec(w_ncc=1.0, w_mse=0.3), optimizer="sgd", lr=1.0, capacity=iters, smooth_weight=4.0)
    whole = eng.FlowSolver(mov, tgt, **kw)
    whole.run(iters)
    slabs = [eng.SlabFlowSolver(mov, tgt[:, :, a:b].contiguous(), a, **kw) for a, b in zip(bounds[:-1], bounds[1:])]
    for _ in range(iters):
        planes = [s.boundary_planes() for s in slabs]
        for r, s in enumerate(slabs):
            if s.has_lo:
                s.halo_lo.copy_(planes[r - 1][1])
            if s.has_hi:
                s.halo_hi.copy_(planes[r + 1][0])
        total = sum(s.local_moments().clone() for s in slabs)
        for s in slabs:
            s.apply(total)
    torch.cuda.synchronize()
    for s in slabs:
        assert torch.allclose(s.losses, whole.losses, rtol=1e-5, atol=1e-6)
    flow = torch.cat([s.flow for s in slabs], dim=2)
    e, b = torch.max(torch.abs(flow - whole.flow)).item(), 1e-5 * max(1.0, whole.flow.abs().max().item())
    print(f"flow3 slab {shape} at {bounds}: flow err {e:.3e} bar {b:.3e}, loss {whole.losses[0, 0].item():.5g} -> {whole.losses[0, -1].item():.5g}")
    assert e <= b and whole.flow.abs().max().item() > 1e-3


# =====================================================================================================================================
# Dense flow, 2-D: the second trip of the grid-stride loops
# =====================================================================================================================================
def _err_and_tail(got, want):
    """max |got - want| over the image and over the second-trip voxels alone"""
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return d.max(), arb.tail(d).max()


def test_flow2_second_trip_warps_loss_and_gradient_vs_oracle(eng):
    """(1025, 1027), B = 1: 4096 blocks of 256 threads hold 1 048 576 voxels, the last 4099 are every kernel's second trip - flow_warp_kernel<2>,
    flow_warp_nearest_kernel<2>, flow_warp_bwd_kernel<2>, flow_moments_kernel<2> and MODE 1 of flow_update_kernel<2>.  Inputs without a kink
    within reach (tests/loop_arbiters.py says why), so the bars are the floors, 1e-4 of the largest gradient; the second-trip voxels are held
    to a bar of their own, from their own largest gradient (tests/test_launch_geometry_host.py asserts that it is 1e-3 of it at most, and
    that the loss without those voxels would miss its bar).  Adam's state after one step from zero is (1 - beta1) g and (1 - beta2) g^2:
    the same gradient bars hold the state arrays of the second trip."""
    c = arb.flow2_big()
    mov, tgt, fl = c["mov"].cuda(), c["tgt"].cuda(), c["fl"].cuda()
    w = eng.flow_warp(mov, fl)
    w32, w64 = c["ncc32"][3], c["ncc64"][3]
    (e, et), b = _err_and_tail(w[0, 0].cpu().numpy(), w64), bar(w32, w64, 2e-6)
    print(f"flow2 second trip warp: err {e:.3e} (second trip {et:.3e}) bar {b:.3e}, max|warped| on the second trip {np.abs(arb.tail(w64)).max():.3e}")
    assert e <= b, ("warp", e, b)
    terms, dfl = eng.flow_loss_grad(mov, tgt, fl, eng.LossSpec(w_ncc=1.0))
    t64 = c["ncc64"][0]
    e, b = abs(terms[0, 0].item() - t64), 2e-5 * max(1.0, abs(t64))
    print(f"flow2 second trip ncc loss: err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss", e, b)
    d64, b, bt = arb.flow2_big_gradient_bars("ncc")
    e, et = _err_and_tail(dfl[0].cpu().numpy(), d64)
    print(f"flow2 second trip ncc gradient: err {e:.3e} bar {b:.3e}; second trip: err {et:.3e} bar {bt:.3e} of max {np.abs(arb.tail(d64)).max():.3e}")
    assert e <= b and et <= bt, ("gradient", e, b, et, bt)
    s = eng.FlowSolver(mov, tgt, loss=eng.LossSpec(w_ncc=1.0), optimizer="adam", lr=1e-3, init=c["fl"], capacity=1)
    s.run(1)
    e, et = _err_and_tail(s.adam_m[0].cpu().numpy() / (1.0 - 0.9), d64)
    e2, et2 = _err_and_tail(np.sqrt(s.adam_v[0].cpu().numpy().astype(np.float64) / (1.0 - 0.999)), np.abs(d64))
    print(f"flow2 second trip adam state after one step: m / 0.1 err {e:.3e} (second trip {et:.3e}), sqrt(v / 0.001) err {e2:.3e} (second trip {et2:.3e}), bars {b:.3e} / {bt:.3e}")
    assert max(e, e2) <= b and max(et, et2) <= bt, ("adam state", e, e2, b, et, et2, bt)
    go = 2.0 * (w - tgt) / w.numel()
    d64, b, bt = arb.flow2_big_gradient_bars("mse")
    e, et = _err_and_tail(eng.flow_warp_backward(mov, fl, go)[0].cpu().numpy(), d64)
    print(f"flow2 second trip warp backward: err {e:.3e} bar {b:.3e}; second trip: err {et:.3e} bar {bt:.3e} of max {np.abs(arb.tail(d64)).max():.3e}")
    assert e <= b and et <= bt, ("warp backward", e, b, et, bt)
    # nearest: out = mov[rint(voxel + flow)], zeros outside - the same fp32 add and round-half-even on the CPU, so bit for bit
    H, W = c["shape"]
    py = torch.arange(H, dtype=torch.float32)[:, None] + c["fl"][0, 0]
    px = torch.arange(W, dtype=torch.float32)[None, :] + c["fl"][0, 1]
    ry, rx = torch.round(py).long(), torch.round(px).long()
    inside = (ry >= 0) & (ry < H) & (rx >= 0) & (rx < W)
    want = torch.where(inside, c["mov"][0, 0][ry.clamp(0, H - 1), rx.clamp(0, W - 1)], torch.zeros(()))
    got = eng.flow_warp(mov, fl, nearest=True)[0, 0].cpu()
    moved = int(((ry != torch.arange(H)[:, None]) | (rx != torch.arange(W)[None, :])).reshape(-1)[arb.FLOW2_TAIL:].sum())
    print(f"flow2 second trip nearest warp: {int((got != want).sum())} of {want.numel()} voxels differ (bar 0), {int((~inside).sum())} outside, "
          f"{moved} of the second trip's {want.numel() - arb.FLOW2_TAIL} voxels take another voxel's value")
    assert torch.equal(got, want) and int((~inside).sum()) > 0 and moved > 1000


@pytest.mark.parametrize("variant", sorted(arb.FLOW2_RUNS))
def test_flow2_second_trip_run_vs_torch_autograd(eng, variant):
    """trx_flow_run on the same image, 4 SGD iterations at lr = 500 without (the pipelined update) and with the smoothness term (the lagged
    fused form), against torch autograd in fp64.  The flow stays off the lattice, so the bar is its floor, 2e-4 voxels, while the second-trip
    voxels move by up to 0.15 voxel, half of them by more than 1.6e-3, and the smoothness term alone moves them by up to 0.04
    (tests/test_launch_geometry_host.py asserts those ratios): a second trip that is skipped, mis-indexed or without its neighbours fails.
    Fused, single-iteration calls and TRX_FLAG_TWO_PASS_FLOW agree bit for bit."""
    c, r, v = arb.flow2_big(), arb.flow2_big_run(variant), arb.FLOW2_RUNS[variant]
    s = _run_three_ways(eng, c["mov"].cuda(), c["tgt"].cuda(), v["iters"], loss=eng.LossSpec(w_ncc=1.0), optimizer=v["optimizer"], lr=v["lr"], init=r["f0"],
                        smooth_weight=v["smooth"])
    l32, l64, f32, f64 = r["l32"], r["l64"], r["f32"], r["f64"]
    e, b = np.max(np.abs(s.losses[0].cpu().numpy() - l64)), bar(l32, l64, 1e-4 * np.max(np.abs(l64)))
    print(f"flow2 second trip {variant}: loss curve {l64[0]:.6g} -> {l64[-1]:.6g} err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss curve", e, b)
    (e, et), b, bt = _err_and_tail(s.flow.cpu().numpy(), f64), bar(f32, f64, 2e-4), bar(arb.tail(f32), arb.tail(f64), 2e-4)
    move = np.abs(arb.tail(f64) - arb.tail(r["f0"].numpy()))
    print(f"flow2 second trip {variant}: flow err {e:.3e} bar {b:.3e}; second trip: err {et:.3e} bar {bt:.3e}, moved by up to {move.max():.3e} (median {np.median(move):.3e})")
    assert e <= b and et <= bt, ("flow", e, b, et, bt)
    assert move.max() >= 50 * bt and np.median(move) >= 2 * bt


def test_flow2_second_trip_adam_fused_equals_two_pass(eng):
    """Adam with the smoothness term on the same image: fused, single-iteration calls and TRX_FLAG_TWO_PASS_FLOW bit for bit.  (No arbiter
    here: Adam normalises the step, so where a gradient is ~0 its sign - and a step of lr - differs between any two precisions, and at a
    million voxels the arbiter's own fp32-vs-fp64 gap is larger than any movement.  The optimiser state of the second trip is held to the
    oracle's gradient in test_flow2_second_trip_warps_loss_and_gradient_vs_oracle, its flow update by the SGD runs above.)"""
    c = arb.flow2_big()
    f0 = arb.flow2_big_flow(0.05, fine=0.03)
    s = _run_three_ways(eng, c["mov"].cuda(), c["tgt"].cuda(), 4, loss=eng.LossSpec(w_ncc=1.0, w_mse=0.3), optimizer="adam", lr=0.02, init=f0, smooth_weight=2.0)
    move = np.abs(arb.tail(s.flow.cpu().numpy()) - arb.tail(f0.numpy()))
    print(f"flow2 second trip adam + smoothness: three ways bit for bit; second trip moved by up to {move.max():.3e}")
    assert move.max() > 0.02 and bool(torch.isfinite(s.losses).all())


# =====================================================================================================================================
# Local NCC: the z-split instances
# =====================================================================================================================================
@pytest.mark.parametrize("name", [n for n, c in lg.LNCC_CASES.items() if not c.get("existing")])
def test_lncc_split_instances_vs_torch(eng, name):
    """test_lncc_loss_and_grad_vs_torch at the shapes that select window 7 in the tile form and window 3 with z segments, with and without a
    segment length that divides D."""
    c = lg.LNCC_CASES[name]
    tgt, wrp = arb.lncc_pair(c["shape"], c["B"])
    alpha = 2.5
    l32, g32 = arb.lncc_ref(tgt, wrp, c["window"], alpha, torch.float32)
    l64, g64 = arb.lncc_ref(tgt, wrp, c["window"], alpha, torch.float64)
    loss, grad = eng.local_ncc_loss_grad(tgt.cuda(), wrp.cuda(), c["window"], alpha)
    loss, grad = loss.cpu().numpy(), grad.cpu().numpy()
    e, b = np.max(np.abs(loss - l64)), bar(l32, l64, 2e-5 * np.max(np.abs(l64)))
    print(f"lncc {name} {c['shape']} w{c['window']}: loss err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss", e, b)
    e, b = np.max(np.abs(grad - g64)), bar(g32, g64, 2e-4 * np.max(np.abs(g64)))
    print(f"lncc {name} {c['shape']} w{c['window']}: gradient err {e:.3e} bar {b:.3e}")
    assert e <= b, ("gradient", e, b)


# =====================================================================================================================================
# B-spline operators
# =====================================================================================================================================
@pytest.mark.parametrize("name", list(lg.BSPLINE_CASES))
def test_bspline_expand_and_reduce_at_the_untested_plans(tr, name):
    """test_expand_and_reduce_match_the_restatement (uniform noise in, every tap checked; with a base) at the shapes of the table.  A case
    with B > 1 also repeats its last pair alone - another grid, the same bits."""
    c = lg.BSPLINE_CASES[name]
    B, sp, d = c["B"], c["shape"], c["spacing"]
    nd, seed = len(sp), 40 + list(lg.BSPLINE_CASES).index(name)
    ctrl, base = arb.rand((B, nd) + bref.grid(sp, d), seed), arb.rand((B, nd) + sp, 500 + seed, -2.0, 2.0)
    got = tr.bspline_expand(ctrl.cuda(), sp, d, base=base.cuda())
    assert got.shape == (B, nd) + sp
    want = bref.expand(ctrl, sp, d, base)
    err, tol = (got.double().cpu() - want).abs().max().item(), 1e-5 * (ctrl.abs().max().item() + base.abs().max().item())
    print(f"bspline {name} expand {B}x{sp} d{d}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)
    if B > 1:
        assert torch.equal(got[-1:], tr.bspline_expand(ctrl[-1:].cuda(), sp, d, base=base[-1:].cuda()))
    del want, got

    dflow = arb.rand((B, nd) + sp, 900 + seed)
    got = tr.bspline_reduce(dflow.cuda(), d)
    assert got.shape == ctrl.shape
    r64, r32 = bref.reduce(dflow, d), bref.reduce(dflow, d, dtype=torch.float32)
    err, tol = (got.double().cpu() - r64).abs().max().item(), bar(r32.numpy(), r64.numpy(), 1e-5 * math.prod(d) * dflow.abs().max().item())
    print(f"bspline {name} reduce {B}x{sp} d{d}: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)
    if B > 1:
        assert torch.equal(got[-1:], tr.bspline_reduce(dflow[-1:].cuda(), d))


def test_bspline_loop_on_a_wide_block_with_spacing_32(tr):
    """trx_bspline_run on (17, 3, 70) with spacing (5, 2, 32): the flow part of the loop (trx_flow_loss_grad) on 128 x 2 blocks with a seam,
    against the arbiter and the bars of test_gpu_bspline.py; and two pairs are independent registrations, bit for bit."""
    shape, spacing, iters, lr = lg.FLOW3_CASES["w70"]["shape"], (5, 2, 32), 8, 0.1
    mov = torch.cat([arb.loop_pair(shape, 10 * b)[0] for b in range(2)])
    tgt = torch.cat([arb.loop_pair(shape, 10 * b)[1] for b in range(2)])
    c0 = arb.bspline_ctrl0(2, shape, spacing, 7)
    l64, c64 = arb.bspline_arbiter(mov[:1], tgt[:1], spacing, c0[:1], lr, iters, "adam", torch.float64, w_ncc=1.0)
    l32, c32 = arb.bspline_arbiter(mov[:1], tgt[:1], spacing, c0[:1], lr, iters, "adam", torch.float32, w_ncc=1.0)
    kw = dict(loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=lr, capacity=iters)
    both = tr.BSplineSolver(mov.cuda(), tgt.cuda(), spacing, init=c0, **kw)
    both.run(iters)
    solo = tr.BSplineSolver(mov[1:].cuda(), tgt[1:].cuda(), spacing, init=c0[1:], **kw)
    solo.run(iters)
    torch.cuda.synchronize()
    e, b = np.max(np.abs(both.losses[0].cpu().numpy() - l64)), bar(l32, l64, 2e-5 * np.max(np.abs(l64)))
    print(f"bspline loop {shape} d{spacing}: loss curve {l64[0]:.5g} -> {l64[-1]:.5g} err {e:.3e} bar {b:.3e}")
    assert e <= b, ("loss curve", e, b)
    e, b = np.max(np.abs(both.ctrl[0].cpu().numpy() - c64[0])), bar(c32, c64, 2e-4)
    print(f"bspline loop {shape} d{spacing}: ctrl err {e:.3e} bar {b:.3e}")
    assert e <= b, ("ctrl", e, b)
    assert torch.equal(both.ctrl[1:], solo.ctrl) and torch.equal(both.losses[1:], solo.losses) and torch.equal(both.flow[1:], solo.flow)
    assert not torch.equal(both.ctrl.cpu(), c0)


# =====================================================================================================================================
# SVF: the block caps
# =====================================================================================================================================
_SVF = {}


def _svf_case(name):
    if name not in _SVF:
        c = lg.SVF_CASES[name]
        v, g = lg.svf_case_inputs(name)
        K = c["squarings"]
        _SVF[name] = dict(v=v, g=g, K=K, f64=sref.exp(v, K), f32=sref.exp(v, K, dtype=torch.float32), b64=sref.exp_backward(v, g, K),
                          b32=sref.exp_backward(v, g, K, dtype=torch.float32))
    return _SVF[name]


def _directions(c, n, eps=1e-4, amplitude=0.01, candidates=8):
    """svf_ref.directions for a case of this file: n smooth directions d (max |eps d| = 1e-6) with the fp64 difference quotient of exp, kept
    only if the restatement's own fp64 adjoint meets the identity to 1e-6 relative (no kink inside the quotient)."""
    v64, g64 = c["v"].double(), c["g"].double()
    kept = []
    for j in range(candidates):
        d = amplitude * sref.smooth_field(v64.shape[0], tuple(v64.shape[2:]), 1.0, 9000 + j, noise=0.0).double()
        rhs = (g64 * (sref.exp(v64 + eps * d, c["K"]) - sref.exp(v64 - eps * d, c["K"])) / (2 * eps)).sum().item()
        lhs = (c["b64"] * d).sum().item()
        if abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)):
            kept.append((d, rhs))
        if len(kept) == n:
            break
    return kept


@pytest.mark.parametrize("name,ndir", [("2d", 2), ("3d", 3)])
def test_svf_exp_and_adjoint_beyond_the_block_caps(tr, name, ndir):
    """test_exp_matches_the_restatement and test_exp_backward_matches_the_restatement where svf_scale_kernel (4096 blocks) and svf_max_kernel
    (1024 blocks per pair) go round again.  The directional identity keeps the allowance honest here too, with 2 (2-D) or 3 (3-D)
    directions instead of 8: each costs two fp64 exponentials of the whole field on the host.  2-D: pair 1 alone gives the bits it has in
    the batch (the scale kernel then runs a single trip)."""
    c = _svf_case(name)
    v, g, K = c["v"].cuda(), c["g"].cuda(), c["K"]
    got = tr.svf_exp(v, K).double().cpu()
    err, tol = (got - c["f64"]).abs().max().item(), bar(c["f32"].numpy(), c["f64"].numpy(), 1e-5 * c["f64"].abs().max().item())
    print(f"svf {name} exp: err {err:.3e} bar {tol:.3e}")
    assert err <= tol, (err, tol)
    back = tr.svf_exp_backward(v, g, K)
    got = back.double().cpu()
    assert bool(torch.isfinite(got).all())
    tol = bar(c["b32"].numpy(), c["b64"].numpy(), 1e-5 * c["b64"].abs().max().item())
    err = (got - c["b64"]).abs()
    left_out, allowed = int((err > tol).sum()), max(4, got.numel() // 1000)
    print(f"svf {name} backward: max err {err.max().item():.3e} bar {tol:.3e}, {left_out} of {got.numel()} elements beyond the bar (allowed {allowed})")
    assert left_out <= allowed, (left_out, allowed, err.max().item(), tol)
    dirs = _directions(c, ndir)
    assert len(dirs) == ndir
    for d, rhs in dirs:
        lhs = (got * d).sum().item()
        print(f"svf {name} directional identity: lhs {lhs:.9g} rhs {rhs:.9g} rel {abs(lhs - rhs) / max(abs(lhs), abs(rhs)):.2e} (bar 1e-4)")
        assert abs(lhs - rhs) <= 1e-4 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    if v.shape[0] > 1:
        assert torch.equal(tr.svf_exp(v, K)[1:2], tr.svf_exp(v[1:2], K)) and torch.equal(back[1:2], tr.svf_exp_backward(v[1:2], g[1:2], K))


def test_svf_zero_squarings_beyond_the_block_cap(tr):
    """squarings = 0: exp and its adjoint are the scale kernel alone, exact - including its second trip."""
    v, g = (t.cuda() for t in lg.svf_case_inputs("2d_k0"))
    for inverse in (False, True):
        assert torch.equal(tr.svf_exp(v, 0, inverse=inverse), -v if inverse else v)
        assert torch.equal(tr.svf_exp_backward(v, g, 0, inverse=inverse), -g if inverse else g)
