"""Round 6: the CARRY form of trx_affine_run (trx_affine_run in csrc/affine.hip; CarryKArgs and carry_prologue in csrc/affine_finalize.h) - launch-bound 3-D steps (one pair up to ~128^3: the two-body GeomA / GeomR
kernel on the classic grid) as ONE launch per iteration: the finalise of iteration k rides in the prologue of iteration k + 1's kernel (every block of a
pair reduces that pair's partial rows of the previous launch and computes the same theta; the pair's first block writes the state), one finalise kernel
behind the last launch flushes the run.  TRX_FLAG_NO_CARRY keeps the two-launch form of rounds 1-5: every test runs both and compares - the folded finalise
sums the rows in another fixed order (fp64), so the two agree to fp32 rounding of the 12-float update, not bit for bit.
The trajectories against the fp32 + fp64 arbiter at BASELINE cfg2's size (128^3, 200 iterations, SGD and Adam) run through this path in
tests/test_gpu_baseline_trajectories.py; the golden trajectories of the reference in tests/test_gpu_affine.py.

Two things an A/B test cannot see are tested in the second half of this module.  (1) THAT THE FORM RAN: every run fills the workspace's carry buffers with a
sentinel first and reads them afterwards (tests/carry_ref.py::carry_ran over AffineSolver.carry_state) - if the launch rule stopped choosing the form, A and B
would be the same code.  (2) THE EPILOGUE BOTH FORMS SHARE (fin_load / fin_apply / fin_update): the runs are held to tests/carry_ref.py::loop, N iterations
restated in fp64 from the oracle's single evaluations.  Bars: loss 2e-5 max(1, |L|) per iteration; theta / parameters 2e-6 + the one-step term (SGD: 3e-4 lr
max|g|; Adam: the reference's own fp32-vs-fp64 gap); gradient 3e-4 max|g|.  PRECONDITION, asserted per case on the CPU legs alone (`arbiter`): the fp32 and fp64
legs of the reference differ by at most HALF the floor - 1e-5 relative in every loss, 1e-6 in the final theta / parameters.  Measured (runs of <= 8 iterations;
the oracle's sums are OpenMP reductions, so the last digit moves from run to run):

  case (seed 71 unless noted)                               lr       n    loss gap   theta gap   theta moves by
  8x16x32     affine SGD NCC (1 row)                        2e-5     6    6.8e-7     1.5e-7      2.8e-3
  8x16x32     rigid  SGD NCC (2 rows)                       2e-5     6    1.8e-7     2.7e-8      3.6e-3
  9x17x33     affine SGD NCC                                2e-5     6    1.0e-6     9.3e-8      2.8e-3
  9x17x33     rigid  SGD NCC                                2e-5     6    1.2e-7     5.7e-8      3.6e-3
  40x52x36    rigid  SGD NCC                                2e-5     2/3/6/8  1.1e-7  4.9e-8 .. 7.4e-8  1.2e-3 .. 4.8e-3
  72x64x80    rigid  SGD NCC (second trip)                  2e-5     6    7.4e-8     5.0e-8      3.7e-3
  48x56x64    affine SGD NCC, seeds 200 / 210 / 220         2e-5     6    1.2e-6 / 9.1e-8 / 7.2e-8   1.2e-7 / 7.4e-8 / 2.4e-7   4.5e-3 / 5.8e-3 / 1.1e-2
  40x52x36    affine SGD NCC                                2e-5     6/8  4.9e-7     9.8e-8 .. 1.1e-7  2.7e-3 .. 3.6e-3
  32x32x64    affine SGD NCC, pairs 1 / 62 / 63 of the batch  2e-5   4    6.6e-7 .. 1.3e-6  5.3e-8 .. 9.5e-8  1.8e-3 .. 1.9e-3
  40x52x36    affine Adam NCC + MSE                         5e-4     6    1.0e-6     5.8e-8      3.0e-3
  40x52x36    affine Adam NCC                               5e-4     2/3/6/8  4.8e-7 .. 9.5e-7  6.0e-8 .. 1.1e-7  1.0e-3 .. 4.0e-3
  40x52x36    rigid  Adam NCC                               5e-4     6    7.4e-8     6.7e-8      5.3e-3
  40x52x36    affine SGD MSE + SSD                          3e-6     6    2.0e-6     7.5e-8      6.7e-3
  40x52x36    affine SGD MSE + SSD, loss falls then rises   1.25e-4  8    1.2e-6     1.3e-7      4.6e-2   (best at iteration 5 of 8)
  40x52x36    affine SGD NCC, seed 91                       2e-5     5    7.9e-7     8.7e-8      6.7e-3
(MSE + SSD at lr 1e-3 on 40x52x36 diverges - loss 16 -> 1083, gaps 1.6e-4 / 1.5e-3 - and at 1.1e-4 / 1.3e-4 the loss gap is 3.5e-5 / 1.1e-5: not used.)"""
import numpy as np
import pytest
import torch

import carry_ref as cr
import oracle
import phantoms as ph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torchregister_amd._engine as e
    assert torch.cuda.is_available()
    return e


def rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def drive(eng, mov, tgt, schedule, capacity=None, **kw):
    """A solver run through the calls of `schedule` -> (solver, [carry_ran of every call]): the carry buffers are filled with the sentinel in front
    of every call and read behind it."""
    s = eng.AffineSolver(mov, tgt, capacity=sum(schedule) if capacity is None else capacity, **kw)
    ran, start = [], 0
    for n in schedule:
        cr.fill_sentinel(s)
        s.run(n)
        ran.append(cr.carry_ran(s, start, n))
        start += n
    torch.cuda.synchronize()
    return s, ran


def forms(c, n, iters):
    """the flags-0 run took the carry form in every call of two iterations or more and in no other; the TRX_FLAG_NO_CARRY run in none"""
    assert c["ran"] == [k >= 2 for k in iters] and n["ran"] == [False] * len(iters), (c["ran"], n["ran"])


def both(eng, mov, tgt, iters, **kw):
    """the same run in the carry form and in the two-launch form: (losses, theta, best theta, best idx, grad, step) of each, and `ran`: which form
    each call of the schedule took (carry_ref.carry_ran)"""
    from torchregister_amd import _lib
    out = []
    for fl in (0, _lib.FLAG_NO_CARRY):
        s, ran = drive(eng, mov, tgt, iters, flags=fl, **kw)
        out.append(dict(solver=s, ran=ran, losses=s.losses.clone(), theta=s.theta.clone(), best=s.best_theta.clone(), best_idx=s.best_idx.clone(), best_loss=s.best_loss.clone(),
                        grad=s.grad.clone(), step=s.step.clone(), m=s.adam_m.clone(), v=s.adam_v.clone(), bodies=s.bodies(), rows=s.rows_used().tolist()))
    return out


def agree(a, b, iters_total, ltol=2e-6, ttol=2e-6):
    assert torch.equal(a["step"], b["step"]) and int(a["step"][0]) == iters_total
    la, lb = a["losses"][:, :iters_total], b["losses"][:, :iters_total]
    assert torch.isfinite(la).all()
    assert torch.max(torch.abs(la - lb) / torch.clamp(lb.abs(), min=1.0)).item() <= ltol, (la - lb).abs().max()
    assert torch.max(torch.abs(a["theta"] - b["theta"])).item() <= ttol
    assert torch.max(torch.abs(a["grad"] - b["grad"])).item() <= 1e-4 * max(b["grad"].abs().max().item(), 1e-30)
    assert a["bodies"] == b["bodies"] and a["rows"] == b["rows"]          # the notes of the LAST iteration sit in the primary buffers in both forms
    # best = first strict minimum: same index unless two recorded losses are within rounding of each other
    for p in range(la.shape[0]):
        ia, ib = int(a["best_idx"][p]), int(b["best_idx"][p])
        assert ia == ib or abs(lb[p, ia].item() - lb[p, ib].item()) <= ltol * max(1.0, abs(lb[p, ib].item())), (p, ia, ib)
        if ia == ib:
            assert torch.max(torch.abs(a["best"][p] - b["best"][p])).item() <= ttol


@pytest.mark.parametrize("shape", [(64, 64, 64), (40, 52, 36), (128, 128, 128)], ids=["64", "ragged", "128"])
@pytest.mark.parametrize("optimizer,lr", [("sgd", 2e-6), ("adam", 5e-4)])
def test_carry_run_equals_the_two_launch_run(eng, shape, optimizer, lr):
    """One pair, affine + NCC: 9 iterations in one call (odd count: the first launch writes the primary buffers) and 2 + 5 + 4 over three calls (the state
    crosses call boundaries through the caller's arrays; an even count starts on the second buffers)."""
    tgt = ph.blobs_fast(shape, 71, device="cuda")
    mov = eng.affine_warp(torch.tensor(ph.THETA_STAR3, device="cuda")[None], tgt) + 0.05 * ph.blobs_fast(shape, 72, device="cuda")
    th0 = torch.tensor(np.eye(3, 4) + 2.5e-3 * np.sin(1.2345 * (np.arange(12.0).reshape(3, 4) + 1.0)), dtype=torch.float32)[None]
    kw = dict(mode="affine", loss=eng.LossSpec(w_ncc=1.0), optimizer=optimizer, lr=lr, init=th0)
    for iters in ((9,), (2, 5, 4)):
        c, n = both(eng, mov, tgt, iters, **kw)
        forms(c, n, iters)
        agree(c, n, sum(iters))
        assert c["losses"][0, sum(iters) - 1] < c["losses"][0, 0] or optimizer == "sgd"


def test_carry_batch_of_pairs_with_their_own_bodies_rigid_and_mse(eng):
    """Three pairs of 48 x 56 x 64 in one launch - near the identity (GeomA), rotated (GeomR), and zoomed out of the volume - in RIGID mode from three poses
    (the pose chain rule rides in the prologue) and in affine mode with an MSE + SSD loss (the 13-sum rows of the MSE-only step kernel)."""
    shape, B = (48, 56, 64), 3
    tgt = torch.cat([ph.blobs_fast(shape, 200 + i, device="cuda") for i in range(B)])
    mov = torch.cat([ph.blobs_fast(shape, 210 + i, device="cuda") for i in range(B)])
    poses = torch.tensor([[0.02, -0.01, 0.03, 0.01, 0.0, -0.02], [0.5, 0.77, 0.09, 0.3, -0.2, 0.1], [0.9, 0.1, 0.6, -0.4, 0.5, 0.2]], dtype=torch.float32)
    c, n = both(eng, mov, tgt, (6,), mode="rigid", loss=eng.LossSpec(w_ncc=1.0), optimizer="adam", lr=2e-3, init=poses)
    forms(c, n, (6,))
    agree(c, n, 6, ltol=5e-6, ttol=5e-6)
    assert len(set(c["bodies"])) >= 2, c["bodies"]
    ths = np.stack([np.eye(3, 4) + 4e-3 * np.sin(np.arange(12.0).reshape(3, 4)), np.concatenate([rot(0.4, 0.3, 0.5), [[0.02], [0.01], [-0.03]]], axis=1),
                    np.concatenate([1.6 * np.eye(3), [[0.1], [-0.2], [0.15]]], axis=1)])
    c, n = both(eng, mov, tgt, (5,), mode="affine", loss=eng.LossSpec(w_mse=1.0, w_ssd=0.1), optimizer="sgd", lr=1e-3, init=torch.tensor(ths, dtype=torch.float32))
    forms(c, n, (5,))
    agree(c, n, 5, ltol=5e-6, ttol=5e-6)


def test_carry_first_iteration_against_the_oracle_and_two_iterations_by_hand(eng):
    """run(2) in the carry form: the recorded loss / gradient of iteration 0 against the C oracle (fp64), and theta after two SGD steps against the two
    oracle evaluations chained by hand (theta1 = theta0 - lr g0; theta2 = theta1 - lr g1) - the prologue's update IS the reference's optimizer.step()."""
    shape = (56, 48, 64)
    tgt = ph.blobs_fast(shape, 301, device="cuda")
    mov = ph.blobs_fast(shape, 302, device="cuda")
    th0 = np.asarray(ph.THETA_ROT3, dtype=np.float64)
    lr = 1e-5
    s = eng.AffineSolver(mov, tgt, mode="affine", loss=eng.LossSpec(w_ncc=1.0), optimizer="sgd", lr=lr, init=torch.tensor(th0, dtype=torch.float32)[None], capacity=2)
    cr.fill_sentinel(s)
    s.run(2)
    assert cr.carry_ran(s, 0, 2)
    m64, t64, tabs = mov[0, 0].double().cpu().numpy(), tgt[0, 0].double().cpu().numpy(), oracle.base_tables(shape, np.float64)
    l0, _, g0, _ = oracle.c_affine_loss_grad(m64, t64, np.asarray(th0, dtype=np.float32).astype(np.float64), oracle.wts(w_ncc=1.0), tabs)
    th1 = np.asarray(th0, dtype=np.float32).astype(np.float64) - lr * g0
    l1, _, g1, _ = oracle.c_affine_loss_grad(m64, t64, th1, oracle.wts(w_ncc=1.0), tabs)
    th2 = th1 - lr * g1
    assert abs(s.losses[0, 0].item() - l0) <= 2e-5 * max(1.0, abs(l0)) and abs(s.losses[0, 1].item() - l1) <= 2e-5 * max(1.0, abs(l1))
    assert np.max(np.abs(s.grad[0, :12].cpu().numpy().reshape(3, 4) - g1)) <= 3e-4 * np.max(np.abs(g1))
    assert np.max(np.abs(s.theta[0, :12].cpu().numpy().reshape(3, 4) - th2)) <= 2e-6 + 3e-4 * lr * np.max(np.abs(g1))


# ---------------------------------------------------------------------------------------------------------------------------------------
# The carry form against tests/carry_ref.py (the loop restated in fp64 from the oracle's single evaluations), with the form asserted.
# ---------------------------------------------------------------------------------------------------------------------------------------
FLOOR_LOSS, FLOOR_THETA, STEP_TERM = 2e-5, 2e-6, 3e-4   # the project's floors; the one-step term 3e-4 * step * max|g| of the oracle test above
ITERS = 6
TH_NEAR = tuple((np.eye(3, 4) + 2.5e-3 * np.sin(1.2345 * (np.arange(12.0).reshape(3, 4) + 1.0))).astype(np.float32).reshape(-1).tolist())
POSE_ROT = (0.5, 0.77, 0.09, 0.3, -0.2, 0.1)
LOSSES = {"ncc": dict(w_ncc=1.0), "ncc+mse": dict(w_ncc=1.0, w_mse=1.0), "mse+ssd": dict(w_mse=1.0, w_ssd=0.1)}
NEAR, ROT = ("affine", TH_NEAR), ("rigid", POSE_ROT)
S_MODES = (40, 52, 36)
_PAIRS, _ARBITER = {}, {}


def cpu_pair(shape, seed):
    """(moving, target) fp32 ndarrays built on the host, so that the kernels and both legs of the arbiter read the same bits: a blob phantom, and
    the same phantom warped by THETA_STAR3 (the oracle's warp) plus 5 % of another one."""
    if (shape, seed) not in _PAIRS:
        tgt = ph.blobs_fast(shape, seed)[0, 0].numpy()
        mov = oracle.c_affine_warp(tgt, np.asarray(ph.THETA_STAR3, dtype=np.float32), oracle.base_tables(shape)) + 0.05 * ph.blobs_fast(shape, seed + 1)[0, 0].numpy()
        _PAIRS[(shape, seed)] = (mov.astype(np.float32), tgt)
    return _PAIRS[(shape, seed)]


def on_gpu(shape, seeds):
    pairs = [cpu_pair(shape, s) for s in seeds]
    return (torch.stack([torch.from_numpy(m) for m, _ in pairs])[:, None].cuda(), torch.stack([torch.from_numpy(t) for _, t in pairs])[:, None].cuda())


def arbiter(shape, seed, loss, optimizer, lr, n, start):
    """(fp32 leg, fp64 leg) of carry_ref.loop for one pair from `start` = (mode, the fp32 start values), computed once.  THE PRECONDITION of every
    comparison below, asserted here on the CPU legs alone: the two legs differ by at most half the floor in every iteration's loss and in the
    final theta / parameters - the bars below are floors of the number format, not of this reference."""
    key = (shape, seed, loss, optimizer, lr, n, start)
    if key not in _ARBITER:
        mov, tgt = cpu_pair(shape, seed)
        legs = []
        for dt in (np.float32, np.float64):
            x0 = np.asarray(start[1], dtype=np.float32).astype(dt)
            kw = dict(pose0=x0) if start[0] == "rigid" else dict(theta0=x0.reshape(3, 4))
            legs.append(cr.loop(mov.astype(dt), tgt.astype(dt), oracle.wts(**LOSSES[loss]), lr, n, optimizer, tables=oracle.base_tables(shape, dt), **kw))
        r32, r64 = legs
        lgap = np.max(np.abs(r32["losses"].astype(np.float64) - r64["losses"]) / np.maximum(1.0, np.abs(r64["losses"])))
        tgap = max(np.max(np.abs(r32[k].astype(np.float64) - r64[k])) for k in ("theta", "param"))
        print(f"\narbiter {shape} seed {seed} {start[0]} {optimizer} {loss} lr {lr:g} n {n}: fp32-vs-fp64 loss gap {lgap:.2e} (<= {0.5 * FLOOR_LOSS:.0e}), "
              f"theta gap {tgap:.2e} (<= {0.5 * FLOOR_THETA:.0e}); theta moves by {np.max(np.abs(r64['theta'] - r64['thetas'][0])):.2e}")
        assert lgap <= 0.5 * FLOOR_LOSS and tgap <= 0.5 * FLOOR_THETA, (key, lgap, tgap)
        _ARBITER[key] = (r32, r64)
    return _ARBITER[key]


def meets(s, b, legs, n, lr, tag):
    """Pair b of solver s, n iterations behind its start, against the fp64 leg: every recorded loss, theta / parameters / (Adam) moments, the last
    gradient, the best record and the step counter.  Bars: loss 2e-5 max(1, |L|); theta and parameters 2e-6 + the step term - SGD: 3e-4 lr max|g|,
    Adam: the arbiter's own fp32-vs-fp64 gap; gradient 3e-4 max|g| (the bar of the oracle test above and of tests/test_gpu_affine.py).  The Adam
    moments have no bar of their own in the project; theirs follow from the gradient's: m = sum_k c_k g_k with c_k >= 0, sum c_k <= 1, so gradients
    within 3e-4 max|g| each leave m within 3e-4 max|g| (max over the run); v is the same combination of g_k^2, and (g + d)^2 - g^2 = 2 g d + d^2 <=
    2 x 3e-4 max g^2 to first order: 6e-4 max g^2.  (The arbiter's own fp32-vs-fp64 gap of m and v is ~1e-7 relative - its fp32 leg accumulates in
    fp64 - and would make a bar no fp32 gradient kernel is asked to meet anywhere else in the suite.)"""
    from torchregister_amd import _lib
    r32, r64 = legs
    adam = s.opt.kind == _lib.OPT_ADAM
    npar = 6 if s.mode == "rigid" else 12
    assert int(s.step[b]) == n == r64["t"]
    cap = min(n, s.capacity)
    L = r64["losses"]
    lerr = np.abs(s.losses[b, :cap].cpu().numpy().astype(np.float64) - L[:cap]) / np.maximum(1.0, np.abs(L[:cap]))
    gmax, gall = np.max(np.abs(r64["grad"])), np.max(np.abs(r64["grads"]))
    term = max(np.max(np.abs(r32[k].astype(np.float64) - r64[k])) for k in ("theta", "param")) if adam else STEP_TERM * lr * gmax
    tbar = FLOOR_THETA + term
    terr = np.max(np.abs(s.theta[b, :12].cpu().numpy().astype(np.float64) - r64["theta"].reshape(-1)))
    perr = np.max(np.abs(s.param[b, :npar].cpu().numpy().astype(np.float64) - r64["param"].reshape(-1)))
    gerr = np.max(np.abs(s.grad[b, :npar].cpu().numpy().astype(np.float64) - r64["grad"].reshape(-1)))
    print(f"{tag} pair {b}: loss err {lerr.max():.2e} of {FLOOR_LOSS:.0e}; theta err {terr:.2e}, param err {perr:.2e} of {tbar:.2e}; grad err {gerr:.2e} of {STEP_TERM * gmax:.2e}")
    assert lerr.max() <= FLOOR_LOSS, (tag, b, lerr)
    assert terr <= tbar and perr <= tbar, (tag, b, terr, perr, tbar)
    assert gerr <= STEP_TERM * gmax, (tag, b, gerr, gmax)
    if adam:
        merr = np.max(np.abs(s.adam_m[b, :npar].cpu().numpy().astype(np.float64) - r64["m"].reshape(-1)))
        verr = np.max(np.abs(s.adam_v[b, :npar].cpu().numpy().astype(np.float64) - r64["v"].reshape(-1)))
        assert merr <= STEP_TERM * gall and verr <= 2 * STEP_TERM * gall * gall, (tag, b, merr, verr, gall)
    # best = the first strict minimum: the same index, unless two recorded losses lie within the floor of each other
    bi, rb = int(s.best_idx[b]), r64["best_idx"]
    assert bi == rb or abs(L[bi] - L[rb]) <= FLOOR_LOSS * max(1.0, abs(L[rb])), (tag, b, bi, rb)
    if bi == rb:
        assert abs(s.best_loss[b].item() - L[rb]) <= FLOOR_LOSS * max(1.0, abs(L[rb]))
        assert np.max(np.abs(s.best_theta[b, :12].cpu().numpy().astype(np.float64) - r64["best_theta"].reshape(-1))) <= tbar


def snapshot(s, ran):
    return dict(solver=s, ran=ran, losses=s.losses.clone(), theta=s.theta.clone(), best=s.best_theta.clone(), best_idx=s.best_idx.clone(), best_loss=s.best_loss.clone(),
                grad=s.grad.clone(), step=s.step.clone(), m=s.adam_m.clone(), v=s.adam_v.clone(), param=s.param.clone(), bodies=s.bodies(), rows=s.rows_used().tolist())


def solver_args(eng, loss, optimizer, lr, starts):
    """keyword arguments of AffineSolver for pairs that start from `starts` = [(mode, fp32 start values)] (one mode)"""
    mode = starts[0][0]
    init = torch.tensor([st[1] for st in starts], dtype=torch.float32)
    return dict(mode=mode, loss=eng.LossSpec(**LOSSES[loss]), optimizer=optimizer, lr=lr, init=init.reshape(-1, 3, 4) if mode == "affine" else init)


def carry_and_plain(eng, mov, tgt, schedule, **kw):
    """`both`, with the forms asserted and the two compared at agree's bars -> the carry run"""
    c, n = both(eng, mov, tgt, schedule, **kw)
    forms(c, n, schedule)
    agree(c, n, sum(schedule))
    return c


# (name, shape, start, what the case exists for: asserted on the row count and the body the last launch notes for the pair)
SHAPE_CASES = [
    ("one-tile", (8, 16, 32), NEAR, lambda rows, body: rows == 1 and body == "tile-A"),                  # fewer rows than the prologue has waves
    ("two-columns", (8, 16, 32), ROT, lambda rows, body: rows == 2 and body == "tile-R"),
    ("ragged-9-17-33-near", (9, 17, 33), NEAR, lambda rows, body: rows >= 1 and body == "tile-A"),
    ("ragged-9-17-33", (9, 17, 33), ROT, lambda rows, body: rows % 8 != 0 and body == "tile-R"),
    ("ragged-40-52-36", (40, 52, 36), ROT, lambda rows, body: rows % 8 != 0 and body == "tile-R"),
    # a second trip of the 16 x 8 batch loop with a clamped tail, on a rotated pair
    ("second-trip", (72, 64, 80), ROT, lambda rows, body: rows > 8 * 16 and rows % 8 != 0 and body == "tile-R"),
]


@pytest.mark.parametrize("name,shape,start,holds", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_carry_row_counts_against_the_fp64_loop(eng, name, shape, start, holds):
    """One pair, NCC, SGD: the prologue's reduction at the row counts the three fixed shapes above never give it.

    WHAT [one-tile] FOUND (fixed in csrc/affine_tile.h): with the block reduction of the step kernels summing its 64 lane partials and 8 wave sums in
    one fp32 chain each, the recorded loss of this case was off by 2.8e-5 of a floor of 2e-5 at iteration 0 (L = 0.861; the six iterations: 2.8e-5,
    9.0e-6, 2.6e-7, 2.9e-6, 1.1e-5, 1.3e-5) - no carry arithmetic has run there, and TRX_FLAG_NO_CARRY recorded the same loss.  8 x 16 x 32 is ONE
    GeomA tile, so the fp64 sums over the rows had nothing to average, and at NCC = 0.991 the floor is an absolute 2e-7 in the NCC.  The same chains
    emulated on the CPU reproduce it (3.3e-5 at iteration 0), fp64 accumulation gives at most 8.2e-6.  The tile bodies now reduce with fp64
    accumulators (block_reduce_store_nw<..., true>): 8.6e-6 of 2e-5 on the MI355X, theta 1.5e-7 of 2.1e-6, gradient 2.4e-5 of 6.7e-3."""
    lr = 2e-5
    legs = arbiter(shape, 71, "ncc", "sgd", lr, ITERS, start)
    mov, tgt = on_gpu(shape, [71])
    c = carry_and_plain(eng, mov, tgt, (ITERS,), **solver_args(eng, "ncc", "sgd", lr, [start]))
    assert holds(c["rows"][0], c["bodies"][0]), (name, c["rows"], c["bodies"])
    meets(c["solver"], 0, legs, ITERS, lr, name)


def test_carry_batch_of_three_bodies_and_row_counts_under_one_stride(eng):
    """Three pairs of 48 x 56 x 64 in one launch - near the identity, rotated, zoomed out of the volume: two bodies and two row counts under the
    one row stride the pairs share, every pair against its own fp64 loop."""
    shape, lr = (48, 56, 64), 2e-5
    ths = np.stack([np.eye(3, 4) + 4e-3 * np.sin(np.arange(12.0).reshape(3, 4)), np.concatenate([rot(0.4, 0.3, 0.5), [[0.02], [0.01], [-0.03]]], axis=1),
                    np.concatenate([1.6 * np.eye(3), [[0.1], [-0.2], [0.15]]], axis=1)]).astype(np.float32)
    starts = [("affine", tuple(t.reshape(-1).tolist())) for t in ths]
    seeds = [200, 210, 220]
    mov, tgt = on_gpu(shape, seeds)
    c = carry_and_plain(eng, mov, tgt, (ITERS,), **solver_args(eng, "ncc", "sgd", lr, starts))
    assert len(set(c["bodies"])) >= 2 and len(set(c["rows"])) >= 2, (c["bodies"], c["rows"])
    for b in range(3):
        meets(c["solver"], b, arbiter(shape, seeds[b], "ncc", "sgd", lr, ITERS, starts[b]), ITERS, lr, "batch of three")


MODE_CASES = [("affine", "sgd", "ncc", 2e-5), ("affine", "adam", "ncc+mse", 5e-4), ("rigid", "adam", "ncc", 5e-4), ("rigid", "sgd", "ncc", 2e-5),
              ("affine", "sgd", "mse+ssd", 3e-6)]   # (the last: no NCC term - the 13-sum rows of the MSE-only step kernel, mse_rows in the prologue)


@pytest.mark.parametrize("mode,optimizer,loss,lr", MODE_CASES, ids=["-".join(c[:3]) for c in MODE_CASES])
def test_carry_modes_against_the_fp64_loop(eng, mode, optimizer, loss, lr):
    start = NEAR if mode == "affine" else ROT
    legs = arbiter(S_MODES, 71, loss, optimizer, lr, ITERS, start)
    mov, tgt = on_gpu(S_MODES, [71])
    c = carry_and_plain(eng, mov, tgt, (ITERS,), **solver_args(eng, loss, optimizer, lr, [start]))
    meets(c["solver"], 0, legs, ITERS, lr, f"{mode} {optimizer} {loss}")


@pytest.mark.parametrize("schedule", [(2,), (3,), (6,), (1, 2, 1, 4), (2, 2, 2)], ids=lambda s: "+".join(map(str, s)))
@pytest.mark.parametrize("mode,optimizer,lr", [("affine", "adam", 5e-4), ("rigid", "sgd", 2e-5)])
def test_carry_call_schedules_against_one_fp64_run(eng, mode, optimizer, lr, schedule):
    """The shortest run, both parities of the first launch, carry -> single step -> carry through the caller's arrays, Adam's t and moments across
    calls: the state behind the last call is the state of ONE reference run of the summed length (`forms`: which calls took the carry form)."""
    start, n = (NEAR if mode == "affine" else ROT), sum(schedule)
    legs = arbiter(S_MODES, 71, "ncc", optimizer, lr, n, start)
    mov, tgt = on_gpu(S_MODES, [71])
    c = carry_and_plain(eng, mov, tgt, schedule, **solver_args(eng, "ncc", optimizer, lr, [start]))
    meets(c["solver"], 0, legs, n, lr, f"{mode} {optimizer} {schedule}")


# The largest batch of identical 32 x 32 x 64 pairs that the launch rule (f1_plan) still gives to the carry form, found by running batches of 1 .. 65
# pairs: up to 63 pairs the launch stays below the partial rows at which the rule turns to the flat grid of persistent blocks - `p.flat = v.B <= 64 &&
# p.rows * v.B >= 2 * slots` in f1_plan, slots = persistent_blocks() = 512 on the MI355X, so 1024 rows (the tile geometry shrinks the rows per pair as
# the batch grows: 16, then 8) - 64 pairs x 16 rows reach it.  (The rule is not monotone - that same line lets the flat grid hold at most 64
# pairs, so 65 pairs are the carry form again - and at the smaller shapes of this module no batch up to 65 pairs leaves the form at all.)  A retuned
# rule moves this number: the test then says so, and the number is found again the same way.
S_BATCH, B_CARRY_MAX = (32, 32, 64), 63


@pytest.mark.parametrize("B", [B_CARRY_MAX, B_CARRY_MAX + 1], ids=["largest-carry-batch", "one-pair-more"])
def test_carry_largest_batch_and_one_pair_more(eng, B):
    """Identical pairs with a theta of their own each: at B_CARRY_MAX the run is the carry form, at one pair more it is not (the region keeps the
    sentinel) and the result meets the same reference.  Two pairs of each batch against the fp64 loop, every pair against the other form."""
    lr, n = 2e-5, 4
    starts = [("affine", tuple((np.asarray(TH_NEAR) + 1e-3 * np.sin(b + np.arange(12.0))).astype(np.float32).tolist())) for b in range(B)]
    m1, t1 = on_gpu(S_BATCH, [71])
    mov, tgt = m1.repeat(B, 1, 1, 1, 1), t1.repeat(B, 1, 1, 1, 1)
    c, p = both(eng, mov, tgt, (n,), **solver_args(eng, "ncc", "sgd", lr, starts))
    assert c["ran"] == [B == B_CARRY_MAX] and p["ran"] == [False], (B, c["ran"], c["rows"][:2], c["bodies"][:2])
    agree(c, p, n)
    for b in (1, B - 1):
        meets(c["solver"], b, arbiter(S_BATCH, 71, "ncc", "sgd", lr, n, starts[b]), n, lr, f"B = {B}")


def test_carry_best_record_inside_the_run(eng):
    """MSE + SSD with a step that is too long: the loss falls for five iterations and rises again, so the best record is written in the middle of
    the run by a prologue and must survive the launches behind it.  The records alone are held to the reference here - best index (exactly), best
    loss, best theta, and the losses up to the minimum: a step past the stability limit is what makes the loss turn, and behind the turn it
    multiplies every rounding difference (measured on the MI355X against the fp64 leg: loss error 8e-7, 5e-6, 1.6e-4, 1.6e-4 relative at
    iterations 4 .. 7, while the state still meets its bar: theta error 7.3e-6 of 1.6e-5) - the diverging tail is no case for the loss floor.  The tail
    is held to what a theta WITHIN ITS OWN BAR may move the loss by, to first order: floor + sum_i |dL/dtheta_i| x (2e-6 + 3e-4 lr max|g|), with the
    reference's gradient of that forward - a state that meets its bar cannot explain more, whatever the step does to it afterwards."""
    lr, n = 1.25e-4, 8
    r32, r64 = arbiter(S_MODES, 71, "mse+ssd", "sgd", lr, n, NEAR)
    rb, L = r64["best_idx"], r64["losses"]
    assert 0 < rb < n - 1 and L[rb] < 0.9 * min(L[rb - 1], L[rb + 1])   # (no tie within reach of any bar)
    mov, tgt = on_gpu(S_MODES, [71])
    c = carry_and_plain(eng, mov, tgt, (n,), **solver_args(eng, "mse+ssd", "sgd", lr, [NEAR]))
    s = c["solver"]
    lerr = np.abs(s.losses[0, :n].cpu().numpy().astype(np.float64) - L) / np.maximum(1.0, np.abs(L))
    tbar = FLOOR_THETA + STEP_TERM * lr * np.max(np.abs(r64["grads"][:rb + 1]))
    terr = np.max(np.abs(s.best_theta[0, :12].cpu().numpy().astype(np.float64) - r64["best_theta"].reshape(-1)))
    print(f"best inside: best_idx {int(s.best_idx[0])} (reference {rb}); loss err per iteration {np.array2string(lerr, precision=2)} of {FLOOR_LOSS:.0e}; best theta err {terr:.2e} of {tbar:.2e}")
    assert int(s.best_idx[0]) == rb and int(s.step[0]) == n
    assert lerr[:rb + 1].max() <= FLOOR_LOSS and abs(s.best_loss[0].item() - L[rb]) <= FLOOR_LOSS * max(1.0, abs(L[rb]))
    assert terr <= tbar
    tbar_run = FLOOR_THETA + STEP_TERM * lr * np.max(np.abs(r64["grads"]))
    tail_bar = FLOOR_LOSS + np.abs(r64["grads"]).reshape(n, -1).sum(axis=1) * tbar_run / np.maximum(1.0, np.abs(L))
    print(f"             tail bar per iteration {' '.join(f'{x:.2e}' for x in tail_bar)}")
    assert (lerr[rb + 1:] <= tail_bar[rb + 1:]).all(), (lerr, tail_bar)


def test_carry_loss_curve_shorter_than_the_run(eng):
    """capacity = 5, two calls of 4 through the C ABI (each call fits the curve, the run does not; AffineSolver.run refuses that, trx_affine_run
    does not): the curve holds its first five losses, nothing is written behind it, state and best record are those of eight iterations."""
    import ctypes
    from torchregister_amd import _lib
    lr, n = 2e-5, 8
    legs = arbiter(S_MODES, 71, "ncc", "sgd", lr, n, NEAR)
    mov, tgt = on_gpu(S_MODES, [71])
    s = eng.AffineSolver(mov, tgt, capacity=5, **solver_args(eng, "ncc", "sgd", lr, [NEAR]))
    for k in range(2):
        cr.fill_sentinel(s)
        _lib.check(s.lib.trx_affine_run(ctypes.byref(s.vol), ctypes.byref(s.loss_c), ctypes.byref(s.opt), ctypes.byref(s.state), 4, _lib.ptr(s.workspace), s.ws_bytes,
                                        _lib.current_stream(s.batch.device)), "trx_affine_run")
        assert cr.carry_ran(s, 4 * k, 4)
    assert s.losses.shape == (1, 5) and int(s.step[0]) == 8
    meets(s, 0, legs, n, lr, "capacity 5")   # (losses[:, :5]; the best record points at iteration 7 of a falling curve)
    assert int(s.best_idx[0]) == legs[1]["best_idx"] == 7


def test_carry_every_block_computes_the_same_theta(eng):
    """Every block of a pair reduces the rows and computes theta for itself.  Two solvers on the same inputs and schedule: bit-equal losses, theta,
    parameters, best record, gradient and Adam moments (blocks that disagreed would feed the next launch tiles of two different transforms)."""
    mov, tgt = on_gpu((48, 56, 64), [200, 210])
    starts = [NEAR, ("affine", tuple(np.concatenate([rot(0.4, 0.3, 0.5), [[0.02], [0.01], [-0.03]]], axis=1).astype(np.float32).reshape(-1).tolist()))]
    runs = []
    for _ in range(2):
        s, ran = drive(eng, mov, tgt, (3, 1, 4), **solver_args(eng, "ncc+mse", "adam", 5e-4, starts))
        assert ran == [True, False, True]
        runs.append(snapshot(s, ran))
    a, b = runs
    for k in ("losses", "theta", "param", "best", "best_idx", "best_loss", "grad", "m", "v", "step"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["losses"]).all() and a["rows"] == b["rows"]


def test_carry_nan_pair_stays_in_its_own_rows(eng):
    """A batch of three whose middle pair has a NaN in its moving image: pairs 0 and 2 give the bits of the same batch with a finite middle pair."""
    seeds, lr, n = [71, 81, 91], 2e-5, 5
    mov, tgt = on_gpu(S_MODES, seeds)
    bad = mov.clone()
    bad[1, 0, 20, 26, 18] = float("nan")
    kw = solver_args(eng, "ncc", "sgd", lr, [NEAR] * 3)
    runs = []
    for m, nf in ((mov, ()), (bad, (1,))):
        s = eng.AffineSolver(m, tgt, capacity=n, **kw)
        cr.fill_sentinel(s)
        s.run(n)
        assert cr.carry_ran(s, 0, n, not_finite=nf)
        runs.append(snapshot(s, [True]))
    good, nan = runs
    assert not torch.isfinite(nan["losses"][1]).any() and torch.isfinite(good["losses"]).all()
    for k in ("losses", "theta", "param", "best", "best_idx", "best_loss", "grad", "step"):
        assert torch.equal(good[k][[0, 2]], nan[k][[0, 2]]), k
    meets(good["solver"], 2, arbiter(S_MODES, 91, "ncc", "sgd", lr, n, NEAR), n, lr, "finite batch")


def test_runs_that_are_not_the_carry_form_leave_the_buffers_alone(eng):
    """run(1), TRX_FLAG_NO_CARRY and 2-D: the sentinel stays (the one-pair-more case above: a launch the rule keeps from the form)."""
    from torchregister_amd import _lib
    mov, tgt = on_gpu(S_MODES, [71])
    kw = solver_args(eng, "ncc", "sgd", 2e-5, [NEAR])
    _, ran = drive(eng, mov, tgt, (1, 1), **kw)
    assert ran == [False, False]
    _, ran = drive(eng, mov, tgt, (4,), flags=_lib.FLAG_NO_CARRY, **kw)
    assert ran == [False]
    m2, t2 = mov[:, :, 20].contiguous(), tgt[:, :, 20].contiguous()
    _, ran = drive(eng, m2, t2, (4,), mode="affine", loss=eng.LossSpec(w_ncc=1.0), lr=2e-5)
    assert ran == [False]
    _, ran = drive(eng, mov, tgt, (4,), **kw)   # (the same helper on the same inputs says True where the form runs)
    assert ran == [True]
