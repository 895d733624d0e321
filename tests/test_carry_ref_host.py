"""tests/carry_ref.py (the fp64 restatement of trx_affine_run's loop that tests/test_gpu_carry.py holds the kernels to) pinned on the CPU: its SGD
legs on the oracle's own driver loop (oracle.c_affine_loop, itself pinned on the golden trajectories of the reference), its Adam leg on
torch.optim.Adam fed the same oracle gradients, and its hand-over between calls on one long call."""
import numpy as np
import pytest
import torch

import carry_ref
import oracle
import phantoms as ph

SHAPE, ITERS = (12, 14, 16), 6
THETA0 = np.eye(3, 4) + 2.5e-3 * np.sin(1.2345 * (np.arange(12.0).reshape(3, 4) + 1.0))
POSE0 = np.array([0.5, 0.77, 0.09, 0.3, -0.2, 0.1])


@pytest.fixture(scope="module")
def pair():
    tgt = ph.blobs(SHAPE, 81)[0, 0].double().numpy()
    mov = ph.blobs(SHAPE, 82)[0, 0].double().numpy()
    return mov, tgt, oracle.base_tables(SHAPE, np.float64)


@pytest.mark.parametrize("mode", ["affine", "rigid"])
@pytest.mark.parametrize("loss,lr", [(dict(w_ncc=1.0), 1e-4), (dict(w_mse=1.0, w_ssd=0.1), 1e-2)], ids=["ncc", "mse+ssd"])
def test_sgd_legs_equal_the_oracle_loop(pair, mode, loss, lr):
    mov, tgt, tabs = pair
    start = dict(pose0=POSE0) if mode == "rigid" else dict(theta0=THETA0)
    want = oracle.c_affine_loop(mov, tgt, oracle.wts(**loss), lr, ITERS, tables=tabs, **start)
    got = carry_ref.loop(mov, tgt, oracle.wts(**loss), lr, ITERS, "sgd", tables=tabs, **start)
    assert np.max(np.abs(got["losses"] - want["losses"])) <= 1e-12 * max(1.0, np.max(np.abs(want["losses"])))
    assert np.max(np.abs(got["thetas"] - want["thetas"][:ITERS])) <= 1e-12 and np.max(np.abs(got["theta"] - want["final_theta"])) <= 1e-12
    assert got["best_idx"] == want["best_idx"] and np.max(np.abs(got["best_theta"] - want["best_theta"])) <= 1e-12
    if mode == "rigid":
        assert np.max(np.abs(got["param"] - want["pose"])) <= 1e-12
    assert np.max(np.abs(got["theta"] - got["thetas"][0])) >= 1e-5   # (the run moves: equality of two standing thetas would say nothing)
    assert got["t"] == ITERS and np.array_equal(got["grad"], got["grads"][-1])


@pytest.mark.parametrize("mode", ["affine", "rigid"])
def test_adam_leg_equals_torch_optim_adam_on_the_same_gradients(pair, mode):
    mov, tgt, tabs = pair
    w, lr = oracle.wts(w_ncc=1.0, w_mse=1.0), 5e-4
    rigid = mode == "rigid"
    got = carry_ref.loop(mov, tgt, w, lr, ITERS, "adam", tables=tabs, **(dict(pose0=POSE0) if rigid else dict(theta0=THETA0)))
    p = torch.tensor(POSE0 if rigid else THETA0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr)
    for k in range(ITERS):
        x = p.detach().numpy()
        th = oracle.c_theta_fwd(x) if rigid else x
        assert np.max(np.abs(th - got["thetas"][k])) <= 1e-12
        total, _, dth, _ = oracle.c_affine_loss_grad(mov, tgt, th, w, tabs)
        assert abs(total - got["losses"][k]) <= 1e-12 * max(1.0, abs(total))
        p.grad = torch.from_numpy(np.array(oracle.c_theta_vjp(x, dth) if rigid else dth, dtype=np.float64).reshape(p.shape))
        opt.step()
    st = opt.state[p]
    assert np.max(np.abs(got["param"] - p.detach().numpy())) <= 1e-12
    assert np.max(np.abs(got["m"] - st["exp_avg"].numpy())) <= 1e-12 * max(1.0, np.max(np.abs(got["m"])))
    assert np.max(np.abs(got["v"] - st["exp_avg_sq"].numpy())) <= 1e-12 * max(1.0, np.max(np.abs(got["v"])))
    assert np.max(np.abs(got["param"] - (POSE0 if rigid else THETA0))) >= 0.5 * lr * ITERS   # (Adam moves every entry by about lr per iteration)


@pytest.mark.parametrize("optimizer,lr", [("sgd", 1e-4), ("adam", 5e-4)])
def test_calls_hand_over_state_moments_step_and_best_record(pair, optimizer, lr):
    """(1, 2, 3) iterations over three calls = 6 in one: Adam's t and moments and the best record cross the calls."""
    mov, tgt, tabs = pair
    w = oracle.wts(w_ncc=1.0)
    one = carry_ref.loop(mov, tgt, w, lr, 6, optimizer, pose0=POSE0, tables=tabs)
    st, losses = None, []
    for n in (1, 2, 3):
        st = carry_ref.loop(mov, tgt, w, lr, n, optimizer, pose0=POSE0 if st is None else None, tables=tabs, state=st)
        losses += list(st["losses"])
    # (1e-12, not bit equality: the oracle's sums are OpenMP reductions, whose order is not fixed from call to call)
    assert np.max(np.abs(np.asarray(losses) - one["losses"])) <= 1e-12 * np.max(np.abs(one["losses"])) and st["t"] == 6
    for k in ("theta", "param", "m", "v", "best_theta"):
        assert np.max(np.abs(st[k] - one[k])) <= 1e-12 * max(1.0, np.max(np.abs(one[k]))), k
    assert st["best_idx"] == one["best_idx"] and abs(st["best_loss"] - one["best_loss"]) <= 2e-7 * abs(one["best_loss"])   # (one fp32 ulp)


def test_best_record_is_the_first_strict_minimum_of_the_fp32_losses(pair):
    """A step far too large: the loss falls, then rises - the best record points inside the run and holds the theta of THAT forward."""
    mov, tgt, tabs = pair
    r = carry_ref.loop(mov, tgt, oracle.wts(w_mse=1.0, w_ssd=0.1), 0.2, 8, "sgd", theta0=THETA0, tables=tabs)
    l32 = r["losses"].astype(np.float32)
    assert 0 < r["best_idx"] < 7, r["losses"]
    assert r["best_idx"] == int(np.argmin(l32)) and r["best_loss"] == float(l32[r["best_idx"]])
    assert np.array_equal(r["best_theta"], r["thetas"][r["best_idx"]])
