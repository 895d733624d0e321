#!/usr/bin/env python3
"""Cubic B-spline free-form deformation (csrc/bspline.hip) at 1 x 256^3 and 8 x 128^3, spacing 8, NCC + Adam (hipEvents, after warm-up,
calls through the C ABI with preallocated buffers so that no allocation sits in a timed window):
  us per trx_bspline_expand (without and with a base), per trx_bspline_reduce, per trx_flow_loss_grad on the expanded flow, per
  iteration of trx_bspline_run, per trx_bspline_bending call (energy and gradient: its three launches) and per iteration of
  trx_bspline_run with bending_weight > 0 (--bending-weight, a second solver from the same start); the two operators as fractions of
  the 8 TB/s HBM roofline on their algorithmic bytes (12 B/voxel each, 24 B/voxel for expand with a base).
The seven legs are timed one after another in rounds (default 3), so that a drift of the machine shows in every leg alike; each figure
is printed per round, the JSON line holds the medians.  --shapes 1x256,8x128 (B x S^3), --spacing 8, --reps 50, --rounds 3;
--only-run N: warm-up and N loop iterations only (the rocprofv3 --kernel-trace --stats run); with --only-run-bending they are iterations
of the solver with the penalty (one call: the Gram kernel must show once, the bending kernel N times)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib  # noqa: E402
from bench import blobs_gpu  # noqa: E402

HBM = 8.0e12


def timed_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def bench_shape(B, S, spacing, reps, rounds, only_run=0, bending_weight=1000.0, only_run_bending=False):
    dev = torch.device("cuda")
    lib = _lib.load()
    shape = (S,) * 3
    mov = torch.cat([blobs_gpu(shape, 2000 + b, dev) for b in range(B)])
    tgt = torch.cat([blobs_gpu(shape, 1000 + b, dev) for b in range(B)])
    solver = tr.BSplineSolver(mov, tgt, spacing, loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.05, capacity=reps * (rounds + 1) + 8 + only_run,
                              init=0.5 * torch.randn((B, 3) + tr.bspline_grid(shape, spacing), generator=torch.Generator().manual_seed(1)))
    bent = tr.BSplineSolver(mov, tgt, spacing, loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.05, capacity=reps * (rounds + 1) + 8 + only_run,
                            init=solver.ctrl.clone(), bending_weight=bending_weight)
    energy = torch.empty(B, device=dev)
    base = torch.randn_like(solver.flow)
    dctrl = torch.empty_like(solver.ctrl)
    terms = torch.empty(B, 4, device=dev)
    fws_bytes = lib.trx_flow_workspace_bytes(ctypes.byref(solver.vol))
    fws = torch.empty(fws_bytes, dtype=torch.uint8, device=dev)
    stream = _lib.current_stream(dev)
    sp3, ws, nws = tuple(solver.sp3), _lib.ptr(solver.workspace), solver.ws_bytes

    def expand(b=None):
        _lib.check(lib.trx_bspline_expand(_lib.ptr(solver.ctrl), _lib.ptr(b), _lib.ptr(solver.flow), 3, B, S, S, S, *sp3, ws, nws, stream), "expand")

    def reduce():
        _lib.check(lib.trx_bspline_reduce(_lib.ptr(solver.dflow), _lib.ptr(dctrl), 3, B, S, S, S, *sp3, ws, nws, stream), "reduce")

    def loss_grad():
        _lib.check(lib.trx_flow_loss_grad(ctypes.byref(solver.vol), ctypes.byref(solver.loss_c), _lib.ptr(solver.flow), _lib.ptr(terms),
                                          _lib.ptr(solver.dflow), _lib.ptr(fws), fws_bytes, stream), "loss_grad")

    def run_iters():
        solver.enqueued += reps
        _lib.check(lib.trx_bspline_run(ctypes.byref(solver.vol), ctypes.byref(solver.loss_c), ctypes.byref(solver.opt), ctypes.byref(solver.state),
                                       solver.sp3, reps, ws, nws, stream), "run")

    def bending():
        _lib.check(lib.trx_bspline_bending(_lib.ptr(solver.ctrl), _lib.ptr(energy), _lib.ptr(dctrl), 1.0, 0, 3, B, S, S, S, *sp3, ws, nws, stream), "bending")

    def run_iters_bending():
        bent.enqueued += reps
        _lib.check(lib.trx_bspline_run(ctypes.byref(bent.vol), ctypes.byref(bent.loss_c), ctypes.byref(bent.opt), ctypes.byref(bent.state),
                                       bent.sp3, reps, _lib.ptr(bent.workspace), bent.ws_bytes, stream), "run")

    # expand without a base comes after the one with a base, so that the loss-and-gradient leg behind it sees the lattice's smooth flow -
    # the flow it sees inside the loop - and not the noise of `base`, whose scattered gathers are another workload
    legs = {"expand_base_us": lambda: timed_us(lambda: expand(base), reps), "expand_us": lambda: timed_us(expand, reps),
            "loss_grad_us": lambda: timed_us(loss_grad, reps), "reduce_us": lambda: timed_us(reduce, reps),
            "run_iteration_us": lambda: timed_us(run_iters, 1) / reps, "bending_us": lambda: timed_us(bending, reps),
            "run_iteration_bending_us": lambda: timed_us(run_iters_bending, 1) / reps}
    for fn in (lambda: expand(base), expand, loss_grad, reduce, bending):      # warm-up: code objects, the caches' steady state
        for _ in range(5):
            fn()
    solver.run(5)
    bent.run(5)
    torch.cuda.synchronize()
    if only_run:                                                      # for a kernel trace: the loop alone
        which = bent if only_run_bending else solver
        which.enqueued += only_run
        _lib.check(lib.trx_bspline_run(ctypes.byref(which.vol), ctypes.byref(which.loss_c), ctypes.byref(which.opt), ctypes.byref(which.state),
                                       which.sp3, only_run, _lib.ptr(which.workspace), which.ws_bytes, stream), "run")
        torch.cuda.synchronize()
        return {"iterations_run": only_run + 5}
    per_round = {k: [] for k in legs}
    for r in range(rounds):
        for k, leg in legs.items():
            per_round[k].append(leg())
        print(f"{B} x {S}^3 spacing {spacing} round {r}: " + ", ".join(f"{k} {v[-1]:.1f}" for k, v in per_round.items()), flush=True)
    out = {k: statistics.median(v) for k, v in per_round.items()}
    nvox = B * S ** 3
    out["expand_roofline"] = 12 * nvox / (out["expand_us"] * 1e-6) / HBM
    out["expand_base_roofline"] = 24 * nvox / (out["expand_base_us"] * 1e-6) / HBM
    out["reduce_roofline"] = 12 * nvox / (out["reduce_us"] * 1e-6) / HBM
    out["expand_plus_reduce_over_loss_grad"] = (out["expand_us"] + out["reduce_us"]) / out["loss_grad_us"]
    out["bending_over_iteration"] = out["bending_us"] / out["run_iteration_us"]
    out["bending_iteration_over_iteration"] = out["run_iteration_bending_us"] / out["run_iteration_us"]
    out["bending_energy"] = energy.tolist()
    out["loss_first_last"] = [solver.losses[0, 0].item(), solver.losses[0, int(solver.step[0]) - 1].item()]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x256,8x128")
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only-run", type=int, default=0, help="warm up, run this many loop iterations and stop (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--bending-weight", type=float, default=1000.0, help="lambda of the solver behind run_iteration_bending_us")
    ap.add_argument("--only-run-bending", action="store_true", help="--only-run iterates the solver with the penalty")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bspline.py needs a GPU: there is no CPU path to time")
    out = {}
    for item in a.shapes.split(","):
        B, S = (int(v) for v in item.split("x"))
        out[f"{B}x{S}^3"] = bench_shape(B, S, a.spacing, a.reps, a.rounds, a.only_run, a.bending_weight, a.only_run_bending)
    print(json.dumps(dict(tool="bench_bspline", spacing=a.spacing, optimizer="adam", loss="ncc", hbm_peak_TBps=HBM / 1e12, **out)))


if __name__ == "__main__":
    main()
