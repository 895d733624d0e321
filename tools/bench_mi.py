#!/usr/bin/env python3
"""Parzen joint-histogram mutual information (csrc/mi.hip) at 1 x 256^3 and 8 x 128^3 with 32 and 64 bins, on a smooth phantom and on uniform
noise (hipEvents, after warm-up, calls through the C ABI with preallocated buffers):
  us per histogram pass alone (trx_mi_histogram), per trx_mi_loss_grad, per iteration of trx_flow_mi_run and of trx_bspline_mi_run (spacing 8,
  Adam), and per iteration of trx_bspline_run (NCC) from the same run; each also as a fraction of the 8 TB/s HBM roofline on the criterion's
  20 B/voxel (histogram 8, gradient 12; the histogram pass alone on its 8).
Smooth images send the lanes of a wave to the same histogram cells, noise spreads them: the difference between the two prices the colliding LDS
adds.  Legs are timed one after another in rounds (default 3); the JSON line holds the medians.  --shapes 1x256,8x128 --bins 32,64 --reps 20."""
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


def bench_case(B, S, bins, images, spacing, reps, rounds):
    dev = torch.device("cuda")
    lib = _lib.load()
    shape = (S,) * 3
    if images == "smooth":
        tgt = torch.cat([blobs_gpu(shape, 1000 + b, dev) for b in range(B)])
        mov = torch.cat([blobs_gpu(shape, 2000 + b, dev) for b in range(B)])
    else:
        g = torch.Generator(device=dev).manual_seed(5)
        tgt, mov = (torch.rand((B, 1) + shape, device=dev, generator=g) for _ in range(2))
    rng = tr._engine.mi_range(tgt, mov)
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, 1.0, 0, rng.data_ptr()
    nws = lib.trx_mi_workspace_bytes(3, B, S, S, S, bins)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    loss, grad = torch.empty(B, device=dev), torch.empty_like(mov)
    stream = _lib.current_stream(dev)
    cap = reps * (rounds + 1) + 8
    mi = dict(bins=bins)
    flow = tr.FlowSolver(mov, tgt, optimizer="adam", lr=0.05, capacity=cap, mi=mi)
    init = 0.5 * torch.randn((B, 3) + tr.bspline_grid(shape, spacing), generator=torch.Generator().manual_seed(1))
    ffd = tr.BSplineSolver(mov, tgt, spacing, optimizer="adam", lr=0.05, capacity=cap, init=init, mi=mi)
    ncc = tr.BSplineSolver(mov, tgt, spacing, loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.05, capacity=cap, init=init)

    def hist():
        _lib.check(lib.trx_mi_histogram(_lib.ptr(tgt), _lib.ptr(mov), 3, B, S, S, S, ctypes.byref(cfg), _lib.ptr(ws), nws, stream), "histogram")

    def loss_grad():
        _lib.check(lib.trx_mi_loss_grad(_lib.ptr(tgt), _lib.ptr(mov), 3, B, S, S, S, ctypes.byref(cfg), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), nws,
                                        stream), "loss_grad")

    legs = {"histogram_us": lambda: timed_us(hist, reps), "loss_grad_us": lambda: timed_us(loss_grad, reps),
            "flow_mi_iteration_us": lambda: timed_us(lambda: flow.run(reps), 1) / reps,
            "bspline_mi_iteration_us": lambda: timed_us(lambda: ffd.run(reps), 1) / reps,
            "bspline_ncc_iteration_us": lambda: timed_us(lambda: ncc.run(reps), 1) / reps}
    for fn in (hist, loss_grad):
        for _ in range(5):
            fn()
    for s in (flow, ffd, ncc):
        s.run(4)
    torch.cuda.synchronize()
    per_round = {k: [] for k in legs}
    for r in range(rounds):
        for k, leg in legs.items():
            per_round[k].append(leg())
        print(f"{B} x {S}^3 K={bins} {images} round {r}: " + ", ".join(f"{k} {v[-1]:.1f}" for k, v in per_round.items()), flush=True)
    out = {k: statistics.median(v) for k, v in per_round.items()}
    nvox = B * S ** 3
    out["histogram_roofline"] = 8 * nvox / (out["histogram_us"] * 1e-6) / HBM
    for k in ("loss_grad", "flow_mi_iteration", "bspline_mi_iteration", "bspline_ncc_iteration"):
        out[k + "_roofline_20B"] = 20 * nvox / (out[k + "_us"] * 1e-6) / HBM
    out["bspline_mi_over_ncc"] = out["bspline_mi_iteration_us"] / out["bspline_ncc_iteration_us"]
    out["loss"] = loss.tolist()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x256,8x128")
    ap.add_argument("--bins", default="32,64")
    ap.add_argument("--images", default="smooth,noise")
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mi.py needs a GPU: there is no CPU path to time")
    out = {}
    for item in a.shapes.split(","):
        B, S = (int(v) for v in item.split("x"))
        for bins in (int(v) for v in a.bins.split(",")):
            res = {im: bench_case(B, S, bins, im, a.spacing, a.reps, a.rounds) for im in a.images.split(",")}
            if "smooth" in res and "noise" in res:
                res["smooth_over_noise_histogram"] = res["smooth"]["histogram_us"] / res["noise"]["histogram_us"]
                res["smooth_over_noise_loss_grad"] = res["smooth"]["loss_grad_us"] / res["noise"]["loss_grad_us"]
            out[f"{B}x{S}^3 K={bins}"] = res
    print(json.dumps(dict(tool="bench_mi", spacing=a.spacing, optimizer="adam", hbm_peak_TBps=HBM / 1e12, **out)))


if __name__ == "__main__":
    main()
