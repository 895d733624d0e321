#!/usr/bin/env python3
"""Nearest-neighbour and cubic B-spline resampling through the final transform (csrc/spline.hip) on two workloads (hipEvents, after warm-up, calls
through the C ABI with preallocated buffers so that no allocation sits in a timed window):
  1 x 256^3 onto itself, and a 512 x 512 x 120 moving volume onto a 256 x 256 x 180 target lattice, both through a composed transform - a rotation
  of --angle rad about z with a small zoom and shift, and a smooth flow of 3 voxels.
  (a) us per trx_spline_coefficients of the moving volume and its share of the 8 TB/s HBM roofline on the algorithmic bytes (4 B read + 4 B written
      per voxel; the kernels move that once per axis pass, three times in 3-D),
  (b) us per trx_transform_resample, order 3 and order 0, beside (c) trx_affine_flow_warp (the linear form) on the same transform, one channel.
The legs are timed one after another in rounds (default 3); each figure is printed per round, the JSON line holds the medians.
--reps 20, --rounds 3, --angle 0.2."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib  # noqa: E402

HBM = 8.0e12
WORKLOADS = {"256^3 -> 256^3": ((256, 256, 256), (256, 256, 256)), "512x512x120 -> 256x256x180": ((120, 512, 512), (180, 256, 256))}   # (moving, target) as D, H, W


def timed_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def smooth_flow(shape, amp, dev):
    z, y, x = torch.meshgrid(*[torch.arange(s, device=dev, dtype=torch.float32) / (s - 1) for s in shape], indexing="ij")
    two_pi = 2 * math.pi
    v = torch.stack([torch.cos(two_pi * (z + 0.5 * y)) * torch.sin(two_pi * x + 0.3), torch.sin(two_pi * (y - 0.5 * x) + 1.1) * torch.cos(two_pi * z),
                     torch.cos(two_pi * (x + y + z) + 2.0)])
    return (amp * v)[None].contiguous()


def bench(mshape, tshape, angle, reps, rounds):
    dev = torch.device("cuda")
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    mov = torch.rand((1, 1) + mshape, device=dev)
    coef, out = torch.empty_like(mov), torch.empty((1, 1) + tshape, device=dev)
    c, s = math.cos(angle), math.sin(angle)
    theta = tr._engine.pad_theta(torch.tensor([[[0.97 * c, -0.97 * s, 0.0, 0.02], [0.97 * s, 0.97 * c, 0.0, -0.01], [0.0, 0.0, 0.95, 0.015]]], device=dev), 3)
    flow = smooth_flow(tshape, 3.0, dev)
    nws = lib.trx_spline_workspace_bytes(3, 1, *mshape)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    v = tr._engine._volumes(coef, None, coef[0].numel(), 0, tshape)
    vlin = tr._engine._volumes(mov, None, mov[0].numel(), 0, tshape)
    mg = tr._engine._moving_grid(mshape)

    def coefficients():
        _lib.check(lib.trx_spline_coefficients(_lib.ptr(mov), _lib.ptr(coef), 3, 1, *mshape, _lib.ptr(ws), nws, stream), "coefficients")

    def gather(order):
        return lambda: _lib.check(lib.trx_transform_resample(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(theta), _lib.ptr(flow), 1, order, _lib.ptr(out), stream),
                                  "resample")

    def linear():
        _lib.check(lib.trx_affine_flow_warp(ctypes.byref(vlin), ctypes.byref(mg), _lib.ptr(theta), _lib.ptr(flow), 1, _lib.ptr(out), stream), "affine_flow_warp")

    legs = {"coefficients_us": coefficients, "cubic_gather_us": gather(3), "nearest_gather_us": gather(0), "affine_flow_warp_us": linear}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    per_round = {k: [] for k in legs}
    for r in range(rounds):
        for k, fn in legs.items():
            per_round[k].append(timed_us(fn, reps))
        print(f"{mshape} -> {tshape} round {r}: " + ", ".join(f"{k} {t[-1]:.1f}" for k, t in per_round.items()), flush=True)
    res = {k: statistics.median(t) for k, t in per_round.items()}
    res["coefficients_roofline_on_8B_per_voxel"] = 8 * mov.numel() / (res["coefficients_us"] * 1e-6) / HBM
    res["cubic_over_linear"] = res["cubic_gather_us"] / res["affine_flow_warp_us"]
    res["nearest_over_linear"] = res["nearest_gather_us"] / res["affine_flow_warp_us"]
    res["outside_share"] = float((out == 0).float().mean())          # of the last leg's output: the linear warp's zero padding
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--angle", type=float, default=0.2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU: there is no CPU path to time")
    res = {name: bench(m, t, a.angle, a.reps, a.rounds) for name, (m, t) in WORKLOADS.items()}
    print(json.dumps(dict(tool="bench_resample", angle=a.angle, flow_amplitude_voxels=3.0, channels=1, hbm_peak_TBps=HBM / 1e12, **res)))


if __name__ == "__main__":
    main()
