#!/usr/bin/env python3
"""Stationary velocity field (csrc/svf.hip) at 1 x 128^3 and 1 x 256^3, K = 6 squarings, a smooth velocity of 3 voxels (hipEvents, after
warm-up, calls through the C ABI with preallocated buffers so that no allocation sits in a timed window):
  (a) us per trx_svf_exp, (b) per trx_svf_exp_backward, (c) per iteration of trx_bspline_svf_run (spacing 8, NCC, Adam), (d) per iteration
  of trx_bspline_run on the same pair, (e) the torch op chain for the same exp on the same GPU - K x (grid_sample + add) forward, autograd
  backward - and, from the kept levels, the share of source voxels per level whose corners all land in the splat's LDS tile (|u_k| < 2).
  Fractions of the 8 TB/s HBM roofline on the algorithmic bytes: exp (K + 1) x 24 B/voxel; backward per level 24 (splat: g, u) + 84
  (finish: g, u, the int64 accumulator read and re-zeroed, the result) B/voxel, not counting the atomic traffic.
The legs are timed one after another in rounds (default 3); each figure is printed per round, the JSON line holds the medians.
--shapes 1x128,1x256 (B x S^3), --squarings 6, --spacing 8, --reps 20, --rounds 3."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

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


def smooth_velocity(B, S, amp, dev):
    ax = torch.arange(S, device=dev, dtype=torch.float32) / (S - 1)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    two_pi = 2 * math.pi
    v = torch.stack([torch.cos(two_pi * (z + 0.5 * y)) * torch.sin(two_pi * x + 0.3), torch.sin(two_pi * (y - 0.5 * x) + 1.1) * torch.cos(two_pi * z),
                     torch.cos(two_pi * (x + y + z) + 2.0)])
    return (amp * v)[None].repeat(B, 1, 1, 1, 1).contiguous()


def torch_exp(v, K, grid):
    """The op chain a torch user writes: u <- u + grid_sample(u, identity + u), K times (align_corners=True, zeros)."""
    S = v.shape[-1]
    u = v * (1.0 / 2 ** K)
    for _ in range(K):
        loc = (grid + u) * (2.0 / (S - 1)) - 1.0
        u = u + F.grid_sample(u, loc.movedim(1, -1).flip(-1), mode="bilinear", padding_mode="zeros", align_corners=True)
    return u


def bench_shape(B, S, K, spacing, reps, rounds):
    dev = torch.device("cuda")
    lib = _lib.load()
    shape = (S,) * 3
    stream = _lib.current_stream(dev)
    vel = smooth_velocity(B, S, 3.0, dev)
    dflow = torch.randn_like(vel)
    flow, dvel = torch.empty_like(vel), torch.empty_like(vel)
    geom = (3, B, S, S, S, K, 0)
    nws = lib.trx_svf_workspace_bytes(*geom[:-1])
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def exp():
        _lib.check(lib.trx_svf_exp(_lib.ptr(vel), _lib.ptr(flow), *geom, _lib.ptr(ws), nws, stream), "exp")

    def backward():
        _lib.check(lib.trx_svf_exp_backward(_lib.ptr(vel), _lib.ptr(dflow), _lib.ptr(dvel), *geom, _lib.ptr(ws), nws, stream), "backward")

    mov = torch.cat([blobs_gpu(shape, 2000 + b, dev) for b in range(B)])
    tgt = torch.cat([blobs_gpu(shape, 1000 + b, dev) for b in range(B)])
    cap = reps * (rounds + 1) + 8
    init = 0.5 * torch.randn((B, 3) + tr.bspline_grid(shape, spacing), generator=torch.Generator().manual_seed(1))
    kw = dict(loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.05, capacity=cap, init=init)
    plain, svf = tr.BSplineSolver(mov, tgt, spacing, **kw), tr.BSplineSolver(mov, tgt, spacing, squarings=K, **kw)

    def run_plain():
        plain.enqueued += reps
        _lib.check(lib.trx_bspline_run(ctypes.byref(plain.vol), ctypes.byref(plain.loss_c), ctypes.byref(plain.opt), ctypes.byref(plain.state), plain.sp3, reps,
                                       _lib.ptr(plain.workspace), plain.ws_bytes, stream), "run")

    def run_svf():
        svf.enqueued += reps
        _lib.check(lib.trx_bspline_svf_run(ctypes.byref(svf.vol), ctypes.byref(svf.loss_c), ctypes.byref(svf.opt), ctypes.byref(svf.state), svf.sp3, K, reps,
                                           _lib.ptr(svf.workspace), svf.ws_bytes, stream), "svf run")

    grid = torch.stack(torch.meshgrid(*[torch.arange(S, device=dev, dtype=torch.float32)] * 3, indexing="ij"))[None]
    vt = vel.clone().requires_grad_()

    def torch_forward_backward():
        """(forward us, backward us) of one pass of the op chain under autograd."""
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        fw = bw = 0.0
        for _ in range(max(1, reps // 4)):
            vt.grad = None
            e[0].record()
            out = torch_exp(vt, K, grid)
            e[1].record()
            out.backward(dflow)
            e[2].record()
            torch.cuda.synchronize()
            fw += e[0].elapsed_time(e[1]) * 1e3
            bw += e[1].elapsed_time(e[2]) * 1e3
        n = max(1, reps // 4)
        return fw / n, bw / n

    for fn in (exp, backward):
        for _ in range(3):
            fn()
    plain.run(3)
    svf.run(3)
    torch_forward_backward()
    torch.cuda.synchronize()
    per_round = {k: [] for k in ("exp_us", "backward_us", "svf_run_iteration_us", "run_iteration_us", "torch_exp_us", "torch_backward_us")}
    for r in range(rounds):
        per_round["exp_us"].append(timed_us(exp, reps))
        per_round["backward_us"].append(timed_us(backward, reps))
        per_round["svf_run_iteration_us"].append(timed_us(run_svf, 1) / reps)
        per_round["run_iteration_us"].append(timed_us(run_plain, 1) / reps)
        fw, bw = torch_forward_backward()
        per_round["torch_exp_us"].append(fw)
        per_round["torch_backward_us"].append(bw)
        print(f"{B} x {S}^3 K {K} round {r}: " + ", ".join(f"{k} {v[-1]:.1f}" for k, v in per_round.items()), flush=True)
    out = {k: statistics.median(v) for k, v in per_round.items()}
    nvox = B * S ** 3
    out["exp_roofline"] = (K + 1) * 24 * nvox / (out["exp_us"] * 1e-6) / HBM
    out["backward_roofline_without_atomics"] = K * 108 * nvox / (out["backward_us"] * 1e-6) / HBM
    out["exp_over_torch"] = out["exp_us"] / out["torch_exp_us"]
    out["backward_over_torch"] = out["backward_us"] / out["torch_backward_us"]
    out["svf_iteration_over_iteration"] = out["svf_run_iteration_us"] / out["run_iteration_us"]
    # the kept levels of the last exp: share of source voxels whose corners all land inside the splat's LDS tile and halo
    exp()
    torch.cuda.synchronize()
    level_floats = (vel.numel() * 4 + 255) // 256 * 64
    lv = ws[: K * level_floats * 4].view(torch.float32).view(K, level_floats)[:, : vel.numel()].view((K,) + tuple(vel.shape))
    out["lds_share_per_level"] = [float((lv[k].abs().amax(dim=1) < 2.0).float().mean()) for k in range(K)]
    out["max_abs_u_per_level"] = [float(lv[k].abs().max()) for k in range(K)]
    exp()
    backward()
    torch.cuda.synchronize()
    vt.grad = None
    torch_exp(vt, K, grid).backward(dflow)
    out["max_abs_dvel_minus_torch_over_max"] = float((dvel - vt.grad).abs().max() / vt.grad.abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x128,1x256")
    ap.add_argument("--squarings", type=int, default=6)
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_svf.py needs a GPU: there is no CPU path to time")
    out = {}
    for item in a.shapes.split(","):
        B, S = (int(v) for v in item.split("x"))
        out[f"{B}x{S}^3"] = bench_shape(B, S, a.squarings, a.spacing, a.reps, a.rounds)
    print(json.dumps(dict(tool="bench_svf", squarings=a.squarings, spacing=a.spacing, optimizer="adam", loss="ncc", hbm_peak_TBps=HBM / 1e12, **out)))


if __name__ == "__main__":
    main()
