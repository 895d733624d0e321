#!/usr/bin/env python3
"""Per-iteration time of the fused rigid / affine mutual-information loop (AffineMISolver.run -> trx_affine_mi_run) against what it replaces:
  (a) chain    the existing entry points enqueued back to back without a sync, buffers preallocated:
               trx_affine_warp -> trx_mi_loss_grad -> trx_affine_warp_backward (no optimiser step: the chain is flattered by that);
  (b) generic  the loop Register(..., criterion=[MILoss()], honor_criterion=True) runs today (warpings._generic_loop: the same three entry points
               behind torch autograd, a torch optimiser step and an .item() per iteration).
One pair at 128^3 and 256^3 and 8 pairs at 256^3, 32 bins, at a pose next to the identity and at a 0.5 rad rotation about z.  Every leg runs with
learning rate 0 (SGD), so the pose it is timed at is the pose it stays at.  hipEvents around `reps` iterations after a warm-up of every leg; the
legs alternate within a round, the line holds the median of the rounds and their spread.  Bytes: the fused loop needs 16 B/voxel and iteration
(moving and target read twice), the chain about 36: both also as a share of 8 TB/s.
--out FILE appends the lines to FILE (profiles/affine_mi_bench.txt is this tool's output)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib, warpings  # noqa: E402
from bench import blobs_gpu  # noqa: E402

HBM = 8.0e12
NEAR = [[1.01, 0.013, -0.007, 0.011], [-0.009, 0.99, 0.012, -0.013], [0.006, -0.011, 1.008, 0.009]]
STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]


def poses():
    c, s = math.cos(0.5), math.sin(0.5)
    return {"near-identity": torch.tensor(NEAR), "rot-0.5rad": torch.tensor([[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]])}


def event_us(fn, reps):
    """fn() enqueues `reps` iterations; microseconds per iteration between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def bench_case(B, S, bins, name, theta, reps, generic_reps, rounds):
    dev = torch.device("cuda")
    lib = _lib.load()
    shape = (S,) * 3
    tgt = torch.cat([blobs_gpu(shape, 1000 + b, dev) for b in range(B)])
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev).expand(B, 3, 4), tgt)
    mov = (4.0 * w * (1.0 - w)).contiguous()
    del w
    th_b = theta.expand(B, 3, 4).contiguous()
    cap = reps * (rounds + 1)
    fused = tr.AffineMISolver(mov, tgt, mode="affine", mi=dict(bins=bins), optimizer="sgd", lr=0.0, init=th_b, capacity=cap)

    # (a) the chain through the C ABI
    batch = tr._engine._Batch(mov, tgt)
    vol = batch.vol()
    th = tr._engine.pad_theta(th_b.to(dev).reshape(B, -1), 3)
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, 1.0, 0, fused.mi_range.data_ptr()
    n_mi, n_aff = lib.trx_mi_workspace_bytes(3, B, S, S, S, bins), lib.trx_affine_workspace_bytes(ctypes.byref(vol))
    ws_mi, ws_aff = torch.empty(n_mi, dtype=torch.uint8, device=dev), torch.empty(n_aff, dtype=torch.uint8, device=dev)
    warped, gw = torch.empty_like(mov), torch.empty_like(mov)
    loss, dth = torch.empty(B, device=dev), torch.zeros(B, 12, device=dev)
    stream = _lib.current_stream(dev)

    def chain():
        for _ in range(reps):
            _lib.check(lib.trx_affine_warp(ctypes.byref(vol), _lib.ptr(th), 1, _lib.ptr(warped), stream), "warp")
            _lib.check(lib.trx_mi_loss_grad(_lib.ptr(tgt), _lib.ptr(warped), 3, B, S, S, S, ctypes.byref(cfg), _lib.ptr(loss), _lib.ptr(gw), _lib.ptr(ws_mi), n_mi,
                                            stream), "mi_loss_grad")
            _lib.check(lib.trx_affine_warp_backward(ctypes.byref(vol), _lib.ptr(th), 1, _lib.ptr(gw), _lib.ptr(dth), _lib.ptr(ws_aff), n_aff, stream), "warp_backward")

    def generic():
        """The generic loop as it stands (one theta for the batch, ranges refitted per call); host clock around the whole call, which ends in a sync."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        warpings._generic_loop(mov, tgt, "affine", [tr.MILoss(bins=bins)], [1.0], 0.0, generic_reps, theta[None], "sgd")
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / generic_reps

    fused.run(reps)                                                # warm-up of every leg
    chain()
    generic()
    torch.cuda.synchronize()
    # the two device paths agree on what they compute at this pose (the fused gradient of the last iteration against the chain's)
    agree = (fused.grad[:, :12] - dth).abs().max().item() / max(dth.abs().max().item(), 1e-30)
    t = {"fused": [], "chain": [], "generic": []}
    for _ in range(rounds):
        t["fused"].append(event_us(lambda: fused.run(reps), reps))
        t["chain"].append(event_us(chain, reps))
        t["generic"].append(generic())
    med = {k: statistics.median(v) for k, v in t.items()}
    nvox = B * S ** 3
    out = dict(case=f"{B}x{S}^3", pose=name, bins=bins, reps=reps, rounds=rounds,
               fused_us=round(med["fused"], 2), chain_us=round(med["chain"], 2), generic_us=round(med["generic"], 1),
               fused_range_us=[round(min(t["fused"]), 2), round(max(t["fused"]), 2)], chain_range_us=[round(min(t["chain"]), 2), round(max(t["chain"]), 2)],
               fused_over_chain=round(med["fused"] / med["chain"], 3), fused_over_generic=round(med["fused"] / med["generic"], 4),
               fused_share_of_8TBps_at_16B=round(16 * nvox / (med["fused"] * 1e-6) / HBM, 3), chain_share_of_8TBps_at_36B=round(36 * nvox / (med["chain"] * 1e-6) / HBM, 3),
               loss=[round(v, 6) for v in loss.tolist()[:2]], dtheta_rel_diff_fused_vs_chain=float(f"{agree:.2e}"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1x128,1x256,8x256")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--generic-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_affine_mi.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_affine_mi.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for item in a.cases.split(","):
        B, S = (int(v) for v in item.split("x"))
        for name, theta in poses().items():
            line = json.dumps(bench_case(B, S, a.bins, name, theta, a.reps, a.generic_reps, a.rounds))
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
