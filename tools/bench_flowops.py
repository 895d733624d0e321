#!/usr/bin/env python3
"""What dense-flow composition and the fused fixed-point inversion cost: microseconds per call, one pair at 128^3 and 256^3, on a
smooth field of `--amp` voxels' amplitude.
  compose    trx_flow_compose with either padding (12 B/voxel of `second` read, 12 gathered from `first`, 12 written: 36) against one
             trx_svf_exp(..., squarings = 1) on the same field - the squaring launch behind a scaling launch of 24 B/voxel of its own;
  invert     trx_flow_invert at tol = 0 with K = 5, 10, 20 updates (12 B/voxel read through the caches, 12 written: 24; 28 with the residual) and at
             tol = 1e-3 within 30 (`converged` and `updates_max` say what the field needed), against the chain it replaces: K x F.grid_sample of u
             at id + v with padding_mode='border', align_corners=True, the negation and the conversion of voxel positions to grid_sample's
             normalised (x, y, z)-last layout included (the identity positions are made once, outside the timing), in torch on the same box;
             `against_chain` is chain time / fused time, `max_diff` the largest difference between the two results.
`share` is the named bytes over the time as a share of 8 TB/s.  hipEvents around `reps` calls after a warm-up of every leg, the legs alternating within
a round; a line holds the median of the rounds and their range.  --out FILE appends the lines to FILE (profiles/flowops_bench.txt is this tool's output)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib  # noqa: E402

PEAK = 8e12      # bytes / s


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def smooth_flow(S, dev, amp, seed=3):
    """[1,3,S,S,S]: three low-frequency waves per channel, amplitudes summing to `amp`, and a little noise."""
    ax = torch.meshgrid(*[torch.linspace(0, 1, S, device=dev)] * 3, indexing="ij")
    g = torch.Generator(device=dev).manual_seed(seed)
    ch = []
    for c in range(3):
        f = sum(torch.cos(2 * torch.pi * ((1 + (c + k) % 3) * ax[(c + k) % 3] + 0.5 * (k + 1) * ax[(c + k + 1) % 3]) + 0.7 * c + k + seed) for k in range(3))
        ch.append(amp / 3 * f)
    return (torch.stack(ch)[None] + 0.02 * (torch.rand((1, 3, S, S, S), generator=g, device=dev) - 0.5)).contiguous()


def timed(legs, reps, rounds):
    """legs: name -> (fn, reps divisor).  Every leg is warmed up, then the legs alternate within each round."""
    for fn, _ in legs.values():
        event_us(fn, 1)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (fn, div) in legs.items():
            t[k].append(event_us(fn, max(1, reps // div)))
    return t


def row(case, op, leg, v, nbytes=None, **extra):
    med = statistics.median(v)
    r = dict(case=case, op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)], **extra)
    if nbytes:
        r.update(bytes_per_voxel=nbytes[0], share_of_8TBs=round(nbytes[0] * nbytes[1] / (med * 1e-6) / PEAK, 4))
    return r


class Chain:
    """K x grid_sample of u at id + v: what a user writes without the fused kernel."""

    def __init__(self, u):
        S = u.shape[2:]
        self.u = u
        self.ident = torch.stack(torch.meshgrid(*[torch.arange(s, dtype=torch.float32, device=u.device) for s in S], indexing="ij"))[None]
        self.scale = torch.tensor([2.0 / max(s - 1, 1) for s in S], device=u.device).view(1, 3, 1, 1, 1)

    def __call__(self, K):
        v = torch.zeros_like(self.u)
        for _ in range(K):
            grid = ((self.ident + v) * self.scale - 1.0).flip(1).permute(0, 2, 3, 4, 1)
            v = -F.grid_sample(self.u, grid, mode="bilinear", padding_mode="border", align_corners=True)
        return v


def bench(S, amp, reps, rounds):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    u, s = smooth_flow(S, dev, amp), smooth_flow(S, dev, amp, seed=5)
    n, geom, case, rows = S ** 3, (3, 1, S, S, S), f"1x{S}^3", []
    out, res = torch.empty_like(u), torch.empty((1, 1, S, S, S), device=dev)
    nws = lib.trx_svf_workspace_bytes(*geom, 1)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    two_u = 2 * u

    def compose(pad):
        return lambda: _lib.check(lib.trx_flow_compose(_lib.ptr(u), _lib.ptr(s), _lib.ptr(out), *geom, pad, stream), "trx_flow_compose")

    legs = {"compose/border": (compose(1), 1), "compose/zeros": (compose(0), 1),
            "svf_exp/squarings=1": (lambda: _lib.check(lib.trx_svf_exp(_lib.ptr(two_u), _lib.ptr(out), *geom, 1, 0, _lib.ptr(ws), nws, stream), "trx_svf_exp"), 1)}
    t = timed(legs, reps, rounds)
    for k, v in t.items():
        op, _, leg = k.partition("/")
        rows.append(row(case, op, leg, v, (36 if op == "compose" else 60, n), reps=reps, rounds=rounds))
    rows[-1]["note"] = "two launches: the scaling (24 B/voxel) and the squaring (36 B/voxel)"

    chain = Chain(u)

    def invert(K, tol, residual):
        return lambda: _lib.check(lib.trx_flow_invert(_lib.ptr(u), None, _lib.ptr(out), _lib.ptr(res) if residual else None, *geom, K, tol, stream), "trx_flow_invert")

    legs = {}
    for K in (5, 10, 20):
        legs[f"fused/K={K}"] = (invert(K, 0.0, False), 1)
        legs[f"chain/K={K}"] = (lambda K=K: chain(K), 10)
    legs["fused+residual/K=20"] = (invert(20, 0.0, True), 1)
    legs["fused+residual/tol=1e-3"] = (invert(30, 1e-3, True), 1)
    t = timed(legs, reps, rounds)
    v_tol, r_tol = tr.invert_flow(u, 30, 1e-3, return_residual=True)
    conv = dict(converged=round((r_tol <= 1e-3).float().mean().item(), 6), residual_max=float(f"{r_tol.max().item():.3e}"), amplitude=round(u.abs().max().item(), 3))
    for k, v in t.items():
        op, _, leg = k.partition("/")
        extra = dict(reps=max(1, reps // legs[k][1]), rounds=rounds)
        if op == "chain":
            K = int(leg[2:])
            fused = statistics.median(t[f"fused/K={K}"])
            extra.update(against_chain=round(statistics.median(v) / fused, 2), max_diff=float(f"{(chain(K) - tr.invert_flow(u, K, 0.0)).abs().max().item():.2e}"))
            rows.append(row(case, "invert", k, v, **extra))
        else:
            if "tol" in leg:
                extra.update(conv)
            rows.append(row(case, "invert", k, v, (28 if "residual" in op else 24, n), **extra))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--amp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flowops.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_flowops.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for S in (int(v) for v in a.sizes.split(",")):
        for r in bench(S, a.amp, a.reps, a.rounds):
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
