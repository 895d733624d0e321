#!/usr/bin/env python3
"""What the affine-then-flow resampler and the point transform cost: microseconds per call on one pair.
  256^3        1 x 256^3 onto 256^3 through a 0.2 rad rotation about z and a smooth flow of `--amp` voxels on the source lattice;
  grids        256 x 256 x 180 (W x H x D) onto 512 x 512 x 120 through the same rotation: the moving and target lattices of a CT / MR pair;
  legs         new/<interpolation>      tr.resample_affine_then_flow ('cubic' includes the coefficients of every call: see the coefficients leg);
               resample/<interpolation> tr.resample(theta=, flow=) on the same data: the other chain order (the flow on the OUTPUT lattice), the same
                                        gather counts - the existing kernels the new one is modelled on;
               torch/<mode>             the chain the new kernel replaces, in torch on the same box: F.grid_sample of the flow (border) at
                                        F.affine_grid(theta), the grid built from it, F.grid_sample of the image, for bilinear and nearest;
               coefficients             tr.spline_coefficients alone;
  points       tr.transform_points at P = 10^6, both chains, theta and flow of the 256^3 case.
Bytes per output voxel are the compulsory ones: 4 of the image and 12 of the flow per SOURCE voxel, 4 written per output voxel (points: 12 read, 12
written per point; the flow's 12 per lattice voxel are not counted).  `share` is those bytes over the time as a share of 8 TB/s.  hipEvents around `reps`
calls after a warm-up of every leg, the legs alternating within a round; a line holds the median of the rounds and their range.  --out FILE appends
the lines to FILE (profiles/chain_bench.txt is this tool's output)."""
import argparse
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

PEAK = 8e12      # bytes / s


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def timed(legs, reps, rounds):
    for fn in legs.values():
        event_us(fn, 1)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, reps))
    return t


def smooth_flow(shape, dev, amp, seed=3):
    ax = torch.meshgrid(*[torch.linspace(0, 1, s, device=dev) for s in shape], indexing="ij")
    g = torch.Generator(device=dev).manual_seed(seed)
    ch = []
    for c in range(3):
        f = sum(torch.cos(2 * torch.pi * ((1 + (c + k) % 3) * ax[(c + k) % 3] + 0.5 * (k + 1) * ax[(c + k + 1) % 3]) + 0.7 * c + k + seed) for k in range(3))
        ch.append(amp / 3 * f)
    return (torch.stack(ch)[None] + 0.02 * (torch.rand((1, 3) + tuple(shape), generator=g, device=dev) - 0.5)).contiguous()


def rotation(angle, dev):
    c, s = math.cos(angle), math.sin(angle)
    return torch.tensor([[[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]], device=dev)


def torch_chain(x, theta, flow, size, mode):
    """x [1,C,*src] at q + flow(q), q = theta applied to the output lattice: what a user writes without the kernel."""
    src = x.shape[2:]
    q = F.affine_grid(theta, [1, 1, *size], align_corners=False)
    v = F.grid_sample(flow, q, mode="bilinear", padding_mode="border", align_corners=False)                      # voxels, channels z, y, x
    scale = torch.tensor([2.0 / src[2], 2.0 / src[1], 2.0 / src[0]], device=x.device)
    return F.grid_sample(x, q + v.flip(1).permute(0, 2, 3, 4, 1) * scale, mode=mode, padding_mode="zeros", align_corners=False)


def row(case, leg, v, nbytes=None, **extra):
    med = statistics.median(v)
    r = dict(case=case, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)], **extra)
    if nbytes:
        r.update(bytes_per_voxel=round(nbytes[0], 2), share_of_8TBs=round(nbytes[0] * nbytes[1] / (med * 1e-6) / PEAK, 4))
    return r


def bench_images(case, src, out, amp, reps, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.rand((1, 1) + src, generator=g, device=dev)
    theta = rotation(0.2, dev)
    flow_src, flow_out = smooth_flow(src, dev, amp), smooth_flow(out, dev, amp)
    nsrc, nout = math.prod(src), math.prod(out)
    legs = {}
    for mode in ("nearest", "linear", "cubic"):
        legs[f"new/{mode}"] = lambda mode=mode: tr.resample_affine_then_flow(x, theta=theta, flow=flow_src, size=out, interpolation=mode)
        legs[f"resample/{mode}"] = lambda mode=mode: tr.resample(x, theta=theta, flow=flow_out, interpolation=mode)
    legs["torch/bilinear"] = lambda: torch_chain(x, theta, flow_src, out, "bilinear")
    legs["torch/nearest"] = lambda: torch_chain(x, theta, flow_src, out, "nearest")
    legs["coefficients"] = lambda: tr.spline_coefficients(x)
    t = timed(legs, reps, rounds)
    rows = []
    for k, v in t.items():
        if k.startswith("new/"):
            nbytes = ((16.0 * nsrc + 4.0 * nout) / nout, nout)
        elif k.startswith("resample/"):
            nbytes = ((4.0 * nsrc + 16.0 * nout) / nout, nout)
        else:
            nbytes = None
        extra = dict(reps=reps, rounds=rounds)
        if k.startswith("torch/"):
            mode = "linear" if k.endswith("bilinear") else "nearest"
            new = statistics.median(t[f"new/{mode}"])
            a, b = legs[k](), legs[f"new/{mode}"]()
            extra.update(against_new=round(statistics.median(v) / new, 2), differing_share=round(((a - b).abs() > 1e-3).float().mean().item(), 6))
        rows.append(row(case, k, v, nbytes, **extra))
    return rows


def bench_points(P, amp, reps, rounds):
    dev = torch.device("cuda")
    S = (256, 256, 256)
    theta, flow = rotation(0.2, dev), smooth_flow(S, dev, amp)
    p = torch.rand((1, P, 3), generator=torch.Generator(device=dev).manual_seed(2), device=dev) * 255.0
    legs = {f"points/{chain}": (lambda chain=chain: tr.transform_points(p, theta=theta, flow=flow, from_shape=S, to_shape=S, chain=chain))
            for chain in ("flow_then_affine", "affine_then_flow")}
    t = timed(legs, reps, rounds)
    return [row(f"P={P}", k, v, (24.0, P), reps=reps, rounds=rounds) for k, v in t.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_chain.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_chain.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    rows = bench_images("1x256^3", (256, 256, 256), (256, 256, 256), a.amp, a.reps, a.rounds)
    rows += bench_images("180x256x256->120x512x512", (180, 256, 256), (120, 512, 512), a.amp, a.reps, a.rounds)
    rows += bench_points(1000000, a.amp, a.reps, a.rounds)
    for r in rows:
        line = json.dumps(r)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
