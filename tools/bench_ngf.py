#!/usr/bin/env python3
"""What the normalised gradient field criterion costs: microseconds per call, one pair at 128^3 and 256^3.
  ngf        trx_ngf_loss_grad with and without a mask (a ball of ~40 % of the voxels): `loss` is the loss-only call (forward + reduce: 8 B/voxel
             read, + 1 with a mask), `grad` the call with a gradient (forward with the q stores, reduce, backward: 8 (+ 1) + 12 read, 12 + 4 written);
  torch      the same restatement as torch ops under autograd (ngf_gradient, clamped-index differences) on the same box: forward, and forward + backward;
  iter       one iteration of trx_bspline_ngf_run beside one of trx_bspline_mi_run (spacing 8, Adam, `--iters` iterations per call, zero control
             tensor) - the same box, the same process, alternating within a round.
`share` is the named bytes over the time as a share of 8 TB/s.  hipEvents around `reps` calls after a warm-up of every leg and one untimed
call in front of every window; the bytes are the ones the algorithm names, computed from the shape - no counter run measures the traffic; a line holds the median of the
rounds and their range.  Not measured here: batches, 2-D, anisotropic voxel sizes.  --out FILE appends the lines to FILE (profiles/ngf_bench.txt is this
tool's output)."""
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

PEAK = 8e12      # bytes / s
STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def timed(legs, reps, rounds, per=1):
    for fn in legs.values():
        event_us(fn, 2)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            fn()      # one untimed call: a leg's window does not start on the clocks and caches the leg before it left behind
            t[k].append(event_us(fn, reps) / per)
    return t


def row(case, op, leg, v, nbytes=None, **extra):
    med = statistics.median(v)
    r = dict(case=case, op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)], **extra)
    if nbytes:
        r.update(bytes_per_voxel=nbytes[0], share_of_8TBs=round(nbytes[0] * nbytes[1] / (med * 1e-6) / PEAK, 4))
    return r


def pair(S, dev):
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev)[None], tgt)
    return (1.0 + 4.0 * w * (1.0 - w)).contiguous(), tgt


def torch_ngf(tgt, wrp, eps, mask):
    """ngf_loss_grad's definition in torch ops (differentiable with respect to wrp)."""
    gT, gW = tr._engine.ngf_gradient(tgt), tr._engine.ngf_gradient(wrp)
    s = (gW * gT).sum(1, keepdim=True)
    ab = ((gW * gW).sum(1, keepdim=True) + eps[:, 1].view(-1, 1, 1, 1, 1) ** 2) * ((gT * gT).sum(1, keepdim=True) + eps[:, 0].view(-1, 1, 1, 1, 1) ** 2)
    r = torch.where(ab == 0, torch.zeros_like(ab), s * s / torch.where(ab == 0, torch.ones_like(ab), ab))
    if mask is None:
        return 1.0 - r.flatten(1).mean(1)
    m = mask.float()
    return 1.0 - (r * m).flatten(1).sum(1) / m.flatten(1).sum(1)


def bench_kernels(S, reps, rounds):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    mov, tgt = pair(S, dev)
    n, geom = S ** 3, (3, 1, S, S, S)
    eps = tr.ngf_edge_parameters(tgt, mov)
    ax = torch.meshgrid(*[torch.linspace(-1, 1, S, device=dev)] * 3, indexing="ij")
    ball = ((ax[0] ** 2 + ax[1] ** 2 + ax[2] ** 2) <= 0.92 ** 2).to(torch.uint8)[None, None].contiguous()
    nws = lib.trx_ngf_workspace_bytes(*geom)
    ws, loss, grad = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev), torch.empty_like(mov)
    cfgs = {"nomask": tr._engine._ngf_cfg_c(1.0, eps, None, None), "mask": tr._engine._ngf_cfg_c(1.0, eps, None, ball)}
    legs = {}
    for k, (cfg, _) in cfgs.items():
        legs[f"ngf/loss/{k}"] = lambda cfg=cfg: _lib.check(lib.trx_ngf_loss_grad(_lib.ptr(tgt), _lib.ptr(mov), *geom, ctypes.byref(cfg), _lib.ptr(loss), None,
                                                                                  _lib.ptr(ws), nws, stream), "trx_ngf_loss_grad")
        legs[f"ngf/grad/{k}"] = lambda cfg=cfg: _lib.check(lib.trx_ngf_loss_grad(_lib.ptr(tgt), _lib.ptr(mov), *geom, ctypes.byref(cfg), _lib.ptr(loss),
                                                                                  _lib.ptr(grad), _lib.ptr(ws), nws, stream), "trx_ngf_loss_grad")
    w = mov.clone().requires_grad_()

    def torch_fwd(mask):
        with torch.no_grad():
            torch_ngf(tgt, mov, eps, mask)

    def torch_both(mask):
        w.grad = None
        torch_ngf(tgt, w, eps, mask).sum().backward()

    for k, m in (("nomask", None), ("mask", ball)):
        legs[f"torch/loss/{k}"] = lambda m=m: torch_fwd(m)
        legs[f"torch/grad/{k}"] = lambda m=m: torch_both(m)
    t = timed(legs, reps, rounds)
    rows = []
    for k, v in t.items():
        op, leg, masked = k.split("/")
        nbytes = None
        if op == "ngf":
            nbytes = ((8 if leg == "loss" else 36) + (1 if masked == "mask" else 0), n)
        rows.append(row(f"1x{S}^3", op, f"{leg}/{masked}", v, nbytes, reps=reps, rounds=rounds, **(dict(masked_share=round(ball.float().mean().item(), 4)) if masked == "mask" else {})))
    return rows


def bench_loops(S, spacing, iters, reps, rounds, bins=32):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    mov, tgt = pair(S, dev)
    d3, sp = (ctypes.c_int * 3)(spacing, spacing, spacing), (spacing,) * 3
    G = tr.bspline_grid((S,) * 3, spacing)
    opt = tr._engine.opt_cfg("adam", 0.05)
    vol = tr._engine._Batch(mov, tgt, tables=False).vol()
    eps = tr.ngf_edge_parameters(tgt, mov)
    ncfg, _ = tr._engine._ngf_cfg_c(1.0, eps, None, None)
    mcfg = tr._engine._mi_cfg_c(bins, 1.0, False, tr._engine.mi_range(tgt, mov), None)
    geom = (3, 1, S, S, S)
    sizes = dict(ngf=lib.trx_bspline_ngf_workspace_bytes(*geom, *sp, None), mi=lib.trx_bspline_mi_workspace_bytes(*geom, *sp, bins))
    assert all(v > 0 for v in sizes.values())
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    c0 = torch.zeros((1, 3) + G, device=dev)
    keep = []

    def state():
        st = _lib.BSplineState()
        t = dict(ctrl=c0.clone(), adam_m=torch.zeros_like(c0), adam_v=torch.zeros_like(c0), flow=torch.empty(1, 3, S, S, S, device=dev),
                 dflow=torch.empty(1, 3, S, S, S, device=dev), step=torch.zeros(1, dtype=torch.int32, device=dev))
        keep.append(t)
        for k, v in t.items():
            setattr(st, k, v.data_ptr())
        st.losses, st.losses_capacity, st.stopped, st.flow_last, st.base, st.bending_weight = None, 0, None, None, None, 0.0
        return t, st

    states = {k: state() for k in ("ngf", "mi")}
    ref = ctypes.byref
    calls = {
        "ngf": lambda: lib.trx_bspline_ngf_run(ref(vol), None, None, ref(ncfg), ref(opt), ref(states["ngf"][1]), d3, None, iters, _lib.ptr(ws), sizes["ngf"], stream),
        "mi": lambda: lib.trx_bspline_mi_run(ref(vol), ref(mcfg), ref(opt), ref(states["mi"][1]), d3, iters, _lib.ptr(ws), sizes["mi"], stream),
    }

    def leg(k):
        def fn():
            t = states[k][0]
            t["ctrl"].copy_(c0)
            t["adam_m"].zero_()
            t["adam_v"].zero_()
            t["step"].zero_()
            _lib.check(calls[k](), k)
        return fn

    t = timed({k: leg(k) for k in calls}, max(1, reps // iters), rounds, per=iters)
    mi = statistics.median(t["mi"])
    return [row(f"1x{S}^3", f"iter-{k}", "-", v, spacing=spacing, iters_per_call=iters, rounds=rounds, against_mi=round(statistics.median(v) / mi, 4))
            for k, v in t.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ngf.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_ngf.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for S in (int(v) for v in a.sizes.split(",")):
        for r in bench_kernels(S, a.reps, a.rounds) + bench_loops(S, a.spacing, a.iters, a.reps, a.rounds):
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
