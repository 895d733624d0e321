#!/usr/bin/env python3
"""What the Jacobian determinant map and the folding penalty cost: microseconds per call, one pair at 128^3 and 256^3.
  jacobian   trx_flow_jacobian: 12 B/voxel read, 4 written;
  folding    trx_flow_folding with dflow and accumulate = 1 (the loop's form: map + partials, second stage, gather) on a smooth field whose threshold is
             set to the field's own determinant quantile, so that 0 %, 5 % and 50 % of the voxels are active: 16 B/voxel for the forward, 4 (det) + 12
             (dflow read) + 12 (dflow written) for the gather; `fwd` is the same call with dflow = NULL;
  iter       one iteration of trx_bspline_run_fold (NCC) against trx_bspline_run, and of trx_bspline_mi_run_fold through an initial affine against
             trx_bspline_mi_run_grids - the same box, the same process, alternating within a round (spacing 8, Adam, `--iters` iterations per call) -
             from a zero control tensor (`zero`: nothing is active) and from a random one of amplitude 8 voxels (`rough`: the share is on the line).
`share` is the named bytes over the time as a share of 8 TB/s.  hipEvents around `reps` calls after a warm-up of every leg; a line holds the median of the
rounds and their range.  --out FILE appends the lines to FILE (profiles/fold_bench.txt is this tool's output)."""
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


def smooth_flow(S, dev, amp=6.0):
    """[1,3,S,S,S]: three low-frequency waves per channel and a little noise - folds in patches, as a rough registration does."""
    ax = torch.meshgrid(*[torch.linspace(0, 1, S, device=dev)] * 3, indexing="ij")
    g = torch.Generator(device=dev).manual_seed(3)
    ch = []
    for c in range(3):
        f = sum(torch.cos(2 * torch.pi * ((1 + (c + k) % 3) * ax[(c + k) % 3] + 0.5 * (k + 1) * ax[(c + k + 1) % 3]) + 0.7 * c + k) for k in range(3))
        ch.append(amp / 3 * f)
    return (torch.stack(ch)[None] + 0.05 * (torch.rand((1, 3, S, S, S), generator=g, device=dev) - 0.5)).contiguous()


def timed(legs, reps, rounds, per=1):
    for fn in legs.values():
        event_us(fn, 2)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, reps) / per)
    return t


def row(case, op, leg, v, nbytes=None, **extra):
    med = statistics.median(v)
    r = dict(case=case, op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)], **extra)
    if nbytes:
        r.update(bytes_per_voxel=nbytes[0], share_of_8TBs=round(nbytes[0] * nbytes[1] / (med * 1e-6) / PEAK, 4))
    return r


def bench_kernels(S, reps, rounds):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    fl = smooth_flow(S, dev)
    n = S ** 3
    geom = (3, 1, S, S, S)
    det = tr.jacobian_determinant(fl)
    flat = det.reshape(-1)
    thr = {"0%": flat.min().item() - 1.0, "5%": torch.kthvalue(flat, int(0.05 * n)).values.item(), "50%": torch.kthvalue(flat, n // 2).values.item()}
    nws = lib.trx_flow_folding_workspace_bytes(*geom)
    ws, pen, dflow = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(1, device=dev), torch.zeros_like(fl)
    legs = {"jacobian": lambda: _lib.check(lib.trx_flow_jacobian(_lib.ptr(fl), *geom, _lib.ptr(det), stream), "trx_flow_jacobian")}
    for k, t in thr.items():
        legs[f"folding/{k}"] = lambda t=t: _lib.check(lib.trx_flow_folding(_lib.ptr(fl), *geom, t, 1.0, _lib.ptr(pen), _lib.ptr(dflow), 1, _lib.ptr(ws), nws, stream),
                                                      "trx_flow_folding")
        legs[f"fwd/{k}"] = lambda t=t: _lib.check(lib.trx_flow_folding(_lib.ptr(fl), *geom, t, 1.0, _lib.ptr(pen), None, 0, _lib.ptr(ws), nws, stream), "trx_flow_folding")
    t = timed(legs, reps, rounds)
    case, rows = f"1x{S}^3", []
    for k, v in t.items():
        op, _, leg = k.partition("/")
        active = None if not leg else round((flat < thr[leg]).float().mean().item(), 4)
        rows.append(row(case, op, leg or "-", v, (16 if op != "folding" else 44, n), **({} if active is None else dict(active=active)), reps=reps, rounds=rounds))
    return rows


def bench_loops(S, spacing, iters, reps, rounds, bins=32):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev)[None], tgt)
    mov_mi, mov_ncc = (1.0 + 4.0 * w * (1.0 - w)).contiguous(), w.contiguous()
    theta = tr._engine.pad_theta(torch.tensor(STAR, device=dev).reshape(1, -1), 3)
    d3, sp = (ctypes.c_int * 3)(spacing, spacing, spacing), (spacing,) * 3
    G = tr.bspline_grid((S,) * 3, spacing)
    opt, loss, fold = tr._engine.opt_cfg("adam", 0.05), tr.LossSpec(w_ncc=1.0).c(), _lib.FoldCfg(100.0, 0.3)
    vol_ncc = tr._engine._Batch(mov_ncc, tgt, tables=False).vol()
    pair = tr._engine._GridPair(mov_mi, tgt)
    vol_mi, grid = pair.vol(), pair.grid()
    cfg = tr._engine._mi_cfg_c(bins, 1.0, False, tr._engine.mi_range(tgt, mov_mi), None)
    geom = (3, 1, S, S, S)
    sizes = dict(ncc=lib.trx_bspline_workspace_bytes(*geom, *sp), ncc_fold=lib.trx_bspline_fold_workspace_bytes(*geom, *sp),
                 mi=lib.trx_bspline_mi_grids_workspace_bytes(*geom, *sp, bins, ctypes.byref(grid)),
                 mi_fold=lib.trx_bspline_mi_fold_workspace_bytes(*geom, *sp, bins, ctypes.byref(grid)))
    assert all(v > 0 for v in sizes.values())
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device=dev)
    keep, rows = [], []
    gen = torch.Generator(device=dev).manual_seed(11)
    starts = {"zero": torch.zeros((1, 3) + G, device=dev), "rough": (torch.rand((1, 3) + G, generator=gen, device=dev) - 0.5) * 16.0}
    for start, c0 in starts.items():
        active = round((tr.jacobian_determinant(tr.bspline_expand(c0, (S,) * 3, spacing)) < fold.threshold).float().mean().item(), 4)

        def state():
            st = _lib.BSplineState()
            t = dict(ctrl=c0.clone(), adam_m=torch.zeros_like(c0), adam_v=torch.zeros_like(c0), flow=torch.empty(1, 3, S, S, S, device=dev),
                     dflow=torch.empty(1, 3, S, S, S, device=dev), step=torch.zeros(1, dtype=torch.int32, device=dev))
            keep.append(t)
            for k, v in t.items():
                setattr(st, k, v.data_ptr())
            st.losses, st.losses_capacity, st.stopped, st.flow_last, st.base, st.bending_weight = None, 0, None, None, None, 0.0
            return t, st

        states = {k: state() for k in ("ncc/plain", "ncc/fold", "mi/plain", "mi/fold")}

        def reset(k):      # every timed call starts from the same control tensor: the active share stays the one on the line
            t = states[k][0]
            t["ctrl"].copy_(c0)
            t["adam_m"].zero_()
            t["adam_v"].zero_()
            t["step"].zero_()

        ref = ctypes.byref
        calls = {
            "ncc/plain": lambda: lib.trx_bspline_run(ref(vol_ncc), ref(loss), ref(opt), ref(states["ncc/plain"][1]), d3, iters, _lib.ptr(ws), sizes["ncc"], stream),
            "ncc/fold": lambda: lib.trx_bspline_run_fold(ref(vol_ncc), ref(loss), ref(opt), ref(states["ncc/fold"][1]), d3, ref(fold), iters, _lib.ptr(ws),
                                                         sizes["ncc_fold"], stream),
            "mi/plain": lambda: lib.trx_bspline_mi_run_grids(ref(vol_mi), ref(grid), _lib.ptr(theta), ref(cfg), ref(opt), ref(states["mi/plain"][1]), d3, iters,
                                                             _lib.ptr(ws), sizes["mi"], stream),
            "mi/fold": lambda: lib.trx_bspline_mi_run_fold(ref(vol_mi), ref(grid), _lib.ptr(theta), ref(cfg), ref(opt), ref(states["mi/fold"][1]), d3, ref(fold),
                                                           iters, _lib.ptr(ws), sizes["mi_fold"], stream),
        }

        def leg(k):
            def fn():
                reset(k)
                _lib.check(calls[k](), k)
            return fn

        def resets_only(k):
            return lambda: reset(k)

        legs = {k: leg(k) for k in calls}
        legs.update({k + "/reset": resets_only(k) for k in ("ncc/plain",)})      # the four small copies every leg carries, timed alone
        t = timed(legs, max(1, reps // iters), rounds, per=iters)
        for k in calls:
            data, which = k.split("/")
            extra = dict(start=start, active_at_start=active, iters_per_call=iters, rounds=rounds)
            if which == "fold":
                plain = statistics.median(t[f"{data}/plain"])
                extra.update(over_plain_us=round(statistics.median(t[k]) - plain, 2), against_plain=round(statistics.median(t[k]) / plain, 4))
            rows.append(row(f"1x{S}^3", f"iter-{data}", which, t[k], **extra))
        rows.append(row(f"1x{S}^3", "iter-reset", "-", t["ncc/plain/reset"], start=start, note="per iteration share of the reset copies inside every iter leg"))
    return rows


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
        raise SystemExit("bench_fold.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_fold.py " + " ".join(sys.argv[1:]),
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
