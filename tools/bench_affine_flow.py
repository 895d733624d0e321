#!/usr/bin/env python3
"""What composing the deformation with an initial affine costs: microseconds per call of
  warp   trx_affine_flow_warp            against trx_flow_warp
  bwd    trx_affine_flow_warp_backward   against trx_flow_warp_backward
  iter   one iteration of trx_bspline_mi_run_grids against one of trx_bspline_mi_run (32 bins, spacing 8, Adam; `--iters` iterations per call)
one pair, one channel, targets of 128^3 and 256^3, a smooth flow of amplitude 1.5 voxels.  Legs:
  base       the plain entry point (trx_flow_warp, ...) through --parent-lib FILE, a libtrx.so built from the parent commit and loaded beside the
             new one in the same process and the same rounds - without --parent-lib, this library's own (csrc/flow.hip is the parent's);
  identity   the composed entry point at theta = I on equal lattices: the same samples as `base`;
  finer      theta = I, the moving image 2x finer per axis (8x the voxels): every gather uses less of each cache line it fetches;
  pose       equal lattices at the rigid pose of 0.2 rad about every axis.
hipEvents around `reps` calls after a warm-up of every leg; the legs alternate within a round, a line holds the median of the rounds and their
range.  bytes_per_voxel counts what the algorithm must move (warp: 12 B flow + 4 B out + 4 B of the moving image; bwd: + 4 B grad_out + 12 B dflow);
gbps and of_8tbs relate them to the time.  --out FILE appends the lines to FILE (profiles/affine_flow_bench.txt is this tool's output)."""
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

STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]
BASE = ("trx_flow_warp", "trx_flow_warp_backward", "trx_bspline_mi_workspace_bytes", "trx_bspline_mi_run")
BYTES = {"warp": 20, "bwd": 32}


def load_other(path):
    """Another libtrx.so with the product's signatures for the entry points the baselines use."""
    lib = ctypes.CDLL(path)
    for name in BASE:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def event_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def moving_image(M, dev):
    """The blob phantom on an M^3 lattice (a function of the normalised cube: the same object at every M), warped and sent through 4w(1 - w)."""
    t = blobs_gpu((M,) * 3, 1000, dev)
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev)[None], t)
    return (4.0 * w * (1.0 - w)).contiguous()


def smooth_flow(S, dev):
    z, y, x = torch.meshgrid(*[torch.linspace(-1, 1, S, device=dev)] * 3, indexing="ij")
    return torch.stack([0.6 * torch.sin(2.1 * y + 0.3), 1.5 * torch.sin(1.7 * x + 2.0 * z), 1.5 * torch.cos(1.9 * y - z)])[None].contiguous()


def bench_case(S, bins, spacing, iters, reps, rounds, parent):
    dev = torch.device("cuda")
    lib = _lib.load()
    base = parent if parent is not None else lib
    stream = _lib.current_stream(dev)
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    movs = {"same": moving_image(S, dev), "finer": moving_image(2 * S, dev)}
    flow, go = smooth_flow(S, dev), torch.rand(1, 1, S, S, S, device=dev) - 0.5
    out, dflow = torch.empty(1, 1, S, S, S, device=dev), torch.empty_like(flow)
    eye = tr._engine.pad_theta(torch.eye(3, 4, device=dev).reshape(1, -1), 3)
    pose = tr._engine.pad_theta(tr._engine.pose_to_theta(torch.tensor([[0.2, 0.2, 0.2, 0.0, 0.0, 0.0]], device=dev)), 3)
    vol = tr._engine._Batch(movs["same"], tgt, tables=False).vol()
    pairs = {k: tr._engine._GridPair(m, tgt) for k, m in movs.items()}
    args = {"identity": (pairs["same"], eye), "finer": (pairs["finer"], eye), "pose": (pairs["same"], pose)}
    # the loop: a state per leg, so that every leg optimises from the same start for as long as it runs
    rng = tr._engine.mi_range(tgt, movs["same"])
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range, cfg.mask = bins, 1.0, 0, rng.data_ptr(), None
    opt = tr._engine.opt_cfg("adam", 0.05)
    d3 = (ctypes.c_int * 3)(spacing, spacing, spacing)
    n = lib.trx_bspline_mi_workspace_bytes(3, 1, S, S, S, spacing, spacing, spacing, bins)
    assert n > 0 and base.trx_bspline_mi_workspace_bytes(3, 1, S, S, S, spacing, spacing, spacing, bins) == n
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    G = tr.bspline_grid((S,) * 3, spacing)
    keep = []

    def state():
        st = _lib.BSplineState()
        t = dict(ctrl=torch.zeros((1, 3) + G, device=dev), adam_m=torch.zeros((1, 3) + G, device=dev), adam_v=torch.zeros((1, 3) + G, device=dev),
                 flow=torch.empty_like(flow), dflow=torch.empty_like(flow), step=torch.zeros(1, dtype=torch.int32, device=dev))
        keep.append(t)
        for k, v in t.items():
            setattr(st, k, v.data_ptr())
        st.losses, st.losses_capacity, st.stopped, st.flow_last, st.base, st.bending_weight = None, 0, None, None, None, 0.0
        return st

    legs = {}
    legs["warp/base"] = lambda: _lib.check(base.trx_flow_warp(ctypes.byref(vol), _lib.ptr(flow), 1, _lib.ptr(out), stream), "trx_flow_warp")
    legs["bwd/base"] = lambda: _lib.check(base.trx_flow_warp_backward(ctypes.byref(vol), _lib.ptr(flow), 1, _lib.ptr(go), _lib.ptr(dflow), stream),
                                          "trx_flow_warp_backward")
    st0 = state()
    legs["iter/base"] = lambda: _lib.check(base.trx_bspline_mi_run(ctypes.byref(vol), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(st0), d3, iters,
                                                                   _lib.ptr(ws), n, stream), "trx_bspline_mi_run")
    for name, (pair, th) in args.items():
        v, g, st = pair.vol(), pair.grid(), state()
        keep.append((v, g, st))
        legs[f"warp/{name}"] = lambda v=v, g=g, th=th: _lib.check(lib.trx_affine_flow_warp(ctypes.byref(v), ctypes.byref(g), _lib.ptr(th), _lib.ptr(flow), 1,
                                                                                          _lib.ptr(out), stream), "trx_affine_flow_warp")
        legs[f"bwd/{name}"] = lambda v=v, g=g, th=th: _lib.check(lib.trx_affine_flow_warp_backward(ctypes.byref(v), ctypes.byref(g), _lib.ptr(th), _lib.ptr(flow), 1,
                                                                                                  _lib.ptr(go), _lib.ptr(dflow), stream),
                                                                 "trx_affine_flow_warp_backward")
        legs[f"iter/{name}"] = lambda v=v, g=g, th=th, st=st: _lib.check(lib.trx_bspline_mi_run_grids(ctypes.byref(v), ctypes.byref(g), _lib.ptr(th), ctypes.byref(cfg),
                                                                                                     ctypes.byref(opt), ctypes.byref(st), d3, iters, _lib.ptr(ws), n,
                                                                                                     stream), "trx_bspline_mi_run_grids")
    nrep = lambda k: max(1, reps // iters) if k.startswith("iter/") else reps  # noqa: E731
    per = lambda k: iters if k.startswith("iter/") else 1  # noqa: E731
    for k, fn in legs.items():                      # warm-up of every leg
        event_us(fn, 3)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, nrep(k)) / per(k))
    rows = []
    for k, v in t.items():
        op, leg = k.split("/")
        med, ref = statistics.median(v), statistics.median(t[f"{op}/base"])
        row = dict(case=f"1x{S}^3", moving=f"{2 * S if leg == 'finer' else S}^3", op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)],
                   spread=round((max(v) - min(v)) / med, 4), against_base=round(med / ref, 4), reps=nrep(k) * per(k), rounds=rounds)
        if op in BYTES:
            gbps = BYTES[op] * S ** 3 / med / 1e3
            row.update(bytes_per_voxel=BYTES[op], gbps=round(gbps, 1), of_8tbs=round(gbps / 8000.0, 4))
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_affine_flow.py needs a GPU: there is no CPU path to time")
    parent = load_other(a.parent_lib) if a.parent_lib else None
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_affine_flow.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for S in (int(v) for v in a.sizes.split(",")):
        for row in bench_case(S, a.bins, a.spacing, a.iters, a.reps, a.rounds, parent):
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
