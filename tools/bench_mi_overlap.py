#!/usr/bin/env python3
"""What the overlap rule costs (trx_moving_grid.overlap / .mask): microseconds per
  fused   one evaluation of trx_affine_mi_loss_grad_grids with dtheta (memset, pass 1, table, pass 2, reduction: an iteration of the fused loop
          without its one-block update kernel)
  iter    one iteration of trx_bspline_mi_run_grids (32 bins, spacing 8, Adam; `--iters` iterations per call)
one pair, equal lattices of 128^3 and 256^3, at two poses (`near`: a near-identity matrix; `pose`: 0.2 rad about every axis), each zoomed by 0.6 so
that every sample lies inside the moving image (`full`) and, with a z translation on top, so that about 60 % do (`part`).  Legs:
  off/parent   the rule off through --parent-lib FILE, a libtrx.so built from the parent commit and loaded beside the new one in the same process
               and the same rounds (the parent reads the struct's first 60 bytes: the members it knows) - without --parent-lib the leg is left out;
  off          the rule off in this library: the same kernels (tools/isa_compare.py: identical code), so `against_parent` must lie inside the
               rounds' own spread;
  on           the rule on;
  on+mask      the rule on with an all-ones moving mask: the same valid set, plus the byte gathered at rint(i) per sample inside the image.
hipEvents around `reps` calls after a warm-up of every leg; the legs alternate within a round, a line holds the median of the rounds and their
range; `valid` is the share of counted samples read back from the counts of one evaluation.  --out FILE appends the lines to FILE
(profiles/mi_overlap_bench.txt is this tool's output)."""
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

NEAR = [[1.01, 0.013, -0.007, 0.011], [-0.009, 0.99, 0.012, -0.013], [0.006, -0.011, 1.008, 0.009]]
STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]
BASE = ("trx_affine_mi_workspace_bytes", "trx_affine_mi_loss_grad_grids", "trx_bspline_mi_workspace_bytes", "trx_bspline_mi_run_grids")
ZOOM, SHIFT = 0.6, 0.88      # every sample inside the moving image; with the z translation about 60 % of them


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


def thetas(dev):
    """{(pose, overlap): theta [1, PSTRIDE]}"""
    rot = tr._engine.pose_to_theta(torch.tensor([[0.2, 0.2, 0.2, 0.0, 0.0, 0.0]])).reshape(3, 4)
    out = {}
    for pose, m in (("near", torch.tensor(NEAR)), ("pose", rot)):
        for cover, shift in (("full", 0.0), ("part", SHIFT)):
            th = m.clone().float()
            th[:, :3] *= ZOOM
            th[2, 3] += shift
            out[(pose, cover)] = tr._engine.pad_theta(th.reshape(1, -1).to(dev), 3)
    return out


def bench_case(S, bins, spacing, iters, reps, rounds, parent):
    dev = torch.device("cuda")
    lib = _lib.load()
    stream = _lib.current_stream(dev)
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev)[None], tgt)
    mov = (1.0 + 4.0 * w * (1.0 - w)).contiguous()      # background 1: the padding value 0 is no intensity of the image
    ones = torch.ones(1, 1, S, S, S, dtype=torch.uint8, device=dev)
    pair = tr._engine._GridPair(mov, tgt)
    vol = pair.vol()
    grids = {"off": pair.grid(), "on": pair.grid(True), "on+mask": pair.grid(True, ones)}
    rng = {False: tr._engine.mi_range(tgt, mov), True: tr._engine.mi_range(tgt, mov, overlap=True)}
    cfgs = {k: tr._engine._mi_cfg_c(bins, 1.0, False, r, None) for k, r in rng.items()}
    n_f = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws_f = torch.empty(n_f, dtype=torch.uint8, device=dev)
    loss, dth = torch.empty(1, device=dev), torch.zeros(1, 12, device=dev)
    d3 = (ctypes.c_int * 3)(spacing, spacing, spacing)
    n_b = lib.trx_bspline_mi_grids_workspace_bytes(3, 1, S, S, S, spacing, spacing, spacing, bins, ctypes.byref(grids["on"]))
    assert n_f > 0 and n_b >= lib.trx_bspline_mi_workspace_bytes(3, 1, S, S, S, spacing, spacing, spacing, bins) > 0
    ws_b = torch.empty(n_b, dtype=torch.uint8, device=dev)
    opt = tr._engine.opt_cfg("adam", 0.05)
    G = tr.bspline_grid((S,) * 3, spacing)
    keep = []

    def state():
        st = _lib.BSplineState()
        t = dict(ctrl=torch.zeros((1, 3) + G, device=dev), adam_m=torch.zeros((1, 3) + G, device=dev), adam_v=torch.zeros((1, 3) + G, device=dev),
                 flow=torch.empty(1, 3, S, S, S, device=dev), dflow=torch.empty(1, 3, S, S, S, device=dev), step=torch.zeros(1, dtype=torch.int32, device=dev))
        keep.append(t)
        for k, v in t.items():
            setattr(st, k, v.data_ptr())
        st.losses, st.losses_capacity, st.stopped, st.flow_last, st.base, st.bending_weight = None, 0, None, None, None, 0.0
        return st

    rows = []
    for (pose, cover), th in thetas(dev).items():
        legs = {}
        for leg, which, g, on in ([("off/parent", parent, grids["off"], False)] if parent is not None else []) + \
                [("off", lib, grids["off"], False), ("on", lib, grids["on"], True), ("on+mask", lib, grids["on+mask"], True)]:
            cfg, st = cfgs[on], state()
            keep.append((cfg, st, g))
            legs[f"fused/{leg}"] = lambda which=which, g=g, cfg=cfg: _lib.check(which.trx_affine_mi_loss_grad_grids(
                ctypes.byref(vol), ctypes.byref(g), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws_f), n_f, stream), "trx_affine_mi_loss_grad_grids")
            legs[f"iter/{leg}"] = lambda which=which, g=g, cfg=cfg, st=st: _lib.check(which.trx_bspline_mi_run_grids(
                ctypes.byref(vol), ctypes.byref(g), _lib.ptr(th), ctypes.byref(cfg), ctypes.byref(opt), ctypes.byref(st), d3, iters, _lib.ptr(ws_b), n_b, stream),
                "trx_bspline_mi_run_grids")
        legs["fused/on"]()
        torch.cuda.synchronize()
        valid = ws_f[: bins * bins * 8].view(torch.int64).sum().item() / 2.0 ** 31 / S ** 3
        nrep = lambda k: max(1, reps // iters) if k.startswith("iter/") else reps  # noqa: E731
        per = lambda k: iters if k.startswith("iter/") else 1  # noqa: E731
        for k, fn in legs.items():                      # warm-up of every leg
            event_us(fn, 3)
        t = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                t[k].append(event_us(fn, nrep(k)) / per(k))
        for k, v in t.items():
            op, leg = k.split("/", 1)
            med, off = statistics.median(v), statistics.median(t[f"{op}/off"])
            row = dict(case=f"1x{S}^3", pose=pose, cover=cover, valid=round(valid, 4), op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)],
                       spread=round((max(v) - min(v)) / med, 4), against_off=round(med / off, 4), reps=nrep(k) * per(k), rounds=rounds)
            if parent is not None and leg == "off":
                row.update(against_parent=round(med / statistics.median(t[f"{op}/off/parent"]), 4))
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--spacing", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mi_overlap.py needs a GPU: there is no CPU path to time")
    parent = load_other(a.parent_lib) if a.parent_lib else None
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_mi_overlap.py " + " ".join(sys.argv[1:]),
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
