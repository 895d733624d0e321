#!/usr/bin/env python3
"""What a moving image on a lattice of its own costs the fused mutual-information passes: microseconds per call of
trx_affine_mi_loss_grad / trx_affine_mi_loss_grad_grids (histogram pass, table, gradient pass, reduction) at a near-identity theta
  one        trx_affine_mi_loss_grad, moving on the target's lattice: the entry point of before;
  parent     the same call through --parent-lib FILE (a libtrx.so built from the parent commit, e.g. by tools/build_variant.sh or a plain `make`
             there), in the same process and the same rounds: `one` against `parent` must stay within the spread of the rounds of either;
  same       trx_affine_mi_loss_grad_grids with equal sizes and scale 1: the cross-lattice kernels doing the one-lattice work;
  finer      the moving image 2x finer per axis than the target (8x the voxels): every gather uses less of each cache line it fetches;
  coarser    the moving image 2x coarser per axis (1/8 of the voxels): neighbouring target voxels share moving voxels.
One pair, targets of 128^3 and 256^3, 32 bins.  hipEvents around `reps` calls after a warm-up of every leg; the legs alternate within a round, a
line holds the median of the rounds and their range.  --out FILE appends the lines to FILE (profiles/affine_mi_grids_bench.txt is this tool's
output)."""
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


def load_other(path):
    """Another libtrx.so with the product's signatures for the entry points it has."""
    lib = ctypes.CDLL(path)
    for name in ("trx_affine_mi_workspace_bytes", "trx_affine_mi_loss_grad"):
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


def bench_case(S, bins, reps, rounds, parent):
    dev = torch.device("cuda")
    lib = _lib.load()
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    movs = {"same": moving_image(S, dev), "finer": moving_image(2 * S, dev), "coarser": moving_image(S // 2, dev)}
    rng = tr._engine.mi_range(tgt, movs["same"])
    th = tr._engine.pad_theta(torch.tensor(NEAR, device=dev).reshape(1, -1), 3)
    vol = tr._engine._Batch(movs["same"], tgt).vol()
    n = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    loss, dth = torch.empty(1, device=dev), torch.zeros(1, 12, device=dev)
    stream = _lib.current_stream(dev)
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = bins, 1.0, 0, rng.data_ptr()

    def one(which):
        return lambda: _lib.check(which.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), n,
                                                                stream), "trx_affine_mi_loss_grad")

    def grids(mov):
        pair = tr._engine._GridPair(mov, tgt)
        v, g = pair.vol(), pair.grid()
        assert lib.trx_affine_mi_workspace_bytes(ctypes.byref(v), bins) == n      # the target lattice alone
        return lambda: _lib.check(lib.trx_affine_mi_loss_grad_grids(ctypes.byref(v), ctypes.byref(g), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth),
                                                                    _lib.ptr(ws), n, stream), "trx_affine_mi_loss_grad_grids")

    legs = {}
    if parent is not None:
        legs["parent"] = one(parent)
    legs["one"] = one(lib)
    for name, mov in movs.items():
        legs[name] = grids(mov)
    for fn in legs.values():                      # warm-up of every leg
        event_us(fn, 5)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, reps))
    out = []
    for k, v in t.items():
        med = statistics.median(v)
        M = {"finer": 2 * S, "coarser": S // 2}.get(k, S)
        out.append(dict(case=f"1x{S}^3", moving=f"{M}^3", bins=bins, leg=k, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)],
                        spread=round((max(v) - min(v)) / med, 4), against_one=round(med / statistics.median(t["one"]), 4), reps=reps, rounds=rounds))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_affine_mi_grids.py needs a GPU: there is no CPU path to time")
    parent = load_other(a.parent_lib) if a.parent_lib else None
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_affine_mi_grids.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for S in (int(v) for v in a.sizes.split(",")):
        for row in bench_case(S, a.bins, a.reps, a.rounds, parent):
            line = json.dumps(row)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
