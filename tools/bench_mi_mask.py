#!/usr/bin/env python3
"""What the region-of-interest mask of the mutual information (trx_mi_cfg.mask) costs and saves: microseconds per call of trx_mi_loss_grad (histogram,
table, gradient of a warped volume) and of trx_affine_mi_loss_grad (the same with the affine warp fused into both passes, at a near-identity theta)
  none       mask = NULL: the unmasked instances of the kernels;
  ones       an all-ones mask: the price of the extra byte stream (the passes read 9 instead of 8 B/voxel);
  ellipsoid  a centred ellipsoid over about half the volume: the fused passes skip the gather of a voxel outside it, the warped-volume passes
             still read t and w;
and, with --parent-lib FILE (a libtrx.so built from the parent commit, e.g. by tools/build_variant.sh or a plain `make` there), the unmasked calls
through that library too, in the same process and the same rounds: `none` against `parent` must stay within the spread of the rounds.
One pair at 128^3 and 256^3, 32 bins.  hipEvents around `reps` calls after a warm-up of every leg; the legs alternate within a round, a line holds
the median of the rounds and their range.  --out FILE appends the lines to FILE (profiles/mi_mask_bench.txt is this tool's output)."""
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

HBM = 8.0e12
NEAR = [[1.01, 0.013, -0.007, 0.011], [-0.009, 0.99, 0.012, -0.013], [0.006, -0.011, 1.008, 0.009]]
STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]


def load_other(path):
    """Another libtrx.so with the product's signatures (a library from before the mask reads the first four fields of trx_mi_cfg only)."""
    lib = ctypes.CDLL(path)
    for name in ("trx_mi_workspace_bytes", "trx_mi_loss_grad", "trx_affine_mi_workspace_bytes", "trx_affine_mi_loss_grad"):
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


def ellipsoid(S, dev, fraction=0.5):
    """uint8 [1,1,S,S,S]: the centred ball of normalised radius r with (4/3) pi r^3 / 8 = fraction."""
    r = (fraction * 6.0 / 3.141592653589793) ** (1.0 / 3.0)
    x = ((2.0 * torch.arange(S, device=dev) + 1.0) / S - 1.0) ** 2
    return ((x[:, None, None] + x[None, :, None] + x[None, None, :]) <= r * r).to(torch.uint8).reshape(1, 1, S, S, S).contiguous()


def bench_case(S, bins, reps, rounds, parent):
    dev = torch.device("cuda")
    lib = _lib.load()
    tgt = blobs_gpu((S,) * 3, 1000, dev)
    w = tr._engine.affine_warp(torch.tensor(STAR, device=dev)[None], tgt)
    mov = (4.0 * w * (1.0 - w)).contiguous()
    del w
    rng = tr._engine.mi_range(tgt, mov)
    masks = {"none": None, "ones": torch.ones(1, 1, S, S, S, dtype=torch.uint8, device=dev), "ellipsoid": ellipsoid(S, dev)}
    vol = tr._engine._Batch(mov, tgt).vol()
    th = tr._engine.pad_theta(torch.tensor(NEAR, device=dev).reshape(1, -1), 3)
    n_mi, n_ami = lib.trx_mi_workspace_bytes(3, 1, S, S, S, bins), lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), bins)
    ws_mi, ws_ami = torch.empty(n_mi, dtype=torch.uint8, device=dev), torch.empty(n_ami, dtype=torch.uint8, device=dev)
    loss, grad, dth = torch.empty(1, device=dev), torch.empty_like(mov), torch.zeros(1, 12, device=dev)
    stream = _lib.current_stream(dev)

    def cfg_of(mask):
        c = _lib.MICfg()
        c.bins, c.alpha, c.normalized, c.range = bins, 1.0, 0, rng.data_ptr()
        c.mask = None if mask is None else mask.data_ptr()
        return c

    def legs_of(which, name, mask):
        c = cfg_of(mask)
        return {
            f"mi_loss_grad/{name}": lambda: _lib.check(which.trx_mi_loss_grad(_lib.ptr(tgt), _lib.ptr(mov), 3, 1, S, S, S, ctypes.byref(c), _lib.ptr(loss), _lib.ptr(grad),
                                                                              _lib.ptr(ws_mi), n_mi, stream), "trx_mi_loss_grad"),
            f"affine_mi_loss_grad/{name}": lambda: _lib.check(which.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(c), _lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth),
                                                                                            _lib.ptr(ws_ami), n_ami, stream), "trx_affine_mi_loss_grad"),
        }

    legs = {}
    if parent is not None:
        legs.update(legs_of(parent, "parent", None))
    for name, mask in masks.items():
        legs.update(legs_of(lib, name, mask))
    for fn in legs.values():                      # warm-up of every leg
        event_us(fn, 5)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, reps))
    nvox = S ** 3
    inside = {"none": 1.0, "parent": 1.0, "ones": 1.0, "ellipsoid": masks["ellipsoid"].float().mean().item()}
    out = []
    for k, v in t.items():
        entry, name = k.split("/")
        med = statistics.median(v)
        # bytes a call must move: t and w (or t and the gathered moving voxels) twice, the mask twice, the gradient once (warped-volume form)
        if entry == "mi_loss_grad":
            nbytes = nvox * (8 + 12 + (0 if name in ("none", "parent") else 2))
        else:
            nbytes = nvox * (16 * inside[name] + (0 if name in ("none", "parent") else 2))
        out.append(dict(case=f"1x{S}^3", bins=bins, entry=entry, mask=name, inside=round(inside[name], 4), us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)],
                        spread=round((max(v) - min(v)) / med, 4), reps=reps, rounds=rounds, share_of_8TBps=round(nbytes / (med * 1e-6) / HBM, 3)))
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
        raise SystemExit("bench_mi_mask.py needs a GPU: there is no CPU path to time")
    parent = load_other(a.parent_lib) if a.parent_lib else None
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_mi_mask.py " + " ".join(sys.argv[1:]),
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
