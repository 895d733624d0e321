#!/usr/bin/env python3
"""World geometry against the voxel-size scale in the fused rigid / affine mutual-information path, on two lattices.

Per size S (1 x S^3 target @ 1 mm, a moving lattice of (7S/8, S, 9S/8) @ 1.1 x 0.95 x 0.9 mm, aligned headers, so that the record and the scale describe
the same transform and every variant samples the same positions):
  scale   trx_affine_mi_loss_grad_grids / trx_affine_mi_run_grids with the voxel-size scale, this library
  world   the same entry points with the world record (the *_world_kernel instances), this library
  parent  the scale path of a library built from the parent commit (--parent-lib; left out when not given)
timed as one fused evaluation (loss + dtheta: memset, pass 1, table, pass 2, finalise) and as one iteration of the device loop, by device events around
EVALS calls / ITERS iterations, in ROUNDS rounds that alternate the variants.  Reported: median, min and max over the rounds per variant, the spread of
the scale path (max - min over its median), and each variant's median against the scale path's.  The loop runs rigid + Adam at lr 1e-7 from a fixed
pose, so that every round of every variant does the same work.
trx_image_moments at 1 x 256^3, raw and masked: time per call and its share of the 8 TB/s roofline on 4 B/voxel (5 with a mask; every voxel counted as
read, also outside the mask).

    python tools/bench_affine_mi_world.py [--sizes 128 256] [--parent-lib PATH/libtrx.so] [--out profiles/affine_mi_world_bench.txt]
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib  # noqa: E402

EVALS, ITERS, ROUNDS = 20, 20, 9
HBM_BYTES_PER_S = 8.0e12
POSE = (0.02, -0.015, 0.01, 0.01, -0.02, 0.015)


def image(shape, seed):
    """A smooth seeded volume in [0, 1]: a few sinusoids of the normalised coordinates."""
    g = torch.Generator().manual_seed(seed)
    axes = torch.meshgrid(*[torch.linspace(-1.0, 1.0, s) for s in shape], indexing="ij")
    v = torch.zeros(shape)
    for _ in range(6):
        k, p = 1.0 + 5.0 * torch.rand(3, generator=g), 6.28 * torch.rand(1, generator=g)
        v += torch.sin(k[0] * axes[0] + k[1] * axes[1] + k[2] * axes[2] + p)
    v = (v - v.min()) / (v.max() - v.min())
    return v[None, None].contiguous()


def diagonal_header(shape, voxel):
    """Voxel-to-world matrix of an aligned lattice centred on the origin (tensor axis a along world axis nd-1-a)."""
    nd = len(shape)
    A = torch.zeros(nd + 1, nd + 1, dtype=torch.float64)
    for a in range(nd):
        A[nd - 1 - a, a], A[nd - 1 - a, nd] = voxel[a], -voxel[a] * (shape[a] - 1) / 2.0
    A[nd, nd] = 1.0
    return A


def parent_library(path):
    lib = ctypes.CDLL(path)
    for name in ("trx_affine_mi_loss_grad_grids", "trx_affine_mi_run_grids", "trx_status_string"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def timed(fn, n):
    """Milliseconds per call of fn() over n calls, by device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


class Variant:
    def __init__(self, name, solver, lib):
        self.name, self.s, self.lib = name, solver, lib
        dev = solver.batch.device
        self.theta = solver.theta.clone()
        self.loss, self.dth = torch.empty(solver.batch.B, device=dev), torch.zeros(solver.batch.B, 12, device=dev)
        self.stream = _lib.current_stream(dev)
        self.evals, self.iters = [], []

    def evaluate(self):
        s = self.s
        rc = self.lib.trx_affine_mi_loss_grad_grids(ctypes.byref(s.vol), ctypes.byref(s.grid), ctypes.byref(s.mi), _lib.ptr(self.theta), _lib.ptr(self.loss),
                                                    _lib.ptr(self.dth), _lib.ptr(s.workspace), s.ws_bytes, self.stream)
        assert rc == 0, rc

    def iterate(self):
        s = self.s
        rc = self.lib.trx_affine_mi_run_grids(ctypes.byref(s.vol), ctypes.byref(s.grid), ctypes.byref(s.mi), ctypes.byref(s.opt), ctypes.byref(s.state), ITERS,
                                              _lib.ptr(s.workspace), s.ws_bytes, self.stream)
        assert rc == 0, rc
        s.step.zero_()      # (the loss curve is overwritten from its start: capacity ITERS serves every round)


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


def bench_size(S, parent, say):
    tshape, mshape = (S, S, S), (7 * S // 8, S, 9 * S // 8)
    tvox, mvox = (1.0, 1.0, 1.0), (1.1, 0.95, 0.9)
    mov, tgt = image(mshape, 1).cuda(), image(tshape, 2).cuda()
    kw = dict(mode="rigid", mi=dict(bins=32), optimizer="adam", lr=1e-7, init=torch.tensor(POSE)[None], capacity=ITERS)
    variants = [Variant("scale", tr.AffineMISolver(mov, tgt, moving_voxel=mvox, target_voxel=tvox, **kw), _lib.load()),
                Variant("world", tr.AffineMISolver(mov, tgt, moving_affine=diagonal_header(mshape, mvox), target_affine=diagonal_header(tshape, tvox), **kw), _lib.load())]
    if parent is not None:
        variants.append(Variant("parent", tr.AffineMISolver(mov, tgt, moving_voxel=mvox, target_voxel=tvox, **kw), parent))
    for v in variants:      # warm-up: code objects, caches
        timed(v.evaluate, 3)
        v.iterate()
    torch.cuda.synchronize()
    # the variants compute the same thing: the record of aligned headers is the scale
    ref = variants[0]
    for v in variants[1:]:
        dl = (v.loss - ref.loss).abs().max().item()
        dg = (v.dth - ref.dth).abs().max().item() / ref.dth.abs().max().item()
        say(f"  {v.name} against scale at the same theta: |loss diff| {dl:.2e} (loss {ref.loss.item():.6f}), dtheta {dg:.2e} relative")
    for r in range(ROUNDS):
        for v in (variants if r % 2 == 0 else variants[::-1]):
            v.evals.append(timed(v.evaluate, EVALS) * 1e3)
            v.iters.append(timed(v.iterate, 1) / ITERS * 1e3)
    say(f"  1 x {S}^3 from {mshape}, {ROUNDS} rounds of {EVALS} evaluations / {ITERS} loop iterations, microseconds (median, min, max):")
    base_e, base_i = stats(ref.evals), stats(ref.iters)
    for v in variants:
        e, i = stats(v.evals), stats(v.iters)
        say(f"    {v.name:6s} evaluation {e[0]:9.1f} {e[1]:9.1f} {e[2]:9.1f}   ({100.0 * (e[0] / base_e[0] - 1.0):+.2f} % of scale)"
            f"   loop iteration {i[0]:9.1f} {i[1]:9.1f} {i[2]:9.1f}   ({100.0 * (i[0] / base_i[0] - 1.0):+.2f} % of scale)")
    say(f"    spread of the scale path over its rounds, (max - min) / median: evaluation {100.0 * (base_e[2] - base_e[1]) / base_e[0]:.2f} %, "
        f"loop iteration {100.0 * (base_i[2] - base_i[1]) / base_i[0]:.2f} %")


def bench_moments(S, say):
    x = image((S, S, S), 3).cuda()
    mask = (image((S, S, S), 4) > 0.5).to(torch.uint8).cuda()
    lib = _lib.load()
    n = lib.trx_image_moments_workspace_bytes(3, 1, S, S, S)
    ws, out = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(1, 4, dtype=torch.float64, device="cuda")
    off = x.reshape(1, -1).amin(1).contiguous()
    stream = _lib.current_stream(torch.device("cuda"))
    for name, mk, bytes_per_voxel in (("raw", None, 4), ("masked", mask, 5)):
        call = lambda: lib.trx_image_moments(_lib.ptr(x), _lib.ptr(mk), _lib.ptr(off), 3, 1, S, S, S, _lib.ptr(out), _lib.ptr(ws), n, stream)  # noqa: E731
        timed(call, 3)
        ts = [timed(call, EVALS) * 1e3 for _ in range(ROUNDS)]
        med, lo, hi = stats(ts)
        floor = S ** 3 * bytes_per_voxel / HBM_BYTES_PER_S * 1e6
        say(f"  trx_image_moments 1 x {S}^3 {name:6s}: {med:8.1f} us per call (min {lo:.1f}, max {hi:.1f}), two launches; {bytes_per_voxel} B/voxel at 8 TB/s = "
            f"{floor:.1f} us: {100.0 * floor / med:.1f} % of the roofline (end to end, launches included)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--parent-lib", default=None, help="libtrx.so built from the parent commit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_affine_mi_world.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"world geometry against the voxel-size scale, fused rigid / affine mutual information, two lattices - {torch.cuda.get_device_name(0)}")
    parent = parent_library(a.parent_lib) if a.parent_lib else None
    say("parent library: " + ("given" if parent is not None else "not given (the parent column is not measured)"))
    for S in a.sizes:
        bench_size(S, parent, say)
    bench_moments(256, say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
