#!/usr/bin/env python3
"""What Gaussian smoothing costs: microseconds per call of trx_gaussian_resample on one volume of 256^3 and one of 120x512x512,
sigma = 1, 2 and 4 voxels on every axis at the same size (R = 4, 8, 16: three passes), and the (1, 4, 4) level of the second shape (sigma (0, 2, 2),
120x512x512 -> 120x128x128: two passes).
  trx        the kernel through the C ABI, workspace allocated once.  Named bytes: every pass reads its input once and writes its output once, 4 B each -
             8 B/voxel per same-size pass; `share` is the named bytes over the time as a share of 8 TB/s.
  torch      what a user writes today on the same box: F.pad(mode='replicate') of all three axes, then three F.conv3d calls with 1-D kernels (same size);
             for the level the same chain followed by F.interpolate(mode='trilinear') to the level's size.
`ratio` = torch / trx.  hipEvents around `reps` calls after a warm-up of every leg, legs alternating inside a round; a line holds the median of the
rounds and their range.  --phantom adds the world phantom of section 4.17 (tests/affine_mi_world_ref.py: the target at 3 x 1 x 1 mm) registered
coarse-to-fine (two levels) twice, with the halving pyramid and with shrink='voxel': the pose error of both against the phantom's truth - and a CT-like
pair of the same phantom family on which the two rules give different levels (anisotropic_phantom), three levels.  --out FILE appends the
lines to FILE (profiles/gaussian_bench.txt is this tool's output)."""
import argparse
import ctypes
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


def timed(legs, reps, rounds):
    for fn in legs.values():
        event_us(fn, 2)
    t = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            t[k].append(event_us(fn, reps))
    return t


def taps(sigma, truncate=4.0):
    R = int(truncate * sigma + 0.5)
    d = (torch.arange(2 * R + 1, dtype=torch.float64) - R) / sigma
    g = torch.exp(-0.5 * d * d)
    return R, (g / g.sum()).float().cuda()


def torch_chain(x, sigma, size=None):
    """replicate pad + three 1-D conv3d calls (+ trilinear interpolation to `size`)."""
    R = [int(4.0 * s + 0.5) for s in sigma]
    y = F.pad(x, (R[2], R[2], R[1], R[1], R[0], R[0]), mode='replicate')
    for a, s in enumerate(sigma):
        if R[a] == 0:
            continue
        shape = [1, 1, 1, 1, 1]
        shape[2 + a] = 2 * R[a] + 1
        y = F.conv3d(y, taps(s)[1].reshape(shape))
    return y if size is None else F.interpolate(y, size=size, mode='trilinear', align_corners=False)


def trx_call(x, out, sigma):
    lib = _lib.load()
    geom = (3, 1, *x.shape[2:], *out.shape[2:])
    nws = lib.trx_gaussian_workspace_bytes(*geom)
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    sig = (ctypes.c_float * 3)(*sigma)
    stream = _lib.current_stream(x.device)
    return lambda: _lib.check(lib.trx_gaussian_resample(_lib.ptr(x), _lib.ptr(out), *geom, sig, 4.0, 0, 1, _lib.ptr(ws), nws, stream), "trx_gaussian_resample")


def pass_bytes(shape, size, sigma):
    """4 B read + 4 B written per pass, in the kernel's pass order (strongest shrink first, ties the inner axis first)."""
    axes = [a for a in (2, 1, 0) if shape[a] != size[a] or int(4.0 * sigma[a] + 0.5) > 0]
    axes.sort(key=lambda a: size[a] / shape[a])
    cur, total = list(shape), 0
    for a in axes:
        n_in = cur[0] * cur[1] * cur[2]
        cur[a] = size[a]
        total += 4 * (n_in + cur[0] * cur[1] * cur[2])
    return total, len(axes)


def bench(shape, size, sigma, reps, rounds):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((1, 1) + shape, device="cuda", generator=g)
    out = torch.empty((1, 1) + size, device="cuda")
    same = size == shape
    legs = {"trx": trx_call(x, out, sigma), "torch": lambda: torch_chain(x, sigma, None if same else size)}
    legs["trx"]()
    ref = torch_chain(x, sigma, None if same else size)
    dev = (out - ref).abs().max().item()      # (the level too: smoothing at full resolution, then interpolating, is the same operator)
    t = timed(legs, reps, rounds)
    nbytes, npass = pass_bytes(shape, size, sigma)
    med = {k: statistics.median(v) for k, v in t.items()}
    case = "x".join(map(str, shape)) + ("" if same else " -> " + "x".join(map(str, size)))
    return dict(case=case, sigma=list(sigma), passes=npass, trx_us=round(med["trx"], 2), trx_range_us=[round(min(t["trx"]), 2), round(max(t["trx"]), 2)],
                named_bytes=nbytes, share_of_8TBs=round(nbytes / (med["trx"] * 1e-6) / PEAK, 4), torch_us=round(med["torch"], 2),
                torch_range_us=[round(min(t["torch"]), 2), round(max(t["torch"]), 2)], ratio_torch_over_trx=round(med["torch"] / med["trx"], 3),
                max_abs_trx_minus_torch=dev)


def phantom():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import affine_mi_grids_ref as gref
    import affine_mi_world_ref as wref
    Am, At, T = wref.world_headers()
    mov, tgt = (x.cuda() for x in wref.world_pair())
    rows = []
    # two levels: the moving lattice (26 x 22 x 18) cannot be halved twice
    for name, kw in (("levels=2, halving pyramid", {}), ("levels=2, shrink='voxel'", dict(shrink='voxel'))):
        reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6), levels=2, **kw)
        reg.optim(mov, tgt, lr=gref.WORLD_LR, max_epochs=[60, 60], moving_affine=Am, target_affine=At)
        pose = reg.final_pose[0].double().cpu().numpy()
        rows.append(dict(case="world phantom " + "x".join(map(str, gref.WORLD_TARGET[0])) + " @ " + "x".join(map(str, gref.WORLD_TARGET[1])) + " mm", run=name,
                         level_shapes=[list(s) for s in reg.level_shapes],
                         moving_factors=None if reg.level_schedule is None else [list(f) for f in reg.level_schedule[1][0]],
                         max_abs_pose_error=round(float(np.max(np.abs(pose - np.asarray(wref.WORLD_POSE)))), 5),
                         max_abs_world_matrix_error_mm=round((reg.world_matrix[0].cpu() - T).abs().max().item(), 4),
                         final_loss=round(reg.losses[0, -1].item(), 5)))
    return rows


def anisotropic_phantom():
    """The same family of phantom (tests/affine_mi_grids_ref.py::world_blobs, stretched four times: blobs of 8 - 20 mm within +-32 mm) on a pair where the
    two rules differ: an MR-like target 80x112x112 at 1.2x0.9x0.9 mm and a CT-like moving image 32x144x144 at 3.0x0.7x0.7 mm, axis-aligned headers, a
    known rigid transform between them; rigid MI, three levels from the identity."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import affine_mi_grids_ref as gref
    import affine_mi_world_ref as wref
    (ts, tv), (ms, mv) = ((80, 112, 112), (1.2, 0.9, 0.9)), ((32, 144, 144), (3.0, 0.7, 0.7))
    At, Am = wref.header(ts, tv), wref.header(ms, mv)
    T = torch.eye(4, dtype=torch.float64)
    T[:3, :3], T[:3, 3] = wref.rotation(0.10, -0.07, 0.12), torch.tensor([4.0, -3.0, 2.5], dtype=torch.float64)
    Ti = torch.linalg.inv(T)
    tgt = gref.world_blobs(wref.lattice_points(ts, At) / 4.0).clamp(max=1.0)
    w = gref.world_blobs((wref.lattice_points(ms, Am) @ Ti[:3, :3].T + Ti[:3, 3]) / 4.0).clamp(max=1.0)
    mov, tgt = (4.0 * w * (1.0 - w)).float()[None, None].cuda(), tgt.float()[None, None].cuda()
    rows = []
    for name, kw in (("levels=3, halving pyramid", {}), ("levels=3, shrink='voxel'", dict(shrink='voxel'))):
        reg = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6), levels=3, **kw)
        reg.optim(mov, tgt, lr=0.01, max_epochs=[60, 40, 20], moving_affine=Am, target_affine=At)
        M = reg.world_matrix[0].cpu()
        cos = ((M[:3, :3].T @ T[:3, :3]).trace().item() - 1.0) / 2.0
        rows.append(dict(case="CT-like phantom: moving " + "x".join(map(str, ms)) + " @ " + "x".join(map(str, mv)) + " mm, target " + "x".join(map(str, ts)) +
                         " @ " + "x".join(map(str, tv)) + " mm", run=name, level_shapes=[list(x) for x in reg.level_shapes],
                         moving_level_shapes=[[-(-n // f) for n, f in zip(ms, fs)] for fs in reg.level_schedule[1][0]] if reg.level_schedule else
                         [list(x) for x in tr.pyramid_shapes(ms, 3)],
                         rotation_error_deg=round(math.degrees(math.acos(max(-1.0, min(1.0, cos)))), 4),
                         translation_error_mm=round((M[:3, 3] - T[:3, 3]).norm().item(), 4),
                         max_abs_world_matrix_error_mm=round((M - T).abs().max().item(), 4),
                         level_final_losses=[round(c[0, -1].item(), 5) for c in reg.level_losses]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--phantom", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gaussian.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_gaussian.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    cases = [(shape, shape, (s, s, s)) for shape in ((256, 256, 256), (120, 512, 512)) for s in (1.0, 2.0, 4.0)]
    cases.append(((120, 512, 512), (120, 128, 128), (0.0, 2.0, 2.0)))
    for r in (bench(*c, a.reps, a.rounds) for c in cases):
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    for r in phantom() + anisotropic_phantom() if a.phantom else ():
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
