#!/usr/bin/env python3
"""What the Euclidean distance transform, the overlap counts and the surface distances cost: microseconds per call, one pair at
128^3 and 256^3, without voxel sizes (the integer path) and with voxel (3.0, 0.7, 0.7) (fp32).
  edt        trx_distance_transform without `nearest` on four masks: a ball of half the extent (the usual organ), the ball's surface (what
             surface_distances transforms), 1 % random voxels, and a single corner voxel - the worst case of the outward search, whose cost grows with
             the distance to the nearest feature: its time next to the ball's is what decides between the search and a lower-envelope pass.
             `edt+nearest` is the ball again with the index map.  Named bytes: 1 (mask) + 4 + 4 + 4 + 4 + 4 = 21 B/voxel in 3-D (each pass reads and
             writes one 4-byte value), + 2 + 2 + 2 + 2 + 12 with `nearest`; the search's re-reads of a line are meant to hit in cache and are not named.
  overlap    trx_label_overlap at 256^3, uint8, L = 32, on two blocky label maps: 2 B/voxel.
  surface    tr.surface_distances on two offset balls: two surfaces, two transforms, the compaction and the sort - wall clock with its host syncs.
  scipy      scipy.ndimage.distance_transform_edt on this box's CPU on the same masks, if scipy imports: the outside comparison.
`share` is the named bytes over the time as a share of 8 TB/s.  hipEvents around `reps` calls after a warm-up of every leg; a line holds the median of the
rounds and their range.  --out FILE appends the lines to FILE (profiles/distance_bench.txt is this tool's output)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _lib  # noqa: E402

PEAK = 8e12      # bytes / s
VOXEL = (3.0, 0.7, 0.7)


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


def row(case, op, leg, v, nbytes=None, **extra):
    med = statistics.median(v)
    r = dict(case=case, op=op, leg=leg, us=round(med, 2), range_us=[round(min(v), 2), round(max(v), 2)], **extra)
    if nbytes:
        r.update(bytes_per_voxel=nbytes[0], share_of_8TBs=round(nbytes[0] * nbytes[1] / (med * 1e-6) / PEAK, 4))
    return r


def ball(S, dev, centre=None, radius=None):
    ax = torch.arange(S, device=dev, dtype=torch.float32)
    c = [(S - 1) / 2] * 3 if centre is None else centre
    r = S / 4 if radius is None else radius
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) <= r * r).to(torch.uint8)[None].contiguous()


def masks(S, dev):
    g = torch.Generator(device=dev).manual_seed(7)
    b = ball(S, dev)
    corner = torch.zeros((1, S, S, S), dtype=torch.uint8, device=dev)
    corner[0, 0, 0, 0] = 1
    return {"ball": b, "ball-surface": tr.mask_surface(b)[:, 0].contiguous(), "random-1%": (torch.rand((1, S, S, S), generator=g, device=dev) < 0.01).to(torch.uint8),
            "corner-voxel": corner}


def bench_edt(S, reps, rounds, with_scipy):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    n, geom = S ** 3, (3, 1, S, S, S)
    nws = lib.trx_distance_workspace_bytes(*geom)
    ws, d2 = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty((1, S, S, S), device=dev)
    idx = torch.empty((1, 3, S, S, S), dtype=torch.int32, device=dev)
    vox = (ctypes.c_float * 3)(*VOXEL)
    ms = masks(S, dev)

    def call(m, v, near):
        return lambda: _lib.check(lib.trx_distance_transform(_lib.ptr(m), *geom, v, _lib.ptr(d2), _lib.ptr(near), _lib.ptr(ws), nws, stream), "trx_distance_transform")

    rows = []
    for path, v in (("voxels", None), ("mm", vox)):
        legs = {k: call(m, v, None) for k, m in ms.items()}
        # the corner voxel costs milliseconds: fewer calls per round there
        t = timed({k: f for k, f in legs.items() if k != "corner-voxel"}, reps, rounds)
        t.update(timed({"corner-voxel": legs["corner-voxel"]}, max(1, reps // 10), rounds))
        for k in ms:
            rows.append(row(f"1x{S}^3", "edt", k, t[k], (21, n), path=path, features=int(ms[k].sum().item())))
        t = timed({"ball": call(ms["ball"], v, idx)}, reps, rounds)
        rows.append(row(f"1x{S}^3", "edt+nearest", "ball", t["ball"], (41, n), path=path))
    if with_scipy:
        try:
            from scipy import ndimage
        except ImportError:
            rows.append(dict(case=f"1x{S}^3", op="scipy", note="scipy does not import on this box: no outside comparison was available"))
        else:
            for k in ("ball", "random-1%"):      # seconds per call at 256^3: two masks are enough for the comparison
                host = (ms[k][0] == 0).cpu().numpy()
                for path, sampling in (("voxels", None), ("mm", VOXEL)):
                    t0 = time.perf_counter()
                    ndimage.distance_transform_edt(host, sampling=sampling)
                    rows.append(dict(case=f"1x{S}^3", op="scipy.ndimage.distance_transform_edt (CPU, one call)", leg=k, path=path,
                                     ms=round((time.perf_counter() - t0) * 1e3, 1)))
    return rows


def bench_overlap(S, reps, rounds):
    dev, lib = torch.device("cuda"), _lib.load()
    stream = _lib.current_stream(dev)
    g = torch.Generator(device=dev).manual_seed(5)
    coarse = torch.randint(0, 32, (1, 1, S // 16, S // 16, S // 16), generator=g, device=dev, dtype=torch.uint8)
    a = torch.nn.functional.interpolate(coarse, size=(S, S, S), mode="nearest")[:, 0].contiguous()
    b = torch.roll(a, (3, 2, 1), (1, 2, 3)).contiguous()
    counts = torch.empty((1, 32, 3), dtype=torch.int64, device=dev)
    legs = {"blocky": lambda: _lib.check(lib.trx_label_overlap(_lib.ptr(a), _lib.ptr(b), 1, 3, 1, S, S, S, 32, _lib.ptr(counts), stream), "trx_label_overlap")}
    t = timed(legs, reps, rounds)
    return [row(f"1x{S}^3", "overlap uint8 L=32", "blocky", t["blocky"], (2, S ** 3))]


def bench_surface(S, rounds):
    dev = torch.device("cuda")
    a, b = ball(S, dev), ball(S, dev, [S / 2 + 4, S / 2 - 3, S / 2 + 6], S / 4 + 2)
    tr.surface_distances(a, b, VOXEL)
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = tr.surface_distances(a, b, VOXEL)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    return [row(f"1x{S}^3", "surface_distances (wall clock, host syncs included)", "two balls", t, hausdorff=round(r.hausdorff.item(), 4),
                hd95=round(r.hd_percentile.item(), 4), assd=round(r.assd.item(), 4), surface_voxels=[r.n_a.item(), r.n_b.item()])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distance.py needs a GPU: there is no CPU path to time")
    props = torch.cuda.get_device_properties(0)
    lines = ["# tools/bench_distance.py " + " ".join(sys.argv[1:]),
             f"# box: {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}"]
    print("\n".join(lines), flush=True)
    for S in (int(v) for v in a.sizes.split(",")):
        rows = bench_edt(S, a.reps, a.rounds, not a.no_scipy)
        if S == 256:
            rows += bench_overlap(S, a.reps, a.rounds)
        rows += bench_surface(S, a.rounds)
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
