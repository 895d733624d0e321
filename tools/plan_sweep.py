#!/usr/bin/env python3
"""Sweep the affine step's launch plans through AffineSolver.run: a refactor of the host dispatch must launch and compute the same thing.
    python tools/plan_sweep.py LIBTRX_SO OUT.json              run the table with that library (needs the GPU)
    python tools/plan_sweep.py --compare OLD1.json OLD2.json NEW.json
    python tools/plan_sweep.py --calls OLD_kernel_stats.csv NEW_kernel_stats.csv      (rocprofv3 --kernel-trace --stats, one run of the sweep each)

The table: 2-D and 3-D; one pair of 64^3 and 128^3, 3 x 192^3, 16 x 64 x 128 x 128 and 1, 2, 6, 8 x 256^3; the identity, a small rotation about z,
a general rotation of 0.5 rad and the rigid mode at a random pose; NCC and MSE-only; 1 and 3 iterations (the plain and the carry form); one_kernel
True / False / "auto"; every path flag of the README alone.  Per case: bodies(), rows_used() and a hash of the bytes of losses, theta, best_theta.

--compare: OLD1 and OLD2 are two runs of the old library.  Where they agree byte for byte, NEW must agree with them byte for byte.  Where they
do not (the exact-footprint kernel hands out work by tickets), bodies and rows must still be equal and the losses agree to 2e-5 relative (the
bar of tests/test_gpu_eft.py); such cases are listed, and more than a tenth of the table in that class fails the comparison.  Exit status 1 on
any mismatch.  --calls: the per-kernel call counts of the two traces must be identical."""
import csv, hashlib, json, math, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(1, (64, 64, 64)), (1, (128, 128, 128)), (3, (192, 192, 192)), (16, (64, 128, 128)), (1, (256, 256, 256)), (2, (256, 256, 256)),
         (6, (256, 256, 256)), (8, (256, 256, 256))]
SIZES_2D = [(1, (64, 64)), (4, (256, 256))]
POSES = ("identity", "rot_z_small", "rot_0.5", "rigid_random")
FLAGS = ("GATHER_PATH", "SINGLE_GEOM", "TWO_PASS_FLOW", "DEEP_TILE", "NO_ROT_DEEP_TILE", "NO_ZSTREAM", "ZSTREAM", "NO_EFT", "EFT", "ZS_FUSED", "ONE_KERNEL",
         "NO_CARRY", "NO_ZS_FLAT", "WALK_DOWN", "NO_PINGPONG")


def table():
    """(ndim, B, shape, pose, loss, iters, one_kernel, flag name)"""
    t = []
    for B, shape in SIZES:
        for pose in POSES:
            for loss in ("ncc", "mse"):
                for iters in (1, 3):
                    t.append((3, B, shape, pose, loss, iters, "auto", None))
        for pose in ("identity", "rot_0.5"):
            for iters in (1, 3):
                for ok in (True, False):
                    t.append((3, B, shape, pose, "ncc", iters, ok, None))
    for B, shape in (SIZES[0], SIZES[2], SIZES[3], SIZES[5], SIZES[7]):
        for flag in FLAGS:
            for pose, loss in (("rot_z_small", "ncc"), ("rigid_random", "ncc"), ("identity", "mse")):
                t.append((3, B, shape, pose, loss, 3, "auto", flag))
    for B, shape in SIZES_2D:
        for pose in POSES:
            for loss in ("ncc", "mse"):
                for iters in (1, 3):
                    t.append((2, B, shape, pose, loss, iters, "auto", None))
    return t


def case_name(c):
    nd, B, shape, pose, loss, iters, ok, flag = c
    return f"{nd}d {B}x{'x'.join(map(str, shape))} {pose} {loss} it{iters} one_kernel={ok} flag={flag}"


def run(lib_path, out_path):
    import torch
    from torchregister_amd import _lib
    _lib.LIB_PATH = os.path.abspath(lib_path)
    import torchregister_amd as tr
    from bench import blobs_gpu, rot
    dev = torch.device("cuda")
    vols = {}

    def volumes(nd, B, shape):
        if (nd, B, shape) not in vols:
            vols.clear()   # (one size at a time on the device; the table is ordered by size)
            s3 = shape if nd == 3 else (8,) + shape
            tgt = torch.cat([blobs_gpu(s3, 7000 + b, dev) for b in range(B)])
            if nd == 2:
                tgt = tgt[:, :, 4].contiguous()
            mov = 0.9 * tgt.roll(shifts=(2, -3), dims=(-2, -1)) + 0.1 * tgt.flip(-1)
            vols[(nd, B, shape)] = (mov, tgt)
        return vols[(nd, B, shape)]

    def init(nd, B, pose):
        g = torch.Generator().manual_seed(11)
        if pose == "rigid_random":
            return "rigid", torch.rand(B, 6 if nd == 3 else 3, generator=g)   # (the reference draws its initial pose uniformly in [0, 1))
        if nd == 2:
            a = {"identity": 0.0, "rot_z_small": 0.02, "rot_0.5": 0.5}[pose]
            th = torch.tensor([[math.cos(a), -math.sin(a), 0.01], [math.sin(a), math.cos(a), -0.01]])
        else:
            r = {"identity": torch.eye(3), "rot_z_small": rot(0.0, 0.0, 0.02).float(), "rot_0.5": rot(0.3, 0.3, 0.3).float()}[pose]   # (|rotation vector| of the last ~ 0.5 rad)
            th = torch.cat([r, torch.tensor([[0.0], [0.0], [0.0]]) if pose == "identity" else torch.tensor([[0.01], [-0.02], [0.015]])], dim=1)
        th = th[None].repeat(B, 1, 1)
        if pose != "identity":
            th = th + 1e-3 * torch.rand(th.shape, generator=g)   # (the pairs differ)
        return "affine", th

    results = {}
    for c in table():
        nd, B, shape, pose, loss, iters, ok, flag = c
        mov, tgt = volumes(nd, B, shape)
        mode, th = init(nd, B, pose)
        spec = tr.LossSpec(w_ncc=1.0) if loss == "ncc" else tr.LossSpec(w_mse=1.0)
        s = tr.AffineSolver(mov, tgt, mode=mode, loss=spec, optimizer="adam", lr=1e-3, init=th, capacity=iters,
                            flags=getattr(_lib, "FLAG_" + flag) if flag else 0, one_kernel=ok)
        s.run(iters)
        torch.cuda.synchronize()
        h = hashlib.sha1()
        for t in (s.losses, s.theta, s.best_theta):
            h.update(t.cpu().numpy().tobytes())
        r = {"bodies": s.bodies() if nd == 3 else [], "rows": s.rows_used().tolist() if nd == 3 else [], "hash": h.hexdigest()[:16],
             "losses": s.losses.cpu().double().tolist()}
        results[case_name(c)] = r
        print(f"{case_name(c)} | {','.join(r['bodies'])} | {r['rows']} | {r['hash']}", flush=True)
        del s
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(results, f)
    print(f"{len(results)} cases -> {out_path}")


def compare(old1, old2, new):
    a, b, n = (json.load(open(p)) for p in (old1, old2, new))
    bad, loose = [], []
    if not (a.keys() == b.keys() == n.keys()):
        print("the three runs hold different case lists")
        return 1
    for k in a:
        if a[k]["hash"] == b[k]["hash"] and (a[k]["bodies"], a[k]["rows"]) == (b[k]["bodies"], b[k]["rows"]):
            if (n[k]["hash"], n[k]["bodies"], n[k]["rows"]) != (a[k]["hash"], a[k]["bodies"], a[k]["rows"]):
                bad.append(k)
            continue
        loose.append(k)
        gap = max(abs(x - y) / max(1.0, abs(y)) for ra, rn in zip(a[k]["losses"], n[k]["losses"]) for x, y in zip(rn, ra))
        if (n[k]["bodies"], n[k]["rows"]) != (a[k]["bodies"], a[k]["rows"]) or not gap <= 2e-5:
            bad.append(k)
        print(f"not reproducible by the old library: {k} (new against old losses: {gap:.2e} relative)")
    for k in bad:
        print(f"MISMATCH {k}: old {a[k]['bodies']} {a[k]['rows']} {a[k]['hash']} new {n[k]['bodies']} {n[k]['rows']} {n[k]['hash']}")
    print(f"{len(a)} cases, {len(a) - len(loose)} reproducible and compared byte for byte, {len(loose)} compared to tolerance, {len(bad)} mismatches")
    if len(loose) * 10 > len(a):
        print("more than a tenth of the table is not reproducible by the old library: pick other cases")
        return 1
    return 1 if bad else 0


def calls(old_csv, new_csv):
    def read(p):
        return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(open(p))}
    a, b = read(old_csv), read(new_csv)
    diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in diff:
        print(f"CALLS DIFFER {k}: {a.get(k)} -> {b.get(k)}")
    print(f"{len(a)} kernels, {sum(a.values())} calls in the old trace; {len(b)} kernels, {sum(b.values())} calls in the new; {len(diff)} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:]))
    if len(sys.argv) == 4 and sys.argv[1] == "--calls":
        sys.exit(calls(*sys.argv[2:]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    run(sys.argv[1], sys.argv[2])
