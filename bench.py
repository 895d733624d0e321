#!/usr/bin/env python3
"""Headline benchmark: registration iterations/sec (3-D 256^3 fp32, affine + NCC) on MI355X.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]   # N = 1
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up the batch, settles the clocks, warms up, times the K steps and prints one JSON line.  `--full` adds
every secondary measurement of the line (config.value_cold, the other optimiser, the legs at other poses, the flow loop,
the converging run, the roofline objects, cfg2 / lncc_loop and cpu_baseline).  `--dump-outputs DIR` writes what the timed
solver holds after its last step (theta, best theta / loss / index, the loss curve, the last gradient) as DIR/<name>.npy;
the inputs are seeded, so two builds run with the same arguments can be compared array for array.

Workload (BASELINE.json configs[3], the configuration the metric is quoted on): every GPU owns
8 independent (moving, target) pairs of 256^3 fp32 volumes (1 GiB resident in HBM), affine mode,
NCC loss (alpha = 100), Adam on theta (north_star; `--optimizer sgd` = the reference's own loop, whose rate is
also reported as config.sgd_value).  One STEP = one optimiser iteration for
all 8 pairs of a rank: fused warp + NCC + analytic backward (one HIP kernel) + finalise/optimiser
kernel; nothing is skipped and there is no host sync inside the timed region.  Pairs are independent,
so N GPUs shard with no collective ("weak" scaling: 8 pairs per GPU at every N).
value = N * 8 * K / max-over-ranks(elapsed)  [pair-iterations / s].
`--scaling strong [--pairs-total 64]` fixes the TOTAL number of pairs instead (64 pairs over G GPUs, 64 / G each - the
shard of rank r is sharding.pair_range(r, G, 64)); value = pairs_total * K / max-over-ranks(elapsed), "scaling": "strong".

Extra objects in the JSON line (--full, rank 0, N = 1 only):
  roofline     - dominant kernel (the fused F1 pass) timed in isolation with events on the launch
                 stream; achieved = 8 B/voxel * 256^3 * 8 pairs / avg kernel time; peak 8.0 TB/s.
  cpu_baseline - the oracle's torch-CPU composition of the reference's loop (kind "port": the
                 reference itself cannot travel), bounded sample at 256^3 on the host cores.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PAIRS_PER_GPU = 8
SIZE = 256
HBM_PEAK = 8.0e12          # MI355X spec sheet
ALG_BYTES_PER_VOXEL = 8    # read moving (4) + target (4) once per pair-iteration
THETA_STAR = [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]


def theta_star_inv():
    """moving = warp(theta*, target), so a registration of (moving -> target) converges to the INVERSE map of theta*:
    x -> A^-1 x - A^-1 t in affine_grid's normalised coordinates (cubic volumes: no aspect factors)."""
    t = torch.tensor(THETA_STAR, dtype=torch.float64)
    ai = torch.linalg.inv(t[:, :3])
    return torch.cat([ai, -(ai @ t[:, 3:])], dim=1).float()


def blobs_gpu(shape, seed, device):
    """Same phantom as tests/phantoms.blobs (6 Gaussian blobs on a [-1,1]^3 lattice), built on the GPU in fp32."""
    g = torch.Generator().manual_seed(int(seed))
    axes = [torch.linspace(-1, 1, s, device=device) for s in shape]
    img = torch.zeros(shape, device=device)
    for _ in range(6):
        c = torch.rand(3, generator=g) - 0.5
        sig = 0.05 + 0.2 * torch.rand(1, generator=g)
        a = torch.rand(1, generator=g)
        r2 = ((axes[0] - float(c[0])) ** 2)[:, None, None] + ((axes[1] - float(c[1])) ** 2)[None, :, None] + ((axes[2] - float(c[2])) ** 2)[None, None, :]
        img += float(a) * torch.exp(-r2 / (2 * float(sig) ** 2))
    return img.view(1, 1, *shape)


def make_batch(rank, device, size=SIZE, pairs=PAIRS_PER_GPU, pair_ids=None):
    import torchregister_amd as tr
    shape = (size,) * 3
    from torchregister_amd.sharding import weak_pair_ids
    ids = list(pair_ids) if pair_ids is not None else weak_pair_ids(rank, pairs)
    pairs = len(ids)
    tgt = torch.cat([blobs_gpu(shape, 1000 + pid, device) for pid in ids])
    th = torch.tensor(THETA_STAR, device=device)[None].expand(pairs, 3, 4).contiguous()
    mov = tr.get_affine_warp(th, tgt)
    return mov, tgt


def rot(ax, ay, az):
    import math
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = torch.tensor([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return rz @ ry @ rx


def pose_rot(device, pairs=PAIRS_PER_GPU):
    """config.value_rot: theta = R(0.5, 0.4, 0.3) diag(1.05, 0.95, 1.02) | (0.01, -0.02, 0.015), for every pair."""
    th = torch.cat([rot(0.5, 0.4, 0.3).float() @ torch.diag(torch.tensor([1.05, 0.95, 1.02])), torch.tensor([[0.01], [-0.02], [0.015]])], dim=1)
    return th.to(device)[None].expand(pairs, 3, 4).contiguous()


def pose_rigid_randinit(device, pairs=PAIRS_PER_GPU):
    """config.value_rigid_randinit: the reference's initial rigid pose, torch.manual_seed(0); torch.rand(6) (ref:utils.py:316-321)."""
    torch.manual_seed(0)
    return torch.rand(6)[None].expand(pairs, 6).contiguous().to(device)


def _cpu_loop(budget_s, max_iters):
    """Reference loop re-composed from torch CPU ops (oracle/compose.py) on ONE 256^3 pair; returns (iterations, seconds)."""
    from oracle import compose
    torch.manual_seed(0)
    shape = (SIZE,) * 3
    tgt = blobs_gpu(shape, 1000, "cpu")
    mov = compose.affine_warp(torch.tensor(THETA_STAR)[None], tgt)
    th = torch.eye(3, 4)[None].clone().requires_grad_()
    opt = torch.optim.SGD([th], 1e-6)

    def it():
        opt.zero_grad()
        e = compose.ncc_loss(tgt, compose.affine_warp(th, mov))
        e.backward()
        opt.step()
        return e.item()

    it()  # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        it()
        n += 1
        el = time.perf_counter() - t0
        if el >= budget_s or n >= max_iters:
            break
    return n, el


def host_cpus():
    """CPUs this process may use: OMP_NUM_THREADS where the host sets one (a share of a large shared machine, which
    os.cpu_count() does not show), else the affinity mask."""
    n = os.environ.get("OMP_NUM_THREADS", "")
    return int(n) if n.isdigit() and int(n) > 0 else len(os.sched_getaffinity(0))


def cpu_baseline(budget_s=10.0):
    """Two bounded samples on the host cores, the better one is reported: (a) one pair with all threads (ATen's sampler
    does not thread over a single volume, so this mostly measures the element-wise ops), (b) one pair per process,
    P processes x T threads side by side - the fair many-core number for a batch of independent pairs."""
    import subprocess
    ncpu = host_cpus()
    n1, el1 = _cpu_loop(budget_s, 64)
    single = n1 / el1
    threads1 = torch.get_num_threads()
    procs = max(1, min(8, ncpu // 8))   # (at most 8 workers: each one loads the GPU runtime with torch)
    tper = max(1, ncpu // procs)
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", str(tper)]
    ps = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for _ in range(procs)]
    res = []
    for q in ps:
        out, _ = q.communicate()
        try:
            n, el = out.strip().split()[-2:]
            res.append((int(n), float(el)))
        except Exception:
            pass
    batch = sum(n for n, _ in res) / max(el for _, el in res) if res else 0.0
    best, cores = (batch, len(res) * tper) if batch > single else (single, threads1)
    return {"value": best, "unit": "pair-iterations/s", "cores": cores, "kind": "port",
            "sample": f"affine+NCC+SGD at 256^3, torch {torch.__version__} CPU ops (oracle/compose.py), {ncpu} logical CPUs: "
                      f"(a) {n1} iterations of one pair on {threads1} threads = {single:.3f} it/s; "
                      f"(b) {len(res)} processes x {tper} threads, one pair each, {sum(n for n, _ in res)} iterations = {batch:.3f} it/s"}


def cpu_worker(threads):
    torch.set_num_threads(threads)
    n, el = _cpu_loop(6.0, 3)
    print(n, el, flush=True)


def dump_outputs(solver, out_dir, suffix=""):
    """--dump-outputs: what a caller of the timed solver receives after its last step, one .npy per array (a few KB in all):
    theta [B,3,4], best_theta [B,3,4], best_loss [B], best_idx [B] (float64), losses [B, warm-up + timed steps], grad [B,12]
    (the last step's gradient of the loss with respect to theta)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"theta": solver.current_theta, "best_theta": solver.best, "best_loss": solver.best_loss, "best_idx": solver.best_idx.double(),
              "losses": solver.losses[:, :solver.enqueued], "grad": solver.grad[:, :12]}
    for name, t in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), t.detach().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=SIZE, help=argparse.SUPPRESS)
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: 8 pairs per GPU at every N (default, what the driver runs); strong: --pairs-total pairs split over the N GPUs")
    ap.add_argument("--pairs-total", type=int, default=64, help="strong scaling: the total number of pairs (BASELINE configs[3]: 64)")
    ap.add_argument("--full", action="store_true",
                    help="also run every secondary measurement (value_cold, the other optimiser, the pose / flow / converging-run legs, "
                         "the roofline objects, cfg2 / lncc_loop, cpu_baseline); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed solver holds after its last step as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the cpu_baseline leg")
    ap.add_argument("--no-pose-legs", action="store_true",
                    help="--full without the config.value_* / flow_value legs (profiling runs: every launch of the step kernel is then a headline-pose launch)")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "sgd"],
                    help="optimiser on theta for the headline number (north_star: Adam; the reference's own loop: SGD)")
    ap.add_argument("--cpu-worker", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--backend", default="nccl", help=argparse.SUPPRESS)           # tests: gloo
    ap.add_argument("--single-device", action="store_true", help=argparse.SUPPRESS)  # tests: every rank on cuda:0
    args = ap.parse_args()
    if args.cpu_worker:
        return cpu_worker(args.cpu_worker)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch multi-GPU runs with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N")
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    if args.single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    if world > 1 or "TORCHELASTIC_RUN_ID" in os.environ:   # under torchrun the RCCL path is exercised even with one rank
        import torch.distributed as dist
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(args.backend)

    import torchregister_amd as tr
    from torchregister_amd.sharding import pair_range
    if args.scaling == "strong":
        lo, hi = pair_range(rank, world, args.pairs_total)
        assert hi > lo, f"--pairs-total {args.pairs_total} leaves rank {rank} of {world} without a pair"
        mov, tgt = make_batch(rank, device, args.size, pair_ids=range(lo, hi))
        job_pairs = args.pairs_total
    else:
        mov, tgt = make_batch(rank, device, args.size)
        job_pairs = world * PAIRS_PER_GPU
    my_pairs = mov.shape[0]
    lr = {"adam": 1e-4, "sgd": 1e-6}

    def new_solver(optimizer):
        return tr.AffineSolver(mov, tgt, mode="affine", loss=tr.LossSpec(w_ncc=1.0), optimizer=optimizer, lr=lr[optimizer],
                               capacity=max(args.steps + args.warmup, 128))

    # Power management: after an idle gap the first ~10 launches run at boost clocks, the next ~50 are throttled by the
    # power-cap overshoot (F1 kernel 0.40-0.43 ms instead of 0.31), then the clock settles (profiles/r01e kernel trace).
    # A registration runs hundreds of iterations, so the steady state is the representative rate: settle the clocks with
    # PRECONDITION untimed iterations on a scratch solver before the W warm-up steps of the measured solver.
    PRECONDITION = 100

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # value_cold: what a registration that starts on an idle GPU gets - no preconditioning, no warm-up, the first `steps`
    # iterations after 2 s of idleness (boost clocks for ~10 launches, then the power-cap transient, then the settled clock).
    # A plain run makes the same iterations without the idle gap and reports nothing of them: they are part of the clock settling
    # in front of the headline (without them the headline measured 0.3-0.6 % lower, alternating runs on one box).
    cold = new_solver(args.optimizer)
    if args.full:
        fence()
        time.sleep(2.0)
    fence()
    t0 = time.perf_counter()
    cold.run(args.steps)
    fence()
    elapsed_cold = time.perf_counter() - t0
    del cold

    scratch = new_solver(args.optimizer)
    scratch.run(PRECONDITION)
    del scratch

    solver = new_solver(args.optimizer)
    solver.run(args.warmup)

    fence()
    t0 = time.perf_counter()
    solver.run(args.steps)
    fence()
    elapsed = time.perf_counter() - t0
    from torchregister_amd.sharding import max_over_ranks
    elapsed = max_over_ranks(elapsed, device)
    losses = solver.losses[:, : args.steps + args.warmup]
    assert torch.isfinite(losses).all(), "non-finite loss in the benchmark run"
    assert (losses[:, -1] < losses[:, 0]).all(), "the optimiser made no progress"
    if args.dump_outputs:
        dump_outputs(solver, args.dump_outputs, f"_rank{rank}" if world > 1 else "")

    # the other optimiser on the same workload (only theta's 12-float update differs), timed the same way: same
    # preconditioning, same warm-up (round 1 timed it inside the post-idle power transient: -20 %)
    other = "sgd" if args.optimizer == "adam" else "adam"
    if args.full:
        elapsed_cold = max_over_ranks(elapsed_cold, device)
        scratch = new_solver(other)
        scratch.run(PRECONDITION)
        del scratch
        solver2 = new_solver(other)
        solver2.run(args.warmup)
        fence()
        t0 = time.perf_counter()
        solver2.run(args.steps)
        fence()
        elapsed2 = max_over_ranks(time.perf_counter() - t0, device)

    # ---- poses away from the identity (rank-local, same 8 x 256^3 batch): the headline starts at theta = I, where
    # every affine run starts; a run that converges to theta* ends 0.05-0.1 away from it and a rigid run starts at a random pose.
    def timed_run(sv, steps):
        sv.run(40)
        fence()
        t = time.perf_counter()
        sv.run(steps)
        fence()
        return time.perf_counter() - t

    pose_steps = min(args.steps, 100)
    legs = args.full and not args.no_pose_legs
    extra = {"value_theta_star": None, "value_rot": None, "value_rigid_randinit": None, "flow_value": None, "value_run": None, "run_loss_ratio_worst": None,
             "run_loss_first_last": None, "run_theta_err_worst": None, "body_histogram": None, "value_theta_star_inv": None}
    # (a) theta* (the map the synthetic moving volumes were made with) and its inverse - the pose a run of this batch CONVERGES to;
    # (b) R(0.5, 0.4, 0.3) x anisotropic scale; (c) the rigid mode from the
    # reference's own initial pose: torch.manual_seed(0); torch.rand(6) radians / tanh-translations (ref:utils.py:316-321)
    if legs:
        th_star = torch.tensor(THETA_STAR, device=device)[None].expand(my_pairs, 3, 4).contiguous()
        th_star_inv = theta_star_inv().to(device)[None].expand(my_pairs, 3, 4).contiguous()
        th_rot = pose_rot(device, my_pairs)
        for key, th0 in (("value_theta_star", th_star), ("value_theta_star_inv", th_star_inv), ("value_rot", th_rot)):
            sv = tr.AffineSolver(mov, tgt, mode="affine", loss=tr.LossSpec(w_ncc=1.0), optimizer=args.optimizer, lr=1e-6, init=th0,
                                 capacity=pose_steps + 40)
            extra[key] = job_pairs * pose_steps / max_over_ranks(timed_run(sv, pose_steps), device)
            del sv
        sv = tr.AffineSolver(mov, tgt, mode="rigid", loss=tr.LossSpec(w_ncc=1.0), optimizer=args.optimizer, lr=1e-6,
                             init=pose_rigid_randinit(device, my_pairs), capacity=pose_steps + 40)
        extra["value_rigid_randinit"] = job_pairs * pose_steps / max_over_ranks(timed_run(sv, pose_steps), device)
        del sv
        # BASELINE.json configs[2]: one 256^3 pair, direct flow field + NCC + smoothness regulariser, Adam, 100 iterations (iterations / s)
        fs = tr.FlowSolver(mov[:1], tgt[:1], loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.01, smooth_weight=1.0, capacity=160)
        fs.run(40)
        fence()
        t0 = time.perf_counter()
        fs.run(100)
        fence()
        extra["flow_value"] = 100 / max_over_ranks(time.perf_counter() - t0, device)
        del fs

    # ---- a registration that CONVERGES: the same batch from theta = identity with a registration-sized step (Adam, lr 2e-3,
    # 300 iterations), timed as one trx_affine_run call; every pair must end below 1 % of its starting NCC loss.  The headline's 200 steps at
    # lr 1e-4 stay next to the identity; this run crosses to theta* (|theta* - I| = 0.1) in its first ~60 iterations and spends the rest there.
    # body_histogram: pair-iterations per kernel body, sampled from a replica run every RUN_CHUNK iterations (AffineSolver.bodies()).
    RUN_ITERS, RUN_LR, RUN_CHUNK = 300, 2e-3, 10
    if legs:
        sv = tr.AffineSolver(mov, tgt, mode="affine", loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=RUN_LR, capacity=RUN_ITERS)
        fence()
        t0 = time.perf_counter()
        sv.run(RUN_ITERS)
        fence()
        el_run = max_over_ranks(time.perf_counter() - t0, device)
        lr_ = sv.losses[:, :RUN_ITERS]
        extra["value_run"] = job_pairs * RUN_ITERS / el_run
        extra["run_loss_ratio_worst"] = float((lr_[:, -1] / lr_[:, 0]).max().item())
        extra["run_loss_first_last"] = [float(lr_[0, 0].item()), float(lr_[0, -1].item())]
        extra["run_theta_err_worst"] = float((sv.theta[:, :12].view(-1, 3, 4) - theta_star_inv().to(device)[None]).abs().max().item())
        del sv
        hist = {}
        rp = tr.AffineSolver(mov, tgt, mode="affine", loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=RUN_LR, capacity=RUN_ITERS)
        for _ in range(RUN_ITERS // RUN_CHUNK):
            rp.run(RUN_CHUNK)
            for name in rp.bodies():
                hist[name] = hist.get(name, 0) + RUN_CHUNK
        extra["body_histogram"] = hist
        del rp

    out = None
    if rank == 0:
        total = job_pairs * args.steps
        out = {"metric": "registration iterations/sec (3D 256^3 fp32, affine+NCC)", "value": total / elapsed,
               "unit": "pair-iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
               "dtype": "f32", "data": "synthetic",
               "config": {"workload": (f"3D {args.size}^3 fp32 affine+NCC, {PAIRS_PER_GPU} independent pairs per GPU "
                                       f"(BASELINE.json configs[3] share of one GPU), {args.optimizer.upper()} on theta") if args.scaling == "weak" else
                                      (f"3D {args.size}^3 fp32 affine+NCC, {args.pairs_total} independent pairs split over {world} GPU(s) "
                                       f"(BASELINE.json configs[3], strong scaling), {args.optimizer.upper()} on theta"),
                          "pairs_per_gpu": my_pairs if args.scaling == "strong" else PAIRS_PER_GPU, "pairs_total": job_pairs, "volume": [args.size] * 3, "loss": "NCC(alpha=100)", "optimizer": args.optimizer,
                          "preconditioning": f"{PRECONDITION} untimed iterations before the warm-up (clock settling); value_cold has none",
                          "parallelism": f"{world} x independent shards, no collective"}}
        if args.full:
            out["config"].update({
                          "value_cold": job_pairs * args.steps / elapsed_cold,
                          "value_cold_note": f"first {args.steps} iterations of a fresh solver after 2 s of idle GPU, no warm-up",
                          f"{other}_value": job_pairs * args.steps / elapsed2,
                          "value_theta_star": extra["value_theta_star"], "value_theta_star_inv": extra["value_theta_star_inv"], "value_rot": extra["value_rot"],
                          "value_rigid_randinit": extra["value_rigid_randinit"],
                          "pose_note": f"pair-iterations/s of {pose_steps} steps at a fixed pose (lr 1e-6), same batch: theta* (the map the synthetic "
                                       "moving volumes were warped with) and its inverse (value_theta_star_inv: the pose a registration of this batch "
                                       "converges to); theta = R(0.5, 0.4, 0.3) diag(1.05, 0.95, 1.02); rigid mode from "
                                       "the reference's initial pose torch.manual_seed(0), torch.rand(6).  The headline value itself starts at "
                                       "theta = identity (where every affine run starts) and moves |theta - I| by at most lr per step",
                          "value_run": extra["value_run"], "run_loss_ratio_worst": extra["run_loss_ratio_worst"], "run_loss_first_last": extra["run_loss_first_last"],
                          "run_theta_err_worst": extra["run_theta_err_worst"], "body_histogram": extra["body_histogram"],
                          "run_note": f"value_run: pair-iterations/s of ONE registration of the same batch that converges - from theta = identity, Adam lr {RUN_LR}, "
                                      f"{RUN_ITERS} iterations in one trx_affine_run call (no warm-up beyond the legs before it); run_loss_ratio_worst = the worst pair's last / first "
                                      "NCC loss (bar: < 0.01); run_theta_err_worst = max |theta_final - inverse(theta*)| over pairs and entries; body_histogram = pair-iterations per kernel body over a replica of that run (sampled every "
                                      f"{RUN_CHUNK} iterations)",
                          "flow_value": extra["flow_value"],
                          "flow_note": "iterations/s of BASELINE configs[2]: one 256^3 pair, direct flow field + NCC + smoothness regulariser, "
                                       "Adam (extension; parity vs torch autograd, not the reference), 100 iterations in one trx_flow_run call"})
        if world == 1 and args.full:
            # ---- roofline leg: the fused F1 kernel alone, events on the launch stream, AT THE POSES OF THE TIMED REGION: a replica of
            # the measured solver (same start, same optimiser, same warm-up) is stepped one iteration at a time and, before each of its K
            # timed iterations, the F1 launch of that iteration's theta is timed on its own (the kernel picks its body per pair from theta:
            # the z-streaming body next to the identity, the tile geometries further out)
            scratch = new_solver(args.optimizer)
            scratch.run(PRECONDITION)
            del scratch
            rep = new_solver(args.optimizer)
            rep.run(args.warmup)
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
            torch.cuda.synchronize()
            REP = 3   # launches per pose between the two events (the bracket itself costs 1-2 us)
            for e0, e1 in ev:
                e0.record()
                for r_ in range(REP):
                    rep.accumulate_only(walk_down=bool(r_ & 1))   # (alternating directions, as the iterations of a run do: TRX_FLAG_WALK_DOWN)
                e1.record()
                rep.run(1)
            torch.cuda.synchronize()
            per_it = [e0.elapsed_time(e1) * 1e-3 / REP for e0, e1 in ev]
            k_s = sum(per_it) / len(per_it)
            rows = rep.rows_used().tolist()
            alg = ALG_BYTES_PER_VOXEL * args.size ** 3 * my_pairs
            # HBM-side traffic and L2 requests come from separate PMC passes of this same command (tools/profile_bench.sh ->
            # tools/summarize_prof.py -> profiles/traffic.json); they are only quoted for the library they were measured on
            traffic, l2req, traffic_note = None, None, "no profiles/traffic.json"
            tf = os.path.join(ROOT, "profiles", "traffic.json")
            if os.path.exists(tf):
                import hashlib
                tj = json.load(open(tf))
                sha = hashlib.sha256(open(os.path.join(ROOT, "torchregister_amd", "lib", "libtrx.so"), "rb").read()).hexdigest()
                if tj.get("lib_sha256") == sha and args.size == SIZE:
                    traffic, l2req = tj.get("hbm_bytes_per_launch"), tj.get("l2_requests_per_launch")
                    traffic_note = f"PMC passes of this command on this library (tag {tj.get('tag')}, sha256 {sha[:12]})"
                else:
                    traffic_note = (f"profiles/traffic.json (tag {tj.get('tag')}) was measured on another build of libtrx.so "
                                    f"(sha256 {str(tj.get('lib_sha256'))[:12]} != {sha[:12]}): not quoted")
            out["roofline"] = {"bound": "hbm", "kernel": "affine_zs_step_kernel<0> (fused warp+NCC fwd/bwd, z-streaming: every pair of this workload; the "
                                                         "exact-footprint and tile kernels behind it take pairs further from the identity and return at once here)",
                               "achieved": alg / k_s / 1e9,
                               "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg / k_s / HBM_PEAK, "traffic": traffic, "traffic_note": traffic_note,
                               "kernel_ms": k_s * 1e3, "kernel_ms_first": per_it[0] * 1e3, "kernel_ms_last": per_it[-1] * 1e3,
                               "kernel_ms_note": f"mean over the {args.steps} timed iterations' poses of the F1 launches of a step at that pose - the z-streaming kernel and "
                                                 f"the two kernels behind it that find nothing to do - (replica run; events around {REP} back-to-back steps' launches per "
                                                 "pose, alternating the walk direction as the iterations of a run do); first / last = the first and last pose",
                               "partial_rows_per_pair_last": rows[0],
                               "algorithmic_bytes_per_launch": alg,
                               "l2_requests_per_launch": l2req, "l2_request_bytes": 128}
            if not args.no_pose_legs:
                # ---- second roofline object: the F1 pass at the rotated pose of config.value_rot (the exact-footprint step kernel takes
                # every pair there; same algorithmic bytes: each operand once).  Events around REP launches of exactly the step's F1 launches.
                def traffic_for(tag_file, key):
                    tfp = os.path.join(ROOT, "profiles", tag_file)
                    if not os.path.exists(tfp):
                        return None, f"no profiles/{tag_file}"
                    import hashlib
                    tj2 = json.load(open(tfp))
                    sha2 = hashlib.sha256(open(os.path.join(ROOT, "torchregister_amd", "lib", "libtrx.so"), "rb").read()).hexdigest()
                    if tj2.get("lib_sha256") != sha2 or args.size != SIZE:
                        return None, f"profiles/{tag_file} was measured on another build of libtrx.so: not quoted"
                    return tj2.get(key), f"PMC passes on this library (tag {tj2.get('tag')}, sha256 {sha2[:12]})"
                sv = tr.AffineSolver(mov, tgt, mode="affine", loss=tr.LossSpec(w_ncc=1.0), optimizer=args.optimizer, lr=0.0, init=th_rot, capacity=4)
                for _ in range(60):
                    sv.accumulate_only()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(60):
                    sv.accumulate_only()
                e1.record()
                torch.cuda.synchronize()
                k_rot = e0.elapsed_time(e1) * 1e-3 / 60
                tr_rot, note_rot = traffic_for("traffic_rot.json", "hbm_bytes_per_launch")
                out["roofline_rot"] = {"bound": "hbm", "kernel": "affine_eft_step_kernel<0> (exact-footprint body: every pair at theta = R(0.5, 0.4, 0.3) diag(1.05, 0.95, 1.02)) "
                                                                 "+ the fused step kernel behind it (no pair left for it)",
                                       "achieved": alg / k_rot / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg / k_rot / HBM_PEAK,
                                       "traffic": tr_rot, "traffic_note": note_rot, "kernel_ms": k_rot * 1e3, "algorithmic_bytes_per_launch": alg}
                del sv
                # ---- third: the dense-flow loop of config.flow_value.  Inside trx_flow_run the moments pass is fused into the previous
                # update, so the bytes that MUST move per iteration are 80 B/voxel with Adam + smoothness (flow r12 w12, m r12 w12, v r12
                # w12, moving 4 + target 4: DESIGN.md 4.3), not the 100 B/voxel of the two-pass step.
                fs = tr.FlowSolver(mov[:1], tgt[:1], loss=tr.LossSpec(w_ncc=1.0), optimizer="adam", lr=0.01, smooth_weight=1.0, capacity=200)
                fs.run(40)
                torch.cuda.synchronize()
                e0.record()
                fs.run(100)
                e1.record()
                torch.cuda.synchronize()
                k_flow = e0.elapsed_time(e1) * 1e-3 / 100
                alg_flow = 80 * args.size ** 3
                tr_flow, note_flow = traffic_for("traffic_flow.json", "hbm_bytes_per_iteration")
                out["roofline_flow"] = {"bound": "hbm", "kernel": "flow_update3_kernel (+ flow_coef_kernel): one iteration of trx_flow_run, 1 x 256^3, Adam + smoothness",
                                        "achieved": alg_flow / k_flow / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": alg_flow / k_flow / HBM_PEAK,
                                        "traffic": tr_flow, "traffic_note": note_flow, "iteration_ms": k_flow * 1e3,
                                        "algorithmic_bytes_per_iteration": alg_flow, "algorithmic_bytes_per_voxel": 80}
                del fs
                # ---- secondary configs the driver should see every round: cfg2 (1 x 128^3 affine + NCC, SGD) per iteration, and the flow +
                # local-window NCC device loop (1 x 256^3, w = 9, Adam + smoothness) per iteration
                t128 = blobs_gpu((128,) * 3, 1000, device)
                m128 = tr.get_affine_warp(torch.tensor(THETA_STAR, device=device)[None], t128)
                s2 = tr.AffineSolver(m128, t128, mode="affine", loss=tr.LossSpec(w_ncc=1.0), lr=1e-6, capacity=700)
                s2.run(100)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s2.run(400)
                torch.cuda.synchronize()
                out["config"]["cfg2_us_per_it"] = (time.perf_counter() - t0) / 400 * 1e6
                del s2
                fl = tr.FlowSolver(mov[:1], tgt[:1], optimizer="adam", lr=0.01, capacity=100, smooth_weight=1.0, lncc=dict(window=9))
                fl.run(20)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fl.run(50)
                torch.cuda.synchronize()
                out["config"]["lncc_loop_us"] = (time.perf_counter() - t0) / 50 * 1e6
                del fl
            if not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
