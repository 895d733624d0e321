#!/usr/bin/env python3
"""Coarse-to-fine measurements (hipEvents, after warm-up):
  (a) pyramid() of 8 x 256^3 moving + 8 x 256^3 target, 3 levels: time, and the fraction of the 8 TB/s HBM roofline on algorithmic bytes
      (every level's input read once + output written once: 16 x 256^3 x 4 B x (1 + 1/8) for the first halving, 1/8 of that again for the
      second);
  (b) one 256^3 rigid pair from the reference's random init (torch.rand pose, MSE, SGD): single level 300 iterations against levels=3 with
      200 / 100 / 50 iterations; wall time and the final full-resolution loss of each.
--only-pyramid: (a) alone (the rocprofv3 --kernel-trace --stats run)."""
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torchregister_amd as tr  # noqa: E402
from bench import blobs_gpu, THETA_STAR  # noqa: E402

HBM = 8.0e12


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


def main():
    dev = torch.device("cuda")
    S, B = 256, 8
    out = {}
    mov = torch.cat([blobs_gpu((S,) * 3, 2000 + b, dev) for b in range(B)])
    tgt = torch.cat([blobs_gpu((S,) * 3, 1000 + b, dev) for b in range(B)])
    both = lambda: (tr.pyramid(mov, 3), tr.pyramid(tgt, 3))  # noqa: E731
    for _ in range(3):
        both()
    torch.cuda.synchronize()
    t = timed(both, 20)
    vox = 2 * B * S ** 3
    alg = vox * 4 * (1 + 1 / 8) + vox / 8 * 4 * (1 + 1 / 8)
    t_half = timed(lambda: (tr.pyramid(mov, 2), tr.pyramid(tgt, 2)), 20)
    out["pyramid_8x256^3_x2_3levels"] = dict(ms=t * 1e3, algorithmic_GB=alg / 1e9, TBps=alg / t / 1e12, roofline_fraction=alg / t / HBM)
    alg1 = vox * 4 * (1 + 1 / 8)
    out["first_halving_only"] = dict(ms=t_half * 1e3, algorithmic_GB=alg1 / 1e9, TBps=alg1 / t_half / 1e12, roofline_fraction=alg1 / t_half / HBM)
    if "--only-pyramid" in sys.argv:
        print(json.dumps(out))
        return
    del mov, tgt
    # (b) one rigid pair from the reference's random init
    m1 = blobs_gpu((S,) * 3, 2000, dev)
    th = torch.tensor(THETA_STAR, device=dev)[None]
    t1 = tr.get_affine_warp(th, m1).contiguous()
    crit = dict(criterion=[nn.MSELoss()], weight=[1.0])
    for name, levels, eps in (("single_300", 1, 300), ("levels3_200_100_50", 3, [200, 100, 50])):
        for rep in range(2):                                  # rep 0 = warm-up (code objects, tables)
            torch.manual_seed(0)
            torch.cuda.manual_seed(0)
            reg = tr.Register("rigid", levels=levels, **crit)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            reg.optim(m1, t1, lr=1e-2, max_epochs=eps)
            e1.record()
            torch.cuda.synchronize()
        loss = torch.mean((reg(m1) - t1) ** 2).item()
        out[f"rigid_256^3_{name}"] = dict(ms=e0.elapsed_time(e1), final_full_res_mse=loss,
                                          theta_err=(reg.theta - th).abs().max().item())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
