#!/usr/bin/env python3
"""What the principal-axes / pose-search initialiser costs.  Device events, medians of three rounds, one process.

  trx_image_moments2 at 1 x 128^3 and 1 x 256^3, raw and masked, beside trx_image_moments in the same process: microseconds per call and the ratio.
  The search at its working sizes: the scoring time of one chunk of 64 candidates at 32^3 and 64^3 (one call of trx_affine_mi_loss_grad_grids with
  image strides 0, loss only), the refinement of 8 candidates x 30 iterations, and the whole world_search - host arithmetic and read-backs included, wall
  clock - for step 45 and step 30 on the coarsest level of a 128^3 pair with levels=3, next to the registration it precedes (rigid, Adam, 3 levels of
  100 iterations, world_init='moments').

    python tools/bench_world_search.py [--out profiles/world_search_bench.txt]
Needs a GPU; there is no fallback."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torchregister_amd as tr  # noqa: E402
from torchregister_amd import _engine as eng, _lib  # noqa: E402
from torchregister_amd.pyramid import pyramid  # noqa: E402
from bench_affine_mi_world import diagonal_header, image, timed  # noqa: E402

CALLS, ROUNDS = 20, 3


def median_us(fn, n=CALLS):
    timed(fn, 3)
    return statistics.median(timed(fn, n) * 1e3 for _ in range(ROUNDS))


def bench_moments(S, say):
    x = image((S, S, S), 3).cuda()
    mask = (image((S, S, S), 4) > 0.5).to(torch.uint8).cuda()
    lib = _lib.load()
    off = x.reshape(1, -1).amin(1).contiguous()
    stream = _lib.current_stream(torch.device("cuda"))
    for name, mk in (("raw", None), ("masked", mask)):
        us = []
        for fn, ncol in (("trx_image_moments", 4), ("trx_image_moments2", 10)):
            n = getattr(lib, fn + "_workspace_bytes")(3, 1, S, S, S)
            ws, out = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(1, ncol, dtype=torch.float64, device="cuda")
            f = getattr(lib, fn)
            us.append(median_us(lambda: f(_lib.ptr(x), _lib.ptr(mk), _lib.ptr(off), 3, 1, S, S, S, _lib.ptr(out), _lib.ptr(ws), n, stream)))
        say(f"  1 x {S}^3 {name:6s}: trx_image_moments {us[0]:8.1f} us, trx_image_moments2 {us[1]:8.1f} us per call (two launches each), ratio {us[1] / us[0]:.2f}")


def pair(S):
    tshape, mshape = (S, S, S), (7 * S // 8, S, 9 * S // 8)
    tvox, mvox = (128.0 / S,) * 3, (1.1 * 128.0 / S, 0.95 * 128.0 / S, 0.9 * 128.0 / S)
    return image(mshape, 1).cuda(), image(tshape, 2).cuda(), diagonal_header(mshape, mvox), diagonal_header(tshape, tvox)


def bench_chunk(S, say):
    """One scoring call as world_search issues it: 64 candidates along the batch axis, image strides 0, dtheta = NULL."""
    mov, tgt, Am, At = pair(S)
    ms, ts = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    T0 = eng._about(tr.rotation_grid(3, 45.0)[:64], torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    rec = tr.world_geometry(ms, ts, Am, At, T0, torch.zeros(3, dtype=torch.float64)).record.cuda()
    lib, n = _lib.load(), 64
    vol = eng._volumes(mov, tgt, 0, 0, ts, tables=eng.base_tables(ts, mov.device))
    vol.B = n
    rng = eng.mi_range(tgt, mov).expand(n, 4).contiguous()
    cfg = eng._mi_cfg_c(32, 1.0, False, rng, None)
    mg = eng._moving_grid(ms, None, False, None, rec)
    th = eng.pad_theta(torch.eye(3, 4, device="cuda").repeat(n, 1, 1), 3)
    nbytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), 32)
    ws, loss = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(n, device="cuda")
    stream = _lib.current_stream(mov.device)

    def call():
        rc = lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), None, _lib.ptr(ws), nbytes, stream)
        assert rc == 0, rc
    us = median_us(call)
    say(f"  scoring, one chunk of 64 candidates at {S}^3 from {ms}: {us:9.1f} us per call = {us / 64:.1f} us per candidate")
    geo = tr.world_geometry(ms, ts, Am, At, T0[:8], torch.zeros(3, dtype=torch.float64))
    rep = lambda t: t.expand(8, *t.shape[1:])  # noqa: E731

    def refine():
        s = tr.AffineMISolver(rep(mov), rep(tgt), mode="rigid", mi=dict(bins=32), optimizer="adam", lr=0.01, init=torch.zeros(8, 6), capacity=30, world=geo)
        s.run(30)
    refine()
    torch.cuda.synchronize()
    ts_ = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        refine()
        torch.cuda.synchronize()
        ts_.append((time.perf_counter() - t0) * 1e3)
    say(f"  refinement, 8 candidates x 30 iterations at {S}^3 (solver set-up included, wall clock): {statistics.median(ts_):8.2f} ms")


def wall_ms(fn):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(ROUNDS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def bench_whole(say):
    mov, tgt, Am, At = pair(128)
    lm, lt = pyramid(mov, 3)[0], pyramid(tgt, 3)[0]
    say(f"  the whole search on a 128^3 pair with levels=3: moments on {tuple(tgt.shape[2:])} / {tuple(mov.shape[2:])}, candidates on {tuple(lt.shape[2:])} / {tuple(lm.shape[2:])}")

    def reg(init, search=None):
        r = tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6), levels=3)
        r.optim(mov, tgt, lr=0.01, max_epochs=100, moving_affine=Am, target_affine=At, world_init=init, world_search=search)
        return r
    base = wall_ms(lambda: reg("moments"))
    say(f"    the registration it precedes (rigid, Adam, 3 x 100 iterations, world_init='moments'): {base:9.2f} ms wall clock")
    for name, init, search in (("principal_axes (4 candidates, keep 4)", "principal_axes", dict(keep=4, iters=30)),
                               ("search, step 45 (4 + 320 candidates, keep 8)", "search", dict(step=45, keep=8, iters=30)),
                               ("search, step 30 (4 + 1008 candidates, keep 8)", "search", dict(step=30, keep=8, iters=30))):
        ms_ = wall_ms(lambda: eng.world_setup(mov, tgt, Am, At, init, world_search=search, mi=dict(bins=32), search_on=(lm, lt, None, None)))
        say(f"    {name:48s}: {ms_:9.2f} ms wall clock = {100.0 * ms_ / base:.1f} % of the registration")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_world_search.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say(f"principal-axes / pose-search initialiser - {torch.cuda.get_device_name(0)}; medians of {ROUNDS} rounds")
    for S in (128, 256):
        bench_moments(S, say)
    for S in (32, 64):
        bench_chunk(S, say)
    bench_whole(say)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
