#!/usr/bin/env python3
"""sha256 digests of what the rigid / affine mutual-information path computes, at fixed seeds: one line per (case, quantity) over the raw bytes of
  eval     loss and dtheta of one affine_mi_loss_grad evaluation;
  run      every state tensor of AffineMISolver after 7 iterations (rigid + Adam, affine + SGD);
  warp     affine_warp(size=), affine_flow_warp forward and affine_flow_warp_backward;
  bspline  ctrl after 3 iterations of BSplineSolver(mi=), through an initial affine and (one lattice only: the plain loop takes no other) without.
Cases: target / moving (19, 23, 41) / (24, 20, 30) - two chunks of 16384 voxels, the second ragged, no size a power of two - and (13, 17) / (21, 15) in 2-D,
the same two targets with the moving image on the target's lattice, each with and without a mask, B = 2 with two different thetas.
Two builds compute the same thing exactly when every line is equal: a change that may move no result bit is checked by running this tool on both
(--root DIR: import torchregister_amd, and so its libtrx.so, from another checkout) and comparing the outputs with diff."""
import argparse
import hashlib
import os
import sys

import torch

LATTICES = [("3d-two", (19, 23, 41), (24, 20, 30)), ("2d-two", (13, 17), (21, 15)), ("3d-one", (19, 23, 41), (19, 23, 41)), ("2d-one", (13, 17), (13, 17))]
THETA3 = [[[1.01, 0.013, -0.007, 0.011], [-0.009, 0.99, 0.012, -0.013], [0.006, -0.011, 1.008, 0.009]],
          [[0.95, -0.1, 0.02, 0.05], [0.1, 0.97, 0.0, -0.03], [0.0, 0.03, 1.02, 0.02]]]
THETA2 = [[[1.01, 0.013, 0.011], [-0.009, 0.99, -0.013]], [[0.95, -0.1, 0.05], [0.1, 0.97, -0.03]]]
POSE3 = [[0.02, -0.015, 0.01, 0.03, -0.02, 0.01], [-0.1, 0.05, 0.08, -0.04, 0.06, 0.02]]
POSE2 = [[0.02, 0.03, -0.02], [-0.1, -0.04, 0.06]]
STATE = ("param", "theta", "adam_m", "adam_v", "best_theta", "best_loss", "best_idx", "losses", "step", "grad")


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torchregister_amd as tr
    eng = tr._engine
    if not torch.cuda.is_available():
        raise SystemExit("ami_state_digest.py needs a GPU: there is no CPU path to digest")
    dev = torch.device("cuda")
    for name, tshape, mshape in LATTICES:
        nd = len(tshape)
        g = torch.Generator().manual_seed(1234 + sum(tshape) + 7 * sum(mshape))      # CPU generator: the same inputs in every process
        tgt, mov = torch.rand((2, 1) + tshape, generator=g).to(dev), torch.rand((2, 1) + mshape, generator=g).to(dev)
        roi = (torch.rand((2, 1) + tshape, generator=g) > 0.4).to(dev)
        flow = (3.0 * (torch.rand((2, nd) + tshape, generator=g) - 0.5)).to(dev)
        gout = torch.rand((2, 1) + tshape, generator=g).to(dev)
        theta = torch.tensor(THETA3 if nd == 3 else THETA2, device=dev)
        pose = torch.tensor(POSE3 if nd == 3 else POSE2, device=dev)

        print(f"{name} warp affine_warp(size=) {digest(eng.affine_warp(theta, mov, size=tshape))}")
        print(f"{name} warp affine_flow_warp {digest(eng.affine_flow_warp(mov, theta, flow))}")
        print(f"{name} warp affine_flow_warp_backward {digest(eng.affine_flow_warp_backward(mov, theta, flow, gout))}")
        for mname, mask in (("unmasked", None), ("masked", roi)):
            case = f"{name} {mname}"
            loss, dth = eng.affine_mi_loss_grad(mov, tgt, theta, eng.mi_range(tgt, mov, mask=mask), mask=mask)
            print(f"{case} eval loss+dtheta {digest(loss, dth)}")
            for mode, opt, lr, init in (("rigid", "adam", 1e-2, pose), ("affine", "sgd", 1e-2, theta)):
                s = tr.AffineMISolver(mov, tgt, mode=mode, mi={}, optimizer=opt, lr=lr, init=init, capacity=8, mask=mask)
                s.run(7)
                for attr in STATE:
                    print(f"{case} run {mode}+{opt} {attr} {digest(getattr(s, attr))}")
            for iname, kw in (("initial", dict(initial=theta)),) + ((("plain", {}),) if tshape == mshape else ()):
                s = tr.BSplineSolver(mov, tgt, 5, mi={}, optimizer="adam", lr=0.05, capacity=4, mask=mask, **kw)
                s.run(3)
                print(f"{case} bspline {iname} ctrl {digest(s.ctrl)}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
