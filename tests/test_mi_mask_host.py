"""Host-side checks of the region-of-interest mask of the mutual information (trx_mi_cfg.mask): the restatement tests/mi_mask_ref.py against a
second formulation, the conditions the GPU tests (tests/test_gpu_mi_mask.py) rely on in it - its own fp32-fp64 gaps stay below the floors of the
bars, and a masked result differs from the unmasked one by far more than any bar, so a kernel that ignores the mask cannot pass -, the premise of
the occluder test, the layout of the grown struct, and the ValueErrors of the public interface on CPU tensors."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import affine_mi_ref as aref
import mi_mask_ref as mref
import mi_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 6, 7), (19, 23, 41), (131, 127)]


def _pair(shape):
    """(target, warped) for the warped-volume entry points: affine_mi_ref's target and its moving image."""
    mov, tgt = aref.pair(shape)
    return tgt, mov


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_selection_equals_weighting(shape):
    """The restatement (select the voxels, call mi_ref) equals a 0 / 1-weighted joint table divided by N_m, to 1e-12 in fp64; the table sums to 1
    and the gradient is zero exactly outside the mask."""
    tgt, wrp = _pair(shape)
    for name in ("ellipsoid", "checkerboard", "single-voxel"):
        mask = mref.MASKS[name](shape)
        rng = mref.fit_range(tgt, wrp, mask)
        for bins in (8, 32, 64):
            P, Pw = mref.joint(tgt, wrp, mask, bins, rng), mref.weighted_joint(tgt, wrp, mask, bins, rng)
            assert (P - Pw).abs().max().item() <= 1e-12 and abs(P.sum().item() - 1.0) <= 1e-12, (name, bins)
            for normalized in (False, True):
                l1 = mref.loss(tgt, wrp, mask, bins, 1.0, normalized, rng)
                l2 = mi_ref.loss_from_table(Pw, 1.0, normalized)
                assert abs(l1.item() - l2.item()) <= 1e-12, (name, bins, normalized)
        _, g = mref.loss_grad(tgt, wrp, mask, rng)
        assert g.shape == wrp.shape and g[~mask].abs().max().item() == 0.0
    empty = mref.zeros(shape)
    loss, g = mref.loss_grad(tgt, wrp, empty, mi_ref.fit_range(tgt, wrp))
    assert loss.tolist() == [0.0] and g.abs().max().item() == 0.0


def test_ellipsoid_sizes():
    assert [int(mref.ellipsoid(s).sum()) for s in SHAPES] == [32, 3249, 6387]
    m = mref.first_chunk_empty((19, 23, 41)).flatten()
    assert not m[: mref.CHUNK].any() and m[mref.CHUNK:].all() and int(m.sum()) == 17917 - 16384


@pytest.mark.parametrize("shape", SHAPES + [(40, 40, 40)], ids=lambda s: "x".join(map(str, s)))
def test_a_kernel_that_ignores_the_mask_cannot_pass(shape):
    """The masked and the unmasked fp64 losses (same range) differ by orders of magnitude more than the 2e-5 relative bar of the GPU tests, for the
    warped-volume form and behind the affine warp, and the restatement's own fp32-fp64 gap stays below 1e-5 relative (loss): the floors bind."""
    tgt, wrp = _pair(shape)
    mask = mref.ellipsoid(shape)
    rng = mref.fit_range(tgt, wrp, mask)
    for bins in (8, 32, 64):
        for normalized in (False, True):
            lm = mref.loss(tgt, wrp, mask, bins, 1.0, normalized, rng).item()
            lm32 = mref.loss(tgt, wrp, mask, bins, 1.0, normalized, rng, torch.float32).item()
            lu = mi_ref.loss(tgt, wrp, bins, 1.0, normalized, rng).item()
            rel, gap = abs(lm - lu) / abs(lm), abs(lm32 - lm) / abs(lm)
            print(f"{shape} K={bins} {'normalized' if normalized else 'plain'}: masked {lm:.6f} unmasked {lu:.6f} rel. difference {rel:.2e}, fp32-fp64 {gap:.1e}")
            assert rel >= 1e-3 and gap <= 1e-5, (shape, bins, normalized, rel, gap)
    th = aref.theta0(len(shape))[None]
    mov = wrp
    lm, gm, _ = mref.evaluate(mov, tgt, th, rng, mask)
    lu, gu, _ = aref.evaluate(mov, tgt, th, rng)
    assert abs(lm.item() - lu.item()) >= 1e-3 * abs(lm.item()) and (gm - gu).abs().max().item() >= 1e-2 * gm.abs().max().item()


@pytest.mark.parametrize("name", list(aref.LOOPS))
def test_masked_arbiter_descends_and_its_precisions_stay_together(name):
    """What the masked loop test on the GPU relies on, as tests/test_affine_mi_host.py asserts for the unmasked arbiter: under the ellipsoid mask the
    fp64 loss falls in every iteration and the fp32 run stays within 1e-5 (loss curve) and 2e-5 (final parameter) - the loop bars are the floors."""
    (l64, p64), (l32, p32) = mref.loop_pair(name)
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    (u64, q64), _ = aref.loop_pair(name)
    print(f"{name}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, lgap {lgap:.1e}, pgap {pgap:.1e}; unmasked curve differs by {np.max(np.abs(u64 - l64)):.1e}, "
          f"parameters by {np.max(np.abs(q64 - p64)):.1e}")
    assert len(l64) == aref.ITERS and np.all(np.isfinite(l64)) and np.all(np.diff(l64) < 0), l64
    assert lgap <= 1e-5 and pgap <= 2e-5, (lgap, pgap)
    assert np.max(np.abs(u64 - l64)) >= 100 * 2e-5 * np.max(np.abs(l64))            # ignoring the mask misses the loss bar a hundred times over


@pytest.mark.parametrize("name", list(mref.FLOW_LOOPS))
def test_masked_flow_arbiters_descend(name):
    _, _, _, _, (l64, p64), (l32, p32) = mref.flow_loop_pair(name)
    print(f"{name}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, lgap {np.max(np.abs(l32 - l64)):.1e}, pgap {np.max(np.abs(p32 - p64)):.1e}")
    assert np.all(np.isfinite(l64)) and np.all(np.diff(l64) < 0), l64


def test_the_occluder_premise_holds_in_the_arbiter():
    """tests/test_gpu_mi_mask.py::test_mask_restores_the_pose_an_occluder_spoils: in fp64 (and in fp32) the masked run ends at most half as far from
    the clean pair's pose as the unmasked run does."""
    assert np.max(np.abs(mref.occluder_clean_pose() - np.asarray(mref.OCC_TRUTH))) <= 1e-7
    masked, unmasked = mref.occluder_errors(torch.float64)
    m32, u32 = mref.occluder_errors(torch.float32)
    print(f"pose error against the clean pair's pose: masked {masked:.5f} unmasked {unmasked:.5f} (fp32: {m32:.5f}, {u32:.5f})")
    assert masked <= 0.5 * unmasked and m32 <= 0.5 * u32
    assert masked <= 0.25 * unmasked and abs(m32 - masked) <= 1e-4 and abs(u32 - unmasked) <= 1e-4     # room for the GPU's fp32 trajectory


def test_struct_layout_matches_the_header():
    """sizeof(trx_mi_cfg) and offsetof(trx_mi_cfg, mask) from a compiled C snippet equal the ctypes mirror's; the version stays 240."""
    from torchregister_amd import _lib
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "trx.h"\nint main(){printf("%zu %zu %zu %d\\n", sizeof(trx_mi_cfg), offsetof(trx_mi_cfg, mask),' \
          ' offsetof(trx_mi_cfg, range), TRX_VERSION);return 0;}'
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    assert got == [ctypes.sizeof(_lib.MICfg), _lib.MICfg.mask.offset, _lib.MICfg.range.offset, 240]
    assert _lib.MICfg().mask is None                                        # a cfg built without the field is the unmasked call


def test_workspace_sizes_do_not_depend_on_the_mask():
    from torchregister_amd import _lib
    lib = _lib.load()
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert lib.trx_mi_workspace_bytes(3, 2, 19, 23, 41, 32) == up(2 * 32 * 32 * 8) + up(2 * 32 * 32 * 4)


def test_mask_u8():
    import torchregister_amd as tr
    f = tr._engine._mask_u8
    like = torch.zeros(2, 1, 4, 5, 6)
    for m in (torch.ones(2, 1, 4, 5, 6, dtype=torch.bool), torch.ones(2, 4, 5, 6), torch.full((2, 1, 4, 5, 6), -3.5), torch.ones(2, 4, 5, 6, dtype=torch.int64)):
        out = f(m, like)
        assert out.dtype == torch.uint8 and out.shape == like.shape and out.is_contiguous() and bool((out == 1).all())
    half = torch.zeros(2, 4, 5, 6)
    half[1] = 0.25
    assert f(half, like).flatten(1).sum(1).tolist() == [0, 120]
    for bad in (torch.ones(1, 1, 4, 5, 6), torch.ones(2, 1, 4, 5), torch.ones(2, 2, 4, 5, 6), torch.ones(4, 5, 6)):
        with pytest.raises(ValueError, match="mask"):
            f(bad, like)
    with pytest.raises(ValueError, match="mask"):
        f([[1]], like)
    rng = tr._engine.mi_range(torch.arange(48.0).reshape(2, 1, 4, 6), torch.ones(2, 1, 4, 6), mask=torch.cat([torch.zeros(1, 4, 6), torch.ones(1, 4, 6)]).roll(3, 2))
    assert rng.tolist() == [[0.0, 23.0, 0.0, 1.0], [24.0, 47.0, 0.0, 1.0]]
    m = torch.zeros(2, 1, 4, 6)
    m[0, 0, 1, 2:4] = 1
    assert tr._engine.mi_range(torch.arange(48.0).reshape(2, 1, 4, 6), torch.ones(2, 1, 4, 6), mask=m).tolist() == [[8.0, 9.0, 0.0, 1.0], [24.0, 47.0, 0.0, 1.0]]


def test_unsupported_routes_raise_before_any_device_work():
    """mask= is for the device-side mutual-information loops only: every other route raises ValueError on CPU tensors (which the GPU path itself
    would refuse with another exception type), and so does a mask of the wrong shape on a supported route."""
    import torch.nn as nn
    import torchregister_amd as tr
    m3 = t3 = torch.zeros(1, 1, 8, 8, 8)
    m2 = t2 = torch.zeros(1, 1, 8, 8)
    k3, k2 = torch.ones(1, 1, 8, 8, 8), torch.ones(1, 8, 8)
    mi = dict(criterion=[tr.MILoss()], weight=[1.0])
    unsupported = [
        (tr.Register("rigid"), m3, t3, k3),
        (tr.Register("affine", honor_criterion=True, **mi), m3, t3, k3),                    # MILoss through the generic loop
        (tr.Register("affine", criterion=[nn.MSELoss()], weight=[1.0], honor_criterion=True), m3, t3, k3),
        (tr.Register("flow", flow_model="direct", criterion=[nn.MSELoss()], weight=[1.0]), m3, t3, k3),
        (tr.Register("flow", flow_model="direct", criterion=[tr.LocalNCCLoss()], weight=[1.0]), m3, t3, k3),
        (tr.Register("flow", flow_model="direct", **mi), m2, t2, k2),                       # 2-D direct flow runs the generic path
        (tr.Register("flow", flow_model="bspline", criterion=[nn.MSELoss()], weight=[1.0]), m3, t3, k3),
        (tr.Register("flow", flow_model="bspline", criterion=[nn.MSELoss()], weight=[1.0], diffeomorphic=True), m3, t3, k3),
        (tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()]), m3, t3, k3),    # no weight: the default criteria run
        (tr.Register("flow", flow_model="unet", **mi), m2, t2, k2),
        (tr.Register("rigid", levels=2), m3, t3, k3),
    ]
    for reg, m, t, k in unsupported:
        with pytest.raises(ValueError, match="device-side mutual-information loops"):
            reg.optim(m, t, max_epochs=1, mask=k)
    supported = [tr.Register("rigid", device_loop=True, **mi), tr.Register("affine", device_loop=True, levels=2, **mi),
                 tr.Register("flow", flow_model="bspline", **mi), tr.Register("flow", flow_model="direct", **mi)]
    for reg in supported:
        with pytest.raises(ValueError, match="does not match the target lattice"):
            reg.optim(m3, t3, max_epochs=1, mask=torch.ones(1, 1, 8, 8, 7))
    for fn in (tr.affine_register, tr.rigid_register):
        with pytest.raises(ValueError, match="device-side mutual-information loops"):
            fn(m3, t3, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, honor_criterion=True, mask=k3)
        with pytest.raises(ValueError, match="does not match the target lattice"):
            fn(m3, t3, criterions=[tr.MILoss()], weights=[1.0], grad_edges=False, device_loop=True, mask=k2)
    fr = tr.flow_register((8, 8, 8), criterions=[nn.MSELoss()], weights=[1.0], flow_model="direct")
    with pytest.raises(ValueError, match="device-side mutual-information loops"):
        fr.optimize(m3, t3, debug=False, mask=k3)
    fr = tr.flow_register((8, 8), criterions=[tr.MILoss()], weights=[1.0], flow_model="direct")
    with pytest.raises(ValueError, match="device-side mutual-information loops"):
        fr.optimize(m2, t2, debug=False, mask=k2)
    fr = tr.flow_register((8, 8), criterions=[tr.MILoss()], weights=[1.0], flow_model="bspline", spacing=4)
    with pytest.raises(ValueError, match="does not match the target lattice"):
        fr.optimize(m2, t2, debug=False, mask=k3)
    with pytest.raises(ValueError, match="does not match the target lattice"):
        tr.MILoss()(t3, m3, mask=k2)
