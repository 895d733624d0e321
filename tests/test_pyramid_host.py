"""CPU-only checks of the coarse-to-fine surface: the level rule, trx_resample's argument checks, Register's validation."""
import ctypes

import pytest
import torch
import torch.nn as nn


def test_pyramid_shapes_level_rule():
    from torchregister_amd import pyramid_shapes
    assert pyramid_shapes((181, 181, 181), 3) == [(46, 46, 46), (91, 91, 91), (181, 181, 181)]        # odd sizes: ceil(s / 2)
    assert pyramid_shapes((9, 130, 7), 3) == [(9, 33, 7), (9, 65, 7), (9, 130, 7)]                    # axes stop at the floor of 8
    assert pyramid_shapes((16, 17, 300), 4) == [(8, 9, 38), (8, 9, 75), (8, 9, 150), (16, 17, 300)]
    assert pyramid_shapes((97, 128), 3) == [(25, 32), (49, 64), (97, 128)]                            # 2-D stays 2-D
    assert pyramid_shapes((64, 64, 64), 1) == [(64, 64, 64)]
    for s in range(32, 300):                                 # ceil(ceil(s / 2) / 2) = ceil(s / 4)
        assert pyramid_shapes((s, 40), 3)[0] == (-(-s // 4), 10)


def test_pyramid_shapes_rejects_levels_that_do_not_shrink():
    from torchregister_amd import pyramid_shapes
    with pytest.raises(ValueError, match="largest levels that works .* is 2"):
        pyramid_shapes((16, 9, 12), 3)              # (16,9,12) -> (8,9,12) -> nothing shrinks
    with pytest.raises(ValueError, match="is 1"):
        pyramid_shapes((9, 14), 2)
    with pytest.raises(ValueError):
        pyramid_shapes((64, 64), 0)


def test_resample_argument_checks_without_gpu():
    """trx_resample returns its status before any HIP call."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    n = lib.trx_resample_workspace_bytes(3, 2, 16, 16, 16, 8, 8, 8)
    assert n >= 2 * (16 * 16 * 8 + 16 * 8 * 8) * 4          # the intermediates of the two passes in front of the last
    assert lib.trx_resample_workspace_bytes(2, 1, 1, 16, 16, 1, 8, 8) >= 16 * 8 * 4
    assert lib.trx_resample_workspace_bytes(4, 1, 8, 8, 8, 4, 4, 4) == 0
    assert lib.trx_resample_workspace_bytes(3, 1, 2048, 1024, 1024, 8, 8, 8) == 0     # 2^31 voxels
    ok = (3, 2, 16, 16, 16, 8, 8, 8)
    assert lib.trx_resample(None, P(16), *ok, 0, 1, None, P(16), n, None) == -1                    # null input
    assert lib.trx_resample(P(16), None, *ok, 0, 1, None, P(16), n, None) == -1                    # null output
    assert lib.trx_resample(P(16), P(16), *ok, 0, 1, None, None, n, None) == -1                    # null workspace
    assert lib.trx_resample(P(16), P(16), 4, 2, 16, 16, 16, 8, 8, 8, 0, 1, None, P(16), n, None) == -2   # ndim 4
    assert lib.trx_resample(P(16), P(16), 2, 2, 3, 16, 16, 1, 8, 8, 0, 1, None, P(16), n, None) == -2    # D != 1 with ndim 2
    assert lib.trx_resample(P(16), P(16), 2, 2, 1, 16, 16, 2, 8, 8, 0, 1, None, P(16), n, None) == -2   # Do != 1 with ndim 2
    for bad in ((3, 0, 16, 16, 16, 8, 8, 8), (3, 2, 0, 16, 16, 8, 8, 8), (3, 2, 16, 16, 16, 8, -1, 8), (3, 2, 16, 16, 16, 8, 8, 0)):
        assert lib.trx_resample(P(16), P(16), *bad, 0, 1, None, P(16), n, None) == -1             # non-positive sizes
    assert lib.trx_resample(P(16), P(16), 3, 1, 2048, 1024, 1024, 8, 8, 8, 0, 1, None, P(16), 1 << 40, None) == -1   # >= 2^31 voxels
    assert lib.trx_resample(P(16), P(16), *ok, 2, 1, None, P(16), n, None) == -1                   # align_corners not 0 / 1
    assert lib.trx_resample(P(16), P(16), *ok, 0, 0, None, P(16), n, None) == -1                   # channels < 1
    scale = (ctypes.c_float * 65)()
    assert lib.trx_resample(P(16), P(16), *ok, 0, 65, scale, P(16), n, None) == -1                 # more channels than the kernel carries
    assert lib.trx_resample(P(16), P(16), *ok, 0, 1, None, P(16), n - 1, None) == -3               # workspace too small


def test_register_levels_validation_before_the_gpu():
    """Bad schedules are refused before any tensor reaches the GPU (CPU tensors would otherwise raise 'no CPU fallback')."""
    import torchregister_amd as tr
    mov, tgt = torch.rand(1, 1, 32, 32, 32), torch.rand(1, 1, 32, 32, 32)
    for mode in ("affine", "rigid"):
        reg = tr.Register(mode, criterion=[nn.MSELoss()], weight=[1.0], levels=3)
        with pytest.raises(ValueError, match="max_epochs"):
            reg.optim(mov, tgt, lr=1e-2, max_epochs=[10, 10])
        with pytest.raises(ValueError, match="lr"):
            reg.optim(mov, tgt, lr=[1e-2, 1e-2, 1e-2, 1e-2], max_epochs=10)
    reg = tr.Register("flow", flow_model="direct", levels=2)
    with pytest.raises(ValueError, match="lr"):
        reg.optim(mov, tgt, lr=(1e-2,), max_epochs=5)
    with pytest.raises(ValueError, match="largest levels"):
        tr.Register("affine", levels=3).optim(torch.rand(1, 1, 16, 9, 12), torch.rand(1, 1, 16, 9, 12), max_epochs=5)
    with pytest.raises(ValueError, match="direct"):
        tr.Register("flow", levels=2)                       # flow_model='unet' (the default) is tied to one image size
    with pytest.raises(ValueError, match="direct"):
        tr.Register("flow", flow_model="unet", levels=3)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            tr.Register("affine", levels=bad)
    tr.Register("flow", levels=1)                            # the U-Net is fine at one level
    with pytest.raises(tr._lib.TrxError, match="no CPU fallback"):
        tr.Register("affine", levels=2).optim(mov, tgt, max_epochs=[3, 3])     # a valid schedule reaches the GPU check


def test_resample_workspace_is_the_chunked_plan():
    """trx_resample_workspace_bytes is exactly the plan's formula (resample_plan_ref): chunk, t1, t2, t2 on a 64-float boundary, 256 bytes
    at least.  The chunked shapes are the ones tests/test_gpu_pyramid_edges.py runs, so a change to the plan shows up here first."""
    from resample_ref import RESAMPLE_CHUNK_BYTES, resample_plan_ref
    from torchregister_amd import _lib
    lib = _lib.load()

    def ws(N, sp, size):
        S = (1,) * (3 - len(sp)) + tuple(sp)
        So = (1,) * (3 - len(size)) + tuple(size)
        return lib.trx_resample_workspace_bytes(len(sp), N, *S, *So)

    # 5 x 256^3 -> 128^3: W, H, D halve (ties: inner axis first); 48 MiB of intermediates per volume -> chunks of 2 + 2 + 1
    t1, t2 = 256 * 256 * 128, 256 * 128 * 128
    assert resample_plan_ref(5, (256,) * 3, (128,) * 3) == (2, t1, t2, 2 * t1, (2 * t1 + 2 * t2) * 4)
    assert ws(5, (256,) * 3, (128,) * 3) == (2 * t1 + 2 * t2) * 4 == 96 << 20
    assert ws(5, (256,) * 3, (128,) * 3) < 5 * (t1 + t2) * 4                # smaller than the un-chunked need
    # upsample_flow of one 128^3 flow to 256^3: 3 volumes, chunks of 2 + 1
    t1, t2 = 128 * 128 * 256, 128 * 256 * 256
    assert resample_plan_ref(3, (128,) * 3, (256,) * 3) == (2, t1, t2, 2 * t1, (2 * t1 + 2 * t2) * 4)
    assert ws(3, (128,) * 3, (256,) * 3) == (2 * t1 + 2 * t2) * 4 < 3 * (t1 + t2) * 4
    # the 64-float rounding of t2's offset: W, D, H: t1 = 9*11*6, t2 = 5*11*6; chunk * t1 = 1782 floats -> t2 starts at 1792
    assert resample_plan_ref(3, (9, 11, 13), (5, 7, 6)) == (3, 594, 330, 1792, (1792 + 3 * 330) * 4)
    assert ws(3, (9, 11, 13), (5, 7, 6)) == (1792 + 3 * 330) * 4
    # the 256-byte floor: one pass has no intermediates, two small passes fewer than 64 floats
    assert ws(7, (12, 10), (6, 10)) == 256 and resample_plan_ref(7, (12, 10), (6, 10))[4] == 256
    assert ws(1, (3, 4), (7, 9)) == 256 and ws(4, (5, 5, 5), (5, 5, 5)) == 256
    assert ws(70000, (3, 4), (7, 9)) == (70000 * 27 + 63) // 64 * 64 * 4       # 2-D grow, W first: t1 = 3 x 9 per volume, one chunk
    # the same formula on a spread of shapes, chunked or not
    for N, sp, size in [(1100 * 64, (12, 10), (6, 5)), (9, (200, 300, 64), (100, 150, 64)), (2, (37, 50, 61), (19, 25, 31)),
                        (3, (9, 130, 7), (9, 65, 7)), (6, (64, 64, 300), (32, 150, 600)), (1, (1, 70), (3, 1)), (40, (160, 192, 224), (80, 96, 112))]:
        plan = resample_plan_ref(N, sp, size)
        assert ws(N, sp, size) == plan[4], (N, sp, size, plan)
        assert plan[0] == N or (plan[0] + 1) * (plan[1] + plan[2]) * 4 > RESAMPLE_CHUNK_BYTES
