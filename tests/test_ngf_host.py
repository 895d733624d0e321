"""Normalised gradient field criterion without a GPU: the adjoint formula the backward kernel implements, the criterion's properties on the CPU
restatement (tests/ngf_ref.py), the CPU reference loop the GPU loop tests are measured against, the C ABI's refusals and the Python surface."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import affine_flow_ref as fr
import bspline_bending_ref as bref
import bspline_ref
import jacobian_ref as jr
import loop_arbiters as la
import ngf_ref
import phantoms as ph
import test_affine_mi_grids_host as ghost
import torchregister_amd as tr

NGFLoss = tr.NGFLoss      # every test of this file (and of tests/test_gpu_ngf.py, which imports it) needs the criterion to exist

OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5
VOXEL = (3.0, 0.7, 0.7)


def multimodal(shape, B=1):
    """The pair of tests/test_gpu_mi.py::_multimodal: a blob phantom; the same phantom warped by a small flow and sent through 4x(1 - x)."""
    from oracle import compose
    tgt = torch.cat([ph.blobs(shape, 3 + b) for b in range(B)])
    flow = ph.flow_field(shape, amp=1.2, f=0.013).expand(B, -1, *shape)
    w = compose.flow_warp(tgt, flow)
    return (4.0 * w * (1.0 - w)).float(), tgt


def random_pair(shape, B=2, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.rand((B, 1) + tuple(shape), generator=g), torch.rand((B, 1) + tuple(shape), generator=g)


def random_mask(shape, B=2, seed=0):
    g = torch.Generator().manual_seed(200 + seed)
    m = torch.rand((B, 1) + tuple(shape), generator=g) < 0.6
    m.reshape(B, -1)[:, 0] = True       # never empty
    return m


def stencil_reach(mask):
    """The mask and the face neighbours of its voxels: where grad_warped of a masked call can be non-zero (warped(y) enters the difference at y +- e_a)."""
    out = mask.clone()
    for d in range(2, mask.dim()):
        n = mask.shape[d]
        out.narrow(d, 1, n - 1).logical_or_(mask.narrow(d, 0, n - 1))
        out.narrow(d, 0, n - 1).logical_or_(mask.narrow(d, 1, n - 1))
    return out


def autograd_grad(tgt, wrp, eps, voxel, mask, alpha, dtype=torch.float64):
    w = wrp.to(dtype).clone().requires_grad_()       # (the leaf in `dtype`: autograd rounds a gradient to its leaf's type)
    loss = ngf_ref.loss(tgt, w, eps, voxel, mask, alpha, dtype)
    (g,) = torch.autograd.grad(loss.sum(), w)
    return loss.detach(), g


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the adjoint formula
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["plain", "voxel", "mask"])
@pytest.mark.parametrize("shape", [(1, 1, 5), (2, 3, 4), (1, 9, 7), (3, 1, 6), (5, 6, 7), (2, 2), (1, 8)], ids=lambda s: "x".join(map(str, s)))
def test_gather_formula_is_the_adjoint(shape, variant):
    """-(alpha / N_m) D^T q written out voxel by voxel equals autograd of the restatement in fp64 to 1e-10 of max|grad|: the face terms, the extent-1
    axes (no term) and the extent-2 axes (both voxels one-sided) are the ones the kernel must reproduce."""
    tgt, wrp = random_pair(shape, seed=len(shape) + sum(shape))
    eps = torch.tensor([[0.3, 0.2], [0.05, 0.4]])
    voxel = VOXEL[-len(shape):] if variant == "voxel" else None
    mask = random_mask(shape) if variant == "mask" else None
    _, g = autograd_grad(tgt, wrp, eps, voxel, mask, 2.5)
    got = ngf_ref.grad_closed_form(tgt, wrp, eps, voxel, mask, 2.5)
    scale = g.abs().max().item()
    assert scale > 0
    assert np.max(np.abs(got - g.numpy())) <= 1e-10 * scale
    if mask is not None:       # q is 0 outside the mask, so D^T q is 0 wherever no stencil neighbour lies inside it: outside the mask's one-voxel rim
        assert np.all(got[~stencil_reach(mask).numpy()] == 0)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. properties of the criterion
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(12, 14, 16), (24, 28)], ids=["3d", "2d"])
def test_contrast_inversion_and_affine_intensity_maps_cost_nothing(shape):
    mov, tgt = multimodal(shape)
    eps = ngf_ref.fit_eps(tgt, mov).double()
    base = ngf_ref.loss(tgt, mov.double(), eps)
    assert 0.0 < base.item() < 1.0
    assert abs(ngf_ref.loss(tgt, 1.0 - mov.double(), eps).item() - base.item()) <= 1e-12
    for c, d in ((-3.0, 0.25), (0.5, -2.0), (7.0, 0.0)):
        e = eps.clone()
        e[:, 1] *= abs(c)
        assert abs(ngf_ref.loss(tgt, c * mov.double() + d, e).item() - base.item()) <= 1e-12, (c, d)
    refit = ngf_ref.fit_eps(tgt, 1.0 - mov)        # a fitted eps_w follows the map by itself
    assert torch.allclose(refit, eps.float(), rtol=1e-5)


def test_the_loss_lies_between_zero_and_alpha():
    for seed, shape in enumerate([(5, 6, 7), (13, 17), (1, 9, 7)]):
        tgt, wrp = random_pair(shape, seed=seed)
        eps = ngf_ref.fit_eps(tgt, wrp, eta=0.5)
        for alpha in (1.0, 2.5):
            loss = ngf_ref.loss(tgt, wrp, eps, alpha=alpha)
            assert bool((loss >= 0).all()) and bool((loss <= alpha).all())
    tgt, _ = random_pair((5, 6, 7))
    assert ngf_ref.loss(tgt, tgt, torch.zeros(2, 2)).abs().max().item() <= 1e-12       # an image against itself without eps: r = 1 wherever it has an edge


def test_a_constant_image_is_defined():
    """Fitted eps of a constant image is 0, its gradient field is 0: a b == 0 everywhere, r = 0 by the select, loss == alpha, gradient 0, no NaN."""
    tgt, _ = random_pair((5, 6, 7))
    const = torch.full_like(tgt, 0.37)
    eps = ngf_ref.fit_eps(tgt, const)
    assert bool((eps[:, 1] == 0).all()) and bool((eps[:, 0] > 0).all())
    for dtype in (torch.float64, torch.float32):
        loss, g = autograd_grad(tgt, const, eps, None, None, 2.5, dtype)
        assert bool((loss == 2.5).all()) and bool((g == 0).all())
    loss, g = autograd_grad(const, const, ngf_ref.fit_eps(const, const), None, None, 1.0)
    assert bool((loss == 1.0).all()) and bool((g == 0).all())
    assert np.all(ngf_ref.grad_closed_form(tgt, const, eps) == 0)
    empty = torch.zeros_like(tgt, dtype=torch.bool)
    loss, g = autograd_grad(tgt, tgt.flip(-1), eps + 0.1, None, empty, 1.0)
    assert bool((loss == 0).all()) and bool((g == 0).all())       # N_m == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. the reference loop on the CPU (shared with tests/test_gpu_ngf.py)
# ---------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def single_thread():
    """torch's CPU kernels on one thread: a reduction's order, and with it the last bits of an fp32 run, must not depend on the host's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def arbiter(*args, **kw):
    """_arbiter on one thread (see single_thread)."""
    with single_thread():
        return _arbiter(*args, **kw)


def _arbiter(mov, tgt, eps, iters, optimizer, lr, dtype, spacing, ctrl0, base=None, lam=0.0, mask=None, voxel=None, alpha=1.0, theta=None, scale=None,
            fold=0.0, fold_eps=0.3, stop_crit=None):
    """bspline_ref.expand + oracle/compose.py::flow_warp (theta given: affine_flow_ref.warp, one interpolation through the affine) + ngf_ref.loss
    (+ bending energy, + folding penalty) under torch autograd + torch.optim on the CPU.  Returns (losses, final control tensor); with stop_crit the
    loop ends behind the iteration whose loss is <= stop_crit, as the device loop does."""
    from oracle import compose
    sp = tuple(tgt.shape[2:])
    mov, tgt = mov.to(dtype), tgt.to(dtype)
    p = ctrl0.to(dtype).clone().requires_grad_()
    opt = torch.optim.SGD([p], lr) if optimizer == "sgd" else torch.optim.Adam([p], lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        flow = bspline_ref.expand(p, sp, spacing, base=None if base is None else base.to(dtype), dtype=dtype)
        warped = compose.flow_warp(mov, flow) if theta is None else fr.warp(mov, theta, flow, scale, dtype)
        e = ngf_ref.loss(tgt, warped, eps, voxel, mask, alpha, dtype).sum()
        if lam:
            e = e + lam * bref.energy_squares(p, sp, spacing, dtype=dtype).sum()
        if fold:
            e = e + fold * jr.penalty(flow, fold_eps).sum()
        e.backward()
        opt.step()
        losses.append(e.item())
        if stop_crit is not None and losses[-1] <= stop_crit:
            break
    return np.asarray(losses), p.detach().numpy()


LOOPS = {"adam": ((12, 14, 16), 4, "adam", 0.1), "sgd": ((12, 14, 16), 4, "sgd", 10.0), "2d-adam": ((24, 28), 5, "adam", 0.1),
         "2d-sgd": ((24, 28), 5, "sgd", 10.0)}
ITERS = 10


def ctrl0(shape, spacing, B=1):
    return la.bspline_ctrl0(B, shape, spacing, 7, amp=0.2)


@functools.lru_cache(maxsize=None)
def arbiter_pair(name, with_base=False, lam=0.0, masked=False, fold=0.0, fold_eps=0.3):
    """(mov, tgt, eps, ctrl0, base, mask, r64, r32) of a LOOPS row, computed once per process."""
    shape, spacing, optimizer, lr = LOOPS[name]
    mov, tgt = multimodal(shape)
    mask = None
    if masked:
        idx = torch.meshgrid(*[torch.arange(s, dtype=torch.float32) - (s - 1) / 2 for s in shape], indexing="ij")
        mask = (sum((i / (0.42 * s)) ** 2 for i, s in zip(idx, shape)) <= 1.0)[None, None]
    eps = ngf_ref.fit_eps(tgt, mov, mask=mask)
    p0 = ctrl0(shape, spacing)
    base = 0.3 * ph.flow_field(shape, 1.0, 0.05) if with_base else None
    kw = dict(spacing=spacing, ctrl0=p0, base=base, lam=lam, mask=mask, fold=fold, fold_eps=fold_eps)
    r64 = arbiter(mov, tgt, eps, ITERS, optimizer, lr, torch.float64, **kw)
    r32 = arbiter(mov, tgt, eps, ITERS, optimizer, lr, torch.float32, **kw)
    return mov, tgt, eps, p0, base, mask, r64, r32


@pytest.mark.parametrize("name", list(LOOPS))
def test_reference_loop_descends_and_its_precisions_stay_together(name):
    """What keeps the GPU bars (4 x the arbiter's own fp32-fp64 gap, with floors) meaningful: the loss falls in every iteration, and the fp32 and fp64
    runs of the arbiter stay together - loss gap <= 5e-8, control gap <= 3e-6.  The arbiter runs on one thread and the restatement adds its voxels in
    fp64, so no reduction's order depends on the host.  Seen on two hosts: loss gap 2.68e-8 / 2.74e-8 / 3.06e-8 / 3.44e-8 and 2.68e-8 / 2.74e-8 /
    4.26e-8 / 3.27e-8 (adam, sgd, 2d-adam, 2d-sgd); control gap 8.3e-8 .. 2.6e-6 on both.  What still differs between hosts is the fp32 matrix
    products of bspline_ref.expand and grid_sample, whose kernels a torch build picks by instruction set; 5e-8 is less than one fp32 ulp of a loss of
    0.8, so the margin is thin (15 % at its narrowest) and the bound is kept as stated."""
    *_, (l64, p64), (l32, p32) = arbiter_pair(name)
    lgap, pgap = np.max(np.abs(l32 - l64)), np.max(np.abs(p32 - p64))
    print(f"{name}: loss {l64[0]:.6f} -> {l64[-1]:.6f}, fp32-fp64 loss gap {lgap:.2e}, control gap {pgap:.2e}")
    assert np.all(np.diff(l64) < 0) and np.all(np.diff(l32) < 0)
    assert lgap <= 5e-8 and pgap <= 3e-6


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def ngf_cfg(_lib, alpha=1.0, eps=4096, voxel=None, mask=None):
    c = _lib.NGFCfg()
    c.alpha, c.eps, c.mask = alpha, eps, mask
    c._voxel = None if voxel is None else (ctypes.c_float * len(voxel))(*voxel)       # kept alive with the struct
    c.voxel = None if voxel is None else ctypes.cast(c._voxel, ctypes.POINTER(ctypes.c_float))
    return c


def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ptr = lambda p: P(p) if p else None  # noqa: E731
    inf, nan = float("inf"), float("nan")
    assert lib.trx_version() == 240

    q = lib.trx_ngf_workspace_bytes
    n = q(3, 2, 5, 6, 7)
    assert n == -(-2 * 3 * 210 * 4 // 256) * 256 + 3 * 256      # q, then the partials, the counts and the scales of 2 pairs x 1 chunk: 256 bytes each
    assert q(2, 1, 1, 13, 17) > 0
    for bad in ((1, 1, 5, 6, 7), (4, 1, 5, 6, 7), (2, 1, 5, 6, 7), (3, 0, 5, 6, 7), (3, 65536, 5, 6, 7), (3, 1, 0, 6, 7), (3, 1, 5, -1, 7), (3, 1, 5, 6, 0),
                (3, 1, 2048, 1024, 1024)):
        assert q(*bad) == 0, bad

    def call(t=4096, w=4096, ndim=3, B=2, dhw=(5, 6, 7), cfg=ngf_cfg(_lib), loss=4096, grad=4096, ws=4096, nbytes=n):
        return lib.trx_ngf_loss_grad(ptr(t), ptr(w), ndim, B, *dhw, ref(cfg), ptr(loss), ptr(grad), ptr(ws), nbytes, None)

    assert call(t=None) == ARG and call(w=None) == ARG and call(cfg=None) == ARG and call(loss=None) == ARG and call(ws=None) == ARG
    assert call(cfg=ngf_cfg(_lib, eps=None)) == ARG
    for bad, want in ((dict(ndim=1), NDIM), (dict(ndim=4), NDIM), (dict(ndim=2), NDIM), (dict(B=0), ARG), (dict(B=65536), ARG), (dict(dhw=(0, 6, 7)), ARG),
                      (dict(dhw=(5, 6, 0)), ARG), (dict(dhw=(2048, 1024, 1024)), ARG)):
        assert call(**bad) == want, bad
    for alpha in (nan, inf, -inf):
        assert call(cfg=ngf_cfg(_lib, alpha=alpha)) == ARG
    for voxel in ((0.0, 1.0, 1.0), (1.0, -2.0, 1.0), (1.0, 1.0, nan), (inf, 1.0, 1.0)):
        assert call(cfg=ngf_cfg(_lib, voxel=voxel)) == ARG, voxel
    assert call(nbytes=n - 1) == WS and call(nbytes=0) == WS
    assert call(grad=None, nbytes=n - 1) == WS and call(cfg=ngf_cfg(_lib, voxel=VOXEL, mask=4096, alpha=-2.0), nbytes=n - 1) == WS      # good arguments get as far as the workspace check
    assert call(ndim=2, B=1, dhw=(1, 13, 17), cfg=ngf_cfg(_lib, voxel=(0.7, 0.7)), nbytes=q(2, 1, 1, 13, 17) - 1) == WS

    # the loop
    vol, d3 = ghost._vol(_lib, B=1), (ctypes.c_int * 3)(4, 4, 4)
    opt = _lib.OptCfg(_lib.OPT_ADAM, 0.1, 0.9, 0.999, 1e-8)
    qb = lib.trx_bspline_ngf_workspace_bytes
    nb = qb(3, 1, 12, 14, 16, 4, 4, 4, None)
    grid = ghost._grid(_lib)
    assert nb > lib.trx_bspline_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4) + q(3, 1, 12, 14, 16) + lib.trx_flow_folding_workspace_bytes(3, 1, 12, 14, 16)
    assert qb(3, 1, 12, 14, 16, 4, 4, 4, ref(grid)) == nb
    assert qb(3, 1, 12, 14, 16, 0, 4, 4, None) == 0 and qb(2, 1, 2, 14, 16, 4, 4, 4, None) == 0 and qb(3, 0, 12, 14, 16, 4, 4, 4, None) == 0
    over, mmask = ghost._grid(_lib), ghost._grid(_lib)
    over.overlap, mmask.mask = 1, 4096
    assert qb(3, 1, 12, 14, 16, 4, 4, 4, ref(over)) == 0 and qb(3, 1, 12, 14, 16, 4, 4, 4, ref(mmask)) == 0

    def state(**kw):
        st = _lib.BSplineState()
        for f in ("ctrl", "adam_m", "adam_v", "flow", "dflow", "losses", "step"):
            setattr(st, f, 4096)
        st.losses_capacity, st.bending_weight = 5, 0.0
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def run(v=vol, g=None, theta=None, c=ngf_cfg(_lib), o=opt, st=state(), sp=d3, f=None, iters=1, ws=4096, nbytes=nb):
        return lib.trx_bspline_ngf_run(ref(v), ref(g), ptr(theta), ref(c), ref(o), ref(st), sp, ref(f), iters, ptr(ws), nbytes, None)

    assert run(v=None) == ARG and run(c=None) == ARG and run(o=None) == ARG and run(st=None) == ARG and run(sp=None) == ARG and run(ws=None) == ARG
    assert run(c=ngf_cfg(_lib, eps=None)) == ARG and run(c=ngf_cfg(_lib, alpha=nan)) == ARG and run(c=ngf_cfg(_lib, voxel=(1.0, 0.0, 1.0))) == ARG
    assert run(iters=-1) == ARG and run(st=state(ctrl=None)) == ARG and run(st=state(adam_m=None)) == ARG and run(st=state(bending_weight=-1.0)) == ARG
    assert run(v=ghost._vol(_lib, ndim=4, B=1)) == NDIM and run(v=ghost._vol(_lib, B=0)) == ARG and run(sp=(ctypes.c_int * 3)(0, 4, 4)) == ARG
    assert run(g=grid) == ARG and run(theta=4096) == ARG      # one lattice: both NULL; two lattices: both given
    assert run(g=over, theta=4096) == ARG and run(g=mmask, theta=4096) == ARG and run(g=ghost._grid(_lib, (0, 13, 18)), theta=4096) == ARG
    for f in (_lib.FoldCfg(nan, 0.3), _lib.FoldCfg(inf, 0.3), _lib.FoldCfg(-1.0, 0.3), _lib.FoldCfg(1.0, nan)):
        assert run(f=f) == ARG, (f.weight, f.threshold)
    for kw in (dict(), dict(f=_lib.FoldCfg(0.0, 0.3)), dict(f=_lib.FoldCfg(1.0, 0.3)), dict(g=grid, theta=4096), dict(c=ngf_cfg(_lib, voxel=VOXEL, mask=4096))):
        assert run(nbytes=nb - 1, **kw) == WS and run(iters=6, **kw) == CAP       # good arguments get as far as the workspace check and the capacity


def test_c_abi_refusals_without_a_device():
    check_refusals()


def test_the_abi_grew_by_new_names_only():
    from torchregister_amd import _lib
    assert [f[0] for f in _lib.NGFCfg._fields_] == ["alpha", "eps", "voxel", "mask"] and ctypes.sizeof(_lib.NGFCfg) == 32
    assert [f[0] for f in _lib.BSplineState._fields_][-1] == "bending_weight"
    for name in ("trx_ngf_workspace_bytes", "trx_ngf_loss_grad", "trx_bspline_ngf_workspace_bytes", "trx_bspline_ngf_run"):
        assert name in _lib.SIGNATURES


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. the Python surface
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_register_takes_ngfloss_alone_and_refuses_what_is_not_built():
    kw = dict(criterion=[NGFLoss()], weight=[1.0], flow_model="bspline", spacing=4)
    reg = tr.Register("flow", **kw)
    assert reg.flow_model == "bspline" and reg._ngf_alone()
    with pytest.raises(ValueError, match="diffeomorphic"):
        tr.Register("flow", diffeomorphic=True, **kw)
    mov, tgt = multimodal((12, 14, 16))
    theta = torch.eye(3, 4)[None]
    with pytest.raises(ValueError):
        reg.optim(mov, tgt, lr=0.1, max_epochs=2, overlap=True)
    with pytest.raises(ValueError):
        reg.optim(mov, tgt, lr=0.1, max_epochs=2, initial=theta, overlap=True)
    with pytest.raises(ValueError):
        reg.optim(mov, tgt, lr=0.1, max_epochs=2, initial=theta, moving_mask=torch.ones_like(mov))
    fr_ = tr.flow_register((12, 14, 16), criterions=[NGFLoss(alpha=2.0)], weights=[0.5], flow_model="bspline", spacing=4)
    assert fr_.ngf_alone() and fr_.mask_supported(3) and fr_.mask_supported(2) and fr_.initial_supported()
    with pytest.raises(ValueError):
        fr_.optimize(mov, tgt, overlap=True)
    with pytest.raises(ValueError, match="diffeomorphic"):
        tr.flow_register((12, 14, 16), criterions=[NGFLoss()], weights=[1.0], flow_model="bspline", diffeomorphic=True)
    with pytest.raises(ValueError):       # a mixed list is not a fused route of the lattice
        tr.flow_register((12, 14, 16), criterions=[NGFLoss(), tr.NCCLoss()], weights=[1.0, 1.0], flow_model="bspline")
    generic = tr.flow_register((12, 14, 16), criterions=[NGFLoss()], weights=[1.0], flow_model="direct")
    assert not generic.ngf_alone() and not generic.mask_supported(3) and not generic.initial_supported()


def test_a_pyramid_level_gets_its_own_voxel_sizes():
    """Register(levels=L) hands a level a copy of an NGFLoss with the level's voxel sizes, v S / S_l per axis; nothing else of the list changes."""
    ncc = tr.NCCLoss()
    reg = tr.Register("flow", criterion=[NGFLoss(eta=0.5, alpha=2.0, voxel=VOXEL, moving_eps=0.1), ncc], weight=[1.0, 1.0], flow_model="direct", levels=2)
    got = reg._level_criteria((24, 28, 32), (12, 14, 8))
    assert got[1] is ncc and got[0].settings() == dict(eta=0.5, alpha=2.0, voxel=(6.0, 1.4, 2.8), target_eps=None, moving_eps=0.1)
    assert reg._level_criteria((24, 28, 32), (24, 28, 32))[0].voxel == VOXEL and reg.criterion[0].voxel == VOXEL
    plain = tr.Register("flow", criterion=[NGFLoss()], weight=[1.0], flow_model="bspline", spacing=4, levels=2)
    assert plain._level_criteria((24, 28, 32), (12, 14, 16))[0] is plain.criterion[0]


def test_ngfloss_settings_and_edge_parameters():
    c = NGFLoss(eta=0.5, alpha=2.0, voxel=VOXEL, moving_eps=0.1)
    assert c.settings(0.25) == dict(eta=0.5, alpha=0.5, voxel=VOXEL, target_eps=None, moving_eps=0.1)
    for bad in (dict(voxel=(1.0, 0.0, 1.0)), dict(voxel=(1.0, float("nan"))), dict(eta=-1.0), dict(target_eps=-0.1)):
        with pytest.raises(ValueError):
            NGFLoss(**bad)
    mov, tgt = multimodal((12, 14, 16), B=2)
    mask = torch.zeros_like(tgt, dtype=torch.bool)
    mask[0, :, 2:9, 3:10, 4:12] = True       # pair 1: empty - the whole image
    for kw in (dict(), dict(eta=0.5, voxel=VOXEL), dict(mask=mask)):
        got = tr.ngf_edge_parameters(tgt, mov, **kw)
        want = ngf_ref.fit_eps(tgt, mov, **kw)
        assert got.shape == (2, 2) and torch.allclose(got, want, rtol=1e-6, atol=0), kw
    assert bool((tr.ngf_edge_parameters(tgt, torch.full_like(mov, 0.5))[:, 1] == 0).all())
    assert torch.equal(tr._engine.ngf_gradient(tgt, VOXEL), ngf_ref.differences(tgt, VOXEL, torch.float32))
    eps = tr._engine.ngf_settings_eps(c.settings(), tgt, mov, VOXEL, None)
    assert bool((eps[:, 1] == 0.1).all()) and torch.allclose(eps[:, 0], 0.5 * ngf_ref.fit_eps(tgt, mov, voxel=VOXEL)[:, 0], rtol=1e-6)
    from torchregister_amd import _lib
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        NGFLoss()(tgt, mov)
    with pytest.raises(ValueError):
        tr.BSplineSolver(mov, tgt, 4, ngf=dict(bins=32))
    for kw in (dict(mi=dict(bins=32)), dict(loss=tr.LossSpec(w_mse=1.0)), dict(squarings=4), dict(overlap=True), dict(moving_mask=torch.ones_like(mov))):
        with pytest.raises(ValueError):
            tr.BSplineSolver(mov, tgt, 4, ngf=dict(), **kw)
