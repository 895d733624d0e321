"""CPU-only checks of points and target-space images through the whole transform: the restatement of tests/chain_ref.py against
independent forms, every refusal of the two C entry points without a device, the Python interface on CPU tensors, invert_theta and the world helpers,
and the conditions tests/test_gpu_chain.py relies on (how many voxels the comparisons leave out)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import chain_ref as cr
import flowops_ref as fr
import spline_ref as sr
import svf_ref

OK, ARG, NDIM = 0, -1, -2


# ---------------------------------------------------------------------------------------------------------------------------------------
# the restatement against independent forms
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["a", "c", "d"])
def test_sampler_is_the_flow_operators(case):
    """sample_at at the positions x + u(x) is flowops_ref.sample_border bit for bit and svf_ref.sample to rounding, in both dtypes."""
    for dtype in (torch.float32, torch.float64):
        f, u = fr.field(case).to(dtype), fr.second_field(case).to(dtype) * 3.0      # amplitude 3: part of the positions leave the volume
        B, nd = u.shape[:2]
        p = (svf_ref.identity(u.shape[2:], dtype) + u).reshape(B, nd, -1).transpose(1, 2)
        for padding, want in (("border", fr.sample_border(f, u)), ("zeros", svf_ref.sample(f, u))):
            got = cr.sample_at(f, p, padding).transpose(1, 2).reshape(f.shape)
            if padding == "border":
                assert torch.equal(got, want), (case, dtype)
            else:      # svf_ref multiplies the corner's factors in another order ((z y) x against the kernels' (y x) z): roundings apart
                assert (got - want).abs().max().item() <= 4 * torch.finfo(dtype).eps * f.abs().max().item(), (case, dtype)


@pytest.mark.parametrize("name", ["composed", "2d", "theta"])
def test_chain0_at_lattice_points_is_the_composed_warp(name):
    """Chain 0 at the voxels of the target lattice gives spline_ref.positions, the positions trx_affine_flow_warp samples at."""
    x, theta, flow = sr.case(name)
    tshape, mshape = sr.CASES[name][:2]
    want = sr.positions(mshape, theta, flow, None, size=tshape)
    got = cr.chain(cr.lattice_points(tshape, 2), theta, flow, tshape, mshape, 0).flip(-1).reshape(want.shape)
    assert (got - want).abs().max().item() <= 1e-12 * max(mshape)


@pytest.mark.parametrize("name", ["9x11x13", "2d", "1x12x20"])
def test_chain1_without_flow_is_affine_grid(name):
    out_shape, src_shape = cr.CASES[name][:2]
    _, theta, _ = cr.case(name)
    grid = F.affine_grid(theta.double(), (2, 1) + out_shape, align_corners=False)
    want = ((grid + 1.0) * torch.tensor(src_shape[::-1], dtype=torch.float64) - 1.0) / 2.0
    got = cr.image_positions(theta, None, out_shape, src_shape)
    assert (got - want).abs().max().item() <= 1e-12 * max(src_shape)


def _hom(theta):
    nd = theta.shape[-2]
    H = torch.eye(nd + 1, dtype=torch.float64).repeat(theta.shape[0], 1, 1)
    H[:, :nd] = theta.double()
    return H


def test_constant_flow_has_a_closed_form_and_the_round_trip_is_the_identity():
    """With a constant flow c and an affine both chains are closed forms; chain1(invert_theta(theta), -c) o chain0(theta, c) is the identity."""
    import torchregister_amd as tr
    Sa, Sb = (9, 11, 13), (12, 10, 7)
    theta = cr.thetas(3, torch.Generator().manual_seed(1))
    c = torch.tensor([1.25, -2.5, 0.75], dtype=torch.float64)
    p = cr.points_for(Sa, 200, 3).double()
    flow_a = c[None, :, None, None, None].expand((2, 3) + Sa)
    flow_b = c[None, :, None, None, None].expand((2, 3) + Sb)

    def affine(q, S_from, S_to, th):
        n = (2.0 * q + 1.0) / torch.tensor(S_from, dtype=torch.float64) - 1.0
        m = torch.einsum("brk,bpk->bpr", th.double(), torch.cat([n.flip(-1), torch.ones_like(n[..., :1])], -1))
        return ((m.flip(-1) + 1.0) * torch.tensor(S_to, dtype=torch.float64) - 1.0) / 2.0

    assert (cr.chain(p, theta, flow_a, Sa, Sb, 0) - affine(p + c, Sa, Sb, theta)).abs().max().item() <= 1e-12 * 13
    assert (cr.chain(p, theta, flow_b, Sa, Sb, 1) - (affine(p, Sa, Sb, theta) + c)).abs().max().item() <= 1e-12 * 13
    inv = tr.invert_theta(theta)
    back = cr.chain(cr.chain(p, theta, flow_a, Sa, Sb, 0), inv, -flow_a, Sb, Sa, 1)
    err = (back - p).abs().max().item()
    print(f"round trip through a constant flow and an affine: {err:.2e} voxels")
    assert err <= 1e-12 * 13
    # theta None / flow None: the missing piece is the identity
    assert torch.equal(cr.chain(p, None, flow_a, Sa, Sa, 0), p + c) and torch.equal(cr.chain(p, None, flow_a, Sa, Sa, 1), p + c)
    assert torch.equal(cr.chain(p, theta, None, Sa, Sb, 0), cr.chain(p, theta, None, Sa, Sb, 1))


def test_a_non_finite_point_gives_nan_and_touches_no_neighbour():
    Sa, Sb = (9, 11, 13), (12, 10, 7)
    theta = cr.thetas(3, torch.Generator().manual_seed(1))
    flow = cr.smooth_flow(Sa, 1.0, torch.Generator().manual_seed(2))
    clean = cr.points_for(Sa, 65, 5)
    p = cr.points_for(Sa, 65, 5, nan_at=17)
    p[1, 3, 0] = float("inf")
    for dtype in (torch.float32, torch.float64):
        out, ref = cr.chain(p, theta, flow, Sa, Sb, 0, dtype=dtype), cr.chain(clean, theta, flow, Sa, Sb, 0, dtype=dtype)
        bad = torch.isnan(out).all(-1)
        assert torch.equal(torch.isnan(out).any(-1), bad) and int(bad.sum()) == 2 and bool(bad[0, 17]) and bool(bad[1, 3])
        assert torch.equal(out[~bad], ref[~bad])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the conditions the GPU tests rely on
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cr.CASES))
def test_the_comparisons_leave_out_at_most_one_percent(name):
    """spline_ref.kept (eps 1e-4) on the restatement alone: a continuous position field is that close to a face or a rounding tie at about 2 nd eps =
    6e-4 of the voxels.  Also: between 5 % and 50 % of every case samples outside the field of view, so the zero padding is exercised."""
    out_shape, src_shape = cr.CASES[name][:2]
    _, theta, flow = cr.case(name)
    for padding in ("border", "zeros"):
        pos = cr.image_positions(theta, flow, out_shape, src_shape, padding)
        drop = 1.0 - sr.kept(pos, src_shape).double().mean().item()
        drop_n = 1.0 - sr.kept(pos, src_shape, nearest=True).double().mean().item()
        outside = sr.outside(pos, src_shape).double().mean().item()
        print(f"{name} {padding}: kept removes {100 * drop:.3f} % (linear, cubic) and {100 * drop_n:.3f} % (nearest); {100 * outside:.1f} % outside the field of view")
        assert drop <= 0.01 and drop_n <= 0.01
        assert 0.05 <= outside <= 0.5
        if flow is None:
            break


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ptr = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
    size = lambda s: None if s is None else (ctypes.c_int * 3)(*s)  # noqa: E731
    MB = 1 << 20

    def pts(points=MB, out=2 * MB, ndim=3, B=1, P=10, theta=3 * MB, flow=4 * MB, frm=(5, 6, 7), to=(5, 6, 7), chain=0, padding=1):
        return lib.trx_transform_points(ptr(points), ptr(out), ndim, B, P, ptr(theta), ptr(flow), size(frm), size(to), chain, padding, None)

    def img(src=MB, stride=None, ssize=(5, 6, 7), theta=3 * MB, flow=4 * MB, ndim=3, B=1, channels=2, osize=(4, 5, 6), order=1, padding=1, out=8 * MB):
        n = ssize[0] * ssize[1] * ssize[2] * channels if ssize is not None and stride is None else (stride or 0)
        return lib.trx_affine_then_flow_resample(ptr(src), max(n, 0), size(ssize), ptr(theta), ptr(flow), ndim, B, channels, size(osize), order, padding, ptr(out), None)

    # NULLs
    assert pts(points=None) == ARG and pts(out=None) == ARG and pts(theta=None, flow=None) == ARG and pts(frm=None) == ARG and pts(to=None) == ARG
    assert pts(to=None, chain=1) == ARG and pts(to=None, theta=None, chain=1) == ARG
    assert img(src=None) == ARG and img(out=None) == ARG and img(theta=None, flow=None) == ARG and img(ssize=None, stride=420) == ARG and img(osize=None) == ARG
    # theta NULL: unequal lattices
    assert pts(theta=None, chain=1, to=(5, 6, 8)) == ARG and img(theta=None) == ARG
    # ndim, first of all
    for bad in (0, 1, 4, -3):
        assert pts(ndim=bad) == NDIM and img(ndim=bad) == NDIM
    assert pts(ndim=5, points=None, chain=9) == NDIM and img(ndim=5, src=None, order=7) == NDIM
    assert pts(ndim=2) == NDIM and pts(ndim=2, frm=(1, 6, 7)) == NDIM and img(ndim=2) == NDIM and img(ndim=2, ssize=(1, 6, 7), stride=84) == NDIM
    # sizes
    for bad in ((0, 6, 7), (5, -1, 7), (5, 6, 0), (2048, 1024, 1024)):
        assert pts(frm=bad) == ARG and pts(to=bad) == ARG, bad
        assert img(osize=bad) == ARG, bad
    for bad in ((0, 6, 7), (5, -1, 7), (5, 6, 0)):
        assert img(ssize=bad, stride=420) == ARG, bad
    assert img(ssize=(2048, 1024, 1024), stride=1 << 32) == ARG
    for bad in (0, -1, 65536):
        assert pts(B=bad) == ARG and img(B=bad) == ARG, bad
    for bad in (0, -5):
        assert pts(P=bad) == ARG and img(channels=bad) == ARG
    assert img(stride=419) == ARG      # fewer elements between pairs than a pair's channels hold
    # enums
    for bad in (-1, 2, 3):
        assert pts(padding=bad) == ARG and img(padding=bad) == ARG and pts(chain=bad) == ARG, bad
    for bad in (-1, 2, 4, 5):
        assert img(order=bad) == ARG, bad
    # overlap: out inside src / flow; out against points only when it is not points itself
    assert img(out=MB) == ARG and img(out=MB + 16) == ARG and img(out=4 * MB) == ARG and img(out=4 * MB + 2516) == ARG
    assert img(out=MB - 4 * 2 * 120 + 4) == ARG      # out's last float is src's first
    assert pts(out=MB + 4) == ARG and pts(out=4 * MB) == ARG and pts(out=4 * MB + 2516) == ARG


def test_c_abi_refusals_without_a_device():
    check_refusals()


def test_lib_signatures():
    from torchregister_amd import _lib
    lib = _lib.load()
    P, I, Z, IP = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int)
    assert _lib.SIGNATURES["trx_transform_points"] == (I, [P, P, I, I, I, P, P, IP, IP, I, I, P])
    assert _lib.SIGNATURES["trx_affine_then_flow_resample"] == (I, [P, Z, IP, P, P, I, I, I, IP, I, I, P, P])
    assert lib.trx_transform_points.restype is I and lib.trx_affine_then_flow_resample.restype is I
    assert lib.trx_version() == 240


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python interface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_invert_theta():
    import torchregister_amd as tr
    for nd, seed in ((3, 1), (2, 2)):
        theta = cr.thetas(nd, torch.Generator().manual_seed(seed))
        inv = tr.invert_theta(theta)
        assert inv.dtype == torch.float64 and tuple(inv.shape) == (2, nd, nd + 1)
        assert torch.equal(inv, torch.linalg.inv(_hom(theta))[:, :nd])
        assert (_hom(inv) @ _hom(theta) - torch.eye(nd + 1, dtype=torch.float64)).abs().max().item() <= 1e-14
        assert torch.allclose(tr.invert_theta(theta[0]), inv[0], rtol=0, atol=1e-15)
    eye = torch.eye(3, 4)[None]
    for bad in (eye * 0, eye * float("nan"), torch.tensor([[[1.0, 2, 3, 0], [2, 4, 6, 0], [0, 0, 1, 0]]]), eye * float("inf")):
        with pytest.raises(ValueError, match="no inverse"):
            tr.invert_theta(bad)
    for bad in (torch.eye(4), torch.zeros(1, 3, 3), torch.zeros(2, 2, 3, 4), "x", None):
        with pytest.raises(ValueError, match="expected theta"):
            tr.invert_theta(bad)


def test_world_points():
    """points_to_world follows optim's header convention (columns in the tensor's axis order, rows world x, y, z): the world position of voxel (z, y, x)
    under nibabel-style A is A (z, y, x, 1); from_world is its inverse; a TRE in mm is a norm of differences."""
    import torchregister_amd as tr
    A = torch.tensor([[0.0, 0.0, 1.2, -30.0], [0.0, 0.9, 0.0, 12.0], [2.5, 0.0, 0.0, 7.0], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)      # axis-aligned: dz = 2.5, dy = 0.9, dx = 1.2
    p = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    w = tr.points_to_world(p, A)
    assert w.dtype == torch.float64
    assert torch.allclose(w, torch.tensor([[-30.0, 12.0, 7.0], [-30.0, 12.0, 9.5], [-30.0, 12.9, 7.0], [-28.8, 12.0, 7.0]], dtype=torch.float64), atol=1e-12)
    assert torch.allclose((w[1:] - w[0]).norm(dim=-1), torch.tensor([2.5, 0.9, 1.2], dtype=torch.float64), atol=1e-12)
    q = torch.rand(2, 7, 3, generator=torch.Generator().manual_seed(1)) * 20
    Ab = torch.stack([A, A @ torch.diag(torch.tensor([1.0, 2.0, 0.5, 1.0], dtype=torch.float64))])
    assert (tr.points_from_world(tr.points_to_world(q, Ab), Ab) - q.double()).abs().max().item() <= 1e-12
    assert torch.allclose(tr.points_to_world(q, Ab)[1], tr.points_to_world(q[1], Ab[1]), rtol=0, atol=1e-12)
    for bad in (torch.zeros(3), torch.zeros(2, 3, 4), "x"):
        with pytest.raises(ValueError, match="points"):
            tr.points_to_world(bad, A)
    with pytest.raises(ValueError, match="affine"):
        tr.points_to_world(p, torch.zeros(4, 4))


def test_python_refusals_on_cpu_tensors():
    import TorchRegister
    import torchregister_amd as tr
    from torchregister_amd import _lib
    for name in ("transform_points", "resample_affine_then_flow", "invert_theta", "points_to_world", "points_from_world"):
        assert getattr(TorchRegister, name) is getattr(tr, name)
    p, th = torch.zeros(2, 5, 3), torch.eye(3, 4)[None]
    u, x = torch.zeros(2, 3, 4, 5, 6), torch.zeros(2, 2, 4, 5, 6)
    shapes = dict(from_shape=(4, 5, 6), to_shape=(7, 8, 9))
    for bad in ("flow", 0, None):
        with pytest.raises(ValueError, match="chain"):
            tr.transform_points(p, theta=th, chain=bad, **shapes)
    for bad in ("reflect", 1, None):
        with pytest.raises(ValueError, match="padding"):
            tr.transform_points(p, theta=th, padding=bad, **shapes)
        with pytest.raises(ValueError, match="padding"):
            tr.resample_affine_then_flow(x, theta=th, size=(4, 5, 6), padding=bad)
    with pytest.raises(ValueError, match="needs a transform"):
        tr.transform_points(p)
    with pytest.raises(ValueError, match="needs a transform"):
        tr.resample_affine_then_flow(x, size=(4, 5, 6))
    for bad in (torch.zeros(5), torch.zeros(2, 5, 4), torch.zeros(2, 0, 3), torch.zeros(1, 2, 5, 3), "p"):
        with pytest.raises(ValueError, match="points"):
            tr.transform_points(bad, theta=th, **shapes)
    for bad in (torch.eye(3, 4), torch.zeros(3, 3, 4), torch.zeros(1, 2, 3), "t"):
        with pytest.raises(ValueError, match="theta"):
            tr.transform_points(p, theta=bad, **shapes)
        with pytest.raises(ValueError, match="theta"):
            tr.resample_affine_then_flow(x, theta=bad, size=(4, 5, 6))
    for bad in (torch.zeros(3, 3, 4, 5, 6), torch.zeros(2, 2, 4, 5, 6), torch.zeros(2, 3, 5, 6), "f"):
        with pytest.raises(ValueError, match="flow"):
            tr.transform_points(p, flow=bad)
        with pytest.raises(ValueError, match="flow"):
            tr.resample_affine_then_flow(x, flow=bad, size=(4, 5, 6))
    with pytest.raises(ValueError, match="give from_shape and to_shape"):
        tr.transform_points(p, theta=th)
    with pytest.raises(ValueError, match="give from_shape and to_shape"):
        tr.transform_points(p, theta=th, flow=u)      # chain 0: the flow gives from_shape, to_shape is missing
    with pytest.raises(ValueError, match="flow's lattice"):
        tr.transform_points(p, theta=th, flow=u, **shapes, chain="affine_then_flow")      # chain 1: the flow lives on to_shape
    with pytest.raises(ValueError, match="without theta"):
        tr.transform_points(p, flow=u, to_shape=(7, 8, 9))
    with pytest.raises(ValueError, match="positive sizes"):
        tr.transform_points(p, theta=th, from_shape=(4, 5), to_shape=(7, 8, 9))
    with pytest.raises(ValueError, match="interpolation"):
        tr.resample_affine_then_flow(x, theta=th, size=(4, 5, 6), interpolation="spline")
    with pytest.raises(ValueError, match="x's lattice"):
        tr.resample_affine_then_flow(x, theta=th, flow=torch.zeros(2, 3, 4, 5, 7), size=(4, 5, 6))
    with pytest.raises(ValueError, match="without theta"):
        tr.resample_affine_then_flow(x, flow=u, size=(4, 5, 7))
    with pytest.raises(ValueError, match="size"):
        tr.resample_affine_then_flow(x, theta=th, size=(4, 5))
    with pytest.raises(ValueError, match="expected x"):
        tr.resample_affine_then_flow(torch.zeros(4, 5, 6), theta=th, size=(4, 5, 6))
    # good arguments on CPU tensors: the GPU-only refusal
    for fn in (lambda: tr.transform_points(p, theta=th, **shapes), lambda: tr.transform_points(p[0], flow=u[:1]),
               lambda: tr.transform_points(p, theta=th, flow=u, from_shape=(7, 8, 9), chain="affine_then_flow", padding="zeros"),
               lambda: tr.resample_affine_then_flow(x, theta=th, flow=u, size=(7, 8, 9), interpolation="nearest"),
               lambda: tr.resample_affine_then_flow(x, flow=u[:1], size=(4, 5, 6), interpolation="linear")):
        with pytest.raises(_lib.TrxError, match="no CPU fallback"):
            fn()


def test_register_methods_before_and_after_optim_on_the_host():
    import torchregister_amd as tr
    from torchregister_amd import _lib
    p, x = torch.zeros(1, 5, 3), torch.zeros(1, 1, 4, 5, 6)
    for reg in (tr.Register("affine"), tr.Register("flow"), tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0])):
        assert reg.moving_shape is None
        for fn in (lambda: reg.transform_points(p), lambda: reg.transform_points(p, inverse=True), reg.inverse_transform, lambda: reg.to_moving(x)):
            with pytest.raises(RuntimeError, match="optim"):
                fn()
        for bad in (0, 1001, 2.0, True):
            with pytest.raises(ValueError, match="iterations"):
                reg.transform_points(p, inverse=True, iterations=bad)
            with pytest.raises(ValueError, match="iterations"):
                reg.to_moving(x, iterations=bad)
            with pytest.raises(ValueError, match="iterations"):
                reg.inverse_transform(iterations=bad)
        with pytest.raises(ValueError, match="tol"):
            reg.inverse_transform(tol=-1.0)
        with pytest.raises(ValueError, match="interpolation"):
            reg.to_moving(x, interpolation="spline")
    # the state an affine optim leaves: the pieces of the inverse are host arithmetic, the points need the GPU
    reg = tr.Register("affine")
    reg.theta, reg.target_shape, reg.moving_shape = cr.thetas(3, torch.Generator().manual_seed(1))[:1], (4, 5, 6), (7, 8, 9)
    th_inv, fl_inv, res = reg.inverse_transform()
    assert torch.equal(th_inv, tr.invert_theta(reg.theta)) and fl_inv is None and res is None
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        reg.transform_points(p)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        reg.to_moving(x)
    # the state optim(initial=...) leaves: the existing refusal stays, the new methods reach the device
    ffd = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0])
    ffd.theta, ffd.initial, ffd.target_shape, ffd.moving_shape = torch.zeros(1, 3, 4, 5, 6), reg.theta, (4, 5, 6), (7, 8, 9)
    with pytest.raises(ValueError, match="initial"):
        ffd.invert_flow()
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        ffd.transform_points(p)
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        ffd.to_moving(x)
