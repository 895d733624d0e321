"""CPU-only checks of dense-flow composition and fixed-point inversion: what the GPU tests of tests/test_gpu_flowops.py rest on
- the convergence table of the cases, the fold field, the constant field, compose against one squaring, compose(u, invert(u)) - every refusal of the C
ABI without a device, the Python interface on CPU tensors and the ctypes signatures."""
import ctypes

import pytest
import torch

import flowops_ref as fr
import jacobian_ref as jr
import svf_ref

OK, ARG, NDIM = 0, -1, -2


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition and the cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(fr.CASES))
def test_convergence_table(case):
    """At tol = 1e-3 within 30 updates, in fp32: every voxel converges, the slowest one after the table's count; the fp64 right-inverse residual
    |v + Sb(u, y + v)| of the fp32 result has the table's maximum and stays below tol; between 7 % and 100 % of the voxels sample outside the volume, so
    the border rule is exercised; the fixed iteration after 40 updates differs between fp32 and fp64 by at most a fifth of the GPU tests' floor."""
    u = fr.field(case)
    v, r, n = fr.reference(case)["stop32"]
    rr = fr.right_residual(u, v)
    outside = svf_ref.share_outside(v.double())
    v32, v64 = fr.invert(u, 40, 0.0)[0], fr.invert(u.double(), 40, 0.0)[0]
    gap = (v32.double() - v64).abs().max().item()
    slowest, largest = fr.TABLE[case]
    print(f"{case}: slowest voxel {int(n.max())} updates, residual {r.max().item():.3e}, |v + Sb(u, y + v)| {rr.max().item():.3e}, {100 * outside:.0f} % outside, "
          f"fp32 - fp64 after 40 updates {gap:.1e}")
    assert bool((r <= fr.TOL).all()) and bool(torch.isfinite(v).all())
    assert int(n.max()) == slowest and 7 <= slowest <= 12
    assert abs(rr.max().item() - largest) <= 0.02 * largest and rr.max().item() <= fr.TOL
    assert 0.07 <= outside <= 1.0
    assert gap <= 0.2 * 1e-5 * max(1.0, u.abs().max().item())
    assert fr.FIXED_K >= slowest


def test_updates_of_a_voxel_do_not_depend_on_the_others():
    """The per-voxel stop: a pair inverted alone and inside a batch gives the same bits, and the early-stopping result of a voxel is the fixed-count
    result for that voxel's own number of updates."""
    u = fr.field("b")
    v, r, n = fr.reference("b")["stop32"]
    v1, r1, n1 = fr.invert(u[1:])
    assert torch.equal(v1, v[1:]) and torch.equal(r1, r[1:]) and torch.equal(n1, n[1:])
    for k in (int(n.min()), int(n.max())):
        vk = fr.invert(u, k, 0.0)[0]
        sel = (n == k)[:, None].expand_as(v)
        assert bool(sel.any()) and torch.equal(vk[sel], v[sel])


def test_the_fold_field_converges_where_it_does_not_fold():
    """svf_ref.fold_field((13, 18, 23)): 89 % of the voxels converge, the rest end finite with a residual of up to 9; the voxels that do not converge
    overlap those whose Jacobian determinant is <= 0."""
    u = fr.fold_field()
    v, r, n = fr.invert(u)
    share, folded = (r <= fr.TOL).double().mean().item(), jr.det(u.double()) <= 0
    print(f"fold: {100 * share:.1f} % converge, largest residual {r.max().item():.2f}, {100 * folded.double().mean().item():.1f} % of the voxels have det <= 0, "
          f"{int(((r > fr.TOL) & folded).sum())} of them among the {int((r > fr.TOL).sum())} that do not converge")
    assert abs(share - fr.FOLD_CONVERGED) <= 0.01
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(r).all()) and 8.0 <= r.max().item() <= 10.0
    assert bool(folded.any()) and bool(((r > fr.TOL) & folded).any())


def test_a_constant_field_inverts_exactly():
    u = fr.constant_field()
    for dtype in (torch.float32, torch.float64):
        v, r, n = fr.invert(u.to(dtype))
        assert torch.equal(v, -u.to(dtype)) and not bool(r.any()) and int(n.max()) == 2


def test_non_finite_values_end_a_voxel_with_nan():
    u = fr.field("a").clone()
    u[0, 1, 4, 5, 6] = float("nan")
    u[0, 2, 9, 12, 20] = float("inf")
    v, r, _ = fr.invert(u, fr.FIXED_K, 0.0)
    clean = fr.reference("a")["v32"]
    bad = torch.isnan(r)
    assert bool(bad[0, 4, 5, 6]) and bool(bad[0, 9, 12, 20]) and 2 <= int(bad.sum()) < 200
    assert torch.equal(torch.isnan(v).all(1), bad) and torch.equal(torch.isnan(v).any(1), bad)
    keep = ~bad[:, None].expand_as(v)
    assert torch.equal(v[keep], clean[keep])      # a voxel that never met the values has the bits of the clean field
    init = torch.zeros_like(u)
    init[0, 0, 2, 2, 2] = float("inf")
    v, r, _ = fr.invert(fr.field("a"), 3, 0.0, init=init)
    assert bool(torch.isnan(v[0, :, 2, 2, 2]).all()) and bool(torch.isnan(r[0, 2, 2, 2])) and int(torch.isnan(r).sum()) == 1


@pytest.mark.parametrize("case", ["a", "c", "d"])
def test_compose_with_zeros_is_one_squaring(case):
    u = fr.field(case)
    for dtype in (torch.float32, torch.float64):
        assert torch.equal(fr.compose(u.to(dtype), u.to(dtype), "zeros"), svf_ref.levels(2 * u.to(dtype), 1)[-1])


@pytest.mark.parametrize("case", list(fr.CASES))
def test_compose_with_the_inverse_has_the_residual_of_the_table(case):
    """compose(u, invert(u)) = v + Sb(u, y + v) is the right-inverse residual: the table's value, in fp64 from the fp32 result."""
    u = fr.field(case)
    v = fr.reference(case)["stop32"][0]
    c = fr.compose(u.double(), v.double(), "border")
    assert torch.equal(c.abs().amax(1), fr.right_residual(u, v))
    assert abs(c.abs().max().item() - fr.TABLE[case][1]) <= 0.02 * fr.TABLE[case][1]
    # the paddings differ where the samples leave the volume, and only there
    z = fr.compose(u.double(), v.double(), "zeros")
    assert not torch.equal(z, c)


def test_sample_border_is_continuous_and_clamps():
    """Sb at lattice points is the field; beyond a face it is the face's value; an axis of one voxel has t = 0."""
    f = fr.field("a").double()
    assert torch.equal(fr.sample_border(f, torch.zeros_like(f)), f)
    far = torch.full_like(f, 100.0)
    assert torch.equal(fr.sample_border(f, far), f[:, :, -1:, -1:, -1:].expand_as(f))
    assert torch.equal(fr.sample_border(f, -far), f[:, :, :1, :1, :1].expand_as(f))
    d = fr.field("d").double()
    shift = torch.zeros_like(d)
    shift[:, 0] = 0.7
    assert torch.equal(fr.sample_border(d, shift), d)


def test_one_resampling_is_closer_than_two():
    """What composition is for, in fp64 and fp32 with the GPU test's inputs: against the analytically composed image, one resampling through
    compose(a, b) has a smaller interior rms than two resamplings (0.094 against 0.162)."""
    for dtype in (torch.float64, torch.float32):
        once, twice = fr.use_errors(dtype)
        print(f"{dtype}: one resampling {once:.4f}, two {twice:.4f}")
        assert once < 0.75 * twice


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    ptr = lambda p: ctypes.c_void_p(p) if p else None  # noqa: E731
    inf, nan = float("inf"), float("nan")

    def comp(first=4096, second=8192, out=12288, ndim=3, B=1, dhw=(5, 6, 7), padding=1):
        return lib.trx_flow_compose(ptr(first), ptr(second), ptr(out), ndim, B, *dhw, padding, None)

    def inv(flow=4096, init=8192, inverse=12288, residual=16384, ndim=3, B=1, dhw=(5, 6, 7), iterations=30, tol=1e-3):
        return lib.trx_flow_invert(ptr(flow), ptr(init), ptr(inverse), ptr(residual), ndim, B, *dhw, iterations, tol, None)

    assert comp(first=None) == ARG and comp(second=None) == ARG and comp(out=None) == ARG
    assert comp(out=4096) == ARG      # out == first
    assert inv(flow=None) == ARG and inv(inverse=None) == ARG
    assert inv(inverse=4096) == ARG      # inverse == flow
    for bad, want in ((dict(ndim=1), NDIM), (dict(ndim=4), NDIM), (dict(ndim=2), NDIM), (dict(ndim=0), NDIM), (dict(B=0), ARG), (dict(B=65536), ARG),
                      (dict(dhw=(0, 6, 7)), ARG), (dict(dhw=(5, -1, 7)), ARG), (dict(dhw=(5, 6, 0)), ARG), (dict(dhw=(2048, 1024, 1025)), ARG)):
        assert comp(**bad) == want and inv(**bad) == want, bad
    for bad in (-1, 2, 3):
        assert comp(padding=bad) == ARG, bad
    for bad in (0, -1, 1001):
        assert inv(iterations=bad) == ARG, bad
    for bad in (nan, inf, -inf, -1e-30, -1.0):
        assert inv(tol=bad) == ARG, bad
    # the first refusal wins over a later one: a bad ndim next to a bad padding / count is TRX_ERR_NDIM
    assert comp(ndim=5, padding=7) == NDIM and inv(ndim=5, iterations=0) == NDIM


def test_c_abi_refusals_without_a_device():
    check_refusals()


def test_lib_signatures():
    from torchregister_amd import _lib
    lib = _lib.load()
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["trx_flow_compose"] == (I, [P, P, P, I, I, I, I, I, I, P])
    assert _lib.SIGNATURES["trx_flow_invert"] == (I, [P, P, P, P, I, I, I, I, I, I, F, P])
    assert lib.trx_flow_compose.restype is I and lib.trx_flow_invert.restype is I
    assert lib.trx_version() == 240


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python interface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_on_cpu_tensors():
    import TorchRegister
    import torchregister_amd as tr
    from torchregister_amd import _lib
    assert TorchRegister.compose_flows is tr.compose_flows and TorchRegister.invert_flow is tr.invert_flow
    u = torch.zeros(1, 3, 4, 5, 6)
    for bad in ("reflect", "zero", None, 1, 0):
        with pytest.raises(ValueError, match="padding"):
            tr.compose_flows(u, u, padding=bad)
    for other in (torch.zeros(1, 3, 4, 5, 7), torch.zeros(2, 3, 4, 5, 6), torch.zeros(1, 2, 5, 6)):
        with pytest.raises(ValueError, match="one shape"):
            tr.compose_flows(u, other)
        with pytest.raises(ValueError, match="one shape"):
            tr.compose_flows(other, u)
        with pytest.raises(ValueError, match="one shape"):
            tr.invert_flow(u, init=other)
    for bad in (0, -3, 1001, 2.0, "5", None, True):
        with pytest.raises(ValueError, match="iterations"):
            tr.invert_flow(u, iterations=bad)
        with pytest.raises(ValueError, match="iterations"):
            tr.Register("flow").invert_flow(iterations=bad)
        with pytest.raises(ValueError, match="iterations"):
            tr.flow_register((8, 8, 8), flow_model="direct").invert_flow(iterations=bad)
    for bad in (-1e-9, float("nan"), float("inf"), "x", None, False):
        with pytest.raises(ValueError, match="tol"):
            tr.invert_flow(u, tol=bad)
        with pytest.raises(ValueError, match="tol"):
            tr.Register("flow").invert_flow(tol=bad)
        with pytest.raises(ValueError, match="tol"):
            tr.flow_register((8, 8, 8), flow_model="direct").invert_flow(tol=bad)
    for shape in ((1, 2, 4, 4, 4), (1, 3, 4, 4), (3, 4, 4), (1, 4, 4, 4, 4, 4)):
        with pytest.raises(ValueError, match="dense flow"):
            tr.compose_flows(torch.zeros(shape), torch.zeros(shape))
        with pytest.raises(ValueError, match="dense flow"):
            tr.invert_flow(torch.zeros(shape))
    # good arguments on CPU tensors: the GPU-only refusal
    for fn in (lambda: tr.compose_flows(u, u), lambda: tr.compose_flows(u, u, "zeros"), lambda: tr.invert_flow(u), lambda: tr.invert_flow(u, 5, 0.0, init=u),
               lambda: tr.invert_flow(torch.zeros(1, 2, 5, 6), return_residual=True)):
        with pytest.raises(_lib.TrxError, match="no CPU fallback"):
            fn()
    # Register / flow_register
    with pytest.raises(RuntimeError, match="optim"):
        tr.Register("flow").invert_flow()
    with pytest.raises(RuntimeError, match="optim"):
        tr.Register("flow", flow_model="bspline", criterion=[tr.NCCLoss()], weight=[1.0]).invert_flow()
    for mode in ("rigid", "affine"):
        with pytest.raises(ValueError, match="closed-form"):
            tr.Register(mode).invert_flow()
    with pytest.raises(RuntimeError, match="optimize"):
        tr.flow_register((8, 8, 8), flow_model="direct").invert_flow()
    reg = tr.Register("flow", flow_model="bspline", criterion=[tr.MILoss()], weight=[1.0])
    reg.theta, reg.initial = u, torch.eye(3, 4)[None]      # the state optim(initial=...) leaves
    with pytest.raises(ValueError, match="initial"):
        reg.invert_flow()
    fl = tr.flow_register((4, 5, 6), flow_model="bspline", criterions=[tr.MILoss()], weights=[1.0])
    fl.flow, fl.initial = u, torch.eye(3, 4)[None]
    with pytest.raises(ValueError, match="initial"):
        fl.invert_flow()
    reg.initial = None
    with pytest.raises(_lib.TrxError, match="no CPU fallback"):
        reg.invert_flow()
    # the existing inverse of the diffeomorphic model stays as it is
    with pytest.raises(RuntimeError, match="diffeomorphic"):
        tr.Register("flow").inverse(u)
