"""CPU-only checks of the Jacobian determinant map and the folding penalty: the restatement tests/jacobian_ref.py against
tests/svf_ref.py and against the closed form the kernel gathers, the conditions the GPU tests rest on (active shares, face coverage, the loop rows),
every refusal of the C ABI without a device, and the Python interface on CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

import jacobian_ref as jr
import svf_ref
import test_affine_mi_grids_host as ghost

OK, ARG, NDIM, WS, CAP = 0, -1, -2, -3, -5


# ---------------------------------------------------------------------------------------------------------------------------------------
# the definition and the field cases
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", jr.CASES, ids=jr.case_id)
def test_field_cases(case):
    """On the interior the map is tests/svf_ref.py::jacobian_det; at eps = 0.3 between 5 % and 60 % of the voxels are active; in the first seven cases
    active voxels lie on both faces of every axis longer than one voxel, so every one-sided stencil carries gradient; the gather the kernel runs
    (jacobian_ref.gather_grad) is the autograd gradient."""
    fl, r = jr.field(case), jr.reference(case)
    B, spatial = case[0], case[1]
    nd = len(spatial)
    d = r["det64"]
    assert d.shape == (B,) + tuple(spatial)
    if all(s >= 3 for s in spatial):
        inner = (slice(None),) + (slice(1, -1),) * nd
        err = np.abs(d[inner] - svf_ref.jacobian_det(fl.double()).numpy()).max()
        print(f"{jr.case_id(case)}: interior against svf_ref.jacobian_det {err:.1e}")
        assert err <= 1e-13
    share = jr.active_share(d)
    print(f"{jr.case_id(case)}: {100 * share:.1f} % active, max |det| {np.abs(d).max():.2f}, P {r['p64']}, max |dP/dflow| {np.abs(r['g64']).max():.3e}")
    assert 0.05 <= share <= 0.60
    if case in jr.FIELD_CASES[:jr.FACES_COVERED] or case in jr.BLOCK_CASES:
        for a, s in enumerate(spatial):
            if s > 1:
                first, last = np.take(d, 0, axis=1 + a), np.take(d, s - 1, axis=1 + a)
                assert (first < jr.EPS).any() and (last < jr.EPS).any(), (case, a)
    g = jr.gather_grad(fl).numpy()
    assert np.abs(g - r["g64"]).max() <= 1e-12 * max(1.0, np.abs(r["g64"]).max())
    assert np.abs(r["g64"]).max() > 0


def test_block_cases_cross_the_kernel_chunk():
    """(7, 19, 37): the blocks of 2048 voxels end in the middle of a row, so a voxel next to a boundary has its x, y and z neighbours in another block;
    (33, 65, 70): more partial sums than the 64 lanes of the second stage."""
    (_, s0, _, _), (_, s1, _, _) = jr.BLOCK_CASES
    n0, n1 = int(np.prod(s0)), int(np.prod(s1))
    assert n0 > 2 * jr.KERNEL_CHUNK and all(k % s0[2] not in (0, s0[2] - 1) and (k // s0[2]) % s0[1] not in (0, s0[1] - 1)
                                            for k in (jr.KERNEL_CHUNK, 2 * jr.KERNEL_CHUNK))
    assert s0[1] * s0[2] < jr.KERNEL_CHUNK      # a z neighbour can lie in another block
    assert -(-n1 // jr.KERNEL_CHUNK) > 64


def test_bump_field_leaves_most_chunks_inactive():
    """The field of the GPU test of the gather's early exit: between 2 and 20 of its 74 chunks hold an active voxel, they are not the first or the last
    one, the ball reaches across a chunk boundary, and the gradient is non-zero in chunks WITHOUT an active voxel (a voxel's gradient comes from its
    neighbours, which may lie in the next chunk: the exit must look at every chunk within reach, not at its own)."""
    fl = jr.bump_field()
    d = jr.det(fl.double()).numpy()
    act = jr.chunk_activity(d)
    print(f"bump: {act.sum()} of {act.size} chunks active, {100 * jr.active_share(d):.2f} % of the voxels, min det {d.min():.3f}")
    assert act.size == 74 and 2 <= act.sum() <= 20 and not act[0] and not act[-1] and d.min() < 0
    assert (act[1:] & act[:-1]).any()
    _, g = jr.penalty_grad(fl)
    gflat = np.abs(g.numpy()[0]).max(0).reshape(-1)
    gchunk = np.concatenate([gflat, np.zeros((-gflat.size) % jr.KERNEL_CHUNK)]).reshape(-1, jr.KERNEL_CHUNK).max(1) > 0
    assert (gchunk & ~act).any() and (~gchunk).sum() >= 40


def test_an_axis_of_one_voxel_and_a_constant_field():
    """D is 0 on an axis of one voxel (the 2-D map of a plane equals the 3-D map of that plane with a zero z channel) and on a constant field det = 1."""
    fl2 = jr.field(jr.FIELD_CASES[5])
    fl3 = torch.cat([torch.zeros_like(fl2[:, :1]), fl2], dim=1)[:, :, None]
    assert torch.equal(jr.det(fl3.double())[:, 0], jr.det(fl2.double()))
    const = torch.full((1, 3, 4, 5, 6), 2.5, dtype=torch.float64)
    assert torch.equal(jr.det(const), torch.ones(1, 4, 5, 6, dtype=torch.float64))
    assert float(jr.penalty(const)) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------------
# the loop rows
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(jr.loop_rows()))
def test_loop_rows(row):
    """What the GPU loop tests rest on, per row (10 iterations, eps = 0.3): the fp64 loss falls in every iteration; the arbiter's fp32 and fp64 runs stay
    within the floors of test_gpu_mi._loop_bars (2e-5 of the loss, 2e-4 on the control tensor); the penalty is active in the first iteration; the
    penalised and the unpenalised fp64 runs differ by at least 100 x the bar on the control tensor.
    Measured here: ncc 183.91 -> 113.56, the penalty 46 % -> 14 % of the loss, 19.7 % -> 10.9 % of the voxels active, gaps 2.6e-5 / 1.0e-5, the penalty
    moves the control tensor by 2.0; the MI rows: gaps <= 2e-6 / 1.3e-5, moved by 0.15 .. 1.9."""
    fn, w = jr.loop_rows()[row], jr.row_weight(row)
    l64, p64, s64, c64 = fn(w, torch.float64)
    l32, _, _, c32 = fn(w, torch.float32)
    _, _, _, c0 = fn(0.0, torch.float64)
    lgap, pgap, moved = np.abs(l32 - l64).max(), np.abs(c32 - c64).max(), np.abs(c64 - c0).max()
    print(f"{row}: loss {l64[0]:.4f} -> {l64[-1]:.4f}, penalty {100 * p64[0] / l64[0]:.1f} % -> {100 * p64[-1] / l64[-1]:.1f} % of it, "
          f"{100 * s64[0]:.1f} % -> {100 * s64[-1]:.1f} % active; fp32-fp64 {lgap:.1e} (loss) {pgap:.1e} (ctrl); penalised - unpenalised {moved:.3f}")
    assert np.all(np.diff(l64) < 0)
    assert lgap <= 2e-5 * np.abs(l64).max() and pgap <= 2e-4
    assert p64[0] > 0 and s64[0] > 0
    assert moved >= 100 * 2e-4


def test_register_arbiters_fold_and_unfold():
    """The two runs of tests/test_gpu_jacobian.py's Register tests in fp64: unpenalised they fold, penalised they do not, at little cost in the data term."""
    n0, n1 = jr.use_run("ncc", 0.0), jr.use_run("ncc", jr.USE_NCC["weight"])
    m0, m1 = jr.use_run("mi", 0.0), jr.use_run("mi", jr.USE_MI["weight"])
    print(f"ncc: unpenalised {n0}\n     penalised {n1}\nmi:  unpenalised {m0}\n     penalised {m1}")
    assert n0["folded"] > 0.2 and n0["min_det"] < -3 and n1["min_det_run"] > 0.15 and n1["data"] <= 1.15 * n0["data"]
    assert m0["folded"] > 0.05 and m0["min_det"] < -1 and m1["min_det_run"] > 0.15 and m1["data"] <= 1.01 * m0["data"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_refusals():
    """Every call is refused with the documented status; none reaches a HIP call (the pointers are not mapped).  Also run by the GPU suite."""
    from torchregister_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ptr = lambda p: P(p) if p else None  # noqa: E731
    inf, nan = float("inf"), float("nan")
    assert lib.trx_version() == 240

    def jac(flow=4096, ndim=3, B=1, dhw=(5, 6, 7), det=4096):
        return lib.trx_flow_jacobian(ptr(flow), ndim, B, *dhw, ptr(det), None)

    q = lib.trx_flow_folding_workspace_bytes
    n = q(3, 2, 5, 6, 7)
    assert n == 1792 + 256      # the map of 2 x 210 voxels (1680 bytes) and 2 partials (16 bytes), each part rounded up to 256 bytes
    assert q(3, 1, 33, 65, 70) == -(-150150 * 4 // 256) * 256 + -(-74 * 8 // 256) * 256

    def fold(flow=4096, ndim=3, B=2, dhw=(5, 6, 7), thr=0.3, w=1.0, pen=4096, dflow=4096, acc=0, ws=4096, nbytes=n):
        return lib.trx_flow_folding(ptr(flow), ndim, B, *dhw, thr, w, ptr(pen), ptr(dflow), acc, ptr(ws), nbytes, None)

    assert jac(flow=None) == ARG and jac(det=None) == ARG
    assert fold(flow=None) == ARG and fold(pen=None) == ARG and fold(ws=None) == ARG
    for bad, want in ((dict(ndim=1), NDIM), (dict(ndim=4), NDIM), (dict(ndim=2), NDIM), (dict(B=0), ARG), (dict(B=65536), ARG), (dict(dhw=(0, 6, 7)), ARG),
                      (dict(dhw=(5, -1, 7)), ARG), (dict(dhw=(5, 6, 0)), ARG), (dict(dhw=(2048, 1024, 1024)), ARG)):
        assert jac(**bad) == want and fold(**bad) == want, bad
        assert q(bad.get("ndim", 3), bad.get("B", 2), *bad.get("dhw", (5, 6, 7))) == 0
    for bad in (dict(thr=nan), dict(thr=inf), dict(thr=-inf), dict(w=nan), dict(w=inf), dict(w=-1.0), dict(w=-1e-30)):
        assert fold(**bad) == ARG, bad
    assert fold(nbytes=n - 1) == WS and fold(nbytes=0) == WS
    assert fold(dflow=None, nbytes=n - 1) == WS      # a nullable dflow is no refusal: the call gets as far as the next one
    assert fold(ndim=2, B=1, dhw=(1, 19, 26), nbytes=q(2, 1, 1, 19, 26) - 1) == WS and fold(thr=-5.0, w=0.0, nbytes=n - 1) == WS

    # the loops
    vol, d3 = ghost._vol(_lib, B=1), (ctypes.c_int * 3)(4, 4, 4)
    opt, loss = _lib.OptCfg(_lib.OPT_ADAM, 0.1, 0.9, 0.999, 1e-8), _lib.LossCfg(0.0, 1.0, 100.0, 0.0, 3.0)
    base, fbytes = lib.trx_bspline_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4), q(3, 1, 12, 14, 16)
    nf = lib.trx_bspline_fold_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4)
    assert base > 0 and nf == -(-base // 256) * 256 + fbytes
    assert lib.trx_bspline_fold_workspace_bytes(3, 1, 12, 14, 16, 0, 4, 4) == 0 and lib.trx_bspline_fold_workspace_bytes(2, 1, 2, 14, 16, 4, 4, 4) == 0

    def state(**kw):
        st = _lib.BSplineState()
        for f in ("ctrl", "adam_m", "adam_v", "flow", "dflow", "losses", "step"):
            setattr(st, f, 4096)
        st.losses_capacity, st.bending_weight = 5, 0.0
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    good = _lib.FoldCfg(1.0, 0.3)

    def run(v=vol, lo=loss, o=opt, st=state(), sp=d3, f=good, iters=1, ws=4096, nbytes=nf):
        return lib.trx_bspline_run_fold(ref(v), ref(lo), ref(o), ref(st), sp, ref(f), iters, ptr(ws), nbytes, None)

    grid, cfg = ghost._grid(_lib), ghost._cfg(_lib)
    mbase = lib.trx_bspline_mi_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32)
    nm = lib.trx_bspline_mi_fold_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32, None)
    assert mbase > 0 and nm == -(-mbase // 256) * 256 + fbytes and lib.trx_bspline_mi_fold_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32, ref(grid)) == nm
    over = ghost._grid(_lib)
    over.overlap = 1
    nmo = lib.trx_bspline_mi_fold_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32, ref(over))
    assert nmo == -(-lib.trx_bspline_mi_grids_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 32, ref(over)) // 256) * 256 + fbytes > nm
    assert lib.trx_bspline_mi_fold_workspace_bytes(3, 1, 12, 14, 16, 4, 4, 4, 7, None) == 0

    def mirun(v=vol, g=grid, theta=4096, c=cfg, o=opt, st=state(), sp=d3, f=good, iters=1, ws=4096, nbytes=nm):
        return lib.trx_bspline_mi_run_fold(ref(v), ref(g), ptr(theta), ref(c), ref(o), ref(st), sp, ref(f), iters, ptr(ws), nbytes, None)

    for call in (run, mirun):
        for f in (None, _lib.FoldCfg(nan, 0.3), _lib.FoldCfg(inf, 0.3), _lib.FoldCfg(-1.0, 0.3), _lib.FoldCfg(1.0, nan), _lib.FoldCfg(1.0, -inf)):
            assert call(f=f) == ARG, (call.__name__, None if f is None else (f.weight, f.threshold))
        for f in (good, _lib.FoldCfg(0.0, 0.3), _lib.FoldCfg(5.0, -2.0)):      # a good struct passes: the call gets as far as the workspace check
            assert call(f=f, nbytes=(nf if call is run else nm) - 1) == WS
        assert call(v=None) == ARG and call(o=None) == ARG and call(st=None) == ARG and call(sp=None) == ARG and call(ws=None) == ARG and call(iters=-1) == ARG
        assert call(st=state(ctrl=None)) == ARG and call(st=state(adam_m=None)) == ARG and call(st=state(bending_weight=-1.0)) == ARG
        assert call(v=ghost._vol(_lib, ndim=4, B=1)) == NDIM and call(v=ghost._vol(_lib, B=0)) == ARG and call(sp=(ctypes.c_int * 3)(0, 4, 4)) == ARG
        assert call(nbytes=0) == WS and call(iters=6) == CAP
    assert run(lo=None) == ARG and run(nbytes=base) == WS
    assert mirun(c=None) == ARG and mirun(c=ghost._cfg(_lib, bins=7)) == ARG and mirun(nbytes=mbase) == WS
    assert mirun(g=None) == ARG and mirun(theta=None) == ARG      # one lattice: both NULL; two lattices: both given
    assert mirun(g=None, theta=None, nbytes=nm - 1) == WS and mirun(g=over, nbytes=nmo - 1) == WS and mirun(g=over, nbytes=nm) == WS
    assert mirun(g=ghost._grid(_lib, (0, 13, 18))) == ARG


def test_c_abi_refusals_without_a_device():
    check_refusals()


def test_bspline_state_did_not_grow():
    from torchregister_amd import _lib
    assert [f[0] for f in _lib.BSplineState._fields_] == ["ctrl", "adam_m", "adam_v", "base", "flow", "dflow", "losses", "losses_capacity", "step", "stop_crit",
                                                           "stopped", "flow_last", "bending_weight"]
    assert ctypes.sizeof(_lib.FoldCfg) == 8 and [f[0] for f in _lib.FoldCfg._fields_] == ["weight", "threshold"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# the Python interface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_on_cpu_tensors():
    import torchregister_amd as tr
    vol = torch.zeros(1, 1, 8, 8, 8)
    ncc = dict(criterion=[tr.NCCLoss()], weight=[1.0])
    for bad in (-1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError, match="folding_weight"):
            tr.Register("flow", flow_model="bspline", folding_weight=bad, **ncc)
        with pytest.raises(ValueError, match="folding_weight"):
            tr.flow_register((8, 8, 8), flow_model="bspline", criterions=[tr.NCCLoss()], weights=[1.0], folding_weight=bad)
        with pytest.raises(ValueError, match="folding_weight"):
            tr.BSplineSolver(vol, vol, 4, folding_weight=bad)
    for bad in (float("nan"), float("inf"), "x", None, False):
        with pytest.raises(ValueError, match="folding_threshold"):
            tr.Register("flow", flow_model="bspline", folding_threshold=bad, **ncc)
        with pytest.raises(ValueError, match="folding_threshold"):
            tr.flow_register((8, 8, 8), flow_model="bspline", criterions=[tr.NCCLoss()], weights=[1.0], folding_threshold=bad)
        with pytest.raises(ValueError, match="folding_threshold"):
            tr.BSplineSolver(vol, vol, 4, folding_threshold=bad)
        with pytest.raises(ValueError, match="folding_threshold"):
            tr.folding_penalty(torch.zeros(1, 3, 4, 4, 4), threshold=bad)
    # flow_model='bspline' only
    for kw in (dict(mode="rigid"), dict(mode="affine"), dict(mode="flow"), dict(mode="flow", flow_model="direct")):
        with pytest.raises(ValueError, match="folding_weight"):
            tr.Register(folding_weight=1.0, **kw)
        tr.Register(folding_weight=0.0, folding_threshold=0.3, **kw)      # the defaults are accepted everywhere
    for fm in ("unet", "direct"):
        with pytest.raises(ValueError, match="folding_weight"):
            tr.flow_register((8, 8, 8), flow_model=fm, n=1, folding_weight=1.0)
    tr.flow_register((8, 8, 8), flow_model="direct", folding_weight=0.0, folding_threshold=0.3)
    # not with the diffeomorphic model
    with pytest.raises(ValueError, match="folding_weight"):
        tr.Register("flow", flow_model="bspline", diffeomorphic=True, folding_weight=1.0, **ncc)
    with pytest.raises(ValueError, match="folding_weight"):
        tr.flow_register((8, 8, 8), flow_model="bspline", criterions=[tr.NCCLoss()], weights=[1.0], diffeomorphic=True, folding_weight=1.0)
    with pytest.raises(ValueError, match="folding_weight"):
        tr.BSplineSolver(vol, vol, 4, squarings=4, folding_weight=1.0)
    tr.Register("flow", flow_model="bspline", diffeomorphic=True, **ncc)
    reg = tr.Register("flow", flow_model="bspline", folding_weight=2.0, folding_threshold=0.1, levels=2, **ncc)
    assert reg.folding_weight == 2.0 and reg.folding_threshold == 0.1
    assert reg._flow_kw(1, 0.1, 5)["folding_weight"] == 2.0 and reg._flow_kw(1, 0.1, 5)["folding_threshold"] == 0.1
    # jacobian()
    with pytest.raises(RuntimeError, match="optim"):
        reg.jacobian()
    with pytest.raises(RuntimeError, match="optim"):
        tr.Register("flow").jacobian()
    for mode in ("rigid", "affine"):
        with pytest.raises(ValueError, match="constant"):
            tr.Register(mode).jacobian()
    # the functions take GPU tensors of the flow's layout
    from torchregister_amd import _lib
    for fn in (tr.jacobian_determinant, tr.folding_penalty, tr.folding_penalty_grad):
        for shape in ((1, 2, 4, 4, 4), (1, 3, 4, 4), (3, 4, 4), (1, 4, 4, 4, 4, 4)):
            with pytest.raises(ValueError, match="dense flow"):
                fn(torch.zeros(shape))
        with pytest.raises(_lib.TrxError, match="no CPU fallback"):
            fn(torch.zeros(1, 3, 4, 4, 4))
