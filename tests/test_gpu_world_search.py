"""GPU checks of the principal-axes / pose-search initialiser (trx_image_moments2, world_search, world_init='principal_axes' / 'search'; DESIGN.md section
4.21) against the fp64 restatement tests/world_search_ref.py.

Bars.  Moments: per column nvox 2^-52 sum |term| - the worst-case error of an fp64 sum of nvox terms in any order (each term itself one rounding), derived,
not measured.  Scores: test_gpu_affine_mi_world.py's evaluation bar, max(2e-5 |l64|, 4 |l32 - l64|), and bit equality with single calls.  The runs: a
rotation distance to the truth of at most 2 x what the fp64 arbiter loop reaches from the same T0."""
import ctypes
import functools
import math

import pytest
import torch

import affine_mi_grids_ref as gref
import affine_mi_world_ref as wref
import mi_mask_ref as mref
import world_search_ref as sref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    import torchregister_amd as tr
    assert torch.cuda.is_available()
    return tr


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. trx_image_moments2
# ---------------------------------------------------------------------------------------------------------------------------------------
def _moments(x, mask=None, offset=None, order=2):
    """trx_image_moments2 (order 2) / trx_image_moments (order 1) through the C ABI: out [N, ncol] fp64."""
    from torchregister_amd import _lib
    lib = _lib.load()
    nd, N = x.dim() - 2, x.shape[0]
    dhw = (1,) * (3 - nd) + tuple(x.shape[2:])
    name = "trx_image_moments2" if order == 2 else "trx_image_moments"
    n = getattr(lib, name + "_workspace_bytes")(nd, N, *dhw)
    assert n == N * ((math.prod(dhw) + 16383) // 16384) * (10 if order == 2 else 4) * 8
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.full((N, 1 + nd + (nd * (nd + 1) // 2 if order == 2 else 0)), float("nan"), dtype=torch.float64, device="cuda")
    _lib.check(getattr(lib, name)(_lib.ptr(x), _lib.ptr(mask), _lib.ptr(offset), nd, N, *dhw, _lib.ptr(out), _lib.ptr(ws), n,
                                  _lib.current_stream(torch.device("cuda"))), name)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("masked", [False, True], ids=["all-voxels", "masked"])
@pytest.mark.parametrize("shape", [(5, 6, 7), (26, 26, 25), (130, 127)], ids=str)
def test_moments2_against_the_restatement(tr, shape, masked):
    """One partial chunk, two chunks with the second nearly empty (16 900 voxels), 2-D with two chunks; N = 2 with different offsets."""
    g = torch.Generator().manual_seed(7)
    x = torch.rand(2, 1, *shape, generator=g) * torch.tensor([1.0, 3.0]).reshape(2, 1, *([1] * len(shape))) + torch.tensor([0.5, -2.0]).reshape(2, 1, *([1] * len(shape)))
    x = x * torch.exp(16.0 * torch.rand(2, 1, *shape, generator=g) - 8.0)      # six decades of dynamic range: the fp64 sums round, so their ORDER shows in the bits
    mask = (torch.rand(2, 1, *shape, generator=g) > 0.4).to(torch.uint8) if masked else None
    off = sref.min_offset(x, mask)
    assert off[0].item() != off[1].item()
    want, mag = sref.raw_moments(x, mask, off)
    xc, mc, oc = x.cuda(), None if mask is None else mask.cuda(), off.cuda()
    got = _moments(xc, mc, oc)
    nvox = math.prod(shape)
    err, bar = (got - want).abs(), nvox * 2.0 ** -52 * mag
    for b in range(2):
        print(f"{shape}{' masked' if masked else ''} volume {b}: err / bar per column", [f"{e:.1e}/{t:.1e}" for e, t in zip(err[b].tolist(), bar[b].tolist())])
    msgs = sref.check_raw_moments(got, _moments(xc, mc, oc, order=1), want, mag, nvox)      # the bar per column; the first-order columns: trx_image_moments' bits
    assert not msgs, msgs
    assert torch.equal(got, _moments(xc, mc, oc))                                    # the same bits on every call
    three = torch.cat([xc[1:], xc[:1], xc[1:]])
    m3 = None if mc is None else torch.cat([mc[1:], mc[:1], mc[1:]])
    g3 = _moments(three, m3, torch.stack([oc[1], oc[0], oc[1]]))
    assert torch.equal(g3[1], got[0]) and torch.equal(g3[0], got[1]) and torch.equal(g3[2], got[1])      # a volume's sums do not depend on N
    assert torch.equal(_moments(xc[:1], None if mc is None else mc[:1], oc[:1])[0], got[0])
    # without an offset: w = v
    assert bool(((_moments(xc, mc, None) - sref.raw_moments(x, mask)[0]).abs() <= nvox * 2.0 ** -52 * sref.raw_moments(x, mask)[1]).all())


@pytest.mark.parametrize("shape", [(26, 26, 25), (130, 127)], ids=str)
def test_image_covariance_against_the_restatement(tr, shape):
    """image_covariance forms c = S1 / m and C = S2 / m - c c^T from the raw sums in fp64.  Bar: the summation bound of the raw sums carried through -
    nvox 2^-52 sum |w| r^2 / m for S2 / m, the same again for c c^T (|c| <= r), doubled for the roundings of the division and the product - 4 x that in
    all; r = the largest index."""
    g = torch.Generator().manual_seed(9)
    x = torch.rand(2, 1, *shape, generator=g) + 0.1
    mask = mref.ellipsoid(shape, 0.8).expand(2, 1, *shape).to(torch.uint8)
    for m in (None, mask):
        mass, c, C = tr.image_covariance(x.cuda(), None if m is None else m.cuda())
        wm, wc, wC = sref.covariance(x, m)
        bar = 4.0 * math.prod(shape) * 2.0 ** -52 * max(shape) ** 2
        print(f"{shape}: mass err {(mass - wm).abs().max().item():.1e}, centre err {(c - wc).abs().max().item():.1e}, covariance err {(C - wC).abs().max().item():.1e}, bar {bar:.1e}")
        assert mass.device.type == "cpu" and C.dtype == torch.float64 and tuple(C.shape) == (2, len(shape), len(shape))
        assert (mass - wm).abs().max().item() <= bar * wm.max().item() and (c - wc).abs().max().item() <= bar and (C - wC).abs().max().item() <= bar
    with pytest.raises(ValueError):
        tr.image_covariance(torch.full((1, 1) + shape, 2.0, device="cuda"))
    with pytest.raises(ValueError):
        tr.image_covariance(x.cuda(), torch.zeros_like(mask))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. candidate scores, 3. the choice
# ---------------------------------------------------------------------------------------------------------------------------------------
def _loss_bar(l64, l32):
    return max(2e-5 * abs(l64), 4.0 * abs(l32 - l64))


@functools.lru_cache(maxsize=None)
def _restated(which="3d", mask_radii=None):
    """(candidates [K,...], c_t, range, [(l64, l32)] of the principal-axes candidates) of a pair in the restatement."""
    mov, tgt, Am, At, _ = sref.pair3() if which == "3d" else sref.pair2()
    mask = mmask = None
    if mask_radii is not None:
        mask, mmask = mref.ellipsoid(tuple(tgt.shape[2:]), mask_radii[0]).to(torch.uint8), mref.ellipsoid(tuple(mov.shape[2:]), mask_radii[1]).to(torch.uint8)
    (cm, Cm), (ct, Ct) = sref.world_moments(mov, Am, mmask), sref.world_moments(tgt, At, mask)
    T0s = sref.candidates(Cm, cm, Ct, ct)
    rng = sref.fit_range(tgt, mov, mask, mmask)
    recs = sref.records(tuple(mov.shape[2:]), tuple(tgt.shape[2:]), Am, At, T0s, ct)
    return T0s, cm, ct, rng, [tuple(sref.score(mov, tgt, r, rng, mask, mmask, dt) for dt in (torch.float64, torch.float32)) for r in recs], mask, mmask


def test_candidate_scores_are_single_calls_bit_for_bit(tr):
    """The rehearsal pair at 24 x 28 x 32 against 32 x 32 x 32 under oblique, flipped headers: the K = 4 principal-axes scores and the first 16 grid scores of
    world_search(candidates='search') - the batched evaluation with image strides 0 - equal single calls of affine_mi_loss_grad at the same T0 bit for bit,
    and lie within the evaluation bar of the fp64 restatement."""
    mov, tgt, Am, At, _ = sref.pair3()
    ms, ts = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    m, t = mov.cuda(), tgt.cuda()
    ws = tr.world_search(m, t, Am, At, candidates="search", step=45, keep=4, iters=0)
    assert tuple(ws.scores.shape) == (1, 4 + 320) and tuple(ws.candidates.shape) == (1, 324, 4, 4) and tuple(ws.kept.shape) == (1, 4)
    T0s, cm, ct, rng_ref, lref, _, _ = _restated()
    assert (ws.candidates[0, :4] - T0s).abs().max().item() <= 1e-9 and (ws.center[0] - ct).abs().max().item() <= 1e-9
    grid = sref.euler_grid(3, 45.0)
    for k in range(16):
        assert (ws.candidates[0, 4 + k] - sref.about(grid[k], ct, cm)).abs().max().item() <= 1e-9
    assert ws.kept[0].tolist() == torch.sort(ws.scores[0], stable=True).indices[:4].tolist() and int(ws.chosen[0]) == int(ws.kept[0, 0])
    assert torch.equal(ws.init[0], ws.candidates[0, int(ws.chosen[0])]) and torch.equal(ws.refined[0], ws.scores[0, ws.kept[0]])
    rng = tr._engine.mi_range(t, m)
    assert torch.equal(rng.cpu(), rng_ref)
    ident = torch.eye(3, 4)[None]
    for k in range(20):
        geo = tr.world_geometry(ms, ts, Am, At, ws.candidates[0, k], ws.center[0])
        for grad in (False, True):
            single = tr.affine_mi_loss_grad(m, t, ident, rng, need_grad=grad, world=geo)[0]
            assert single[0].item() == ws.scores[0, k].item(), (k, grad, single[0].item(), ws.scores[0, k].item())
        rec = wref.record(ms, ts, Am, At, ws.candidates[0, k], ws.center[0])
        l64, l32 = lref[k] if k < 4 else tuple(sref.score(mov, tgt, rec, rng_ref, None, None, dt) for dt in (torch.float64, torch.float32))
        err, bar = abs(ws.scores[0, k].item() - l64), _loss_bar(l64, l32)
        print(f"candidate {k}: score {ws.scores[0, k].item():.6f} restated {l64:.6f} err {err:.2e} bar {bar:.2e}")
        assert err <= bar, (k, err, bar)
    # the candidates past one chunk of 64 are scored like the first: spot checks in the third and the last chunk
    for k in (130, 323):
        geo = tr.world_geometry(ms, ts, Am, At, ws.candidates[0, k], ws.center[0])
        assert tr.affine_mi_loss_grad(m, t, ident, rng, need_grad=False, world=geo)[0][0].item() == ws.scores[0, k].item()


@functools.lru_cache(maxsize=None)
def _restated_search():
    mov, tgt, Am, At, _ = sref.pair3()
    T0s, _, ct = _restated()[:3]
    return tuple(sref.search(mov, tgt, Am, At, T0s, ct, 4, 20, dt) for dt in (torch.float64, torch.float32))


def test_the_choice_is_the_restatement_s(tr):
    """world_search(candidates='principal_axes', keep=4, iters=20): kept, chosen and the refined losses against the restated search (fp64 scoring, four rigid
    Adam loops of 20 iterations, the lowest best loss).  The condition - asserted - under which the choice cannot hinge on precision: the restatement's
    best and second-best refined losses differ by more than 100 x its own fp32-fp64 gap (0.243 against 1.1e-6 in the rehearsal)."""
    mov, tgt, Am, At, T = sref.pair3()
    r64, r32 = _restated_search()
    s = torch.sort(r64[2]).values
    gap = (r64[2] - r32[2]).abs().max().item()
    print(f"restated refined {r64[2].tolist()}: margin {(s[1] - s[0]).item():.4f}, fp32-fp64 gap {gap:.2e}")
    assert (s[1] - s[0]).item() > 100.0 * gap and r64[3] == r32[3]
    ws = tr.world_search(mov.cuda(), tgt.cuda(), Am, At, candidates="principal_axes", keep=4, iters=20)
    print(f"scores {ws.scores[0].tolist()} kept {ws.kept[0].tolist()} refined {ws.refined[0].tolist()} chosen {int(ws.chosen[0])}; eigenvalues {[e[0].tolist() for e in ws.eigenvalues]}")
    assert tuple(ws.scores.shape) == (1, 4) and ws.kept[0].tolist() == r64[1].tolist() and int(ws.chosen[0]) == r64[3]
    assert (ws.refined[0].double() - r64[2]).abs().max().item() <= max(100.0 * gap, 1e-4)
    assert sref.rotation_error(ws.init[0], T) <= sref.rotation_error(ws.candidates[0, r64[3]], T) and (ws.init[0] - r64[4]).abs().max().item() <= 1e-2
    (wm, wt) = ws.eigenvalues
    assert (wm[0] - sref.axes(sref.world_moments(mov, Am)[1])[0]).abs().max().item() <= 1e-8 and (wt[0] - sref.axes(sref.world_moments(tgt, At)[1])[0]).abs().max().item() <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. the run
# ---------------------------------------------------------------------------------------------------------------------------------------
def _register(tr, levels=1):
    return tr.Register("rigid", criterion=[tr.MILoss()], weight=[1.0], optimizer="adam", device_loop=True, init=torch.zeros(6), levels=levels)


def _arbiter_distance(mov, tgt, Am, At, T, T0, c, iters):
    """Rotation distance to the truth of the fp64 arbiter loop (rigid, Adam 0.01, pose 0, the transform at its best loss) from T0 about c."""
    ms, ts = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    _, pose = sref.refine(mov, tgt, wref.record(ms, ts, Am, At, T0, c), sref.fit_range(tgt, mov), iters)
    return sref.rotation_error(wref.world_matrix(gref.pose_to_theta(pose.double())[0], wref.geometry(ms, ts, Am, At, T0, c)), T)


@pytest.mark.parametrize("init", ["principal_axes", "search"])
def test_the_run_ends_at_the_truth(tr, init):
    """Register('rigid', device_loop=True).optim(..., world_init=init) on the rehearsal pair, 130 degrees from the headers' orientation: the world matrix ends
    within 2 x the rotation distance the fp64 arbiter loop reaches from the same T0 (the run's own .world_init about its .world_center, as many iterations
    at full resolution as the run has in all).  'principal_axes': one level, 60 iterations (rehearsed: the arbiter ends 0.073 degrees from the truth);
    'search': step 45, keep 4, iters 20, levels=2 with 30 + 60 iterations."""
    mov, tgt, Am, At, T = sref.pair3()
    two = init == "search"
    reg = _register(tr, levels=2 if two else 1)
    reg.optim(mov.cuda(), tgt.cuda(), lr=0.01, max_epochs=[30, 60] if two else 60, moving_affine=Am, target_affine=At, world_init=init,
              world_search=dict(step=45, keep=4, iters=20) if two else dict(keep=4, iters=20))
    ws = reg.world_search
    assert ws is not None and torch.equal(reg.world_init, ws.init) and torch.equal(reg.world_center, ws.center)
    assert tuple(ws.scores.shape) == (1, 324 if two else 4)
    start, end = sref.rotation_error(reg.world_init[0], T), sref.rotation_error(reg.world_matrix[0].cpu(), T)
    arb = _arbiter_distance(mov, tgt, Am, At, T, reg.world_init[0], reg.world_center[0], 90 if two else 60)
    print(f"world_init={init!r}: chosen {int(ws.chosen[0])}, T0 {start:.3f} degrees from the truth, the run ends at {end:.3f}, the arbiter at {arb:.3f}")
    assert end <= 2.0 * arb, (init, end, arb)


def test_moments_alone_do_not_reach_it(tr):
    """The same call with world_init='moments' ends farther than 90 degrees away (the arbiter: 118.9)."""
    mov, tgt, Am, At, T = sref.pair3()
    reg = _register(tr)
    reg.optim(mov.cuda(), tgt.cuda(), lr=0.01, max_epochs=60, moving_affine=Am, target_affine=At, world_init="moments")
    end = sref.rotation_error(reg.world_matrix[0].cpu(), T)
    print(f"world_init='moments': the run ends {end:.1f} degrees from the truth")
    assert end > 90.0 and reg.world_search is None


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. other cases
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_dimensions(tr):
    """40 x 48 against a flipped, oblique 44 x 40 lattice, 150 degrees: K = 2, the right candidate is chosen, as the restatement chooses."""
    mov, tgt, Am, At, T = sref.pair2()
    T0s, _, ct = _restated("2d")[:3]
    want = sref.search(mov, tgt, Am, At, T0s, ct, 2, 20)
    ws = tr.world_search(mov.cuda(), tgt.cuda(), Am, At, candidates="principal_axes", keep=8, iters=20)
    print(f"2-D: scores {ws.scores[0].tolist()} refined {ws.refined[0].tolist()} chosen {int(ws.chosen[0])}, {sref.rotation_error(ws.init[0], T):.3f} degrees from the truth")
    assert tuple(ws.candidates.shape) == (1, 2, 3, 3) and tuple(ws.kept.shape) == (1, 2) and (ws.candidates[0] - T0s).abs().max().item() <= 1e-9
    assert int(ws.chosen[0]) == want[3] and sref.rotation_error(ws.candidates[0, int(ws.chosen[0])], T) <= 5.0 and sref.rotation_error(ws.init[0], T) <= 1.0
    assert sref.rotation_error(ws.candidates[0, 1 - int(ws.chosen[0])], T) >= 170.0
    assert tuple(tr.world_search(mov.cuda(), tgt.cuda(), Am, At, candidates="search", step=90, iters=0).scores.shape) == (1, 2 + 4)


MASK_RADII = (0.95, 0.85)


def test_masks_are_honoured(tr):
    """mask (target) and moving_mask: the moments are those inside the masks, and the scores are the restatement's under the overlap rule with both masks
    (mi_overlap_ref; the candidates are border-stable there, which is asserted: no validity decision within 1e-4 voxels of changing)."""
    mov, tgt, Am, At, T = sref.pair3()
    ms, ts = tuple(mov.shape[2:]), tuple(tgt.shape[2:])
    T0s, cm, ct, rng, lref, mask, mmask = _restated("3d", MASK_RADII)
    m, t = mov.cuda(), tgt.cuda()
    _, c, C = tr.image_covariance(m, mmask.cuda())
    _, wc, wC = sref.covariance(mov, mmask)
    assert (c - wc).abs().max().item() <= 1e-9 and (C - wC).abs().max().item() <= 1e-8
    assert (c - sref.covariance(mov)[1]).abs().max().item() > 1e-3          # the mask matters
    ws = tr.world_search(m, t, Am, At, candidates="principal_axes", mask=mask.cuda(), moving_mask=mmask.cuda(), iters=0)
    assert (ws.candidates[0] - T0s).abs().max().item() <= 1e-9 and (ws.center[0] - ct).abs().max().item() <= 1e-9
    plain = tr.world_search(m, t, Am, At, candidates=ws.candidates, iters=0)
    for k in range(4):
        assert sref.score_is_border_stable(mov, tgt, wref.record(ms, ts, Am, At, T0s[k], ct), mask, mmask)
        l64, l32 = lref[k]
        err, bar = abs(ws.scores[0, k].item() - l64), _loss_bar(l64, l32)
        print(f"masked candidate {k}: score {ws.scores[0, k].item():.6f} restated {l64:.6f} err {err:.2e} bar {bar:.2e}; without masks {plain.scores[0, k].item():.6f}")
        assert err <= bar and abs(plain.scores[0, k].item() - l64) > 100.0 * bar
    assert sref.rotation_error(ws.init[0], T) <= 10.0


def test_callers_candidates(tr):
    """candidates=tensor: the true transform among three wrong ones is returned - scored alone (iters=0) and after refinement; a batch of two pairs is two
    independent searches with the bits of the single ones."""
    mov, tgt, Am, At, T = sref.pair3()
    c = wref.centre_of(tuple(tgt.shape[2:]), At)
    wrong = [wref.translation(c) @ sref._homog(sref.axis_angle(a, d)) @ wref.translation(-c) @ T for a, d in (((1.0, 0.0, 0.0), 90.0), ((0.0, 1.0, 0.2), 170.0), ((0.5, 0.5, 0.0), -60.0))]
    cands = torch.stack([wrong[0], wrong[1], T, wrong[2]])
    m, t = mov.cuda(), tgt.cuda()
    for iters in (0, 10):
        ws = tr.world_search(m, t, Am, At, candidates=cands, keep=2, iters=iters)
        print(f"caller's candidates, iters {iters}: scores {ws.scores[0].tolist()} refined {ws.refined[0].tolist()} chosen {int(ws.chosen[0])}")
        assert int(ws.chosen[0]) == 2 and ws.eigenvalues is None and (ws.center[0] - c).abs().max().item() <= 1e-12
        assert torch.equal(ws.init[0], T) if iters == 0 else sref.rotation_error(ws.init[0], T) <= 1.0      # (as it is / within a degree after ten steps)
    two = tr.world_search(torch.cat([m, m.flip(2)]), torch.cat([t, t]), Am, At, candidates=torch.stack([cands, cands.flip(0)]), keep=2, iters=10)
    assert torch.equal(two.scores[0], ws.scores[0]) and torch.equal(two.refined[0], ws.refined[0]) and torch.equal(two.init[0], ws.init[0])
    assert int(two.chosen[0]) == 2 and tuple(two.scores.shape) == (2, 4)
    with pytest.raises(ValueError):
        tr.world_search(m, t, Am, At, candidates=torch.eye(3)[None])
    with pytest.raises(ValueError):
        tr.world_search(m, t, Am, At, candidates="principal")
