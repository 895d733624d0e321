"""CPU restatement of csrc/distance.hip (include/trx.h: trx_distance_transform, trx_mask_surface, trx_label_overlap) in numpy, the
cases of tests/test_distance_host.py and tests/test_gpu_distance.py, and a brute force over all feature / voxel pairs for the tiny ones.

The transform is the definition taken one axis at a time: g(i) = min_j f(j) + w (i - j)^2 over ALL j of a line, x first, then y, then z (the kernel's
order, which matters for the fp32 roundings only).  Without voxel sizes it runs in int64 and is exact; with voxel sizes in the dtype asked for: fp64 is the
reference, fp32 - the weight voxel^2 rounded once, (i - j)^2 an exact integer converted, one product and one sum per candidate, as the kernel has them -
is what conftest.bar() measures the fp32 error of the definition with."""
import functools

import numpy as np

NONE_INT = np.int64(1) << 40      # "no feature" in the integer run: above every sum of three squares of sizes <= 16384, far from overflow


# ---------------------------------------------------------------------------------------------------------------------------------------
# the transform
# ---------------------------------------------------------------------------------------------------------------------------------------
def minplus(f, w, axis):
    """g(i) = min_j f(j) + w (i - j)^2 along `axis`, every j, in f's dtype (int64: w must be 1)."""
    f = np.ascontiguousarray(np.moveaxis(f, axis, -1))
    n = f.shape[-1]
    k = np.arange(n)
    sq = (k[:, None] - k[None, :]) ** 2
    cost = sq.astype(np.int64) if f.dtype == np.int64 else (f.dtype.type(w) * sq.astype(f.dtype)).astype(f.dtype)
    out = np.empty(f.shape, dtype=f.dtype)      # C-contiguous: the reshapes below are views
    flat_in, flat_out = f.reshape(-1, n), out.reshape(-1, n)
    with np.errstate(over="ignore", invalid="ignore"):
        step = max(1, 4_000_000 // (n * n))      # [lines, i, j] in slabs of about 4 M candidates
        for s in range(0, flat_in.shape[0], step):
            flat_out[s:s + step] = (flat_in[s:s + step, None, :] + cost[None]).min(axis=2)
    return np.moveaxis(out, -1, axis)


def dist2(mask, voxel=None, dtype=np.float64):
    """mask [B, *spatial] (non-zero = feature) -> the squared distance [B, *spatial]: int64 without voxel sizes (NONE_INT where the pair has no feature),
    else `dtype` (+inf there)."""
    m = np.asarray(mask) != 0
    nd = m.ndim - 1
    if voxel is None:
        g = np.where(m, np.int64(0), NONE_INT)
        for a in range(nd, 0, -1):
            g = np.minimum(minplus(g, 1, a), NONE_INT)
        return g
    dt = np.dtype(dtype).type
    g = np.where(m, dt(0), dt(np.inf)).astype(dtype)
    for a in range(nd, 0, -1):
        w = dt(np.float32(voxel[a - 1])) * dt(np.float32(voxel[a - 1]))      # the voxel size as the C ABI receives it (a float), squared in `dtype`
        g = minplus(g, w, a)
    return g


def dist2_f32(mask, voxel=None):
    """What dist2 means in fp32 [B, *spatial]: the integer run rounded (inf for NONE_INT), or the fp32 run."""
    if voxel is None:
        g = dist2(mask)
        return np.where(g >= NONE_INT, np.float32(np.inf), g.astype(np.float32)).astype(np.float32)
    return dist2(mask, voxel, np.float32)


def brute(mask, voxel=None):
    """The definition without separability, one pair [*spatial]: min over every feature of the squared centre distance; int64 or fp64."""
    m = np.asarray(mask) != 0
    pts = np.stack(np.meshgrid(*[np.arange(s) for s in m.shape], indexing="ij"), -1).reshape(-1, m.ndim)
    feat = pts[m.reshape(-1)]
    if voxel is None:
        if len(feat) == 0:
            return np.full(m.shape, NONE_INT)
        return ((pts[:, None, :] - feat[None]) ** 2).sum(-1).min(1).reshape(m.shape).astype(np.int64)
    if len(feat) == 0:
        return np.full(m.shape, np.inf)
    v = np.asarray([np.float32(x) for x in voxel], dtype=np.float64)
    return (((pts[:, None, :] - feat[None]) * v) ** 2).sum(-1).min(1).reshape(m.shape)


def dist2_from_index(idx, voxel=None):
    """The squared distance from every voxel to the index it was given, idx [B, nd, *spatial] -> int64 or fp64 [B, *spatial]."""
    idx = np.asarray(idx).astype(np.int64)
    nd = idx.shape[1]
    own = np.stack(np.meshgrid(*[np.arange(s) for s in idx.shape[2:]], indexing="ij"))[None]
    d = own - idx
    if voxel is None:
        return (d ** 2).sum(1)
    v = np.asarray([np.float32(x) for x in voxel], dtype=np.float64).reshape((1, nd) + (1,) * nd)
    return ((d * v) ** 2).sum(1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# what a transform is held to: shared by tests/test_gpu_distance.py (the fixed cases) and tests/fuzz_ops.py (the random ones)
# ---------------------------------------------------------------------------------------------------------------------------------------
def run_reference(mask, voxel):
    """dict(int, f32) without voxel sizes, dict(f64, f32) with them, of a mask [B, *spatial]: the keys of reference()."""
    if voxel is None:
        g = dist2(mask)
        return dict(int=g, f32=np.where(g >= NONE_INT, np.float32(np.inf), g.astype(np.float32)).astype(np.float32))
    return dict(f64=dist2(mask, voxel, np.float64), f32=dist2(mask, voxel, np.float32))


def d2_bar(r, b):
    """|delta d^2| <= max(1e-6 max d^2, twice the restatement's own fp32 - fp64 gap) of a pair with voxel sizes.  The floor covers about 16 fp32 roundings;
    the value needs one rounding of each squared voxel size, three products and two sums, and a near-tie that picks the other candidate costs no more."""
    return max(1e-6 * float(r["f64"][b].max()), 2.0 * float(np.max(np.abs(r["f32"][b].astype(np.float64) - r["f64"][b]))))


def check_transform(got, near, mask, voxel, r, worst=None, report=None):
    """got [B, *spatial] fp32 (the squared distance), near [B, nd, *spatial] int32 against the runs r of the mask [B, *spatial]: the messages of what does
    not hold, none when all does.  Without voxel sizes the squared distance is the int64 restatement cast to fp32, bit for bit; with them it is within
    d2_bar of the fp64 one.  0 on every feature.  A pair without a feature is +inf with nearest == -1.  nearest, without assuming a tie rule: in range, on
    a feature, and the distance recomputed from it is dist2 (equal integers / within the bar).  worst: a dict that receives the largest error / bar and
    counts of unequal voxels; report: called with one line per pair that has voxel sizes."""
    msgs = []
    worst = {} if worst is None else worst

    def up(key, value):
        worst[key] = max(worst.get(key, 0.0), float(value))

    sp = mask.shape[1:]
    for b in range(mask.shape[0]):
        feat = mask[b] != 0
        if not feat.any():
            if not (np.isposinf(got[b]).all() and (near[b] == -1).all()):
                msgs.append(f"pair {b} (empty): not all +inf / -1")
            continue
        if not (got[b][feat] == 0).all():
            msgs.append(f"pair {b}: d^2 != 0 on {int((got[b][feat] != 0).sum())} features")
        if not all((near[b, a] >= 0).all() and (near[b, a] < s).all() for a, s in enumerate(sp)):
            msgs.append(f"pair {b}: nearest out of range")
            continue
        if not feat[tuple(near[b])].all():
            msgs.append(f"pair {b}: nearest is no feature at {int((~feat[tuple(near[b])]).sum())} voxels")
        back = dist2_from_index(near[b:b + 1], voxel)[0]
        if voxel is None:
            bad, bad_back = int((got[b] != r["f32"][b]).sum()), int((back != r["int"][b]).sum())
            up("iso-unequal", bad)
            up("iso-nearest-unequal", bad_back)
            if bad or bad_back:
                at = tuple(int(v) for v in np.argwhere((got[b] != r["f32"][b]) | (back != r["int"][b]))[0])
                msgs.append(f"pair {b}: {bad} voxels differ from the integer run, {bad_back} through nearest; first at {at}: "
                            f"got {got[b][at]}, want {r['f32'][b][at]}, nearest {near[b][(slice(None),) + at].tolist()}")
        else:
            limit = d2_bar(r, b)
            e, e_back = float(np.abs(got[b] - r["f64"][b]).max()), float(np.abs(back - got[b].astype(np.float64)).max())
            ratio = lambda v: 0.0 if v == 0 else (np.inf if limit == 0 else v / limit)  # noqa: E731
            up("d2", ratio(e))
            up("d2-from-nearest", ratio(e_back))
            if report is not None:
                report(f"pair {b}: max d^2 {r['f64'][b].max():.4f} err {e:.3e}, recomputed from nearest {e_back:.3e}, bar {limit:.3e} "
                       f"(restatement fp32-fp64 {np.abs(r['f32'][b] - r['f64'][b]).max():.3e})")
            if not (e <= limit and e_back <= limit):
                msgs.append(f"pair {b}: d^2 err {e:.3e}, recomputed from nearest {e_back:.3e}, bar {limit:.3e}")
    return msgs


# ---------------------------------------------------------------------------------------------------------------------------------------
# surface, overlap, surface distances
# ---------------------------------------------------------------------------------------------------------------------------------------
def surface(mask):
    """mask [B, *spatial] -> uint8: set, and a face neighbour not set or outside the volume."""
    m = np.asarray(mask) != 0
    nd = m.ndim - 1
    p = np.pad(m, [(0, 0)] + [(1, 1)] * nd, constant_values=False)
    inner = (slice(None),) + (slice(1, -1),) * nd
    closed = np.ones_like(m)
    for a in range(1, nd + 1):
        closed &= np.roll(p, 1, a)[inner] & np.roll(p, -1, a)[inner]
    return (m & ~closed).astype(np.uint8)


def overlap_counts(a, b, L):
    """[B, L, 3] int64: |a = l|, |b = l|, |a = l and b = l|."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    B = a.shape[0]
    out = np.zeros((B, L, 3), dtype=np.int64)
    for p in range(B):
        fa, fb = a[p].reshape(-1), b[p].reshape(-1)
        out[p, :, 0] = np.bincount(fa[(fa >= 0) & (fa < L)], minlength=L)
        out[p, :, 1] = np.bincount(fb[(fb >= 0) & (fb < L)], minlength=L)
        same = fa[(fa == fb) & (fa >= 0) & (fa < L)]
        out[p, :, 2] = np.bincount(same, minlength=L)
    return out


def dice(counts):
    c = counts.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2.0 * c[..., 2] / (c[..., 0] + c[..., 1])


def surface_metrics(a, b, voxel=None, percentile=95.0, dtype=np.float64):
    """One pair [*spatial] each -> dict(hausdorff, hd_percentile, assd, n_a, n_b) in fp64 from the transform run in `dtype`."""
    sa, sb = surface(np.asarray(a)[None])[0] != 0, surface(np.asarray(b)[None])[0] != 0
    na, nb = int(sa.sum()), int(sb.sum())
    if na == 0 or nb == 0:
        return dict(hausdorff=np.nan, hd_percentile=np.nan, assd=np.nan, n_a=na, n_b=nb)

    def edt(s):
        if voxel is None:
            return np.sqrt(dist2_f32(s[None])[0]).astype(np.float64) if dtype == np.float32 else np.sqrt(dist2(s[None])[0].astype(np.float64))
        g = dist2(s[None], voxel, dtype)[0]
        return np.sqrt(g).astype(np.float64)

    d_ab, d_ba = edt(sb)[sa], edt(sa)[sb]
    return dict(hausdorff=max(d_ab.max(), d_ba.max()), hd_percentile=float(np.percentile(np.concatenate([d_ab, d_ba]), percentile)),
                assd=0.5 * (d_ab.mean() + d_ba.mean()), n_a=na, n_b=nb)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases: (name, B, spatial, voxel) and their masks [B, *spatial] uint8
# ---------------------------------------------------------------------------------------------------------------------------------------
CASES = [
    ("corner", 1, (5, 6, 7), None),
    ("aniso-and-empty", 2, (9, 10, 11), (3.0, 0.7, 0.9)),
    ("plane", 1, (19, 26), None),
    ("one-voxel-axis", 1, (12, 1, 67), None),
    ("ball", 1, (33, 65, 70), None),
    ("checkerboard", 1, (33, 65, 70), None),
    ("row-ends", 1, (3, 4, 130), (1.0, 1.0, 2.5)),
    ("far-on-z", 1, (130, 3, 4), None),
    ("full", 1, (8, 9, 10), None),
]
BRUTE = 3      # the first cases are also checked against brute()


def case_id(case):
    return case[0]


def ball(shape, centre=None, radius=None):
    """[*shape] bool: the voxels within `radius` (default: a quarter of the smallest extent) of `centre` (default: the middle)."""
    c = [(s - 1) / 2 for s in shape] if centre is None else centre
    r = min(shape) / 4 if radius is None else radius
    g = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    return sum((x - cx) ** 2 for x, cx in zip(g, c)) <= r * r


def case_mask(case):
    name, B, sp, _ = case
    rng = np.random.default_rng(sum(map(ord, name)))
    m = np.zeros((B,) + sp, dtype=np.uint8)
    if name == "corner":
        m[0, 4, 0, 6] = 1
    elif name == "aniso-and-empty":
        m[0] = rng.random(sp) < 0.05      # pair 1 stays empty
    elif name == "plane":
        m[0] = rng.random(sp) < 0.30
    elif name == "one-voxel-axis":
        m[0] = rng.random(sp) < 0.10
    elif name == "ball":
        m[0] = ball(sp)
    elif name == "checkerboard":
        m[0] = np.indices(sp).sum(0) % 2
    elif name == "row-ends":
        m[0, 1, 2, 0] = m[0, 1, 2, 129] = 1
    elif name == "far-on-z":
        m[0, 0, 1, 2] = 1
    elif name == "full":
        m[:] = 1
    assert name == "aniso-and-empty" or m.any()
    return m


@functools.lru_cache(maxsize=None)
def _reference(name):
    case = next(c for c in CASES if c[0] == name)
    m, voxel = case_mask(case), case[3]
    r = dict(mask=m, surface=surface(m))
    if voxel is None:
        r["int"] = dist2(m)
        r["f32"] = dist2_f32(m)
    else:
        r["f64"], r["f32"] = dist2(m, voxel, np.float64), dist2(m, voxel, np.float32)
    for v in r.values():
        v.setflags(write=False)
    return r


def reference(case):
    """dict(mask, surface, int | f64, f32) of a case, computed once and read-only."""
    return _reference(case[0])


def label_maps(B, sp, L, dtype, seed):
    """Two random label maps [B, *sp] that agree on about half of the voxels: values 0 .. L + 1 (two of them >= L), for a signed dtype also some negative;
    label L - 1 is absent from both."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, L + 2, size=(B,) + sp)
    b = np.where(rng.random((B,) + sp) < 0.5, a, rng.integers(0, L + 2, size=(B,) + sp))
    if np.issubdtype(dtype, np.signedinteger):
        a[rng.random(a.shape) < 0.05] = -3
        b[rng.random(b.shape) < 0.05] = -1
    a[a == L - 1] = 0
    b[b == L - 1] = 0
    return a.astype(dtype), b.astype(dtype)


def blobs(sp, seed, count=3):
    """[*sp] bool: the union of a few small balls."""
    rng = np.random.default_rng(seed)
    m = np.zeros(sp, dtype=bool)
    for _ in range(count):
        m |= ball(sp, centre=[rng.uniform(1, s - 2) for s in sp], radius=rng.uniform(1.5, 3.0))
    return m


def between_attainable(d2_values, radius):
    """True when `radius` lies strictly between two attainable distances, at least 1e-3 from either: no rounding decides a threshold at it."""
    d = np.sqrt(np.unique(np.asarray(d2_values, dtype=np.float64)))
    d = d[np.isfinite(d)]
    return bool((d < radius).any() and (d > radius).any() and np.abs(d - radius).min() > 1e-3)
