"""The case generator of the randomised operator sweeps (tests/fuzz_ops.py): CPU, numpy and torch only, nothing of the package.

draw(family, rng) returns a small record (a dict of ints, floats, tuples and strings) that names a case completely; the *_inputs functions build the
tensors of a record.  Case k of a sweep (family, seed) is drawn from np.random.default_rng([seed, crc32 of the family's name, k]) - a stream of its own, so
the case does not depend on which other cases are evaluated.

The shape rule is shared by all families and is built from the sizes at which the kernels branch:
  nd is 3 with probability 0.65, else 2;
  an axis comes from {1..5}, [6, 40], {63, 64, 65, 66, 70} (one wave), {127, 128, 129, 130} (two waves) or [257, 330] (a second round of 256 in
  edt_line_kernel's range scan, a line longer than one block of the cubic prefilter), at most one axis of a shape from the last group;
  the other axes are halved, the largest first, until the shape has at most 60 000 voxels;
  one shape in eight instead has exactly k 16384 + r voxels, k in {1, 2, 3}, r in {-1, 0, 1, 37}: the seams of the 16384-voxel chunks of
  moments_partial_kernel and label_overlap_kernel and of the 2048-voxel blocks of the Jacobian kernels;
  B is 1, 2 or 3.
Not a test."""
import itertools
import math
import zlib

import numpy as np
import torch

import affine_mi_grids_ref as gref
import bspline_ref
import chain_ref as cr
import flowops_ref as fr
import phantoms as ph
import svf_ref

FAMILIES = ("distance", "surface", "overlap", "moments", "compose", "invert", "jacobian", "spline", "chain", "svf", "bspline", "pyramid")
MAX_VOXELS = 60000
CHUNK = 16384
GROUPS = {"small": (1, 2, 3, 4, 5), "mid": tuple(range(6, 41)), "wave": (63, 64, 65, 66, 70), "two": (127, 128, 129, 130), "long": tuple(range(257, 331))}
GROUP_P = {"small": 0.20, "mid": 0.30, "wave": 0.22, "two": 0.14, "long": 0.14}
AIM_R = (-1, 0, 1, 37)
AIM_CAP = 400      # the longest axis of a shape with an aimed voxel count: the arbiters' cost grows with the square of an axis
LIPSCHITZ = 0.8    # what the invert sweep scales its fields to
# (cases, seed) of the sweeps that tests/test_gpu_fuzz_ops.py runs; tests/test_fuzz_ops_host.py asserts that they select every class that matters
PINNED = {"distance": (32, 1), "surface": (24, 1), "overlap": (24, 1), "moments": (24, 2), "compose": (24, 1), "invert": (24, 1), "jacobian": (24, 1),
          "spline": (24, 1), "chain": (24, 1), "svf": (12, 6), "bspline": (24, 1), "pyramid": (24, 1)}


def case_rng(family, seed, k):
    return np.random.default_rng([int(seed), zlib.crc32(family.encode()), int(k)])      # the name, not its place in FAMILIES: a new family moves no case


def cases(family, n, seed):
    """The records of a sweep, in order."""
    return [draw(family, case_rng(family, seed, k)) for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------------------
def _axis(rng, allow_long):
    names = [g for g in GROUPS if allow_long or g != "long"]
    p = np.array([GROUP_P[g] for g in names])
    g = names[int(rng.choice(len(names), p=p / p.sum()))]
    return int(rng.choice(GROUPS[g])), g


def aimed_shapes(nvox, nd, cap=AIM_CAP):
    """Every shape of nd axes, none above cap, with exactly nvox voxels, sorted."""
    div = [d for d in range(1, cap + 1) if nvox % d == 0]
    out = []
    for head in itertools.product(div, repeat=nd - 1):
        rest, prod = divmod(nvox, math.prod(head))
        if prod == 0 and 1 <= rest <= cap:
            out.append(tuple(head) + (rest,))
    return sorted(out)


def draw_shape(rng, nd=None, long_axis=False):
    """(shape, aimed): aimed is (k, r) where the voxel count was aimed at k 16384 + r, else None.  long_axis: one axis is drawn from [260, 330] (room for
    a sub-box beyond index 256 that does not touch the end), and the count is not aimed."""
    if nd is None:
        nd = 3 if rng.random() < 0.65 else 2
    aim = rng.random() < 0.125
    kr = [(int(rng.choice((1, 2, 3))), int(rng.choice(AIM_R))) for _ in range(8)]      # always drawn: the stream does not depend on the branch
    pick = rng.random()
    if aim and not long_axis:
        for k, r in kr:
            shapes = aimed_shapes(k * CHUNK + r, nd)
            if shapes:
                return shapes[int(pick * len(shapes))], (k, r)
    shape, protected = [], None
    if long_axis:
        protected = int(rng.integers(nd))
    for a in range(nd):
        if a == protected:
            shape.append(int(rng.integers(260, 331)))
            continue
        s, g = _axis(rng, allow_long=protected is None)
        if g == "long":
            protected = a
        shape.append(s)
    if protected is None:
        protected = max(range(nd), key=lambda a: (shape[a], a))
    others = [a for a in range(nd) if a != protected]
    while math.prod(shape) > MAX_VOXELS:
        j = max(others, key=lambda a: (shape[a], a))
        shape[j] = (shape[j] + 1) // 2
    return tuple(shape), None


# ---------------------------------------------------------------------------------------------------------------------------------------
# the records
# ---------------------------------------------------------------------------------------------------------------------------------------
MASK_KINDS = ("single", "d0.002", "d0.05", "d0.5", "subbox")
OVERLAP_L = (1, 2, 5, 255, 256, 257, 4096)
POINT_COUNTS = cr.POINT_COUNTS


def _box(rng, shape, beyond=None):
    """A sub-box [(lo, hi)] per axis (inclusive) that touches neither end of at least one axis, or None when no axis has three voxels.  beyond: that axis,
    and the box lies beyond index 256 of it."""
    free = [a for a, s in enumerate(shape) if s >= 3]
    if not free:
        return None
    inner = beyond if beyond is not None else free[int(rng.integers(len(free)))]
    box = []
    for a, s in enumerate(shape):
        if a == inner:
            lo = int(rng.integers(257 if beyond is not None else 1, s - 1))
            hi = int(rng.integers(lo, s - 1))
        else:
            lo = int(rng.integers(0, s))
            hi = int(rng.integers(lo, s))
        box.append((lo, hi))
    return tuple(box)


def _draw_masks(family, rng):
    beyond = rng.random() < 0.25
    shape, aimed = draw_shape(rng, long_axis=beyond)
    nd = len(shape)
    B = int(rng.choice((1, 2, 3)))
    pool = MASK_KINDS + (("d0.9",) if family == "surface" else ())
    kinds = [pool[i] for i in rng.permutation(len(pool))[:B]]
    empty = rng.random(3) < 0.15
    long_ax = max(range(nd), key=lambda a: shape[a])
    boxes = [None] * B
    if beyond:      # pair 0 holds the sub-box; the kinds stay different per pair
        if "subbox" in kinds:
            kinds[kinds.index("subbox")] = kinds[0]
        kinds[0] = "subbox"
    for b in range(B):
        if empty[b] and not (beyond and b == 0):
            kinds[b] = "empty"
        if kinds[b] == "subbox":
            boxes[b] = _box(rng, shape, long_ax if beyond and b == 0 else None)
            if boxes[b] is None:
                kinds[b] = "d0.05"
    voxel = None
    vox = tuple(float(np.float32(math.exp(v))) for v in rng.uniform(math.log(0.2), math.log(4.0), 3))[:nd]
    if rng.random() < 0.5:
        voxel = vox
    return dict(family=family, shape=shape, aimed=aimed, B=B, kinds=tuple(kinds), boxes=tuple(boxes), beyond256=bool(beyond), voxel=voxel,
                seed=int(rng.integers(1 << 30)))


def _draw_overlap(rng):
    shape, aimed = draw_shape(rng)
    return dict(family="overlap", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), L=int(rng.choice(OVERLAP_L)), dtype=str(rng.choice(("uint8", "int32"))),
                runs=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def _draw_moments(rng):
    shape, aimed = draw_shape(rng)
    return dict(family="moments", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), masked=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def _draw_fields(family, rng):
    shape, aimed = draw_shape(rng)
    amps = {"compose": (0.5, 1.0, 1.5, 2.0), "invert": (0.5, 1.0, 1.5, 2.0)}[family]
    return dict(family=family, shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), amp=float(rng.choice(amps)), noise=float(rng.choice((0.0, 0.01))),
                seed=int(rng.integers(1 << 30)), seed2=int(rng.integers(1 << 30)))


def _draw_jacobian(rng):
    """The fixed cases' fields: svf_ref.smooth_field with noise 0.3 and an amplitude of 0.15 .. 0.45 of the shortest axis of more than one voxel (between
    3 and 40): folds, and determinants on both sides of the threshold, in every case."""
    shape, aimed = draw_shape(rng)
    ref = min([s for s in shape if s > 1] or [3])
    amp = round(float(rng.uniform(0.15, 0.45)) * min(max(ref, 3), 40), 2)
    return dict(family="jacobian", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), amp=amp, seed=int(rng.integers(1 << 30)))


def _draw_chain(rng):
    """out: the output lattice of the image operator; src: the lattice of the image and of the flow.  Without a theta the lattices are equal."""
    out, aimed = draw_shape(rng)
    src, aimed_src = draw_shape(rng, nd=len(out))
    has_theta = bool(rng.random() < 0.8)
    amp = None if has_theta and rng.random() < 0.2 else float(rng.choice((0.8, 1.0, 1.2, 1.4)))
    if not has_theta:
        src, aimed_src = out, aimed
    return dict(family="chain", shape=out, src_shape=src, aimed=aimed, aimed_src=aimed_src, B=int(rng.choice((1, 2, 3))), has_theta=has_theta, amp=amp,
                which=int(rng.integers(2)), padding=str(rng.choice(("border", "zeros"))), order=int(rng.choice((0, 1, 3))), P=int(rng.choice(POINT_COUNTS)),
                seed=int(rng.integers(1 << 30)))


def _draw_spline(rng):
    """shape: the target lattice (the flow's); src: the lattice of x.  Without a theta the lattices are equal.  world: theta is handed over unscaled,
    with the scale of two random voxel-size triples (tests/affine_mi_grids_ref.py::scale_of)."""
    t, aimed = draw_shape(rng)
    m, aimed_src = draw_shape(rng, nd=len(t))
    has_theta = bool(rng.random() < 0.7)
    amp = None if has_theta and rng.random() < 0.3 else float(rng.choice((0.6, 0.8, 1.2, 1.6)))
    world = bool(has_theta and rng.random() < 0.3)
    vox = [tuple(float(np.float32(math.exp(v))) for v in rng.uniform(math.log(0.5), math.log(2.0), len(t))) for _ in range(2)]
    if not has_theta:
        m, aimed_src = t, aimed
    return dict(family="spline", shape=t, src_shape=m, aimed=aimed, aimed_src=aimed_src, B=int(rng.choice((1, 2, 3))), has_theta=has_theta, amp=amp,
                voxels=tuple(vox) if world else None, zoom=float(rng.choice((0.9, 1.0))), order=int(rng.choice((0, 1, 3))), seed=int(rng.integers(1 << 30)))


def _draw_svf(rng):
    shape, aimed = draw_shape(rng)
    return dict(family="svf", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), K=int(rng.integers(1, 8)), inverse=bool(rng.random() < 0.5),
                amp=float(rng.choice((1.0, 2.0, 3.0, 4.0))), seed=int(rng.integers(1 << 30)))


def _draw_bspline(rng):
    shape, aimed = draw_shape(rng)
    return dict(family="bspline", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), spacing=tuple(int(d) for d in rng.integers(1, 10, len(shape))),
                with_base=bool(rng.random() < 0.5), seed=int(rng.integers(1 << 30)))


def out_sizes(S):
    """tests/test_gpu_pyramid_edges.py's output sizes of an axis of S voxels."""
    return sorted({1, 2, -(-S // 4), S // 2, -(-S // 2), S, S + 1, 2 * S, 3 * S + 1} - {0})


def pyramid_levels(shape, most=3, min_size=8):
    """The largest number of levels <= most that torchregister_amd.pyramid_shapes accepts for a shape (its rule, restated)."""
    levels, prev = 1, tuple(shape)
    while levels < most:
        nxt = tuple(s if math.ceil(s / 2) < min_size else math.ceil(s / 2) for s in prev)
        if nxt == prev:
            break
        levels, prev = levels + 1, nxt
    return levels


def _draw_pyramid(rng):
    """size: per axis one of out_sizes (every axis on its own shrinks, grows or keeps its size), at most 2 x 60 000 voxels; up: the lattice upsample_flow
    moves a flow to, every axis keeps its size or grows."""
    shape, aimed = draw_shape(rng)
    nd = len(shape)
    size = shape
    for cand in [tuple(int(rng.choice(out_sizes(s))) for s in shape) for _ in range(6)]:
        if math.prod(cand) <= 2 * MAX_VOXELS:
            size = cand
            break
    up = shape
    for cand in [tuple(int(rng.choice((s, s + 1, 2 * s - 1, 2 * s))) for s in shape) for _ in range(6)]:
        if math.prod(cand) <= 2 * MAX_VOXELS and min(cand) >= 1:
            up = cand
            break
    C = int(rng.choice((1, 2, 3)))
    scale = tuple(round(float(v), 3) for v in rng.uniform(-2.0, 2.0, 3))[:C]
    return dict(family="pyramid", shape=shape, aimed=aimed, B=int(rng.choice((1, 2, 3))), C=C, size=size, up=up, align=int(rng.integers(2)),
                channel_scale=scale if rng.random() < 0.5 else None, levels=pyramid_levels(shape), seed=int(rng.integers(1 << 30)))


def draw(family, rng):
    if family in ("distance", "surface"):
        return _draw_masks(family, rng)
    if family in ("compose", "invert"):
        return _draw_fields(family, rng)
    return {"overlap": _draw_overlap, "moments": _draw_moments, "jacobian": _draw_jacobian, "chain": _draw_chain, "spline": _draw_spline, "svf": _draw_svf,
            "bspline": _draw_bspline, "pyramid": _draw_pyramid}[family](rng)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the inputs of a record
# ---------------------------------------------------------------------------------------------------------------------------------------
def _blobs(rng, shape):
    m = np.zeros(shape, dtype=bool)
    g = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    for _ in range(3):
        c, r = [rng.uniform(0, s - 1) for s in shape], rng.uniform(1.0, 3.0)
        m |= sum((x - cx) ** 2 for x, cx in zip(g, c)) <= r * r
    return m


def mask_inputs(rec):
    """[B, *shape] uint8 of a distance / surface record.  A pair that is not 'empty' has at least one feature."""
    rng = np.random.default_rng(rec["seed"])
    shape = rec["shape"]
    m = np.zeros((rec["B"],) + shape, dtype=np.uint8)
    for b, kind in enumerate(rec["kinds"]):
        one = tuple(int(rng.integers(s)) for s in shape)
        if kind == "empty":
            continue
        if kind == "single":
            m[b][one] = 1
        elif kind == "subbox":
            sl = tuple(slice(lo, hi + 1) for lo, hi in rec["boxes"][b])
            sub = m[b][sl]
            sub[...] = _blobs(rng, sub.shape) | (rng.random(sub.shape) < 0.1)
            if not sub.any():
                sub[tuple(int(rng.integers(s)) for s in sub.shape)] = 1
        else:
            m[b] = rng.random(shape) < float(kind[1:])
            if not m[b].any():
                m[b][one] = 1
    return m


def overlap_inputs(rec):
    """Two label maps [B, *shape] of the record's dtype that agree on about half of the voxels: values 0 .. L + 1 (as far as the dtype reaches), negative
    ones for int32; runs: a is constant over stretches of 1 .. 5000 voxels in memory order (the kernel keeps a run of equal pairs in a register)."""
    rng = np.random.default_rng(rec["seed"])
    full = (rec["B"],) + rec["shape"]
    n = math.prod(full)
    top = min(rec["L"] + 2, 256) if rec["dtype"] == "uint8" else rec["L"] + 2
    if rec["runs"]:
        lengths = rng.choice((1, 7, 300, 5000), size=n)
        lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n)) + 1]
        a = np.repeat(rng.integers(0, top, size=len(lengths)), lengths)[:n].reshape(full)
        b = np.where(rng.random(full) < 0.9, a, rng.integers(0, top, size=full))
    else:
        a = rng.integers(0, top, size=full)
        b = np.where(rng.random(full) < 0.5, a, rng.integers(0, top, size=full))
    if top > rec["L"]:      # values the kernel must count nowhere: 3 % of each map, whatever L is
        a = np.where(rng.random(full) < 0.03, rng.integers(rec["L"], top, size=full), a)
        b = np.where(rng.random(full) < 0.03, rng.integers(rec["L"], top, size=full), b)
    if rec["dtype"] == "int32":
        a = np.where(rng.random(full) < 0.05, -3, a)
        b = np.where(rng.random(full) < 0.05, rng.choice((-1, -3), size=full), b)
    return a.astype(rec["dtype"]), b.astype(rec["dtype"])


def moments_inputs(rec):
    """(x [B,1,*shape] fp32, mask uint8 or None): the fixed test's volumes - a scale and a shift per volume, six decades of dynamic range, so that the
    order of the fp64 sums shows in the bits.  A mask counts at least two voxels of every volume where the volume has two."""
    g = torch.Generator().manual_seed(rec["seed"])
    B, shape = rec["B"], rec["shape"]
    per = lambda v: torch.tensor(v[:B]).reshape(B, 1, *([1] * len(shape)))  # noqa: E731
    x = torch.rand(B, 1, *shape, generator=g) * per([1.0, 3.0, 2.0]) + per([0.5, -2.0, 1.0])
    x = x * torch.exp(16.0 * torch.rand(B, 1, *shape, generator=g) - 8.0)
    mask = None
    if rec["masked"]:
        mask = (torch.rand(B, 1, *shape, generator=g) > 0.4).to(torch.uint8)
        mask.reshape(B, -1)[:, :2] = 1
    return x, mask


def field_inputs(rec):
    """(u, second) fp32 [B, nd, *shape] of a compose / invert record: svf_ref.smooth_field at two seeds.  invert: u is scaled so that
    flowops_ref.lipschitz_bound(u) is at most LIPSCHITZ for every pair, whatever the shape."""
    u = svf_ref.smooth_field(rec["B"], rec["shape"], rec["amp"], rec["seed"], rec["noise"])
    s = svf_ref.smooth_field(rec["B"], rec["shape"], rec["amp"], rec["seed2"], rec["noise"])
    if rec["family"] == "invert":
        lip = fr.lipschitz_bound(u)
        u = (u.double() * torch.clamp(LIPSCHITZ / lip, max=1.0).reshape(-1, *([1] * (u.dim() - 1)))).float()
    return u, s


def jacobian_inputs(rec):
    return svf_ref.smooth_field(rec["B"], rec["shape"], rec["amp"], rec["seed"], noise=0.3)


def chain_inputs(rec):
    """(x [B,2,*src] fp32, theta [B,nd,nd+1] or None, flow [B,nd,*src] or None, points [B,P,nd] on the lattice chain `which` starts from): the fixed
    cases' recipe (chain_ref.case) at the record's shapes and batch."""
    out, src, B = rec["shape"], rec["src_shape"], rec["B"]
    nd = len(out)
    g = torch.Generator().manual_seed(rec["seed"])
    x = torch.cat([torch.cat([ph.blobs(src, rec["seed"] % 1000 + 2 * b + c) for c in range(2)], dim=1) for b in range(B)]) + 0.3 * torch.rand((B, 2) + src, generator=g)
    theta = cr.thetas(nd, g, flat=nd == 3 and out[0] == 1 and src[0] == 1, B=B) if rec["has_theta"] else None
    flow = None if rec["amp"] is None else cr.smooth_flow(src, rec["amp"], g, B=B)
    a = src if rec["which"] == 0 else out
    pts = cr.points_for(a, rec["P"], rec["seed"] % 100000 + rec["P"], B=B)
    return x.float(), theta, flow, pts


def spline_inputs(rec):
    """(x [B,2,*src] fp32, labels [B,2,*src] fp32 of values 0 .. 7, theta [B,nd,nd+1] fp32 or None - the UNSCALED theta -, flow [B,nd,*shape] fp32 or
    None, scale [nd,nd+1] fp64 or None): the fixed cases' recipe (spline_ref.case) at the record's shapes and batch."""
    t, m, B = rec["shape"], rec["src_shape"], rec["B"]
    nd = len(t)
    g = torch.Generator().manual_seed(rec["seed"])
    x = torch.cat([torch.cat([ph.blobs(m, rec["seed"] % 1000 + 2 * b + c) for c in range(2)], dim=1) for b in range(B)]) + 0.3 * torch.rand((B, 2) + m, generator=g)
    labels = torch.randint(0, 8, (B, 2) + m, generator=g).float()
    scale = None if rec["voxels"] is None else gref.scale_of(m, t, rec["voxels"][0], rec["voxels"][1])
    theta = None
    if rec["has_theta"]:
        base = torch.tensor(ph.THETA_ROT3 if nd == 3 else ph.THETA_STAR2, dtype=torch.float64)
        rows = []
        for b in range(B):
            te = base.clone()
            te[:, :nd] = te[:, :nd] * (rec["zoom"] + 0.08 * b) + 0.06 * (torch.rand(nd, nd, generator=g, dtype=torch.float64) - 0.5)
            te[:, nd] = 0.12 * (torch.rand(nd, generator=g, dtype=torch.float64) - 0.5) + (0.06 if b else -0.06)
            rows.append(te if scale is None else te / scale)
        theta = torch.stack(rows).float()
    flow = None if rec["amp"] is None else cr.smooth_flow(t, rec["amp"], g, B=B)
    return x.float(), labels, theta, flow, scale


def svf_inputs(rec):
    """(velocity, dflow) fp32 [B, nd, *shape]: svf_ref.case_inputs' fields - dflow is a smooth field plus noise 0.5."""
    return (svf_ref.smooth_field(rec["B"], rec["shape"], rec["amp"], rec["seed"]),
            svf_ref.smooth_field(rec["B"], rec["shape"], 1.0, rec["seed"] // 2 + 5000, noise=0.5))


def _uniform(shape, g, lo, hi):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def bspline_inputs(rec):
    """(ctrl [B,nd,*grid], base [B,nd,*shape] or None, dflow [B,nd,*shape]) fp32: uniform noise, so that every weight is checked tap by tap."""
    g = torch.Generator().manual_seed(rec["seed"])
    B, sp = rec["B"], rec["shape"]
    nd = len(sp)
    ctrl = _uniform((B, nd) + bspline_ref.grid(sp, rec["spacing"]), g, -1.0, 3.0)
    base = _uniform((B, nd) + sp, g, -2.0, 2.0) if rec["with_base"] else None
    return ctrl, base, _uniform((B, nd) + sp, g, -1.0, 3.0)


def pyramid_inputs(rec):
    """(x [B,C,*shape], flow [B,nd,*shape]) fp32: uniform noise in [-1, 3)."""
    g = torch.Generator().manual_seed(rec["seed"])
    return _uniform((rec["B"], rec["C"]) + rec["shape"], g, -1.0, 3.0), _uniform((rec["B"], len(rec["shape"])) + rec["shape"], g, -1.0, 3.0)


def point_lattices(rec):
    """(from, to) of the points: the flow lives on the source lattice, which chain 0 starts from and chain 1 ends on."""
    return (rec["src_shape"], rec["shape"]) if rec["which"] == 0 else (rec["shape"], rec["src_shape"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the classes the sweeps must select (tests/test_fuzz_ops_host.py counts them over the pinned sweeps)
# ---------------------------------------------------------------------------------------------------------------------------------------
def classes(rec):
    """The names of the classes a record belongs to."""
    shape = rec["shape"]
    nd, nvox = len(shape), math.prod(shape)
    out = set()
    if nd == 2:
        out.add("2d")
    if 1 in shape:
        out.add("axis-of-1")
    if 63 <= shape[-1] <= 66:
        out.add("W-63..66")
    if shape[-1] >= 128:
        out.add("W>=128")
    if shape[-2] >= 257:
        out.add("y>=257")
    if nd == 3 and shape[0] >= 257:
        out.add("z>=257")
    if nvox > CHUNK:
        out.add(">=2-chunks")
    if any(nvox == k * CHUNK + r for k in (1, 2, 3) for r in (-1, 1)):
        out.add("k*16384+-1")
    if rec["family"] in ("distance", "surface"):
        if rec["beyond256"]:
            out.add("sub-box-beyond-256")
        if "subbox" in rec["kinds"]:
            out.add("sub-box")
        if "empty" in rec["kinds"]:
            out.add("empty-pair")
        if rec["B"] == 3 and "empty" not in rec["kinds"]:
            out.add("B3-all-non-empty")
        if rec["B"] >= 2 and sum(k != "empty" for k in rec["kinds"]) >= 2:
            out.add("two-non-empty-pairs")
        if nd == 2 and rec["voxel"] is not None:
            out.add("voxel-2d")
        if rec["voxel"] is not None:
            out.add("voxel")
    if rec["family"] == "chain":
        out.add(f"chain-{rec['which']}")
        if rec["amp"] is not None:
            out.add(f"padding-{rec['padding']}")
    if rec["family"] == "bspline" and any(d > s for d, s in zip(rec["spacing"], shape)):
        out.add("spacing>axis")
    if rec["family"] == "spline" and rec["voxels"] is not None:
        out.add("world-scale")
    if rec["family"] in ("chain", "spline"):
        out.add(f"order-{rec['order']}")
        if max(shape + rec["src_shape"]) >= 257:
            out.add("axis>=257")
        if rec["shape"] != rec["src_shape"]:
            out.add("unequal-lattices")
            if nd == 2:
                out.add("unequal-2d")
    if rec["family"] in ("compose",):
        out.update({"padding-border", "padding-zeros"})      # every compose case runs both
    return out
