"""fp64 numpy restatement of trx_gaussian_resample (include/trx.h), axis by axis.

fp32=True runs the same statements in fp32 - the weights rounded to fp32, every product and every sum in fp32, the taps in the stated order
t = 0 .. 2R, s(i0) before s(i1) - so that conftest.bar(ref32, ref64, floor) can be formed.  floor(x) = 2^-22 max|x|: four ulp at the image's
amplitude; the weights are positive and sum to one, so each pass has condition one, and the growth with R is carried by the bar's own term.
"""
import numpy as np


def radius(sigma, truncate=4.0):
    """R of a sigma in voxels: (int)(truncate sigma + 0.5), scipy.ndimage.gaussian_filter's radius.  (The C ABI receives sigma as fp32: a test that
    compares against the kernel hands the fp32-rounded value to both.)"""
    return int(float(truncate) * float(sigma) + 0.5)


def taps(sigma, truncate=4.0):
    """(R, g): the normalised weights g_t = exp(-((t - R) / sigma)^2 / 2) / sum, t = 0 .. 2R, in fp64."""
    R = radius(sigma, truncate)
    if R == 0:
        return 0, np.ones(1)
    d = (np.arange(2 * R + 1) - R) / float(sigma)
    g = np.exp(-0.5 * d * d)
    return R, g / g.sum()


def positions(S, So, align_corners):
    """(i0, i1, l) of the So outputs along an axis of S voxels: F.interpolate's source positions, u in fp64."""
    j = np.arange(So, dtype=np.float64)
    if S == So:
        i = np.arange(S)
        return i, i, np.zeros(S)
    if align_corners:
        u = j * ((S - 1) / (So - 1) if So > 1 else 0.0)
    else:
        u = np.maximum((j + 0.5) * (S / So) - 0.5, 0.0)
    i0 = np.minimum(u.astype(np.int64), S - 1)
    i1 = i0 + (i0 < S - 1)
    return i0, i1, np.where(i1 == i0, 0.0, u - i0)


def axis_pass(x, axis, So, sigma, truncate, align_corners, padding, fp32):
    dt = np.float32 if fp32 else np.float64
    x = np.moveaxis(np.asarray(x, dtype=dt), axis, -1)
    S = x.shape[-1]
    R, g = taps(sigma, truncate)
    g = g.astype(np.float32).astype(dt) if fp32 else g
    q = np.arange(-R, S + R)
    xp = x[..., np.clip(q, 0, S - 1)]
    if padding == 'zeros':
        xp = xp * ((q >= 0) & (q < S)).astype(dt)
    s = np.zeros(x.shape, dtype=dt)
    for t in range(2 * R + 1):
        s = s + g[t] * xp[..., t:t + S]
    if S != So:
        i0, i1, l = positions(S, So, align_corners)
        l = l.astype(np.float32).astype(dt) if fp32 else l
        s = (dt(1) - l) * s[..., i0] + l * s[..., i1]
    return np.moveaxis(s.astype(dt), -1, axis)


def gaussian_resample(x, size, sigma, align_corners=False, truncate=4.0, padding='border', fp32=False):
    """x [..., *sp] (the last len(size) axes are spatial) -> [..., *size]; sigma: one value per spatial axis, voxels of x.  Passes in the kernel's
    order: strongest shrink first, ties the inner axis first."""
    nd = len(size)
    sp = x.shape[-nd:]
    sigma = [float(s) for s in (sigma if np.ndim(sigma) else [sigma] * nd)]
    axes = [a for a in range(nd - 1, -1, -1) if sp[a] != size[a] or radius(sigma[a], truncate) > 0]
    axes.sort(key=lambda a: size[a] / sp[a])      # (stable: ties keep the inner axis first)
    out = np.asarray(x, dtype=np.float32 if fp32 else np.float64)
    for a in axes:
        out = axis_pass(out, x.ndim - nd + a, size[a], sigma[a], truncate, align_corners, padding, fp32)
    return out


def floor(x):
    return 2.0 ** -22 * float(np.max(np.abs(x)))
