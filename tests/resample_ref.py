"""fp64 CPU restatement of trx_resample (include/trx.h) with torch ops: per shrinking axis F.pad(replicate) + a 1-D [1,4,6,4,1]/16
convolution, then F.interpolate(size, align_corners), then the per-channel scale.  Also the level rule's pyramid and the flow
hand-over built from it."""
import torch
import torch.nn.functional as F

BINOMIAL = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16


def blur_axis(x, dim):
    """[1,4,6,4,1]/16 along spatial dim `dim` (0-based after [B, C]) with replicate boundaries."""
    xm = x.movedim(2 + dim, -1)
    shp = xm.shape
    flat = xm.reshape(-1, 1, shp[-1])
    flat = F.pad(flat, (2, 2), mode="replicate")
    flat = F.conv1d(flat, BINOMIAL.to(flat.dtype).view(1, 1, 5))
    return flat.reshape(shp).movedim(-1, 2 + dim)


def resample_ref(x, size, align_corners=False, channel_scale=None):
    x = x.detach().to("cpu", torch.float64)
    nd = x.dim() - 2
    size = tuple(int(s) for s in size)
    for d in range(nd):
        if size[d] < x.shape[2 + d]:
            x = blur_axis(x, d)
    if size != tuple(x.shape[2:]):
        x = F.interpolate(x, size=size, mode="trilinear" if nd == 3 else "bilinear", align_corners=bool(align_corners))
    if channel_scale is not None:
        x = x * torch.tensor(channel_scale, dtype=torch.float64).view(1, -1, *([1] * nd))
    return x


def pyramid_ref(x, shapes, align_corners=False):
    """Levels for `shapes` (coarsest first, the last one x's own), each resampled from the level directly above it."""
    out = [x.detach().to("cpu", torch.float64)]
    for s in shapes[-2::-1]:
        out.append(resample_ref(out[-1], s, align_corners))
    return out[::-1]


def upsample_flow_ref(flow, size):
    sp = tuple(flow.shape[2:])
    scale = [1.0 if (S == s or s == 1) else (S - 1) / (s - 1) for S, s in zip(size, sp)]
    return resample_ref(flow, size, align_corners=True, channel_scale=scale)


RESAMPLE_CHUNK_BYTES = 96 << 20   # csrc/pyramid.hip: intermediates of one chunk of volumes


def resample_plan_ref(N, sp, size):
    """The workspace plan of trx_resample, restated on the host: (chunk, t1, t2, t2_offset, ws_bytes).  Axes whose size changes run
    strongest shrink first (smallest So / S; ties: the inner axis first); t1 / t2 are the floats per volume after pass 1 / pass 2 where
    another pass follows; a chunk's intermediates fit RESAMPLE_CHUNK_BYTES; t2 starts on a 64-float boundary; at least 256 bytes."""
    S = (1,) * (3 - len(sp)) + tuple(sp)
    So = (1,) * (3 - len(size)) + tuple(size)
    axes = [a for a in (2, 1, 0) if S[a] != So[a]]
    axes.sort(key=lambda a: So[a] / S[a])             # stable: equal ratios keep the inner axis first
    cur, after = list(S), []
    for a in axes:
        cur[a] = So[a]
        after.append(cur[0] * cur[1] * cur[2])
    t1 = after[0] if len(axes) >= 2 else 0
    t2 = after[1] if len(axes) >= 3 else 0
    per_vol = (t1 + t2) * 4
    chunk = N if per_vol == 0 else max(1, min(N, RESAMPLE_CHUNK_BYTES // per_vol))
    t2_offset = (chunk * t1 + 63) // 64 * 64
    return chunk, t1, t2, t2_offset, max(256, (t2_offset + chunk * t2) * 4)
