"""Host-side drivers over the C ABI: device state, workspaces and launch wrappers.

PyTorch is used for device memory and streams only; all arithmetic of the hot path happens in
libtrx.so.  Tensors must be fp32 CUDA(HIP) tensors; anything else raises.
"""
import ctypes
import math

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import PSTRIDE


class LossSpec:
    """L = w_mse*MSE + w_ncc*alpha*(1-NCC) + w_ssd*alpha_ssd*SSD (include/trx.h trx_loss_cfg)."""

    def __init__(self, w_mse=0.0, w_ncc=0.0, ncc_alpha=100.0, w_ssd=0.0, ssd_alpha=3.0):
        self.w_mse, self.w_ncc, self.ncc_alpha, self.w_ssd, self.ssd_alpha = map(float, (w_mse, w_ncc, ncc_alpha, w_ssd, ssd_alpha))

    def c(self):
        return _lib.LossCfg(self.w_mse, self.w_ncc, self.ncc_alpha, self.w_ssd, self.ssd_alpha)

    def __repr__(self):
        return f"LossSpec(mse={self.w_mse}, ncc={self.w_ncc}*{self.ncc_alpha}, ssd={self.w_ssd}*{self.ssd_alpha})"


def opt_cfg(optimizer, lr, betas=(0.9, 0.999), eps=1e-8):
    kind = {"sgd": _lib.OPT_SGD, "adam": _lib.OPT_ADAM}.get(str(optimizer).lower())
    if kind is None:
        raise ValueError(f"optimizer must be 'sgd' or 'adam', got {optimizer!r}")
    return _lib.OptCfg(kind, float(lr), float(betas[0]), float(betas[1]), float(eps))


def _reserve(solver, iters):
    """Book `iters` more iterations on a solver's loss curve (`enqueued`: the host-side mirror of the device counter `step`) -> int(iters)."""
    iters = int(iters)
    if solver.enqueued + iters > solver.capacity:
        raise _lib.TrxError(f"loss-curve capacity exceeded: {solver.enqueued} iterations enqueued + {iters} requested > capacity "
                            f"{solver.capacity} (create the solver with a larger `capacity`)")
    solver.enqueued += iters
    return iters


def _require_gpu(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.TrxError(f"{name} is on {t.device}: torchregister_amd runs only on an AMD GPU through its HIP "
                            f"library (no CPU fallback). Move the tensors to 'cuda'.")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")


_TABLES = {}


def base_tables(spatial, device):
    """affine_grid's base coordinates, built with ATen's own CPU expression (bit-exact), on device.  Cached per
    (size, device): the tables are read-only and every warp / solver of that size shares them (no H2D copy per call)."""
    out = []
    for s in spatial:
        key = (int(s), str(device))
        if key not in _TABLES:
            _TABLES[key] = (torch.linspace(-1, 1, int(s), dtype=torch.float32) * (int(s) - 1) / int(s)).to(device)
        out.append(_TABLES[key])
    return out


def _volumes(moving, target, moving_stride, target_stride, spatial, flags=0, tables=None):
    """trx_volumes of B = moving.shape[0] pairs on the lattice `spatial` (the sizes the kernels walk and, on one lattice, sample in): moving / target
    tensors (target None: NULL), their per-pair strides in elements, the flags, and the lattice's base-coordinate tables ((z,) y, x as base_tables
    gives them) or None = the closed form.  The tensors are kept alive by the caller."""
    v = _lib.Volumes()
    v.moving, v.target = moving.data_ptr(), None if target is None else target.data_ptr()
    v.moving_stride, v.target_stride = moving_stride, target_stride
    v.ndim, v.B = len(spatial), moving.shape[0]
    v.D, v.H, v.W = _dhw(spatial)
    v.flags = flags
    if tables is not None:
        v.zn, v.yn, v.xn = (None,) * (3 - len(tables)) + tuple(t.data_ptr() for t in tables)
    return v


class _Batch:
    """A batch of volumes [B, C, *spatial] described for the C ABI."""

    def __init__(self, moving, target=None, tables=True, flags=0):
        self.flags = int(flags)
        _require_gpu(moving, "moving")
        if moving.dim() not in (4, 5):
            raise ValueError(f"expected [B,C,H,W] or [B,C,D,H,W], got {tuple(moving.shape)}")
        self.moving = moving.contiguous()
        self.nd = moving.dim() - 2
        self.B, self.C = moving.shape[0], moving.shape[1]
        self.spatial = tuple(moving.shape[2:])
        self.nvox = 1
        for s in self.spatial:
            self.nvox *= s
        self.device = moving.device
        self.target = None
        if target is not None:
            _require_gpu(target, "target")
            if target.shape[2:] != moving.shape[2:]:
                raise ValueError(f"moving {tuple(moving.shape)} and target {tuple(target.shape)} differ in spatial size")
            self.target = target.contiguous()
        self.tables = base_tables(self.spatial, self.device) if tables else None

    def vol(self, moving_stride=None, target_stride=None):
        if moving_stride is None:
            moving_stride = self.C * self.nvox
        if target_stride is None:
            target_stride = self.target.shape[1] * self.nvox if self.target is not None else 0
        return _volumes(self.moving, self.target, moving_stride, target_stride, self.spatial, self.flags, self.tables)


def pad_theta(theta, nd):
    """[B, nd, nd+1] (or [B, nd*(nd+1)]) -> [B, PSTRIDE] contiguous fp32."""
    B = theta.shape[0]
    out = torch.zeros(B, PSTRIDE, dtype=torch.float32, device=theta.device)
    out[:, : nd * (nd + 1)] = theta.reshape(B, -1).to(torch.float32)
    return out


def pose_to_theta(pose):
    """Theta (ref:utils.py:287-310) in plain torch, used only to initialise the device state."""
    if pose.shape[-1] == 6:
        psi, th, phi = pose[..., 0], pose[..., 1], pose[..., 2]
        c, s = torch.cos, torch.sin
        t = 0.25 * torch.tanh(pose[..., 3:6])
        rows = [c(psi) * c(th), s(phi) * s(psi) * c(th) - c(phi) * s(th), c(phi) * s(psi) * c(th) + s(phi) * s(th), t[..., 0],
                c(psi) * s(th), s(phi) * s(psi) * s(th) + c(phi) * c(th), c(phi) * s(psi) * s(th) - s(phi) * c(th), t[..., 1],
                -s(psi), s(phi) * c(psi), c(phi) * c(psi), t[..., 2]]
        return torch.stack(rows, dim=-1)
    a = pose[..., 0]
    return torch.stack([torch.cos(a), -torch.sin(a), pose[..., 1], torch.sin(a), torch.cos(a), pose[..., 2]], dim=-1)


class _AffineParams:
    """The parameter state of the rigid / affine loops (AffineSolver, AffineMISolver; include/trx.h: trx_affine_state), living on the GPU."""

    def _init_params(self, b, nd, dev, mode, init, capacity):
        """param / theta from the mode and `init`, the optimiser's moments, the records (best_*, losses, step, grad) and `state`, which points at them."""
        self.nd, self.mode = nd, mode
        if mode == "affine":
            th0 = torch.eye(nd, nd + 1, device=dev).repeat(b, 1, 1) if init is None else init.to(dev).reshape(b, nd, nd + 1)
            self.param = pad_theta(th0, nd)
            self.theta = self.param.clone()
        elif mode == "rigid":
            npose = 6 if nd == 3 else 3
            if init is None:
                raise ValueError("rigid mode needs an initial pose (init=[B,%d])" % npose)
            pose = init.to(device=dev, dtype=torch.float32).reshape(b, npose)
            self.param = torch.zeros(b, PSTRIDE, device=dev)
            self.param[:, :npose] = pose
            self.theta = torch.zeros(b, PSTRIDE, device=dev)
            # same fp32 -> fp64 -> fp32 chain as the device finalise / update kernel
            self.theta[:, : nd * (nd + 1)] = pose_to_theta(pose.double()).float()
        else:
            raise ValueError(f"mode must be 'affine' or 'rigid', got {mode!r}")
        self.capacity = int(capacity)
        self.adam_m = torch.zeros(b, PSTRIDE, device=dev)
        self.adam_v = torch.zeros(b, PSTRIDE, device=dev)
        self.best_theta = torch.zeros(b, PSTRIDE, device=dev)
        self.best_loss = torch.full((b,), float("inf"), device=dev)
        self.best_idx = torch.full((b,), -1, dtype=torch.int32, device=dev)
        self.losses = torch.full((b, self.capacity), float("nan"), device=dev)
        self.step = torch.zeros(b, dtype=torch.int32, device=dev)
        self.grad = torch.zeros(b, PSTRIDE, device=dev)
        st = _lib.AffineState()
        st.mode = _lib.PARAM_AFFINE if mode == "affine" else _lib.PARAM_RIGID
        st.param, st.theta = self.param.data_ptr(), self.theta.data_ptr()
        st.adam_m, st.adam_v = self.adam_m.data_ptr(), self.adam_v.data_ptr()
        st.best_theta, st.best_loss, st.best_idx = self.best_theta.data_ptr(), self.best_loss.data_ptr(), self.best_idx.data_ptr()
        st.losses, st.losses_capacity = self.losses.data_ptr(), self.capacity
        st.step, st.grad = self.step.data_ptr(), self.grad.data_ptr()
        self.state = st
        self.enqueued = 0   # iterations enqueued so far (host-side mirror of the device counter `step`)

    def _unpad(self, t):
        nd = self.nd
        return t[:, : nd * (nd + 1)].reshape(-1, nd, nd + 1)

    @property
    def current_theta(self):
        return self._unpad(self.theta).clone()

    @property
    def best(self):
        return self._unpad(self.best_theta).clone()


class AffineSolver(_AffineParams):
    """Batched rigid/affine registration state living on the GPU.

    moving, target: [B,1,*spatial] fp32 on the GPU (B independent pairs).
    mode 'affine': parameters are theta, initialised to identity (or `init` [B,nd,nd+1]).
    mode 'rigid' : parameters are the pose vector (init [B,6] / [B,3]), theta = Theta(pose).
    """

    def __init__(self, moving, target, mode="affine", loss=None, optimizer="sgd", lr=1e-5, init=None, capacity=1000,
                 betas=(0.9, 0.999), eps=1e-8, flags=0, one_kernel="auto"):
        self.lib = _lib.load()
        self.batch = _Batch(moving, target, flags=flags)
        if self.batch.C != 1 or self.batch.target.shape[1] != 1:
            raise ValueError("the optimiser path takes single-channel volumes [B,1,...]")
        if self.batch.target.shape[0] != self.batch.B:
            raise ValueError("moving and target batch sizes differ")
        b, nd, dev = self.batch.B, self.batch.nd, self.batch.device
        self.loss = loss or LossSpec(w_mse=1.0)
        self.opt = opt_cfg(optimizer, lr, betas, eps)
        self._init_params(b, nd, dev, mode, init, capacity)
        self.vol = self.batch.vol()
        self.ws_bytes = self.lib.trx_affine_workspace_bytes(ctypes.byref(self.vol))
        if self.ws_bytes == 0:
            raise _lib.TrxError("trx_affine_workspace_bytes rejected the batch geometry")
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.loss_c = self.loss.c()
        # TRX_FLAG_ONE_KERNEL (include/trx.h): next to the identity a step of a chip-filling 3-D launch is the z-streaming kernel alone.  A hint about
        # speed only (the kernel runs stray pairs itself, slower), so it is set from what the HOST knows without waiting for the device: the
        # initial thetas (trx_affine_near_identity, the kernel's own window test) and, from the second run() call on, the kernel bodies the previous
        # call ended on - copied to pinned memory behind that call and read only if the copy has landed.  one_kernel: "auto" | True | False.
        self._one_policy = one_kernel
        self._note_host = self._note_event = None
        self._base_flags = int(self.vol.flags)
        # ("auto" only for launches of up to 4 x 256^3 voxels: the two empty launches the flag removes cost a fixed ~3.3 us per step - 51.5 against 55.0 us
        # for 16 x 64 x 128 x 128, 77.3 against 80.4 for 2 x 256^3 - while the kernel instance that carries GeomR's body streams 0.5-3 % slower; at the
        # 8 x 256^3 of the headline the two cancel: profiles/r06a_one_kernel_ab.txt)
        small = b * self.batch.nvox <= 4 * 256 ** 3
        if nd == 3 and one_kernel is not False and not (self._base_flags & _lib.FLAG_ONE_KERNEL) and (one_kernel is True or small):
            if one_kernel is True:
                self.vol.flags = self._base_flags | _lib.FLAG_ONE_KERNEL
            else:
                eye = pad_theta(torch.eye(nd, nd + 1).repeat(b, 1, 1), nd)
                if self.lib.trx_affine_near_identity(ctypes.byref(self.vol), ctypes.c_void_p(eye.data_ptr())):   # (is the z-streaming kernel offered to this batch at all?)
                    th_host = self.theta.detach().cpu().contiguous()
                    if self.lib.trx_affine_near_identity(ctypes.byref(self.vol), ctypes.c_void_p(th_host.data_ptr())):
                        self.vol.flags = self._base_flags | _lib.FLAG_ONE_KERNEL
                    self._note_host = torch.empty(b, dtype=torch.int32).pin_memory()
                    self._note_event = torch.cuda.Event()
                    self._note_pending = False

    def _refresh_one_kernel(self):
        """"auto" policy: if the notes of the previous run() call have landed in pinned memory, keep TRX_FLAG_ONE_KERNEL exactly when that call's last
        step ran every pair on the z-streaming tiles (bodies 6 / 8; 3 = GeomR's body inside the one-kernel form, anything else = the kernels behind)."""
        if self._note_host is None or not self._note_pending or not self._note_event.query():
            return
        self._note_pending = False
        body = (self._note_host.abs() >> 24) & 15
        near = bool(((body == 6) | (body == 8)).all().item())
        self.vol.flags = (self._base_flags | _lib.FLAG_ONE_KERNEL) if near else self._base_flags

    def run(self, iters):
        """Enqueue `iters` iterations on the current stream (no host sync)."""
        iters = _reserve(self, iters)
        policy = self._note_host is not None and not torch.cuda.is_current_stream_capturing()   # (a captured run records kernels only: no event, no copy to the host)
        if policy:
            self._refresh_one_kernel()
        with torch.cuda.device(self.batch.device):
            rc = self.lib.trx_affine_run(ctypes.byref(self.vol), ctypes.byref(self.loss_c), ctypes.byref(self.opt),
                                         ctypes.byref(self.state), int(iters), _lib.ptr(self.workspace), self.ws_bytes,
                                         _lib.current_stream(self.batch.device))
            if rc == 0 and iters > 0 and policy and not self._note_pending:
                off = int(self.lib.trx_affine_workspace_rows_offset(ctypes.byref(self.vol)))
                self._note_host.copy_(self.workspace[off:off + 4 * self.batch.B].view(torch.int32), non_blocking=True)
                self._note_event.record(torch.cuda.current_stream(self.batch.device))
                self._note_pending = True
        _lib.check(rc, "trx_affine_run")

    @property
    def one_kernel(self):
        """Is TRX_FLAG_ONE_KERNEL set for the next run() call?"""
        return bool(self.vol.flags & _lib.FLAG_ONE_KERNEL)

    BODIES = {0: "none", 1: "tile-D", 2: "tile-A", 3: "tile-R", 4: "tile-RD", 5: "zstream-fused", 6: "zstream", 7: "eft", 8: "zstream-flat"}

    def _rows_notes(self):
        off = int(self.lib.trx_affine_workspace_rows_offset(ctypes.byref(self.vol)))
        return self.workspace[off:off + 4 * self.batch.B].view(torch.int32).cpu()

    def rows_used(self):
        """Partial rows the last 3-D step's streaming launches wrote per pair ([B] int32; negative: the pair was taken by a kernel launched in
        front of the tile kernel - the z-streaming or the exact-footprint kernel).  Diagnostics / tests; host sync."""
        v = self._rows_notes()
        return torch.sign(v) * (v.abs() & 0xFFFFFF)

    def bodies(self):
        """Which kernel body ran each pair of the last 3-D step (include/trx.h: the note in bits 24-27 of rows_used): list of names."""
        v = self._rows_notes()
        return [self.BODIES.get(int(x), "?") for x in ((v.abs() >> 24) & 15).tolist()]

    CARRY_STRIDE, CARRY_THETA, CARRY_PARAM, CARRY_M, CARRY_V, CARRY_STEP = 64, 0, 12, 24, 36, 48   # csrc/affine_finalize.h: kCarryStride and the record's fields

    def carry_state(self):
        """The two carry buffers of trx_affine_run's one-launch iterations, viewed from the workspace (no copy, no sync): a pair of [B, 64] float
        tensors - per pair theta[12] | param[12] | Adam m[12] | Adam v[12] | step (int bits) | 15 unused floats.  Only launches of the carry form write
        them; 3-D only.  Diagnostics / tests."""
        off = int(self.lib.trx_affine_workspace_carry_offset(ctypes.byref(self.vol)))
        if off == 0:
            raise _lib.TrxError("this batch has no carry buffers (trx_affine_workspace_carry_offset: 2-D or a refused volume)")
        n = 4 * self.batch.B * self.CARRY_STRIDE
        return tuple(self.workspace[off + k * n:off + (k + 1) * n].view(torch.float32).view(self.batch.B, self.CARRY_STRIDE) for k in (0, 1))

    def accumulate_only(self, walk_down=False):
        """Launch only the streaming F1 kernel (partials into the workspace); used for kernel timing.  walk_down: this launch walks the
        z-streaming columns downward (TRX_FLAG_WALK_DOWN) - what every second iteration of run() does."""
        flags = self.vol.flags
        if walk_down:
            self.vol.flags = flags ^ _lib.FLAG_WALK_DOWN
        try:
            with torch.cuda.device(self.batch.device):
                rc = self.lib.trx_affine_accumulate(ctypes.byref(self.vol), _lib.ptr(self.theta), _lib.ptr(self.workspace), self.ws_bytes,
                                                    _lib.current_stream(self.batch.device))
        finally:
            self.vol.flags = flags
        _lib.check(rc, "trx_affine_accumulate")

    def eval_loss(self, theta=None):
        """Loss terms [B,4] = (total, mse, ncc, ssd) at `theta` (default: current theta)."""
        th = self.theta if theta is None else pad_theta(theta.reshape(self.batch.B, -1), self.nd)
        terms = torch.empty(self.batch.B, 4, device=self.batch.device)
        with torch.cuda.device(self.batch.device):
            rc = self.lib.trx_affine_loss(ctypes.byref(self.vol), ctypes.byref(self.loss_c), _lib.ptr(th), _lib.ptr(terms),
                                          _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
        _lib.check(rc, "trx_affine_loss")
        return terms


def affine_warp(theta, moving, *, size=None):
    """get_affine_warp forward on the GPU: moving [B,C,*sp], theta [B,nd,nd+1] -> warped [B,C,*sp].
    size (keyword-only extension): the spatial shape of the output lattice when it is not moving's own - warped [B,C,*size] =
    F.grid_sample(moving, F.affine_grid(theta, [B,C,*size]), align_corners=False), theta being the effective theta affine_grid takes
    (include/trx.h: trx_affine_warp_grids).  No backward on that route."""
    lib = _lib.load()
    if size is not None and tuple(int(s) for s in size) != tuple(moving.shape[2:]):
        return _affine_warp_grids(lib, theta, moving, tuple(int(s) for s in size))
    batch = _Batch(moving)
    th = pad_theta(theta.detach().reshape(batch.B, -1), batch.nd)
    out = torch.empty_like(batch.moving)
    vol = batch.vol()
    with torch.cuda.device(batch.device):
        rc = lib.trx_affine_warp(ctypes.byref(vol), _lib.ptr(th), batch.C, _lib.ptr(out), _lib.current_stream(batch.device))
    _lib.check(rc, "trx_affine_warp")
    return out


def affine_warp_backward(theta, moving, grad_out):
    """d(sum grad_out*warped)/d theta -> [B,nd,nd+1]."""
    lib = _lib.load()
    batch = _Batch(moving)
    _require_gpu(grad_out, "grad_out")
    th = pad_theta(theta.detach().reshape(batch.B, -1), batch.nd)
    go = grad_out.contiguous()
    dth = torch.zeros(batch.B, PSTRIDE, device=batch.device)
    vol = batch.vol()
    ws_bytes = lib.trx_affine_workspace_bytes(ctypes.byref(vol))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=batch.device)
    with torch.cuda.device(batch.device):
        rc = lib.trx_affine_warp_backward(ctypes.byref(vol), _lib.ptr(th), batch.C, _lib.ptr(go), _lib.ptr(dth), _lib.ptr(ws),
                                          ws_bytes, _lib.current_stream(batch.device))
    _lib.check(rc, "trx_affine_warp_backward")
    nd = batch.nd
    return dth[:, : nd * (nd + 1)].reshape(batch.B, nd, nd + 1)


class FlowSolver:
    """Direct dense flow-field optimisation (the flow itself is the parameter), batched."""

    def __init__(self, moving, target, loss=None, optimizer="sgd", lr=1e-3, init=None, capacity=1000, smooth_weight=0.0,
                 betas=(0.9, 0.999), eps=1e-8, stop_crit=None, keep_last=False, flags=0, lncc=None, mi=None, mask=None):
        """stop_crit: the reference's early stop (ref:warpings.py:231-233), tested on the device per pair - a pair whose recorded loss
        is <= stop_crit keeps that iteration's update and ignores every later iteration; `step[b]` = number of recorded losses.
        keep_last: also keep `flow_last`, the flow of the last forward (what the reference's flow_register.flow holds).
        lncc: dict(window=9, alpha=1.0, eps=1e-5) - the data term is the LOCAL-window NCC (extension) instead of `loss`: the whole loop
        (warp, window sums, gradient, smoothness, SGD / Adam) runs in trx_flow_lncc_run, 3-D only.
        mi: dict(bins=32, alpha=1.0, normalized=False, target_range=None, moving_range=None) - the data term is the Parzen joint-histogram
        mutual information (extension, mi_loss_grad) instead of `loss`: the whole loop runs in trx_flow_mi_run, 3-D only.  A range of None
        is fitted once, here, to (target, moving).
        mask (with mi only; see _mask_u8): a region of interest on the target lattice, one per pair - only voxels inside it enter the mutual
        information, so the flow of a voxel outside it gets no data-term gradient; the target's range is fitted inside it; kept alive as `.mask`."""
        if mi is not None and (lncc is not None or loss is not None):
            raise ValueError("mi is a data term of its own: give it without `loss` and without `lncc`")
        if mask is not None:
            if mi is None:
                raise ValueError("mask is the region of interest of the mutual-information data term: give it with `mi`")
            mask = _mask_u8(mask, target)
        self.mask = None
        self.lib = _lib.load()
        self.batch = _Batch(moving, target, tables=False, flags=flags)
        if self.batch.C != 1:
            raise ValueError("the optimiser path takes single-channel volumes [B,1,...]")
        b, nd, dev = self.batch.B, self.batch.nd, self.batch.device
        self.nd = nd
        self.loss = loss or LossSpec(w_mse=1.0)
        self.loss_c = self.loss.c()
        self.opt = opt_cfg(optimizer, lr, betas, eps)
        shape = (b, nd) + self.batch.spatial
        self.flow = torch.zeros(shape, device=dev) if init is None else init.to(device=dev, dtype=torch.float32).reshape(shape).contiguous().clone()
        adam = self.opt.kind == _lib.OPT_ADAM
        self.adam_m = torch.zeros(shape, device=dev) if adam else None
        self.adam_v = torch.zeros(shape, device=dev) if adam else None
        self.flow_tmp = torch.empty(shape, device=dev) if smooth_weight else None
        self.capacity = int(capacity)
        self.losses = torch.full((b, self.capacity), float("nan"), device=dev)
        self.step = torch.zeros(b, dtype=torch.int32, device=dev)
        self.vol = self.batch.vol()
        self.lncc = self.mi = None
        if lncc is not None:
            if nd != 3:
                raise ValueError("the fused local-NCC loop is 3-D only (2-D: LocalNCCLoss through the generic autograd path)")
            self.lncc = (int(lncc.get("window", 9)), float(lncc.get("alpha", 1.0)), float(lncc.get("eps", 1e-5)))
            self.ws_bytes = self.lib.trx_flow_lncc_workspace_bytes(ctypes.byref(self.vol))
        elif mi is not None:
            if nd != 3:
                raise ValueError("the fused mutual-information flow loop is 3-D only (2-D: MILoss through the generic autograd path, or BSplineSolver)")
            self.mi, self.mi_range, self.mask = _mi_cfg(mi, self.batch.target, self.batch.moving, mask)
            self.ws_bytes = self.lib.trx_flow_mi_workspace_bytes(ctypes.byref(self.vol), self.mi.bins)
        else:
            self.ws_bytes = self.lib.trx_flow_workspace_bytes(ctypes.byref(self.vol))
        if self.ws_bytes == 0:
            raise _lib.TrxError("the flow workspace query rejected the batch geometry")
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        st = _lib.FlowState()
        st.flow = self.flow.data_ptr()
        st.flow_tmp = self.flow_tmp.data_ptr() if self.flow_tmp is not None else None
        st.adam_m = self.adam_m.data_ptr() if adam else None
        st.adam_v = self.adam_v.data_ptr() if adam else None
        st.losses, st.losses_capacity, st.step = self.losses.data_ptr(), self.capacity, self.step.data_ptr()
        st.smooth_weight = float(smooth_weight)
        self.stopped = torch.zeros(b, dtype=torch.int32, device=dev) if stop_crit is not None else None
        self.flow_last = torch.empty(shape, device=dev) if (keep_last or stop_crit is not None) else None
        st.stop_crit = float(stop_crit) if stop_crit is not None else 0.0
        st.stopped = self.stopped.data_ptr() if self.stopped is not None else None
        st.flow_last = self.flow_last.data_ptr() if self.flow_last is not None else None
        self.state = st
        self.enqueued = 0

    def run(self, iters):
        iters = _reserve(self, iters)
        with torch.cuda.device(self.batch.device):
            if self.lncc is not None:
                rc = self.lib.trx_flow_lncc_run(ctypes.byref(self.vol), self.lncc[0], self.lncc[1], self.lncc[2], ctypes.byref(self.opt),
                                                ctypes.byref(self.state), int(iters), _lib.ptr(self.workspace), self.ws_bytes,
                                                _lib.current_stream(self.batch.device))
                _lib.check(rc, "trx_flow_lncc_run")
                return
            if self.mi is not None:
                rc = self.lib.trx_flow_mi_run(ctypes.byref(self.vol), ctypes.byref(self.mi), ctypes.byref(self.opt), ctypes.byref(self.state), int(iters),
                                              _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
                _lib.check(rc, "trx_flow_mi_run")
                return
            rc = self.lib.trx_flow_run(ctypes.byref(self.vol), ctypes.byref(self.loss_c), ctypes.byref(self.opt),
                                       ctypes.byref(self.state), int(iters), _lib.ptr(self.workspace), self.ws_bytes,
                                       _lib.current_stream(self.batch.device))
        _lib.check(rc, "trx_flow_run")


def _spacing3(spacing, nd):
    """An int or a per-axis sequence -> the (sz, sy, sx) of the C ABI (2-D: sz = 1) as a tuple of ints >= 1."""
    if isinstance(spacing, bool):
        raise ValueError(f"spacing must be an int >= 1 or {nd} of them, got {spacing!r}")
    sp = list(spacing) if isinstance(spacing, (list, tuple)) else [spacing] * nd
    if len(sp) != nd or any(isinstance(s, bool) or not isinstance(s, int) or s < 1 for s in sp):
        raise ValueError(f"spacing must be an int >= 1 or {nd} of them, got {spacing!r}")
    if max(sp) > 1024:
        raise ValueError(f"spacing {spacing!r}: at most 1024 voxels per axis")
    return (1,) * (3 - nd) + tuple(sp)


def _dhw(spatial):
    return (1,) * (3 - len(spatial)) + tuple(int(s) for s in spatial)


def bspline_grid(spatial, spacing):
    """Control-lattice size of a cubic B-spline free-form deformation: per axis G = (S - 1) // spacing + 4 (trx_bspline_grid; host only)."""
    spatial = tuple(int(s) for s in spatial)
    nd = len(spatial)
    if nd not in (2, 3):
        raise ValueError(f"expected 2 or 3 spatial sizes, got {spatial}")
    grid = (ctypes.c_int * 3)()
    rc = _lib.load().trx_bspline_grid(nd, *_dhw(spatial), *_spacing3(spacing, nd), grid)
    _lib.check(rc, "trx_bspline_grid")
    return tuple(grid)[3 - nd:]


def _bspline_workspace(lib, nd, B, spatial, sp3, device):
    ws_bytes = lib.trx_bspline_workspace_bytes(nd, B, *_dhw(spatial), *sp3)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_bspline_workspace_bytes rejected {B} x {tuple(spatial)} with spacing {sp3[3 - nd:]}")
    return torch.empty(ws_bytes, dtype=torch.uint8, device=device), ws_bytes


def bspline_expand(ctrl, spatial, spacing, base=None):
    """trx_bspline_expand: control tensor [B, nd, *grid] (fp32, GPU) -> dense flow [B, nd, *spatial] (+ base, a dense flow of that shape)."""
    _require_gpu(ctrl, "ctrl")
    spatial = tuple(int(s) for s in spatial)
    nd = len(spatial)
    sp3 = _spacing3(spacing, nd)
    B = ctrl.shape[0]
    if tuple(ctrl.shape) != (B, nd) + bspline_grid(spatial, spacing):
        raise ValueError(f"ctrl shape {tuple(ctrl.shape)} is not [B, {nd}, *{bspline_grid(spatial, spacing)}]")
    lib = _lib.load()
    ctrl = ctrl.detach().contiguous()
    flow = torch.empty((B, nd) + spatial, dtype=torch.float32, device=ctrl.device)
    if base is not None:
        _require_gpu(base, "base")
        if base.shape != flow.shape:
            raise ValueError(f"base shape {tuple(base.shape)} does not match the flow {tuple(flow.shape)}")
        base = base.detach().contiguous()
    ws, ws_bytes = _bspline_workspace(lib, nd, B, spatial, sp3, ctrl.device)
    with torch.cuda.device(ctrl.device):
        rc = lib.trx_bspline_expand(_lib.ptr(ctrl), _lib.ptr(base), _lib.ptr(flow), nd, B, *_dhw(spatial), *sp3, _lib.ptr(ws), ws_bytes,
                                    _lib.current_stream(ctrl.device))
    _lib.check(rc, "trx_bspline_expand")
    return flow


def bspline_reduce(dflow, spacing):
    """trx_bspline_reduce, the adjoint of bspline_expand: dL/dflow [B, nd, *spatial] (fp32, GPU) -> dL/dctrl [B, nd, *grid]."""
    _require_gpu(dflow, "dflow")
    nd = dflow.dim() - 2
    if nd not in (2, 3) or dflow.shape[1] != nd:
        raise ValueError(f"expected a dense flow gradient [B,nd,*spatial], got {tuple(dflow.shape)}")
    spatial = tuple(dflow.shape[2:])
    sp3 = _spacing3(spacing, nd)
    B = dflow.shape[0]
    lib = _lib.load()
    dflow = dflow.detach().contiguous()
    dctrl = torch.empty((B, nd) + bspline_grid(spatial, spacing), dtype=torch.float32, device=dflow.device)
    ws, ws_bytes = _bspline_workspace(lib, nd, B, spatial, sp3, dflow.device)
    with torch.cuda.device(dflow.device):
        rc = lib.trx_bspline_reduce(_lib.ptr(dflow), _lib.ptr(dctrl), nd, B, *_dhw(spatial), *sp3, _lib.ptr(ws), ws_bytes,
                                    _lib.current_stream(dflow.device))
    _lib.check(rc, "trx_bspline_reduce")
    return dctrl


def _bending_weight(value):
    """A finite float >= 0, or ValueError."""
    try:
        w = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"bending_weight must be a finite number >= 0, got {value!r}") from None
    if isinstance(value, bool) or not (w >= 0.0) or w == float("inf"):
        raise ValueError(f"bending_weight must be a finite number >= 0, got {value!r}")
    return w


def bspline_bending(ctrl, spatial, spacing, grad=False):
    """trx_bspline_bending: the bending energy E [B] of a control tensor [B, nd, *grid] (fp32, GPU) - per voxel, the squared second
    derivatives of the B-spline displacement, mixed ones twice - and with grad=True (E, dE/dctrl)."""
    _require_gpu(ctrl, "ctrl")
    spatial = tuple(int(s) for s in spatial)
    nd = len(spatial)
    sp3 = _spacing3(spacing, nd)
    B = ctrl.shape[0]
    if tuple(ctrl.shape) != (B, nd) + bspline_grid(spatial, spacing):
        raise ValueError(f"ctrl shape {tuple(ctrl.shape)} is not [B, {nd}, *{bspline_grid(spatial, spacing)}]")
    lib = _lib.load()
    ctrl = ctrl.detach().contiguous()
    energy = torch.empty(B, dtype=torch.float32, device=ctrl.device)
    dctrl = torch.empty_like(ctrl) if grad else None
    ws, ws_bytes = _bspline_workspace(lib, nd, B, spatial, sp3, ctrl.device)
    with torch.cuda.device(ctrl.device):
        rc = lib.trx_bspline_bending(_lib.ptr(ctrl), _lib.ptr(energy), _lib.ptr(dctrl), 1.0, 0, nd, B, *_dhw(spatial), *sp3, _lib.ptr(ws), ws_bytes,
                                     _lib.current_stream(ctrl.device))
    _lib.check(rc, "trx_bspline_bending")
    return (energy, dctrl) if grad else energy


def _squarings(value):
    """An int in 0 .. 12, or ValueError."""
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= 12:
        raise ValueError(f"squarings must be an int in 0 .. 12, got {value!r}")
    return value


def _svf_call(velocity, squarings, inverse):
    _require_gpu(velocity, "velocity")
    nd = velocity.dim() - 2
    if nd not in (2, 3) or velocity.shape[1] != nd:
        raise ValueError(f"expected a velocity field [B,nd,*spatial], got {tuple(velocity.shape)}")
    K = _squarings(squarings)
    lib = _lib.load()
    vel = velocity.detach().to(torch.float32).contiguous()
    geom = (nd, vel.shape[0]) + _dhw(vel.shape[2:]) + (K, 1 if inverse else 0)
    ws_bytes = lib.trx_svf_workspace_bytes(*geom[:-1])
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_svf_workspace_bytes rejected {tuple(vel.shape)} with {K} squarings")
    return lib, vel, geom, torch.empty(ws_bytes, dtype=torch.uint8, device=vel.device), ws_bytes


def _svf_forward(velocity, squarings, inverse):
    """flow and what the backward needs: (lib, vel, geom, workspace with the kept levels, its size)."""
    call = _svf_call(velocity, squarings, inverse)
    lib, vel, geom, ws, ws_bytes = call
    flow = torch.empty_like(vel)
    with torch.cuda.device(vel.device):
        rc = lib.trx_svf_exp(_lib.ptr(vel), _lib.ptr(flow), *geom, _lib.ptr(ws), ws_bytes, _lib.current_stream(vel.device))
    _lib.check(rc, "trx_svf_exp")
    return flow, call


def _svf_backward(call, dflow):
    lib, vel, geom, ws, ws_bytes = call
    if dflow.shape != vel.shape:
        raise ValueError(f"dflow shape {tuple(dflow.shape)} does not match the velocity {tuple(vel.shape)}")
    _require_gpu(dflow, "dflow")
    dflow = dflow.detach().to(torch.float32).contiguous()
    dvel = torch.empty_like(vel)
    with torch.cuda.device(vel.device):
        rc = lib.trx_svf_exp_backward(_lib.ptr(vel), _lib.ptr(dflow), _lib.ptr(dvel), *geom, _lib.ptr(ws), ws_bytes, _lib.current_stream(vel.device))
    _lib.check(rc, "trx_svf_exp_backward")
    return dvel


class _SvfExpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, velocity, squarings, inverse):
        flow, ctx.call = _svf_forward(velocity, squarings, inverse)
        return flow

    @staticmethod
    def backward(ctx, grad_out):
        call, ctx.call = ctx.call, None      # the kept levels serve one backward
        if call is None:
            raise RuntimeError("svf_exp: backward through the same graph a second time (the kept levels are released after the first)")
        return _svf_backward(call, grad_out), None, None


def svf_exp(velocity, squarings=6, inverse=False):
    """The exponential of a stationary velocity field [B, nd, *spatial] (fp32, GPU; voxel units, channel i along spatial axis i) by scaling and
    squaring (trx_svf_exp): u_0 = +-2^-squarings v, u_{k+1}(x) = u_k(x) + u_k(x + u_k(x)) (bi / trilinear, zeros outside); inverse=True
    integrates -v, the inverse deformation.  Differentiable: the backward is the exact adjoint (trx_svf_exp_backward), so a velocity from
    any torch module can be integrated."""
    _squarings(squarings)
    if torch.is_grad_enabled() and velocity.requires_grad:
        return _SvfExpFn.apply(velocity, squarings, bool(inverse))
    return _svf_forward(velocity, squarings, bool(inverse))[0]


def svf_exp_backward(velocity, dflow, squarings=6, inverse=False):
    """dL/dvelocity for flow = svf_exp(velocity, squarings, inverse) and dL/dflow = dflow: trx_svf_exp followed by trx_svf_exp_backward."""
    return _svf_backward(_svf_forward(velocity, squarings, bool(inverse))[1], dflow)


def _folding_weight(value):
    """A finite float >= 0, or ValueError."""
    try:
        w = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"folding_weight must be a finite number >= 0, got {value!r}") from None
    if isinstance(value, bool) or not (w >= 0.0) or w == float("inf"):
        raise ValueError(f"folding_weight must be a finite number >= 0, got {value!r}")
    return w


def _folding_threshold(value):
    """A finite float, or ValueError."""
    try:
        t = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"folding_threshold must be a finite number, got {value!r}") from None
    if isinstance(value, bool) or not math.isfinite(t):
        raise ValueError(f"folding_threshold must be a finite number, got {value!r}")
    return t


def _dense_flow(flow, name="flow"):
    """flow [B, nd, *spatial] on the GPU -> (lib, fp32 contiguous detached flow, nd, (nd, B, D, H, W))."""
    if not isinstance(flow, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    nd = flow.dim() - 2
    if nd not in (2, 3) or flow.shape[1] != nd or flow.shape[0] < 1:
        raise ValueError(f"expected a dense flow [B,nd,*spatial], got {tuple(flow.shape)}")
    _require_gpu(flow, name)
    fl = flow.detach().contiguous()
    return _lib.load(), fl, nd, (nd, fl.shape[0]) + _dhw(fl.shape[2:])


def jacobian_determinant(flow):
    """The Jacobian determinant map [B, 1, *spatial] of x -> x + flow(x) for a dense flow [B, nd, *spatial] (fp32, GPU; voxel units, channel a along
    spatial axis a - svf_exp's and reg.theta's convention): det(delta_ab + D_b flow_a) with D the central difference, one-sided on the first and last
    voxel of an axis and 0 on an axis of one voxel (trx_flow_jacobian).  det <= 0: the deformation folds there.  The determinant in voxels is the
    determinant in millimetres; behind an initial affine the whole transform's local volume change is this map times the affine's constant determinant."""
    lib, fl, nd, geom = _dense_flow(flow)
    det = torch.empty((fl.shape[0], 1) + tuple(fl.shape[2:]), dtype=torch.float32, device=fl.device)
    with torch.cuda.device(fl.device):
        rc = lib.trx_flow_jacobian(_lib.ptr(fl), *geom, _lib.ptr(det), _lib.current_stream(fl.device))
    _lib.check(rc, "trx_flow_jacobian")
    return det


def folding_penalty_grad(flow, threshold=0.3, weight=1.0, into=None, need_grad=True):
    """trx_flow_folding: (P [B], dflow) for a dense flow [B, nd, *spatial] (fp32, GPU) - P_b = mean_x max(0, threshold - det(x))^2, unweighted, and
    dflow = weight * dP/dflow, added onto `into` (fp32, contiguous, the flow's shape; written in place and returned) when it is given.
    need_grad=False: (P, None)."""
    lib, fl, nd, geom = _dense_flow(flow)
    threshold, weight = _folding_threshold(threshold), _folding_weight(weight)
    ws_bytes = lib.trx_flow_folding_workspace_bytes(*geom)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_flow_folding_workspace_bytes rejected {tuple(fl.shape)}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=fl.device)
    penalty = torch.empty(fl.shape[0], dtype=torch.float32, device=fl.device)
    dflow = None
    if into is not None:
        _require_gpu(into, "into")
        if into.shape != fl.shape or into.dtype != torch.float32 or not into.is_contiguous():
            raise ValueError(f"into must be a contiguous fp32 tensor of the flow's shape {tuple(fl.shape)}")
        dflow = into
    elif need_grad:
        dflow = torch.empty_like(fl)
    with torch.cuda.device(fl.device):
        rc = lib.trx_flow_folding(_lib.ptr(fl), *geom, threshold, weight, _lib.ptr(penalty), _lib.ptr(dflow), 1 if into is not None else 0, _lib.ptr(ws),
                                  ws_bytes, _lib.current_stream(fl.device))
    _lib.check(rc, "trx_flow_folding")
    return penalty, dflow


class _FoldingPenaltyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, threshold):
        penalty, dflow = folding_penalty_grad(flow, threshold)
        ctx.save_for_backward(dflow)
        ctx.dtype = flow.dtype
        return penalty

    @staticmethod
    def backward(ctx, grad_out):
        (dflow,) = ctx.saved_tensors
        return (dflow * grad_out.reshape((-1,) + (1,) * (dflow.dim() - 1))).to(ctx.dtype), None


def folding_penalty(flow, threshold=0.3):
    """The folding penalty P [B] of a dense flow [B, nd, *spatial] (fp32, GPU): P_b = mean_x max(0, threshold - det(x))^2 with det =
    jacobian_determinant(flow) - C^1, and zero where nothing is near a fold (trx_flow_folding).  Differentiable: a flow from any torch module
    (a U-Net, a direct flow) gets the penalty's gradient through autograd, formed with the value in one call.
    The default threshold 0.3 is a choice: the finite-difference determinant is sampled at voxel centres, and the margin above 0 is for what lies
    between them - a field whose sampled determinant stays above 0.3 has room before the interpolated deformation folds."""
    threshold = _folding_threshold(threshold)
    if torch.is_grad_enabled() and flow.requires_grad:
        return _FoldingPenaltyFn.apply(flow, threshold)
    return folding_penalty_grad(flow, threshold, need_grad=False)[0]


_FLOW_PADDING = {"zeros": 0, "border": 1}


def _invert_args(iterations, tol):
    """(iterations, tol) of invert_flow: an int in 1 .. 1000 and a finite float >= 0, or ValueError."""
    if isinstance(iterations, bool) or not isinstance(iterations, int) or not 1 <= iterations <= 1000:
        raise ValueError(f"iterations must be an int in 1 .. 1000, got {iterations!r}")
    try:
        t = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}") from None
    if isinstance(tol, bool) or not (t >= 0.0) or t == float("inf"):
        raise ValueError(f"tol must be a finite number >= 0, got {tol!r}")
    return iterations, t


def _same_field(a, b, what):
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor):
        raise TypeError(f"{what} must be torch.Tensors")
    if a.shape != b.shape:
        raise ValueError(f"{what} must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")


def compose_flows(first, second, padding="border"):
    """c = compose(first, second) for two dense flows [B, nd, *spatial] of one shape (fp32, GPU; voxel units, channel a along spatial axis a):
    c(x) = second(x) + first(x + second(x)) (trx_flow_compose), so that flow_warp(image, c) is flow_warp(flow_warp(image, first), second) with one
    interpolation of the image in place of two.  padding='border' (the default) samples `first` with border extension - a position outside the volume
    takes the value of the nearest face; 'zeros' is svf_exp's sampler, corners outside the volume contributing zero: compose_flows(u, u, 'zeros') is
    one squaring, the bits of svf_exp(2 * u, 1).  Not differentiable."""
    if padding not in _FLOW_PADDING:
        raise ValueError(f"padding must be 'border' or 'zeros', got {padding!r}")
    _same_field(first, second, "first and second")
    lib, f, nd, geom = _dense_flow(first, "first")
    _, s, _, _ = _dense_flow(second, "second")
    f, s = f.to(torch.float32), s.to(torch.float32)
    out = torch.empty_like(s)
    with torch.cuda.device(f.device):
        rc = lib.trx_flow_compose(_lib.ptr(f), _lib.ptr(s), _lib.ptr(out), *geom, _FLOW_PADDING[padding], _lib.current_stream(f.device))
    _lib.check(rc, "trx_flow_compose")
    return out


def invert_flow(flow, iterations=30, tol=1e-3, init=None, return_residual=False):
    """v = the right inverse of a dense flow u [B, nd, *spatial] (fp32, GPU; voxel units) on its lattice: (id + u) o (id + v) = id, by the fixed-point
    iteration v <- -u(y + v) with border extension (trx_flow_invert; one launch, every update of a voxel in registers).  A voxel stops after the first
    update that moves no channel by more than `tol` voxels, or after `iterations` updates; tol=0 runs the fixed count.  init (the flow's shape): the
    starting v, zero when None - a run can be continued from an earlier result.  return_residual=True: (v, residual [B, 1, *spatial]), the size of
    each voxel's last update; a voxel has converged exactly when residual <= tol.  Where u folds it has no inverse: the iteration need not converge
    there, v stays finite, and residual says where - (residual > tol).float().mean() and residual.amax() are the usual summaries.  A non-finite value
    gives NaN in v and residual at the voxels that meet it.  Carry x from the target back: resample(x, flow=invert_flow(u)).  Not differentiable."""
    iterations, tol = _invert_args(iterations, tol)
    if init is not None:
        _same_field(flow, init, "flow and init")
    lib, u, nd, geom = _dense_flow(flow)
    u = u.to(torch.float32)
    v0 = None
    if init is not None:
        v0 = _dense_flow(init, "init")[1].to(torch.float32)
    v = torch.empty_like(u)
    res = torch.empty((u.shape[0], 1) + tuple(u.shape[2:]), dtype=torch.float32, device=u.device) if return_residual else None
    with torch.cuda.device(u.device):
        rc = lib.trx_flow_invert(_lib.ptr(u), _lib.ptr(v0), _lib.ptr(v), _lib.ptr(res), *geom, iterations, tol, _lib.current_stream(u.device))
    _lib.check(rc, "trx_flow_invert")
    return (v, res) if return_residual else v


class BSplineSolver:
    """Cubic B-spline free-form deformation (extension): the control lattice `ctrl` [B, nd, *grid] is the parameter, the displacement field
    is base + expand(ctrl); the whole loop (expand, fused loss and dL/dflow, reduce, SGD / Adam, early stop) runs in trx_bspline_run.
    bending_weight = lambda > 0 adds lambda * (bending energy of ctrl, bspline_bending) to each pair's loss: `losses` and the early stop see
    the total; `base` is not penalised.  After run(): `flow` = expand of the current ctrl (+ base), `flow_last` (keep_last or stop_crit) = the flow of the last forward.
    mi = dict(bins=32, alpha=1.0, normalized=False, target_range=None, moving_range=None): the data term is the Parzen joint-histogram mutual
    information (mi_loss_grad) instead of `loss`, and the loop runs in trx_bspline_mi_run; a range of None is fitted once, here, to (target, moving).
    mask (with mi only; see _mask_u8): a region of interest on the target lattice, one per pair; the target's range is fitted inside it; kept alive as `.mask`.
    squarings = None: the above, launch for launch.  squarings = K (an int in 0 .. 12): diffeomorphic - base + expand(ctrl) is a stationary
    VELOCITY, the deformation is its exponential (svf_exp, K squarings) and the loop runs in trx_bspline_svf_run.  Then `velocity` is the
    expanded lattice (+ base), `flow` = svf_exp(velocity), `flow_last` the exponential of the last forward's velocity (`velocity_last`),
    inverse_flow() = svf_exp(velocity, inverse=True); `base` is a velocity.  Not with `mi`.
    initial (with mi only, not with squarings; ValueError otherwise) = an affine theta [B,nd,nd+1] the deformation is composed with: the warp of
    the loop is affine_flow_warp(moving, initial, flow, initial_scale) and the loop runs in trx_bspline_mi_run_grids.  `moving` may then have a
    spatial shape of its own; ctrl, flow and mask stay on the target lattice, in target voxels; initial_scale [nd,nd+1] (grid_scale; None = ones:
    `initial` is the effective theta).  theta is read on the device on every iteration (kept as `.initial`) and never written.
    folding_weight = w > 0 adds w * folding_penalty(flow, folding_threshold) to each pair's loss, on the TOTAL flow base + expand(ctrl) of every
    forward (the *_fold entry points: trx_bspline_run_fold, trx_bspline_mi_run_fold): `losses` and the early stop see the total, `base` gets no
    gradient.  It works with every route above - fused criteria, mi, initial, mask, overlap, bending_weight - except squarings (ValueError: the
    exponential of a velocity field does not fold).  0 (default): the entry points, launches and bits of before.  The threshold's default 0.3 is
    a margin, see folding_penalty.
    ngf = dict(eta=1.0, alpha=1.0, voxel=None, target_eps=None, moving_eps=None) (NGFLoss.settings): the data term is the normalised gradient field
    (ngf_loss_grad) instead of `loss` / `mi`, and the loop runs in trx_bspline_ngf_run; an eps of None is fitted once, here, to (target, moving)
    (ngf_edge_parameters; kept as `.ngf_eps`).  It takes mask, initial, base, bending_weight and folding_weight; squarings, overlap and
    moving_mask raise ValueError."""

    def __init__(self, moving, target, spacing, loss=None, optimizer="sgd", lr=1e-3, init=None, base=None, capacity=1000, stop_crit=None,
                 keep_last=False, betas=(0.9, 0.999), eps=1e-8, bending_weight=0.0, mi=None, squarings=None, mask=None, initial=None,
                 initial_scale=None, overlap=None, moving_mask=None, folding_weight=0.0, folding_threshold=0.3, ngf=None):
        self.folding_weight, self.folding_threshold = _folding_weight(folding_weight), _folding_threshold(folding_threshold)
        if ngf is not None:
            unknown = set(ngf) - {"eta", "alpha", "voxel", "target_eps", "moving_eps"}
            if unknown:
                raise ValueError(f"unknown normalised-gradient-field settings {sorted(unknown)}")
            if loss is not None or mi is not None:
                raise ValueError("ngf is a data term of its own: give it without `loss` and without `mi`")
            if squarings is not None:
                raise ValueError("squarings (the diffeomorphic model) runs the fused criteria only: the normalised gradient field on a velocity field is not built")
            if overlap or moving_mask is not None:
                raise ValueError("overlap / moving_mask (the overlap rule) are not built for the normalised gradient field: `mask` is its region of interest")
        if squarings is not None and self.folding_weight != 0:
            raise ValueError("folding_weight is the folding penalty of the displacement models: with squarings the deformation is the exponential of a "
                             "velocity field, which does not fold")
        if initial is not None and ((mi is None and ngf is None) or squarings is not None):
            raise ValueError("initial (an affine composed into the deformation) runs the mutual-information loop only: give it with `mi` and without `squarings`")
        self.overlap, moving_mask = overlap_args(overlap, moving_mask, moving)
        if self.overlap and initial is None:
            raise ValueError("overlap / moving_mask (the overlap rule) run in the loop composed with an initial affine: give them with `mi` and `initial`")
        if initial is None and initial_scale is not None:
            raise ValueError("initial_scale is the scale of `initial`: give it with `initial`")
        if mask is not None:
            if mi is None and ngf is None:
                raise ValueError("mask is the region of interest of the mutual-information data term: give it with `mi`")
            mask = _mask_u8(mask, target)
        self.mask = None
        if squarings is not None:
            _squarings(squarings)
            if mi is not None:
                raise ValueError("squarings (the diffeomorphic model) runs the fused criteria only: mutual information on a velocity field is not built")
        self.squarings = squarings
        if mi is not None and loss is not None:
            raise ValueError("mi is a data term of its own: give it without `loss`")
        self.lib = _lib.load()
        self.bending_weight = _bending_weight(bending_weight)
        self.batch = _Batch(moving, target, tables=False) if initial is None else _GridPair(moving, target, scale=initial_scale)
        if self.batch.C != 1:
            raise ValueError("the optimiser path takes single-channel volumes [B,1,...]")
        b, nd, dev = self.batch.B, self.batch.nd, self.batch.device
        self.initial = self.moving_grid = None
        self.moving_mask = None if moving_mask is None else moving_mask.to(dev)
        if initial is not None:
            self.initial, self.moving_grid = _initial_theta(initial, b, nd, dev), self.batch.grid(self.overlap, self.moving_mask)
        self.nd = nd
        self.spacing = _spacing3(spacing, nd)[3 - nd:]
        self.sp3 = (ctypes.c_int * 3)(*_spacing3(spacing, nd))
        self.grid = bspline_grid(self.batch.spatial, self.spacing)
        self.loss = loss or LossSpec(w_mse=1.0)
        self.loss_c = self.loss.c()
        self.opt = opt_cfg(optimizer, lr, betas, eps)
        cshape, fshape = (b, nd) + self.grid, (b, nd) + self.batch.spatial
        if init is None:
            self.ctrl = torch.zeros(cshape, device=dev)
        else:
            if tuple(init.shape) != cshape:
                raise ValueError(f"init shape {tuple(init.shape)} is not the control tensor's {cshape}")
            self.ctrl = init.to(device=dev, dtype=torch.float32).contiguous().clone()
        self.base = None
        if base is not None:
            _require_gpu(base, "base")
            if tuple(base.shape) != fshape:
                raise ValueError(f"base shape {tuple(base.shape)} is not the flow's {fshape}")
            self.base = base.detach().contiguous()
        adam = self.opt.kind == _lib.OPT_ADAM
        self.adam_m = torch.zeros(cshape, device=dev) if adam else None
        self.adam_v = torch.zeros(cshape, device=dev) if adam else None
        self.flow = torch.empty(fshape, device=dev)       # squarings: the velocity the loop writes; .flow is replaced by its exponential
        self.dflow = torch.empty(fshape, device=dev)
        self.velocity = self.flow if squarings is not None else None
        self.capacity = int(capacity)
        self.losses = torch.full((b, self.capacity), float("nan"), device=dev)
        self.step = torch.zeros(b, dtype=torch.int32, device=dev)
        self.stopped = torch.zeros(b, dtype=torch.int32, device=dev) if stop_crit is not None else None
        self.flow_last = torch.empty(fshape, device=dev) if (keep_last or stop_crit is not None) else None
        self.velocity_last = self.flow_last if squarings is not None else None
        self.vol = self.batch.vol()
        self.mi = self.ngf = None
        self.fold = _lib.FoldCfg(self.folding_weight, self.folding_threshold) if self.folding_weight > 0 else None
        if ngf is not None:
            # eps is fitted once, here, to (target, moving); with `initial` to the moving image as that affine puts it on the target lattice
            voxel = _ngf_voxel(ngf.get("voxel"), nd)
            self.mask = None if mask is None else mask.to(dev)
            seen = self.batch.moving
            if initial is not None and ngf.get("moving_eps") is None:
                seen = affine_flow_warp(self.batch.moving, initial.detach().to(dev), torch.zeros(fshape, device=dev), initial_scale)
            self.ngf_eps = ngf_settings_eps(ngf, self.batch.target, seen, voxel, self.mask)
            self.ngf, self._ngf_voxel = _ngf_cfg_c(ngf.get("alpha", 1.0), self.ngf_eps, voxel, self.mask)
            self.ws_bytes = self.lib.trx_bspline_ngf_workspace_bytes(nd, b, *_dhw(self.batch.spatial), *self.sp3,
                                                                     None if self.moving_grid is None else ctypes.byref(self.moving_grid))
            if self.ws_bytes == 0:
                raise _lib.TrxError(f"trx_bspline_ngf_workspace_bytes rejected {b} x {tuple(self.batch.spatial)} with spacing {self.spacing}")
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        elif squarings is not None:
            self.ws_bytes = self.lib.trx_bspline_svf_workspace_bytes(nd, b, *_dhw(self.batch.spatial), *self.sp3, squarings)
            if self.ws_bytes == 0:
                raise _lib.TrxError(f"trx_bspline_svf_workspace_bytes rejected {b} x {tuple(self.batch.spatial)} with spacing {self.spacing}")
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        elif mi is not None:
            self.mi, self.mi_range, self.mask = _mi_cfg(mi, self.batch.target, self.batch.moving, mask, self.overlap, self.moving_mask)
            query = self.lib.trx_bspline_mi_grids_workspace_bytes if self.fold is None else self.lib.trx_bspline_mi_fold_workspace_bytes
            self.ws_bytes = query(nd, b, *_dhw(self.batch.spatial), *self.sp3, self.mi.bins, None if self.moving_grid is None else ctypes.byref(self.moving_grid))
            if self.ws_bytes == 0:
                raise _lib.TrxError(f"trx_bspline_mi_grids_workspace_bytes rejected {b} x {tuple(self.batch.spatial)} with spacing {self.spacing}")
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        elif self.fold is not None:
            self.ws_bytes = self.lib.trx_bspline_fold_workspace_bytes(nd, b, *_dhw(self.batch.spatial), *self.sp3)
            if self.ws_bytes == 0:
                raise _lib.TrxError(f"trx_bspline_fold_workspace_bytes rejected {b} x {tuple(self.batch.spatial)} with spacing {self.spacing}")
            self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        else:
            self.workspace, self.ws_bytes = _bspline_workspace(self.lib, nd, b, self.batch.spatial, tuple(self.sp3), dev)
        st = _lib.BSplineState()
        st.ctrl = self.ctrl.data_ptr()
        st.adam_m = self.adam_m.data_ptr() if adam else None
        st.adam_v = self.adam_v.data_ptr() if adam else None
        st.base = self.base.data_ptr() if self.base is not None else None
        st.flow, st.dflow = self.flow.data_ptr(), self.dflow.data_ptr()       # (squarings: self.flow is still the velocity buffer here)
        st.losses, st.losses_capacity, st.step = self.losses.data_ptr(), self.capacity, self.step.data_ptr()
        st.stop_crit = float(stop_crit) if stop_crit is not None else 0.0
        st.stopped = self.stopped.data_ptr() if self.stopped is not None else None
        st.flow_last = self.flow_last.data_ptr() if self.flow_last is not None else None
        st.bending_weight = self.bending_weight
        self.state = st
        self.enqueued = 0
        self._expand()

    def _expand(self):
        """flow = base + expand(ctrl): the same call the loop makes, so the bits are those of a forward at the current ctrl.  With squarings
        that is the velocity, and flow / flow_last become the exponentials of velocity / velocity_last."""
        D, H, W = _dhw(self.batch.spatial)
        dst = self.flow if self.squarings is None else self.velocity
        with torch.cuda.device(self.batch.device):
            rc = self.lib.trx_bspline_expand(_lib.ptr(self.ctrl), _lib.ptr(self.base), _lib.ptr(dst), self.nd, self.batch.B, D, H, W, *self.sp3,
                                             _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
        _lib.check(rc, "trx_bspline_expand")
        if self.squarings is not None:
            self.flow = svf_exp(self.velocity, self.squarings)
            if self.velocity_last is not None and self.enqueued > 0:
                self.flow_last = svf_exp(self.velocity_last, self.squarings)

    def valid_fraction(self, flow=None):
        """[B] fp32: the voxels that enter the criterion at `flow` [B,nd,*target spatial] over the target-mask voxels (or N) - 1 without the
        overlap rule.  flow None: `.flow`, the expansion of the CURRENT control points - after run() that is the flow of the updated lattice, one
        step past the last forward whose loss was recorded; pass `.flow_last` for that one (what flow_register returns and reports).  One
        trx_affine_flow_valid call whose bytes are summed."""
        B, dev = self.batch.B, self.batch.device
        total = torch.full((B,), float(math.prod(self.batch.spatial)), device=dev) if self.mask is None else self.mask.reshape(B, -1).sum(1).float()
        if not self.overlap:
            return (total > 0).float()
        valid = affine_flow_valid(self.batch.moving.shape[2:], self.initial, self.flow if flow is None else flow, self.batch.scale, self.mask, self.moving_mask)
        return valid.reshape(B, -1).sum(1).float() / total.clamp(min=1.0)

    def inverse_flow(self):
        """svf_exp(velocity, inverse=True): the inverse of `flow` (diffeomorphic model only)."""
        if self.squarings is None:
            raise ValueError("inverse_flow() needs the diffeomorphic model: create the solver with squarings=K")
        return svf_exp(self.velocity, self.squarings, inverse=True)

    def _run_fold(self, iters):
        """The *_fold entry point of this solver's route (folding_weight > 0)."""
        stream = _lib.current_stream(self.batch.device)
        if self.mi is not None:
            mg, theta = (None, None) if self.initial is None else (ctypes.byref(self.moving_grid), _lib.ptr(self.initial))
            rc = self.lib.trx_bspline_mi_run_fold(ctypes.byref(self.vol), mg, theta, ctypes.byref(self.mi), ctypes.byref(self.opt), ctypes.byref(self.state),
                                                  self.sp3, ctypes.byref(self.fold), iters, _lib.ptr(self.workspace), self.ws_bytes, stream)
            return rc, "trx_bspline_mi_run_fold"
        rc = self.lib.trx_bspline_run_fold(ctypes.byref(self.vol), ctypes.byref(self.loss_c), ctypes.byref(self.opt), ctypes.byref(self.state), self.sp3,
                                           ctypes.byref(self.fold), iters, _lib.ptr(self.workspace), self.ws_bytes, stream)
        return rc, "trx_bspline_run_fold"

    def run(self, iters):
        iters = _reserve(self, iters)
        if self.ngf is not None:      # one entry point for every route: one lattice or through `initial`, with or without the folding penalty
            mg, theta = (None, None) if self.initial is None else (ctypes.byref(self.moving_grid), _lib.ptr(self.initial))
            with torch.cuda.device(self.batch.device):
                rc = self.lib.trx_bspline_ngf_run(ctypes.byref(self.vol), mg, theta, ctypes.byref(self.ngf), ctypes.byref(self.opt), ctypes.byref(self.state),
                                                  self.sp3, None if self.fold is None else ctypes.byref(self.fold), iters, _lib.ptr(self.workspace),
                                                  self.ws_bytes, _lib.current_stream(self.batch.device))
            _lib.check(rc, "trx_bspline_ngf_run")
            return self._expand()
        if self.fold is not None:
            with torch.cuda.device(self.batch.device):
                rc, what = self._run_fold(iters)
            _lib.check(rc, what)
            return self._expand()
        with torch.cuda.device(self.batch.device):
            if self.squarings is not None:
                rc = self.lib.trx_bspline_svf_run(ctypes.byref(self.vol), ctypes.byref(self.loss_c), ctypes.byref(self.opt), ctypes.byref(self.state),
                                                  self.sp3, self.squarings, iters, _lib.ptr(self.workspace), self.ws_bytes,
                                                  _lib.current_stream(self.batch.device))
            elif self.initial is not None:
                rc = self.lib.trx_bspline_mi_run_grids(ctypes.byref(self.vol), ctypes.byref(self.moving_grid), _lib.ptr(self.initial), ctypes.byref(self.mi),
                                                       ctypes.byref(self.opt), ctypes.byref(self.state), self.sp3, iters, _lib.ptr(self.workspace),
                                                       self.ws_bytes, _lib.current_stream(self.batch.device))
            elif self.mi is not None:
                rc = self.lib.trx_bspline_mi_run(ctypes.byref(self.vol), ctypes.byref(self.mi), ctypes.byref(self.opt), ctypes.byref(self.state),
                                                 self.sp3, iters, _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
            else:
                rc = self.lib.trx_bspline_run(ctypes.byref(self.vol), ctypes.byref(self.loss_c), ctypes.byref(self.opt), ctypes.byref(self.state),
                                              self.sp3, iters, _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
        _lib.check(rc, "trx_bspline_svf_run" if self.squarings is not None else "trx_bspline_mi_run_grids" if self.initial is not None else
                   "trx_bspline_mi_run" if self.mi is not None else "trx_bspline_run")
        self._expand()


def flow_warp(moving, flow, nearest=False):
    """SpatialTransformer forward: moving [B,C,*sp], flow [B,nd,*sp] -> [B,C,*sp]; nearest: mode='nearest' (round half to even, zeros outside)."""
    lib = _lib.load()
    batch = _Batch(moving, tables=False, flags=_lib.FLAG_NEAREST if nearest else 0)
    _require_gpu(flow, "flow")
    fl = flow.detach().contiguous()
    if fl.shape != (batch.B, batch.nd) + batch.spatial:
        raise ValueError(f"flow shape {tuple(fl.shape)} does not match moving {tuple(moving.shape)}")
    out = torch.empty_like(batch.moving)
    vol = batch.vol()
    with torch.cuda.device(batch.device):
        rc = lib.trx_flow_warp(ctypes.byref(vol), _lib.ptr(fl), batch.C, _lib.ptr(out), _lib.current_stream(batch.device))
    _lib.check(rc, "trx_flow_warp")
    return out


def flow_warp_backward(moving, flow, grad_out):
    lib = _lib.load()
    batch = _Batch(moving, tables=False)
    fl, go = flow.detach().contiguous(), grad_out.contiguous()
    dfl = torch.empty_like(fl)
    vol = batch.vol()
    with torch.cuda.device(batch.device):
        rc = lib.trx_flow_warp_backward(ctypes.byref(vol), _lib.ptr(fl), batch.C, _lib.ptr(go), _lib.ptr(dfl),
                                        _lib.current_stream(batch.device))
    _lib.check(rc, "trx_flow_warp_backward")
    return dfl


def flow_loss_grad(moving, target, flow, loss, need_grad=True):
    """Fused loss (+ dL/dflow) for a given flow: returns (terms [B,4], dflow or None)."""
    lib = _lib.load()
    batch = _Batch(moving, target, tables=False)
    fl = flow.detach().contiguous()
    terms = torch.empty(batch.B, 4, device=batch.device)
    dfl = torch.empty_like(fl) if need_grad else None
    vol = batch.vol()
    ws_bytes = lib.trx_flow_workspace_bytes(ctypes.byref(vol))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=batch.device)
    lc = loss.c()
    with torch.cuda.device(batch.device):
        rc = lib.trx_flow_loss_grad(ctypes.byref(vol), ctypes.byref(lc), _lib.ptr(fl), _lib.ptr(terms), _lib.ptr(dfl), _lib.ptr(ws),
                                    ws_bytes, _lib.current_stream(batch.device))
    _lib.check(rc, "trx_flow_loss_grad")
    return terms, dfl


class _PeerMemory:
    """Fine-grained device memory of the peer transport: an allocation of this process (trx_peer_alloc) or the mapping of a peer's
    (trx_peer_import), handed to torch through __cuda_array_interface__ (no copy; the tensor keeps this object alive)."""

    def __init__(self, ptr, nbytes, owned):
        self.lib = _lib.load()
        self.ptr, self.nbytes, self.owned = int(ptr), int(nbytes), bool(owned)

    @staticmethod
    def allocate(nbytes):
        lib = _lib.load()
        p = ctypes.c_void_p()
        _lib.check(lib.trx_peer_alloc(int(nbytes), ctypes.byref(p)), "trx_peer_alloc")
        return _PeerMemory(p.value, nbytes, True)

    @staticmethod
    def open(handle, nbytes):
        lib = _lib.load()
        buf = ctypes.create_string_buffer(bytes(handle), 64)
        p = ctypes.c_void_p()
        _lib.check(lib.trx_peer_import(buf, ctypes.byref(p)), "trx_peer_import")
        return _PeerMemory(p.value, nbytes, False)

    def export(self):
        buf = ctypes.create_string_buffer(64)
        _lib.check(self.lib.trx_peer_export(self.ptr, buf), "trx_peer_export")
        return bytes(buf.raw)

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2, "strides": None}

    def tensor(self):
        t = torch.as_tensor(self)   # (no device argument: a mapping of a peer's memory must stay where it is, not be copied here)
        if t.data_ptr() != self.ptr or t.numel() != self.nbytes or t.dtype != torch.uint8:
            raise RuntimeError("torch did not wrap the peer memory in place")
        t._trx_mem = self
        return t

    def close(self):
        if self.ptr:
            (self.lib.trx_peer_free if self.owned else self.lib.trx_peer_close)(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.close()
        except Exception:   # noqa: BLE001 - interpreter shutdown
            pass


class SlabPeers:
    """Peer-mapped transport for SlabFlowSolver (include/trx.h: trx_peer_*): one MAILBOX per rank - device memory that the other ranks
    of the node write into directly (HIP IPC / peer access; xGMI between GPUs) - instead of torch.distributed P2P and all_reduce.

    Mailbox of rank r (one uint8 tensor): [parity 0, 1] x (halo_lo [3,H,W] f32, halo_hi [3,H,W] f32, slots [N,8] f64) | flags: lo, hi,
    sums[N] (uint32 iteration numbers, only ever raised).  Use:
        box = SlabPeers.allocate(device, H, W, world)            # on every rank
        peers = SlabPeers.exchange(box, group)                   # IPC handles through the process group -> the N mailboxes, mapped
        solver = SlabFlowSolver(..., peers=SlabPeers(rank, peers, H, W))
    In one process (several slabs driven in lock step on one or several GPUs: run_slabs_lockstep) the mailboxes are passed as they are."""

    TIMEOUT_US = 5_000_000          # per wait
    FIRST_WAIT_FACTOR = 6           # the FIRST iteration of a transport waits this many times as long (peers still build their solvers)

    @staticmethod
    def layout(H, W, world):
        plane = 3 * H * W * 4
        slots = world * 8 * 8
        per_parity = 2 * plane + slots
        flags_off = 2 * per_parity
        total = flags_off + (2 + world) * 4
        return plane, slots, per_parity, flags_off, (total + 255) // 256 * 256

    @staticmethod
    def allocate(device, H, W, world, finegrained=True):
        """This rank's mailbox as a uint8 tensor.  finegrained (default): memory from trx_peer_alloc - hipExtMallocWithFlags(
        hipDeviceMallocFinegrained) - whose remote writes a polling kernel sees without a kernel boundary, shared with the peers by its raw
        HIP IPC handle; False: a tensor of torch's caching allocator (coarse-grained: only for slabs driven from ONE process)."""
        nbytes = SlabPeers.layout(H, W, world)[4]
        if not finegrained:
            return torch.zeros(nbytes, dtype=torch.uint8, device=device)
        device = torch.device(device)
        with torch.cuda.device(device):
            mem = _PeerMemory.allocate(nbytes)
        return mem.tensor()

    @staticmethod
    def export_handle(box):
        """LOCAL half of exchange(): what this rank sends to its peers so that they can map `box` (no collective inside).  Fine-grained
        mailbox: its raw HIP IPC handle (no dependence on the sender's device numbering); torch tensor: torch's CUDA-IPC tuple."""
        mem = getattr(box, "_trx_mem", None)
        if mem is not None:
            return ("raw", mem.export(), box.numel())
        return ("torch", box.untyped_storage()._share_cuda_(), box.numel())

    @staticmethod
    def open_handles(box, handles, rank):
        """LOCAL half of exchange(): maps the peers' mailboxes from the gathered handles (this rank's own entry is `box` itself)."""
        boxes = []
        for r, h in enumerate(handles):
            if r == rank:
                boxes.append(box)
                continue
            if h is None:
                raise RuntimeError(f"rank {r} sent no mailbox handle")
            kind, payload, n = h
            if kind == "raw":
                with torch.cuda.device(box.device):
                    boxes.append(_PeerMemory.open(payload, n).tensor())
            else:
                if int(payload[0]) >= torch.cuda.device_count():
                    raise RuntimeError(f"mailbox of rank {r} lives on device {int(payload[0])}, which this process cannot see "
                                       f"({torch.cuda.device_count()} visible): the peer transport needs every GPU of the node visible in every rank")
                st = torch.UntypedStorage._new_shared_cuda(*payload)
                boxes.append(torch.empty(0, dtype=torch.uint8, device=st.device).set_(st))
        return boxes

    @staticmethod
    def exchange(box, group=None):
        """All-gathers the IPC handles of the ranks' mailboxes over `group` and maps them: the list of the N mailboxes (this rank's own
        entry is `box` itself).  The mailbox must be the only tensor of its storage (allocate() guarantees it).  Every rank must see
        every GPU of the group (no per-rank HIP_VISIBLE_DEVICES): a handle is re-opened on the SENDER's device index.  A local failure
        raises on that rank only - use try_exchange() where the ranks must reach one decision."""
        import torch.distributed as dist
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        handles = [None] * world
        dist.all_gather_object(handles, SlabPeers.export_handle(box), group=group)
        return SlabPeers.open_handles(box, handles, rank)

    @staticmethod
    def agree(ok_local, group=None):
        """True iff EVERY rank of the group reports success (a MIN all-reduce through the group's own backend): the decision to use a
        transport must be the same on all ranks - one rank on mailboxes and its neighbour on torch.distributed would dead-lock."""
        import torch.distributed as dist
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
        t = torch.tensor([1 if ok_local else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN, group=group)
        return bool(t.item())

    @staticmethod
    def try_exchange(device, H, W, rank, group=None, _alloc=None, _export=None, _open=None):
        """Mailbox transport if it can be set up on EVERY rank, else None (the caller keeps torch.distributed): returns (SlabPeers or None,
        reason).  What can fail: the allocation or the IPC export of the mailbox, the IPC import of a peer's, peer access between two
        devices, a GPU that is not visible in some rank.  Every rank runs the SAME sequence of collectives whatever fails locally
        (ADVICE r4): [local] allocate + export -> agree -> all-gather of the handles -> [local] import + peer-access probe -> agree;
        the local steps contain no collective, so a rank that fails in one still meets the others in the next.  `_alloc` / `_export` /
        `_open` replace allocate / export_handle / open_handles in the tests."""
        import logging
        import torch.distributed as dist
        world = dist.get_world_size(group)
        log = logging.getLogger("torchregister_amd")

        def give_up(reason):
            why = reason or "another rank could not set up its mailbox"
            log.warning("peer transport unavailable (%s): falling back to torch.distributed", why)
            return None, why

        box, payload, reason = None, None, ""
        try:   # local: this rank's mailbox and its handle
            box = (_alloc or SlabPeers.allocate)(device, H, W, world)
            payload = (_export or SlabPeers.export_handle)(box)
        except Exception as e:   # noqa: BLE001 - any failure means "use the other transport"
            box, reason = None, f"{type(e).__name__}: {e}"
        if not SlabPeers.agree(box is not None, group):
            return give_up(reason)
        handles = [None] * world
        dist.all_gather_object(handles, payload, group=group)
        boxes = None
        try:   # local: map the peers' mailboxes; a cross-device mapping that cannot be read shows here, not in the middle of a run
            boxes = (_open or SlabPeers.open_handles)(box, handles, dist.get_rank(group))
            for b in boxes:
                if b.device != box.device:
                    if not torch.cuda.can_device_access_peer(box.device.index, b.device.index):
                        raise RuntimeError(f"no peer access from device {box.device.index} to device {b.device.index}")
                    _ = b[:4].to(box.device)   # (also makes torch enable peer access between the two devices: hipDeviceEnablePeerAccess)
        except Exception as e:   # noqa: BLE001
            boxes, reason = None, f"{type(e).__name__}: {e}"
        if not SlabPeers.agree(boxes is not None, group):
            return give_up(reason)
        return SlabPeers(rank, boxes, H, W), "peer-mapped mailboxes"

    def __init__(self, rank, boxes, H, W):
        self.lib = _lib.load()
        self.rank, self.world, self.boxes = int(rank), len(boxes), boxes
        self.H, self.W = int(H), int(W)
        self.plane, self.slots_bytes, self.per_parity, self.flags_off, total = SlabPeers.layout(H, W, self.world)
        for b in boxes:
            if b.numel() < total:
                raise ValueError("mailbox smaller than SlabPeers.layout")
        self.mine = boxes[self.rank]
        dev = self.mine.device
        self.device = dev
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.t = 0          # iterations completed through this transport (flag values are t + 1)
        # this rank's slot and flag inside every peer's mailbox, as device arrays of pointers, per parity
        self._slot_ptrs, self._flag_ptrs = [], None
        for par in (0, 1):
            ptrs = [b.data_ptr() + par * self.per_parity + 2 * self.plane + self.rank * 64 for b in boxes]
            self._slot_ptrs.append(torch.tensor(ptrs, dtype=torch.int64, device=dev))
        self._flag_ptrs = torch.tensor([b.data_ptr() + self.flags_off + (2 + self.rank) * 4 for b in boxes], dtype=torch.int64, device=dev)

    # -- views into mailboxes
    def halo(self, box, par, which):
        off = par * self.per_parity + (0 if which == "lo" else self.plane)
        return box[off:off + self.plane].view(torch.float32).view(3, self.H, self.W)

    def _flag_ptr(self, box, idx):
        return box.data_ptr() + self.flags_off + idx * 4

    def _stream(self):
        return _lib.current_stream(self.device)

    def put_halos(self, lo_plane, hi_plane, has_lo, has_hi):
        """This rank's lowest / highest flow plane into the halo_hi slot of the rank below / the halo_lo slot of the rank above, then
        their flags; on the current stream."""
        par, v = self.t & 1, self.t + 1
        with torch.cuda.device(self.device):
            if has_lo:
                below = self.boxes[self.rank - 1]
                self.halo(below, par, "hi").copy_(lo_plane, non_blocking=True)
                _lib.check(self.lib.trx_peer_signal(self._flag_ptr(below, 1), v, self._stream()), "trx_peer_signal")
            if has_hi:
                above = self.boxes[self.rank + 1]
                self.halo(above, par, "lo").copy_(hi_plane, non_blocking=True)
                _lib.check(self.lib.trx_peer_signal(self._flag_ptr(above, 0), v, self._stream()), "trx_peer_signal")

    def _timeout(self):
        return min(int(self.TIMEOUT_US * (self.FIRST_WAIT_FACTOR if self.t == 0 else 1)), 0xFFFFFFFF)

    def wait_halo(self, which):
        """Blocks the current stream until the neighbour's plane of this iteration has arrived; returns the plane (a view of the mailbox)."""
        par, v = self.t & 1, self.t + 1
        with torch.cuda.device(self.device):
            _lib.check(self.lib.trx_peer_wait(self._flag_ptr(self.mine, 0 if which == "lo" else 1), v, self._timeout(), _lib.ptr(self.status), self._stream()), "trx_peer_wait")
        return self.halo(self.mine, par, which)

    def publish(self, sums):
        """sums ([1,8] fp64 on this device) into this rank's slot of every mailbox."""
        par, v = self.t & 1, self.t + 1
        with torch.cuda.device(self.device):
            _lib.check(self.lib.trx_peer_publish(_lib.ptr(sums), _lib.ptr(self._slot_ptrs[par]), _lib.ptr(self._flag_ptrs), self.world, v, self._stream()), "trx_peer_publish")

    def gather(self, out):
        """The whole-volume sums into `out` ([1,8] fp64): waits for every rank's publish of this iteration, adds in rank order; ends the iteration."""
        par, v = self.t & 1, self.t + 1
        slots = self.mine.data_ptr() + par * self.per_parity + 2 * self.plane
        with torch.cuda.device(self.device):
            _lib.check(self.lib.trx_peer_gather(slots, self.mine.data_ptr() + self.flags_off + 8, self.world, v, self._timeout(), _lib.ptr(out), _lib.ptr(self.status),
                                                self._stream()), "trx_peer_gather")
        self.t += 1

    def check(self):
        """Host sync: raises when a wait timed out (a peer never wrote).  The time-out is STICKY on the device (every later wait of this
        transport returns at once and the sums are NaN) until reset()."""
        st = int(self.status.item())
        if st:
            raise _lib.TrxError(f"peer transport timed out (status {st}: 1 = halo plane, 2 = sums); the transport stays disabled until SlabPeers.reset()")

    def reset(self):
        """Clears a sticky time-out so that the transport can be used again.  The iteration counter is NOT rewound: flag
        values only ever rise, so every rank of the transport must call reset() after the same number of iterations - e.g. all of them
        after a run() that raised - and the flows they continue from must be the ones they agree on (a timed-out iteration has
        produced NaN sums on this rank)."""
        self.status.zero_()


class SlabFlowSolver:
    """One rank's Z-slab of a single-volume direct-flow registration (BASELINE config 5).

    moving_full: [1,1,D,H,W] the WHOLE moving volume (replicated on every rank; it is constant).
    target_slab: [1,1,Ds,H,W] planes [z_offset, z_offset+Ds) of the target.
    The flow / Adam state of the slab live here.  Each iteration: (with the smoothness regulariser) one flow
    plane is exchanged with each Z neighbour (P2P over xGMI) -> pass A on the slab -> 8 fp64 sums -> all-reduce
    over `group` (RCCL via torch.distributed when initialised) -> pass B on the slab with the whole-volume sums.
    The loss curve holds the WHOLE-volume loss on every rank."""

    def __init__(self, moving_full, target_slab, z_offset, loss=None, optimizer="sgd", lr=1e-3, capacity=1000, betas=(0.9, 0.999),
                 eps=1e-8, group=None, smooth_weight=0.0, stop_crit=None, flags=0, peers=None):
        self.lib = _lib.load()
        self.peers = peers      # SlabPeers: halo planes and the sum of moments as direct writes into the peers' mailboxes instead of torch.distributed
        _require_gpu(moving_full, "moving_full")
        _require_gpu(target_slab, "target_slab")
        if moving_full.dim() != 5 or target_slab.dim() != 5 or moving_full.shape[:2] != (1, 1) or target_slab.shape[:2] != (1, 1):
            raise ValueError("slab mode takes one single-channel 3-D volume: moving [1,1,D,H,W], target slab [1,1,Ds,H,W]")
        if moving_full.shape[3:] != target_slab.shape[3:]:
            raise ValueError("moving and target slab differ in (H, W)")
        self.D_full, self.z_offset = int(moving_full.shape[2]), int(z_offset)
        self.Ds = int(target_slab.shape[2])
        if self.z_offset < 0 or self.z_offset + self.Ds > self.D_full:
            raise ValueError("slab does not lie inside the moving volume")
        self.moving, self.target = moving_full.contiguous(), target_slab.contiguous()
        dev = self.moving.device
        self.device, self.group = dev, group
        H, W = int(self.moving.shape[3]), int(self.moving.shape[4])
        self.loss = loss or LossSpec(w_mse=1.0)
        self.loss_c = self.loss.c()
        self.opt = opt_cfg(optimizer, lr, betas, eps)
        self.smooth = float(smooth_weight)
        shape = (1, 3, self.Ds, H, W)
        self.flow = torch.zeros(shape, device=dev)
        self.flow_tmp = torch.empty(shape, device=dev) if self.smooth else None
        adam = self.opt.kind == _lib.OPT_ADAM
        self.adam_m = torch.zeros(shape, device=dev) if adam else None
        self.adam_v = torch.zeros(shape, device=dev) if adam else None
        self.capacity = int(capacity)
        self.losses = torch.full((1, self.capacity), float("nan"), device=dev)
        self.step_t = torch.zeros(1, dtype=torch.int32, device=dev)
        self.moments = torch.zeros(1, 8, dtype=torch.float64, device=dev)
        # neighbour planes of the flow (only with the regulariser): None at the ends of the volume
        self.has_lo, self.has_hi = self.z_offset > 0, self.z_offset + self.Ds < self.D_full
        self.halo_lo = torch.zeros(3, H, W, device=dev) if (self.smooth and self.has_lo) else None
        self.halo_hi = torch.zeros(3, H, W, device=dev) if (self.smooth and self.has_hi) else None
        v = _lib.Volumes()
        v.moving, v.target = self.moving.data_ptr(), self.target.data_ptr()
        v.moving_stride, v.target_stride = self.D_full * H * W, self.Ds * H * W
        v.ndim, v.B, v.D, v.H, v.W = 3, 1, self.Ds, H, W
        v.flags = int(flags)
        self.vol = v
        self.ws_bytes = self.lib.trx_flow_workspace_bytes(ctypes.byref(v))
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self._adam = adam
        self._partials_valid = False
        self._fuse = not (int(flags) & _lib.FLAG_TWO_PASS_FLOW)
        # early stop (same device-side test as FlowSolver: the whole-volume loss is identical on every rank, so every rank stops at
        # the same iteration without exchanging anything); flow_last = this slab of the flow of the last forward
        self.stop_crit = stop_crit
        self.stopped = torch.zeros(1, dtype=torch.int32, device=dev) if stop_crit is not None else None
        self.flow_last = torch.empty(shape, device=dev) if stop_crit is not None else None
        self.enqueued = 0

    def _state(self):
        st = _lib.FlowState()
        st.flow = self.flow.data_ptr()
        st.flow_tmp = self.flow_tmp.data_ptr() if self.flow_tmp is not None else None
        st.adam_m = self.adam_m.data_ptr() if self._adam else None
        st.adam_v = self.adam_v.data_ptr() if self._adam else None
        st.losses, st.losses_capacity, st.step = self.losses.data_ptr(), self.capacity, self.step_t.data_ptr()
        st.smooth_weight = self.smooth
        st.stop_crit = float(self.stop_crit) if self.stop_crit is not None else 0.0
        st.stopped = self.stopped.data_ptr() if self.stopped is not None else None
        st.flow_last = self.flow_last.data_ptr() if self.flow_last is not None else None
        return st

    def boundary_planes(self):
        """(lowest, highest) plane of this slab's flow, each [3,H,W] — what the Z neighbours need as halo."""
        return self.flow[0, :, 0].contiguous(), self.flow[0, :, -1].contiguous()

    def exchange_halos(self, rank=None, world=None):
        """P2P exchange of one flow plane with each Z neighbour (rank r owns the slab below rank r+1)."""
        import torch.distributed as dist
        if not self.smooth or not (dist.is_available() and dist.is_initialized()):
            return
        from .sharding import neighbour_global_ranks
        below, above = neighbour_global_ranks(self.group)           # P2POp takes GLOBAL ranks; a sub-group need not start at global rank 0
        lo, hi = self.boundary_planes()
        ops = []
        if self.has_lo:
            ops += [dist.P2POp(dist.isend, lo, below, self.group), dist.P2POp(dist.irecv, self.halo_lo, below, self.group)]
        if self.has_hi:
            ops += [dist.P2POp(dist.isend, hi, above, self.group), dist.P2POp(dist.irecv, self.halo_hi, above, self.group)]
        if ops:
            for r in dist.batch_isend_irecv(ops):
                r.wait()

    def local_moments(self):
        """Pass A: this slab's raw sums into self.moments (device, fp64 [1,8]).  Without the smoothness term the previous apply() has
        already left the block partials of the current flow in the workspace and only their reduction runs (anything that changes
        self.flow in between must set self._partials_valid = False)."""
        if self._partials_valid:
            with torch.cuda.device(self.device):
                rc = self.lib.trx_flow_slab_moments_ready(ctypes.byref(self.vol), self.z_offset, self.D_full, _lib.ptr(self.moments),
                                                          _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.device))
            _lib.check(rc, "trx_flow_slab_moments_ready")
            return self.moments
        with torch.cuda.device(self.device):
            rc = self.lib.trx_flow_slab_moments(ctypes.byref(self.vol), self.z_offset, self.D_full, _lib.ptr(self.flow), int(bool(self.smooth)),
                                                _lib.ptr(self.halo_hi), _lib.ptr(self.moments), _lib.ptr(self.workspace), self.ws_bytes,
                                                _lib.current_stream(self.device))
        _lib.check(rc, "trx_flow_slab_moments")
        return self.moments

    def apply(self, global_moments, last=None):
        """Pass B with the whole-volume sums ([1,8] fp64 on this device).  `last`: also store the flow this update starts from into
        flow_last (TRX_FLAG_SAVE_LAST, +12 B/voxel of stores).  run() / the peer steps ask for it on their last iteration only; a caller
        that drives the building blocks itself (local_moments -> all-reduce -> apply) gets it on EVERY call unless it says last=False,
        so that flow_last is never stale (the flag-less default used to leave it uninitialised)."""
        gm = global_moments.contiguous()
        if self.flow_last is not None and not getattr(self, "_driven", False):
            want = True if last is None else bool(last)
            self.vol.flags = (int(self.vol.flags) & ~_lib.FLAG_SAVE_LAST) | (_lib.FLAG_SAVE_LAST if want else 0)
        st = self._state()
        if not self.smooth and self._fuse:   # one pass: the update also produces the partials of the updated flow
            with torch.cuda.device(self.device):
                rc = self.lib.trx_flow_slab_update_fused(ctypes.byref(self.vol), self.z_offset, self.D_full, ctypes.byref(self.loss_c), ctypes.byref(self.opt),
                                                         ctypes.byref(st), _lib.ptr(gm), _lib.ptr(self.workspace), self.ws_bytes,
                                                         _lib.current_stream(self.device))
            _lib.check(rc, "trx_flow_slab_update_fused")
            self._partials_valid = True
            return
        with torch.cuda.device(self.device):
            rc = self.lib.trx_flow_slab_update(ctypes.byref(self.vol), self.z_offset, self.D_full, ctypes.byref(self.loss_c), ctypes.byref(self.opt),
                                               ctypes.byref(st), _lib.ptr(gm), _lib.ptr(self.halo_lo), _lib.ptr(self.halo_hi),
                                               _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.device))
        _lib.check(rc, "trx_flow_slab_update")
        if self.smooth:
            self.flow, self.flow_tmp = self.flow_tmp, self.flow   # the update was written to the other buffer

    def local_moments_without_halo(self):
        """Pass A with the cross-slab smoothness term left out (it needs the upper neighbour's plane): self.moments."""
        with torch.cuda.device(self.device):
            rc = self.lib.trx_flow_slab_moments(ctypes.byref(self.vol), self.z_offset, self.D_full, _lib.ptr(self.flow), int(bool(self.smooth)),
                                                None, _lib.ptr(self.moments), _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.device))
        _lib.check(rc, "trx_flow_slab_moments")
        return self.moments

    def add_boundary_smooth(self, moments):
        """Adds the cross-slab smoothness term (top plane against halo_hi) to `moments` ([1,8] fp64), on the current stream."""
        if not (self.smooth and self.has_hi):
            return
        with torch.cuda.device(self.device):
            rc = self.lib.trx_flow_slab_boundary_smooth(ctypes.byref(self.vol), _lib.ptr(self.flow), _lib.ptr(self.halo_hi), _lib.ptr(moments),
                                                        _lib.current_stream(self.device))
        _lib.check(rc, "trx_flow_slab_boundary_smooth")

    def run(self, iters):
        """`iters` iterations.  With more than one rank and the smoothness term, the exchange of the boundary flow planes with the Z
        neighbours (P2P over xGMI, 3 MB per face at 512^2) runs on a side stream while pass A covers the slab: pass A leaves the one
        term that needs the neighbour's plane to a small kernel behind the exchange (trx_flow_slab_boundary_smooth).  The 64-byte
        all-reduce of the sums stays between pass A and pass B, where the algorithm needs it.  With `peers` (SlabPeers) both exchanges
        are direct writes into the peers' mailboxes and no torch.distributed call is made."""
        import torch.distributed as dist
        if self.enqueued + int(iters) > self.capacity:
            raise _lib.TrxError(f"loss-curve capacity exceeded: {self.enqueued} + {int(iters)} > {self.capacity}")
        if self.peers is not None:
            self.enqueued += int(iters)
            try:
                for it in range(int(iters)):
                    self.peer_post(last=(it == int(iters) - 1))
                    self.peer_join()
                    self.peer_finish()
            finally:   # an exception between peer_post and peer_finish must not leave the SAVE_LAST handling to a loop that is gone
                self._peer_restore()
            self.peers.check()   # (host sync at the end of the call: a peer that never wrote is an exception here, not a silent NaN curve)
            return
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        self.enqueued += int(iters)
        overlap = multi and bool(self.smooth)
        if overlap and getattr(self, "_side", None) is None:
            self._side = torch.cuda.Stream(device=self.device)
            self._edge = torch.zeros(1, 8, dtype=torch.float64, device=self.device)
        main = torch.cuda.current_stream(self.device)
        base_flags = int(self.vol.flags) & ~_lib.FLAG_SAVE_LAST
        self._driven = True   # (apply() leaves the SAVE_LAST bit to this loop)
        try:
            for it in range(int(iters)):
                # flow_last (the flow of the last forward) is written by the iteration that meets stop_crit, or by the last one of the run:
                # only that one pays the extra 12 B/voxel of stores
                self.vol.flags = base_flags | (_lib.FLAG_SAVE_LAST if (self.flow_last is not None and it == int(iters) - 1) else 0)
                if overlap:
                    self._side.wait_stream(main)                 # the previous update has produced the planes to send
                    with torch.cuda.stream(self._side):
                        self.exchange_halos()
                        self._edge.zero_()
                        self.add_boundary_smooth(self._edge)
                    m = self.local_moments_without_halo()        # main stream: the whole slab, no halo needed
                    main.wait_stream(self._side)
                    m += self._edge
                else:
                    if multi:
                        self.exchange_halos()
                    m = self.local_moments()
                if multi:
                    dist.all_reduce(m, op=dist.ReduceOp.SUM, group=self.group)   # 64 bytes per iteration
                self.apply(m)
        finally:
            self.vol.flags = base_flags
            self._driven = False

    def _peer_restore(self):
        """Ends a peer-driven iteration: the flags the caller set are back and apply() handles SAVE_LAST itself again."""
        base = getattr(self, "_base_flags", None)
        if base is not None:
            self.vol.flags = base
        self._base_flags = None
        self._driven = False

    # -- one iteration over the peer-mapped transport, in three steps so that ONE process can drive several slabs in lock step
    # (run_slabs_lockstep: every slab posts, then every slab joins, then every slab finishes - no wait is enqueued before the write it
    # waits for); run() calls them back to back for its own slab.
    def peer_post(self, last=False, side_stream=True):
        """Sends the boundary planes (their copies and flags on a side stream, so they travel while pass A runs) and runs pass A."""
        pr = self.peers
        if getattr(self, "_base_flags", None) is None:   # (per iteration: peer_finish / _peer_restore clear it, so a change of vol.flags between runs is seen)
            self._base_flags = int(self.vol.flags) & ~_lib.FLAG_SAVE_LAST
        self._driven = True
        self.vol.flags = self._base_flags | (_lib.FLAG_SAVE_LAST if (self.flow_last is not None and last) else 0)
        if not self.smooth:
            self._m = self.local_moments()
            return
        if getattr(self, "_edge", None) is None:
            self._edge = torch.zeros(1, 8, dtype=torch.float64, device=self.device)
            self._side = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        self._use_side = bool(side_stream)
        lo, hi = self.boundary_planes()
        if self._use_side:
            self._side.wait_stream(main)
            lo.record_stream(self._side); hi.record_stream(self._side)
            with torch.cuda.stream(self._side):
                pr.put_halos(lo, hi, self.has_lo, self.has_hi)
        else:
            pr.put_halos(lo, hi, self.has_lo, self.has_hi)
        self._m = self.local_moments_without_halo()

    def peer_join(self):
        """Waits for the neighbours' planes, adds the cross-slab smoothness term, publishes this slab's sums to every mailbox."""
        pr = self.peers
        if self.smooth:
            main = torch.cuda.current_stream(self.device)

            def arrive():
                self._edge.zero_()
                if self.has_hi:
                    self.halo_hi = pr.wait_halo("hi")
                    self.add_boundary_smooth(self._edge)
                if self.has_lo:
                    self.halo_lo = pr.wait_halo("lo")
            if self._use_side:
                with torch.cuda.stream(self._side):
                    arrive()
                main.wait_stream(self._side)
            else:
                arrive()
            self._m += self._edge
        pr.publish(self._m)

    def peer_finish(self):
        """Whole-volume sums (every rank adds the N slots in rank order) and pass B."""
        try:
            self.peers.gather(self._m)
            self.apply(self._m)
        finally:
            self._peer_restore()


def run_slabs_lockstep(solvers, iters):
    """One process driving several SlabFlowSolvers that share a SlabPeers transport (each with its own SlabPeers of the same mailboxes,
    on one GPU or several): all post, all join, all finish - per iteration.  The single-process counterpart of N ranks calling run()."""
    for s in solvers:
        if s.enqueued + int(iters) > s.capacity:
            raise _lib.TrxError(f"loss-curve capacity exceeded: {s.enqueued} + {int(iters)} > {s.capacity}")
        s.enqueued += int(iters)
    for it in range(int(iters)):
        last = it == int(iters) - 1
        for s in solvers:
            with torch.cuda.device(s.device):
                s.peer_post(last=last, side_stream=False)
        for s in solvers:
            with torch.cuda.device(s.device):
                s.peer_join()
        for s in solvers:
            with torch.cuda.device(s.device):
                s.peer_finish()
    for s in solvers:
        s.peers.check()


def _mi_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, int) or not 8 <= bins <= 64:
        raise ValueError(f"bins must be an int in 8 .. 64, got {bins!r}")
    return bins


def _mask_u8(mask, like):
    """A region-of-interest mask on the target lattice of `like` [B,1,*spatial]: bool / uint8 / any numeric tensor of shape [B,1,*spatial] or
    [B,*spatial], non-zero = the voxel counts -> contiguous uint8 [B,1,*spatial] of 0 / 1 on like's device (what trx_mi_cfg.mask points to: the
    caller keeps it alive).  ValueError on a shape mismatch, before anything touches a device."""
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a tensor of shape {tuple(like.shape)}, got {type(mask).__name__}")
    want = (like.shape[0], 1) + tuple(like.shape[2:])
    if tuple(mask.shape) not in (want, (want[0],) + want[2:]):
        raise ValueError(f"mask {tuple(mask.shape)} does not match the target lattice: expected {want} or {(want[0],) + want[2:]}")
    return (mask.detach().reshape(want) != 0).to(device=like.device, dtype=torch.uint8).contiguous()


def overlap_args(overlap, moving_mask, moving):
    """overlap= / moving_mask= of the mutual-information entry points -> (whether the overlap rule is on, the uint8 moving mask [B,1,*moving
    spatial] or None).  overlap: None (off, unless a moving mask implies it), False or True.  moving_mask goes through _mask_u8 against `moving`
    and implies the rule; together with an explicit overlap=False it is a ValueError.  Looks at shapes only."""
    if moving_mask is None:
        return bool(overlap), None
    if overlap is not None and not overlap:
        raise ValueError("moving_mask is part of the overlap rule (a sample outside the mask is dropped like one outside the moving image): it cannot go with overlap=False")
    return True, _mask_u8(moving_mask, moving)


def _mi_cfg_c(bins, alpha, normalized, rng, mask):
    """trx_mi_cfg over the range tensor [B,4] and the uint8 mask (or None) it points to: the caller keeps both alive."""
    cfg = _lib.MICfg()
    cfg.bins, cfg.alpha, cfg.normalized, cfg.range = _mi_bins(bins), float(alpha), int(bool(normalized)), rng.data_ptr()
    cfg.mask = None if mask is None else mask.data_ptr()
    return cfg


def mi_range(target, moving, target_range=None, moving_range=None, mask=None, overlap=False, moving_mask=None):
    """[B,4] fp32 on the tensors' device: (lo_t, hi_t, lo_w, hi_w) per pair.  None: the target's min / max, the moving (or warped) image's min /
    max widened to contain 0 - the value of a zero-padded warp outside the field of view.  A (lo, hi) pair of numbers serves every pair of the
    batch.  mask (see _mask_u8): the target's min / max are taken over the voxels that count - a pair whose mask is empty falls back to its whole
    target; the moving side does not change.  overlap (the overlap rule, include/trx.h: trx_moving_grid - no padded sample is counted): the moving
    image's own min / max, NOT widened, taken inside moving_mask (on the moving lattice) when there is one.  No host sync."""
    B = target.shape[0]
    cols = []
    for x, r, widen in ((target, target_range, False), (moving, moving_range, True)):
        if r is None:
            flat = x.detach().float().reshape(B, -1)
            lo, hi = flat.amin(1), flat.amax(1)
            if widen and not overlap:
                lo, hi = lo.clamp(max=0.0), hi.clamp(min=0.0)
            elif (moving_mask if widen else mask) is not None:
                m = (_mask_u8(moving_mask, moving) if widen else _mask_u8(mask, target)).reshape(B, -1) != 0
                inf = torch.full_like(flat, float("inf"))
                some = m.any(1)
                lo, hi = torch.where(some, torch.where(m, flat, inf).amin(1), lo), torch.where(some, torch.where(m, flat, -inf).amax(1), hi)
        else:
            lo, hi = (torch.full((B,), float(v), dtype=torch.float32, device=target.device) for v in r)
        cols += [lo, hi]
    return torch.stack(cols, dim=1).contiguous()


def _mi_cfg(mi, target, moving, mask=None, overlap=False, moving_mask=None):
    """dict -> (trx_mi_cfg, the range tensor it points to, the uint8 mask it points to or None: the caller keeps both alive).  overlap,
    moving_mask: how mi_range fits the moving side."""
    unknown = set(mi) - {"bins", "alpha", "normalized", "target_range", "moving_range"}
    if unknown:
        raise ValueError(f"unknown mutual-information settings {sorted(unknown)}")
    m8 = None if mask is None else _mask_u8(mask, target)
    rng = mi_range(target, moving, mi.get("target_range"), mi.get("moving_range"), m8, overlap, moving_mask)
    return _mi_cfg_c(mi.get("bins", 32), mi.get("alpha", 1.0), mi.get("normalized", False), rng, m8), rng, m8


def mi_loss_grad(target, warped, rng, bins=32, alpha=1.0, normalized=False, need_grad=True, mask=None):
    """Parzen joint-histogram mutual information (extension, include/trx.h: trx_mi_loss_grad): target / warped [B,1,*spatial] fp32 on the GPU,
    rng [B,4] (mi_range), mask (see _mask_u8) or None = every voxel.  Returns (loss [B], d loss / d warped (same shape as warped, zero outside
    the mask) or None)."""
    if mask is not None:
        mask = _mask_u8(mask, target)
    lib = _lib.load()
    if not (target.is_cuda and warped.is_cuda):
        raise _lib.TrxError("mi_loss_grad needs CUDA (HIP) tensors: there is no CPU fallback")
    if target.shape != warped.shape or target.dim() not in (4, 5) or target.shape[1] != 1:
        raise ValueError(f"expected two [B,1,*spatial] tensors of equal shape, got {tuple(target.shape)} and {tuple(warped.shape)}")
    nd = target.dim() - 2
    y, w = target.detach().contiguous().float(), warped.detach().contiguous().float()
    B = y.shape[0]
    if tuple(rng.shape) != (B, 4):
        raise ValueError(f"expected a range tensor [{B}, 4], got {tuple(rng.shape)}")
    rng = rng.detach().to(device=y.device, dtype=torch.float32).contiguous()
    D, H, W = (1, *y.shape[2:]) if nd == 2 else y.shape[2:]
    cfg = _mi_cfg_c(bins, alpha, normalized, rng, mask)
    loss = torch.empty(B, device=y.device)
    grad = torch.empty_like(w) if need_grad else None
    ws_bytes = lib.trx_mi_workspace_bytes(nd, B, D, H, W, cfg.bins)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_mi_workspace_bytes rejected {B} x {tuple(y.shape[2:])} with {bins} bins")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        rc = lib.trx_mi_loss_grad(_lib.ptr(y), _lib.ptr(w), nd, B, D, H, W, ctypes.byref(cfg), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws_bytes,
                                  _lib.current_stream(y.device))
    _lib.check(rc, "trx_mi_loss_grad")
    return loss, grad


def _ngf_voxel(voxel, nd):
    """voxel= of the normalised-gradient-field entry points -> None or a tuple of nd positive finite floats in the tensor's axis order."""
    if voxel is None:
        return None
    try:
        v = tuple(float(h) for h in voxel)
    except TypeError:
        raise ValueError(f"voxel is one size per axis, (z, y, x) or (y, x), got {voxel!r}") from None
    if len(v) != nd or not all(math.isfinite(h) and h > 0 for h in v):
        raise ValueError(f"voxel is {nd} positive finite sizes in the tensor's axis order, got {voxel!r}")
    return v


def ngf_gradient(x, voxel=None):
    """[B,nd,*spatial]: the differences of include/trx.h (trx_ngf_loss_grad) of x [B,1,*spatial] - central inside, one-sided on the faces, 0 on an
    axis of one voxel, over the voxel sizes - as plain torch ops with clamped indices (differentiable)."""
    nd = x.dim() - 2
    v = _ngf_voxel(voxel, nd) or (1.0,) * nd
    out = []
    for a in range(nd):
        S = x.shape[2 + a]
        idx = torch.arange(S, device=x.device)
        ip, im = (idx + 1).clamp(max=S - 1), (idx - 1).clamp(min=0)
        sc = torch.where(ip - im == 2, 0.5, 1.0).to(x.dtype) / v[a]
        shape = [1] * x.dim()
        shape[2 + a] = S
        out.append((x.index_select(2 + a, ip) - x.index_select(2 + a, im)) * sc.reshape(shape))
    return torch.cat(out, dim=1)


def ngf_edge_parameters(target, moving, eta=1.0, voxel=None, mask=None):
    """[B,2] fp32 on the tensors' device: (eps_t, eps_w) of the normalised gradient field per pair - eta times the mean of |grad I| (ngf_gradient:
    the kernel's differences, over `voxel`) of the target and of the moving (or warped) image; 0 for a constant image, which the criterion
    defines (r = 0 where the denominator is 0).  mask (see _mask_u8, on the target lattice): the mean is taken over the voxels that count, for
    every image on that lattice - an image of another shape, and a pair whose mask is empty, use the whole image.  Plain torch ops, no host
    sync: it runs once per optimisation."""
    B = target.shape[0]
    m = None if mask is None else _mask_u8(mask, target).reshape(B, -1).float()
    cols = []
    for x in (target, moving):
        x = x.detach().float()
        mag = ngf_gradient(x, voxel).square().sum(1).sqrt().reshape(B, -1)
        mean = mag.mean(1)
        if m is not None and mag.shape == m.shape:
            n = m.sum(1)
            mean = torch.where(n > 0, (mag * m).sum(1) / n.clamp(min=1.0), mean)
        cols.append(float(eta) * mean)
    return torch.stack(cols, dim=1).contiguous()


def _ngf_cfg_c(alpha, eps, voxel, mask):
    """(trx_ngf_cfg, the host voxel array it points to or None) over the eps tensor [B,2] and the uint8 mask (or None): the caller keeps all alive."""
    cfg = _lib.NGFCfg()
    vox = None if voxel is None else (ctypes.c_float * len(voxel))(*voxel)
    cfg.alpha, cfg.eps = float(alpha), eps.data_ptr()
    cfg.voxel = None if vox is None else ctypes.cast(vox, ctypes.POINTER(ctypes.c_float))
    cfg.mask = None if mask is None else mask.data_ptr()
    return cfg, vox


def _ngf_eps(eps, B, device):
    if not isinstance(eps, torch.Tensor) or tuple(eps.shape) != (B, 2):
        raise ValueError(f"expected an eps tensor [{B}, 2] (ngf_edge_parameters), got {tuple(eps.shape) if isinstance(eps, torch.Tensor) else type(eps).__name__}")
    return eps.detach().to(device=device, dtype=torch.float32).contiguous()


def ngf_settings_eps(ngf, target, moving, voxel, mask):
    """eps [B,2] of a settings dict (NGFLoss.settings): a given target_eps / moving_eps serves every pair, None is fitted (ngf_edge_parameters)."""
    eps = ngf_edge_parameters(target, moving, ngf.get("eta", 1.0), voxel, mask)
    for col, key in enumerate(("target_eps", "moving_eps")):
        if ngf.get(key) is not None:
            eps[:, col] = float(ngf[key])
    return eps


def ngf_loss_grad(target, warped, eps, alpha=1.0, voxel=None, need_grad=True, mask=None):
    """Normalised gradient field criterion (extension, include/trx.h: trx_ngf_loss_grad): target / warped [B,1,*spatial] fp32 on the GPU, eps [B,2]
    (ngf_edge_parameters), voxel = the voxel sizes in the tensor's axis order or None = 1, mask (see _mask_u8) or None = every voxel.  Returns
    (loss [B], d loss / d warped (same shape as warped; zero beyond the face neighbours of the mask's voxels, whose differences read them) or None)."""
    if target.shape != warped.shape or target.dim() not in (4, 5) or target.shape[1] != 1:
        raise ValueError(f"expected two [B,1,*spatial] tensors of equal shape, got {tuple(target.shape)} and {tuple(warped.shape)}")
    nd = target.dim() - 2
    voxel = _ngf_voxel(voxel, nd)
    if mask is not None:
        mask = _mask_u8(mask, target)
    lib = _lib.load()
    if not (target.is_cuda and warped.is_cuda):
        raise _lib.TrxError("ngf_loss_grad needs CUDA (HIP) tensors: there is no CPU fallback")
    y, w = target.detach().contiguous().float(), warped.detach().contiguous().float()
    B = y.shape[0]
    eps = _ngf_eps(eps, B, y.device)
    D, H, W = (1, *y.shape[2:]) if nd == 2 else y.shape[2:]
    cfg, _vox = _ngf_cfg_c(alpha, eps, voxel, mask)
    loss = torch.empty(B, device=y.device)
    grad = torch.empty_like(w) if need_grad else None
    ws_bytes = lib.trx_ngf_workspace_bytes(nd, B, D, H, W)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_ngf_workspace_bytes rejected {B} x {tuple(y.shape[2:])}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        rc = lib.trx_ngf_loss_grad(_lib.ptr(y), _lib.ptr(w), nd, B, D, H, W, ctypes.byref(cfg), _lib.ptr(loss), _lib.ptr(grad), _lib.ptr(ws), ws_bytes,
                                   _lib.current_stream(y.device))
    _lib.check(rc, "trx_ngf_loss_grad")
    return loss, grad


def _mi_pair_batch(moving, target):
    """_Batch of B single-channel (moving, target) pairs for the fused affine mutual-information entry points."""
    batch = _Batch(moving, target)
    if batch.C != 1 or batch.target.shape[1] != 1:
        raise ValueError("the mutual-information path takes single-channel volumes [B,1,...]")
    if batch.target.shape[0] != batch.B:
        raise ValueError("moving and target batch sizes differ")
    return batch


def _half_extents(shape, voxel, name):
    """Half extents in mm of a lattice, in theta's row order (x, y(, z)): size * voxel size / 2.  shape / voxel: the tensor's axis order."""
    voxel = tuple(float(v) for v in voxel)
    if len(voxel) != len(shape):
        raise ValueError(f"{name} must have {len(shape)} entries in the tensor's axis order {'(dz, dy, dx)' if len(shape) == 3 else '(dy, dx)'}, got {voxel}")
    if not all(v > 0.0 and v != float("inf") for v in voxel):       # (NaN fails v > 0)
        raise ValueError(f"{name} must be positive and finite, got {voxel}")
    return torch.tensor([s * v / 2.0 for s, v in zip(shape, voxel)][::-1], dtype=torch.float64)


def grid_scale(moving_shape, target_shape, moving_voxel=None, target_voxel=None):
    """The scale [nd, nd+1] (fp64, CPU; host arithmetic only) that the cross-lattice entry points multiply theta by, theta_eff = theta * scale
    (include/trx.h: trx_moving_grid).  Without voxel sizes: all ones - the two normalised cubes coincide, theta means what F.affine_grid(theta,
    target.shape) + F.grid_sample(moving, ...) make of it.  With both: scale[r][c] = e_target[c] / e_moving[r] on the matrix and 1 on the
    translation column, e = size * voxel size / 2 in mm, so that theta acts between the two volumes in millimetres (centres coinciding, axes
    aligned): Theta(pose) is then rigid whatever the voxel sizes.  Shapes and voxel sizes in the tensors' axis order, (dz, dy, dx) / (dy, dx)."""
    moving_shape, target_shape = tuple(int(s) for s in moving_shape), tuple(int(s) for s in target_shape)
    nd = len(target_shape)
    if nd not in (2, 3) or len(moving_shape) != nd or min(moving_shape + target_shape) < 1:
        raise ValueError(f"expected two spatial shapes of 2 or 3 positive sizes, got {moving_shape} and {target_shape}")
    if (moving_voxel is None) != (target_voxel is None):
        raise ValueError("moving_voxel and target_voxel go together: give both voxel sizes (theta acts in millimetres) or neither (theta acts "
                         "between the two normalised cubes)")
    scale = torch.ones(nd, nd + 1, dtype=torch.float64)
    if moving_voxel is not None:
        e_m, e_t = _half_extents(moving_shape, moving_voxel, "moving_voxel"), _half_extents(target_shape, target_voxel, "target_voxel")
        scale[:, :nd] = e_t[None, :] / e_m[:, None]
    return scale


def _norm_to_voxel(shape, inverse=False):
    """N(S) [nd+1, nd+1] fp64: affine_grid's normalised coordinate (x, y(, z) order) -> the voxel index in the tensor's axis order (d, h, w),
    i_a = ((n_a + 1) S_a - 1) / 2 with x <-> w, y <-> h, z <-> d; inverse: its exact inverse n_a = (2 i_a + 1) / S_a - 1."""
    nd = len(shape)
    N = torch.zeros(nd + 1, nd + 1, dtype=torch.float64)
    for a, S in enumerate(shape):
        if inverse:
            N[nd - 1 - a, a], N[nd - 1 - a, nd] = 2.0 / S, 1.0 / S - 1.0
        else:
            N[a, nd - 1 - a], N[a, nd] = S / 2.0, (S - 1) / 2.0
    N[nd, nd] = 1.0
    return N


def _world_shapes(moving_shape, target_shape):
    moving_shape, target_shape = tuple(int(s) for s in moving_shape), tuple(int(s) for s in target_shape)
    nd = len(target_shape)
    if nd not in (2, 3) or len(moving_shape) != nd or min(moving_shape + target_shape) < 1:
        raise ValueError(f"expected two spatial shapes of 2 or 3 positive sizes, got {moving_shape} and {target_shape}")
    return moving_shape, target_shape, nd


def _world_affine(A, nd, name, B=None):
    """A voxel-to-world matrix [nd+1, nd+1] (shared) or [B, nd+1, nd+1] -> fp64 [B | 1, nd+1, nd+1] on the CPU.  ValueError for a wrong shape, a
    non-finite entry, a last row that is not (0, ..., 0, 1) within 1e-6, or a linear part whose condition number exceeds 1e8."""
    A = torch.as_tensor(A).detach().to("cpu", torch.float64)
    if A.dim() == 2:
        A = A[None]
    if A.dim() != 3 or tuple(A.shape[1:]) != (nd + 1, nd + 1) or (B is not None and A.shape[0] not in (1, B)):
        raise ValueError(f"{name} must be [{nd + 1}, {nd + 1}] or [B, {nd + 1}, {nd + 1}]" + ("" if B is None else f" with B = {B}") + f", got {tuple(A.shape)}")
    if not bool(torch.isfinite(A).all()):
        raise ValueError(f"{name} has a non-finite entry")
    last = torch.zeros(nd + 1, dtype=torch.float64)
    last[nd] = 1.0
    if float((A[:, nd] - last).abs().max()) > 1e-6:
        raise ValueError(f"{name}: the last row must be (0, ..., 0, 1), got {A[:, nd].tolist()}")
    sv = torch.linalg.svdvals(A[:, :nd, :nd])
    if bool((sv[:, -1] <= 0).any()) or float((sv[:, 0] / sv[:, -1]).max()) > 1e8:
        raise ValueError(f"{name}: the linear part is singular or ill-conditioned (condition number above 1e8)")
    A = A.clone()
    A[:, nd] = last
    return A


def _translation(t):
    """[B, nd] -> homogeneous translations [B, nd+1, nd+1] fp64."""
    B, nd = t.shape
    T = torch.eye(nd + 1, dtype=torch.float64).repeat(B, 1, 1)
    T[:, :nd, nd] = t
    return T


def lattice_center(shape, affine):
    """[B | 1, nd] fp64: the world position (x, y(, z)) of the geometric centre of a lattice, affine . ((S - 1) / 2)."""
    shape = tuple(int(s) for s in shape)
    A = _world_affine(affine, len(shape), "affine")
    mid = torch.tensor([(s - 1) / 2.0 for s in shape] + [1.0], dtype=torch.float64)
    return (A @ mid)[:, : len(shape)]


def level_affine(affine, full_shape, level_shape):
    """The voxel-to-world matrix of a pyramid level (align_corners=False keeps the field of view): A . [diag(S / S_l) | S / (2 S_l) - 1/2]."""
    nd = len(full_shape)
    A = _world_affine(affine, nd, "affine")
    M = torch.eye(nd + 1, dtype=torch.float64)
    for a, (S, Sl) in enumerate(zip(full_shape, level_shape)):
        M[a, a], M[a, nd] = S / Sl, S / (2.0 * Sl) - 0.5
    return A @ M


class WorldGeometry:
    """What world_geometry makes, all fp64 on the CPU: record [B, 32] (include/trx.h: trx_moving_grid.world - L | R | l),
    center [B, nd] = c, init [B, nd+1, nd+1] = T0, extent [B, nd] = l.  Iterates as (record, center)."""

    def __init__(self, record, center, init, extent):
        self.record, self.center, self.init, self.extent = record, center, init, extent
        self.B, self.nd = center.shape
        self.search = None       # world_setup(world_init='principal_axes' / 'search'): the WorldSearch behind init

    def __iter__(self):
        return iter((self.record, self.center))

    def pair(self, b):
        return WorldGeometry(self.record[b:b + 1], self.center[b:b + 1], self.init[b:b + 1], self.extent[b:b + 1])

    def L(self):
        nd = self.nd
        return self.record[:, _lib.WORLD_L:_lib.WORLD_L + nd * (nd + 1)].reshape(-1, nd, nd + 1)

    def R(self):
        nd = self.nd
        return self.record[:, _lib.WORLD_R:_lib.WORLD_R + nd * (nd + 1)].reshape(-1, nd, nd + 1)

    def matrix(self, theta):
        """T [B, nd+1, nd+1] fp64 of the UNSCALED theta [B, nd, nd+1]: p_moving = T p_target = T0 Tr(c) Theta Tr(-c) p_target (world mm, x, y(, z))."""
        nd = self.nd
        th = theta.detach().to("cpu", torch.float64).reshape(-1, nd, nd + 1)
        Th = torch.eye(nd + 1, dtype=torch.float64).repeat(th.shape[0], 1, 1)
        Th[:, :nd, :nd] = th[:, :, :nd]
        Th[:, :nd, nd] = th[:, :, nd] * self.extent
        return self.init @ _translation(self.center) @ Th @ _translation(-self.center)


def world_geometry(moving_shape, target_shape, moving_affine, target_affine, init=None, center=None):
    """The world-geometry record of the fused rigid / affine mutual-information loop (include/trx.h: trx_moving_grid.world).
    Host arithmetic in fp64 only.  Shapes in the tensors' axis order; an affine is the voxel-to-world matrix [nd+1, nd+1] (one for every pair) or
    [B, nd+1, nd+1], columns in the tensor's axis order (d, h, w) - nibabel's img.affine for get_fdata() put into [B,1,*shape] - rows world x, y(, z).
    init: T0, a world transform [nd+1, nd+1] / [B, nd+1, nd+1] in front of what is optimised, None = identity, or 'centers' = the translation
    taking the target's geometric centre to the moving image's.  center: c [nd] / [B, nd] in world mm, None = the target's geometric centre.
    With T = T0 Tr(c) Theta Tr(-c), Theta = [theta[:, :nd] | l (.) theta[:, nd]]:  R = Tr(-c) A_t N(S_t),  L = N(S_m)^-1 A_m^-1 T0 Tr(c),
    l_r = sum_a |A_m[r][a]| S_m,a / 2, and theta_eff = (L Theta R)[:nd].  Returns a WorldGeometry; `record, c = world_geometry(...)` unpacks it."""
    ms, ts, nd = _world_shapes(moving_shape, target_shape)
    if moving_affine is None or target_affine is None:
        raise ValueError("moving_affine and target_affine go together: give both voxel-to-world matrices or neither")
    Am, At = _world_affine(moving_affine, nd, "moving_affine"), _world_affine(target_affine, nd, "target_affine")
    B = max(Am.shape[0], At.shape[0])
    if isinstance(init, str):
        if init != "centers":
            raise ValueError(f"init must be None, 'centers' or a matrix, got {init!r}")
        T0 = _translation((lattice_center(ms, Am) - lattice_center(ts, At)).expand(B, nd))
    else:
        T0 = torch.eye(nd + 1, dtype=torch.float64)[None] if init is None else _world_affine(init, nd, "init")
    c = lattice_center(ts, At) if center is None else torch.as_tensor(center).detach().to("cpu", torch.float64).reshape(-1, nd)
    if not bool(torch.isfinite(c).all()):
        raise ValueError("center has a non-finite entry")
    B = max(B, T0.shape[0], c.shape[0])
    for t, name in ((Am, "moving_affine"), (At, "target_affine"), (T0, "init"), (c, "center")):
        if t.shape[0] not in (1, B):
            raise ValueError(f"{name} is given for {t.shape[0]} pairs, the others for {B}")
    Am, At, T0, c = (t.expand(B, *t.shape[1:]).contiguous() for t in (Am, At, T0, c))
    R = _translation(-c) @ At @ _norm_to_voxel(ts)
    L = _norm_to_voxel(ms, inverse=True) @ torch.stack([torch.linalg.inv(a) for a in Am]) @ T0 @ _translation(c)      # (one matrix at a time: a pair's record does not depend on its batch)
    ext = (Am[:, :nd, :nd].abs() * torch.tensor(ms, dtype=torch.float64)[None, None, :]).sum(2) / 2.0
    rec = torch.zeros(B, _lib.WORLD_STRIDE, dtype=torch.float64)
    rec[:, _lib.WORLD_L:_lib.WORLD_L + nd * (nd + 1)] = L[:, :nd].reshape(B, -1)
    rec[:, _lib.WORLD_R:_lib.WORLD_R + nd * (nd + 1)] = R[:, :nd].reshape(B, -1)
    rec[:, _lib.WORLD_EXT:_lib.WORLD_EXT + nd] = ext
    return WorldGeometry(rec, c, T0, ext)


def world_theta_host(theta, record, nd):
    """theta_eff [B, nd, nd+1] fp32 of the UNSCALED theta under a record, on the host with the device function's own operations (include/trx.h: fp64, one
    multiply and one add per term, ascending index order, the homogeneous term last, one rounding to fp32): the bits of trx_affine_world_theta."""
    import numpy as np
    th = theta.detach().to("cpu", torch.float32).reshape(-1, nd, nd + 1).double().numpy()
    rec = record.detach().to("cpu", torch.float64).numpy()
    B, NC = th.shape[0], nd + 1
    out = np.zeros((B, nd, NC), dtype=np.float32)
    for b in range(B):
        L = rec[b, _lib.WORLD_L:_lib.WORLD_L + nd * NC].reshape(nd, NC)
        R = rec[b, _lib.WORLD_R:_lib.WORLD_R + nd * NC].reshape(nd, NC)
        ext = rec[b, _lib.WORLD_EXT:_lib.WORLD_EXT + nd]
        M = np.zeros((nd, NC))
        for r in range(nd):
            for j in range(NC):
                s = th[b, r, 0] * R[0, j]
                for c in range(1, nd):
                    s = s + th[b, r, c] * R[c, j]
                if j == nd:
                    s = s + ext[r] * th[b, r, nd]
                M[r, j] = s
        for i in range(nd):
            for j in range(NC):
                s = L[i, 0] * M[0, j]
                for r in range(1, nd):
                    s = s + L[i, r] * M[r, j]
                if j == nd:
                    s = s + L[i, nd]
                out[b, i, j] = np.float32(s)
    return torch.from_numpy(out)


def world_chain_host(g_eff, record, nd):
    """dL/dtheta [B, nd, nd+1] fp64 (the UNSCALED theta) from g_eff = dL/dtheta_eff [B, nd, nd+1] under a record: P = L[:, :nd]^T g,
    dtheta[:, :nd] = P R^T, dtheta[:, nd] = l (.) P[:, nd] - the chain rule the kernels apply behind the reduction."""
    g = g_eff.detach().to("cpu", torch.float64).reshape(-1, nd, nd + 1)
    rec = record.detach().to("cpu", torch.float64)
    L = rec[:, _lib.WORLD_L:_lib.WORLD_L + nd * (nd + 1)].reshape(-1, nd, nd + 1)
    R = rec[:, _lib.WORLD_R:_lib.WORLD_R + nd * (nd + 1)].reshape(-1, nd, nd + 1)
    ext = rec[:, _lib.WORLD_EXT:_lib.WORLD_EXT + nd]
    P = L[:, :, :nd].transpose(1, 2) @ g
    out = torch.zeros_like(g)
    out[:, :, :nd] = P @ R.transpose(1, 2)
    out[:, :, nd] = ext * P[:, :, nd]
    return out


def _homogeneous(theta, nd):
    th = torch.as_tensor(theta).detach().to("cpu", torch.float64).reshape(-1, nd, nd + 1)
    H = torch.eye(nd + 1, dtype=torch.float64).repeat(th.shape[0], 1, 1)
    H[:, :nd] = th
    return H


def theta_from_world(matrix, moving_affine, target_affine, moving_shape, target_shape):
    """A world transform from any tool, p_moving = matrix p_target (mm, [nd+1, nd+1] or [B, nd+1, nd+1]) -> the EFFECTIVE theta [B, nd, nd+1] fp64 that
    resample(theta=), affine_warp(size=) and optim(initial=) take: (N(S_m)^-1 A_m^-1 matrix A_t N(S_t))[:nd].  Host arithmetic in fp64."""
    ms, ts, nd = _world_shapes(moving_shape, target_shape)
    T, Am, At = _world_affine(matrix, nd, "matrix"), _world_affine(moving_affine, nd, "moving_affine"), _world_affine(target_affine, nd, "target_affine")
    return (_norm_to_voxel(ms, inverse=True) @ torch.linalg.inv(Am) @ T @ At @ _norm_to_voxel(ts))[:, :nd]


def world_from_theta(theta, moving_affine, target_affine, moving_shape, target_shape):
    """The inverse of theta_from_world: an effective theta [nd, nd+1] / [B, nd, nd+1] -> the world transform [B, nd+1, nd+1] fp64,
    A_m N(S_m) theta N(S_t)^-1 A_t^-1."""
    ms, ts, nd = _world_shapes(moving_shape, target_shape)
    Am, At = _world_affine(moving_affine, nd, "moving_affine"), _world_affine(target_affine, nd, "target_affine")
    return Am @ _norm_to_voxel(ms) @ _homogeneous(theta, nd) @ _norm_to_voxel(ts, inverse=True) @ torch.linalg.inv(At)


def image_moments(x, mask=None):
    """(mass [B], centre [B, nd]) fp64 on x's device (include/trx.h: trx_image_moments): x [B,1,*spatial] fp32 on the GPU, mask (see _mask_u8, on
    x's lattice) or None.  The weights are v - the volume's minimum over the counted voxels, so the centre is that of the contrast; it is in voxel
    indices, in the TENSOR's axis order.  ValueError for a volume without contrast (mass 0) or an empty mask.  Deterministic; reads the result back."""
    _require_gpu(x, "x")
    if x.dim() not in (4, 5) or x.shape[1] != 1:
        raise ValueError(f"expected [B,1,H,W] or [B,1,D,H,W], got {tuple(x.shape)}")
    lib = _lib.load()
    vol = x.detach().float().contiguous()
    B, nd, dev = vol.shape[0], vol.dim() - 2, vol.device
    D, H, W = _dhw(tuple(vol.shape[2:]))
    flat = vol.reshape(B, -1)
    m8 = None
    if mask is not None:
        m8 = _mask_u8(mask, vol)
        if bool((m8.reshape(B, -1).sum(1) == 0).any()):
            raise ValueError("image_moments: a mask is empty")
        offset = torch.where(m8.reshape(B, -1) != 0, flat, torch.full_like(flat, float("inf"))).amin(1).contiguous()
    else:
        offset = flat.amin(1).contiguous()
    ws_bytes = lib.trx_image_moments_workspace_bytes(nd, B, D, H, W)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_image_moments_workspace_bytes rejected {B} x {tuple(vol.shape[2:])}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 1 + nd, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.trx_image_moments(_lib.ptr(vol), _lib.ptr(m8), _lib.ptr(offset), nd, B, D, H, W, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream(dev))
    _lib.check(rc, "trx_image_moments")
    mass = out[:, 0]
    if bool((mass <= 0).any()) or not bool(torch.isfinite(out).all()):
        raise ValueError("image_moments: a volume has no contrast over the counted voxels (or a non-finite voxel)")
    return mass, (out[:, 1:] / mass[:, None]).flip(1)


def image_covariance(x, mask=None):
    """(mass [B], centre [B, nd], cov [B, nd, nd]) fp64 on the CPU (include/trx.h: trx_image_moments2): x, mask and the weights
    w = v - the volume's minimum over the counted voxels as image_moments; centre and covariance in voxel indices, the TENSOR's axis order.  The kernel
    hands out the raw sums; the central moments cov = sum w p p^T / m - c c^T are formed here, on the host, in fp64.  ValueError where image_moments
    raises it.  Deterministic; reads the result back."""
    _require_gpu(x, "x")
    if x.dim() not in (4, 5) or x.shape[1] != 1:
        raise ValueError(f"expected [B,1,H,W] or [B,1,D,H,W], got {tuple(x.shape)}")
    lib = _lib.load()
    vol = x.detach().float().contiguous()
    B, nd, dev = vol.shape[0], vol.dim() - 2, vol.device
    D, H, W = _dhw(tuple(vol.shape[2:]))
    flat = vol.reshape(B, -1)
    m8 = None
    if mask is not None:
        m8 = _mask_u8(mask, vol)
        if bool((m8.reshape(B, -1).sum(1) == 0).any()):
            raise ValueError("image_covariance: a mask is empty")
        offset = torch.where(m8.reshape(B, -1) != 0, flat, torch.full_like(flat, float("inf"))).amin(1).contiguous()
    else:
        offset = flat.amin(1).contiguous()
    ws_bytes = lib.trx_image_moments2_workspace_bytes(nd, B, D, H, W)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_image_moments2_workspace_bytes rejected {B} x {tuple(vol.shape[2:])}")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 1 + nd + nd * (nd + 1) // 2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.trx_image_moments2(_lib.ptr(vol), _lib.ptr(m8), _lib.ptr(offset), nd, B, D, H, W, _lib.ptr(out), _lib.ptr(ws), ws_bytes, _lib.current_stream(dev))
    _lib.check(rc, "trx_image_moments2")
    return covariance_from_sums(out.cpu(), nd, "image_covariance")


def covariance_from_sums(sums, nd, what="covariance_from_sums"):
    """trx_image_moments2's rows [B, ncol] (fp64, host) -> (mass [B], centre [B, nd], cov [B, nd, nd]) in the TENSOR's axis order.  The rows are in x, y(, z)
    order with the products as xx, xy, yy(, xz, yz, zz)."""
    sums = sums.to("cpu", torch.float64)
    mass = sums[:, 0]
    if bool((mass <= 0).any()) or not bool(torch.isfinite(sums).all()):
        raise ValueError(f"{what}: a volume has no contrast over the counted voxels (or a non-finite voxel)")
    c = sums[:, 1:1 + nd] / mass[:, None]
    M2 = torch.zeros(sums.shape[0], nd, nd, dtype=torch.float64)
    k = 1 + nd
    for j in range(nd):          # xx | xy yy | xz yz zz: column j of the upper triangle, rows 0 .. j
        for i in range(j + 1):
            M2[:, i, j] = M2[:, j, i] = sums[:, k]
            k += 1
    cov = M2 / mass[:, None, None] - c[:, :, None] * c[:, None, :]
    return mass, c.flip(1), cov.flip(1).flip(2)


def _sign_matrices(nd):
    """The 2^nd diagonals of +-1 in the documented order: itertools.product((1, -1), repeat=nd) - the first axis slowest, +1 before -1."""
    import itertools
    return [torch.tensor(s, dtype=torch.float64) for s in itertools.product((1.0, -1.0), repeat=nd)]


def principal_axes(cov):
    """(eigenvalues [B, nd] ascending, axes [B, nd, nd] in columns) of symmetric matrices [B, nd, nd]: torch.linalg.eigh, each eigenvector's sign fixed
    so that its entry of largest magnitude (the first such) is positive - the candidates' order must not depend on LAPACK's choice."""
    w, V = torch.linalg.eigh(cov.to("cpu", torch.float64))
    pick = V.abs().argmax(dim=1, keepdim=True)
    sgn = torch.sign(torch.gather(V, 1, pick))
    return w, V * torch.where(sgn == 0, torch.ones_like(sgn), sgn)


def _about(R, c_t, c_m):
    """Homogeneous [..., nd+1, nd+1] fp64 of p_m = R (p_t - c_t) + c_m: R [..., nd, nd], the centres [..., nd] broadcasting against it."""
    nd = R.shape[-1]
    T = torch.zeros(R.shape[:-2] + (nd + 1, nd + 1), dtype=torch.float64)
    T[..., :nd, :nd] = R
    T[..., :nd, nd] = c_m - (R @ c_t[..., None])[..., 0]
    T[..., nd, nd] = 1.0
    return T


def principal_axes_candidates(cov_m, centre_m, cov_t, centre_t):
    """The principal-axes candidates T0 [B, K, nd+1, nd+1] fp64 (host) from the two images' WORLD covariances [B, nd, nd]
    (A[:nd,:nd] C A[:nd,:nd]^T of image_covariance's C) and world centres of mass [B, nd], rows x, y(, z) in mm:
    T0_k : p_m = R_k (p_t - c_t) + c_m,  R_k = V_m S_k V_t^T, V = principal_axes (eigenvalues ascending, signs fixed), S_k = diag(+-1) with det R_k = +1.
    K = 4 in 3-D, 2 in 2-D; the order is that of itertools.product((1, -1), repeat=nd) over the diagonal of S, those with det R = -1 left out.
    No degeneracy threshold: near-equal eigenvalues make the axes meaningless - the mutual information of world_search is what rejects a candidate."""
    cov_m, cov_t = (torch.as_tensor(c).detach().to("cpu", torch.float64) for c in (cov_m, cov_t))
    c_m, c_t = (torch.as_tensor(c).detach().to("cpu", torch.float64) for c in (centre_m, centre_t))
    if cov_m.dim() != 3 or cov_m.shape != cov_t.shape or cov_m.shape[1] not in (2, 3) or cov_m.shape[1] != cov_m.shape[2] or \
            tuple(c_m.shape) != tuple(cov_m.shape[:2]) or c_t.shape != c_m.shape:
        raise ValueError(f"expected covariances [B,nd,nd] and centres [B,nd], got {tuple(cov_m.shape)}, {tuple(c_m.shape)}, {tuple(cov_t.shape)}, {tuple(c_t.shape)}")
    nd = cov_m.shape[1]
    Vm, Vt = principal_axes(cov_m)[1], principal_axes(cov_t)[1]
    out = []
    for b in range(cov_m.shape[0]):
        Rs = [Vm[b] @ torch.diag(s) @ Vt[b].T for s in _sign_matrices(nd)]
        Rs = torch.stack([R for R in Rs if float(torch.linalg.det(R)) > 0.0])
        out.append(_about(Rs, c_t[b], c_m[b]))
    return torch.stack(out)


def rotation_grid(nd, step_deg):
    """Rotations [C, nd, nd] fp64 on a regular Euler grid.  3-D: Rz(gamma) Ry(beta) Rx(alpha) with alpha, gamma in {-180, -180 + step,
    ... < 180} and beta in {-90, ..., 90}, C = (360 / step)^2 (180 / step + 1); 2-D: the rotation by gamma alone, C = 360 / step.  The identity is
    candidate 0; the others follow in the order alpha (slowest), beta, gamma.  Duplicates at beta = +-90 degrees stay.  ValueError unless step divides 90."""
    step = float(step_deg)
    if nd not in (2, 3) or not (step > 0.0) or abs(90.0 / step - round(90.0 / step)) > 1e-9:
        raise ValueError(f"rotation_grid: nd must be 2 or 3 and the step must divide 90 degrees, got nd = {nd}, step = {step_deg}")
    n = int(round(360.0 / step))
    full = [-180.0 + step * i for i in range(n)]
    half = [-90.0 + step * i for i in range(n // 2 + 1)]

    def rot(axis, deg):
        a = math.radians(deg)
        c, s = math.cos(a), math.sin(a)
        if nd == 2:
            return torch.tensor([[c, -s], [s, c]], dtype=torch.float64)
        return torch.tensor({0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis],
                            dtype=torch.float64)
    if nd == 2:
        angles = [(g,) for g in full]
        mats = [rot(2, g) for g in full]
    else:
        angles = [(a, b, g) for a in full for b in half for g in full]
        mats = [rot(2, g) @ rot(1, b) @ rot(0, a) for a, b, g in angles]
    first = angles.index((0.0,) * (1 if nd == 2 else 3))
    mats[first] = torch.eye(nd, dtype=torch.float64)
    return torch.stack([mats[first]] + mats[:first] + mats[first + 1:])


class WorldSearch:
    """What world_search found, all on the CPU: init [B,nd+1,nd+1] fp64 (the chosen candidate after its refinement, p_moving = init p_target), center [B,nd]
    (the world point theta acted about), candidates [B,K,nd+1,nd+1], scores [B,K] fp32 (the mutual-information loss of every candidate), kept [B,keep]
    (indices of the lowest scores, ascending score, ties by index), refined [B,keep] fp32 (their best losses over the refinement), chosen [B] (the
    candidate index behind init) and eigenvalues (moving [B,nd], target [B,nd]; ascending, mm^2; None for a caller's candidates) - near-equal ones say
    that the principal axes carried no information."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


SEARCH_CHUNK = 64       # candidates per evaluation call (the batch axis of trx_affine_mi_loss_grad_grids)


def world_moments(x, affine, mask=None):
    """(centre [B,nd], cov [B,nd,nd]) fp64 on the CPU of x [B,1,*spatial] in WORLD mm under its voxel-to-world matrices [nd+1,nd+1] / [B,nd+1,nd+1]:
    A c + t and A[:nd,:nd] C A[:nd,:nd]^T of image_covariance's centre and covariance."""
    nd = x.dim() - 2
    A = _world_affine(affine, nd, "affine", x.shape[0]).expand(x.shape[0], nd + 1, nd + 1)
    _, ctr, cov = image_covariance(x, mask)
    lin = A[:, :nd, :nd]
    return (lin @ ctr[:, :, None])[:, :, 0] + A[:, :nd, nd], lin @ cov @ lin.transpose(1, 2)


def world_search(moving, target, moving_affine, target_affine, candidates="principal_axes", mask=None, moving_mask=None, overlap=None, mi=None, step=45.0,
                 keep=8, iters=30, lr=0.01, optimizer="adam", moments=None):
    """A rigid starting transform for world-geometry registration when the headers' orientation cannot be trusted: candidates
    scored by the mutual information of the fused evaluation, the best few refined by the rigid device loop.  Returns a WorldSearch.
    moving / target [B,1,*spatial] fp32 on the GPU with voxel-to-world matrices as world_geometry takes them; mask / moving_mask / overlap / mi as
    AffineMISolver.  candidates: 'principal_axes' - the K of principal_axes_candidates from the two images' second moments (image_covariance inside
    mask / moving_mask); 'search' - those K, then the centre-of-mass alignment composed with every rotation of rotation_grid(nd, step) about the target's
    centre of mass; or a tensor [K,nd+1,nd+1] / [B,K,nd+1,nd+1] of world transforms p_moving = T0 p_target.  moments: (centre_m, cov_m, centre_t, cov_t)
    in world mm taken elsewhere (world_setup takes them on the full-resolution images and searches on a coarse level) instead of image_covariance here.
    Every candidate is scored at theta = identity, loss only, by trx_affine_mi_loss_grad_grids: per pair, the candidates along the batch axis in chunks
    of SEARCH_CHUNK with image strides 0 - the images are not copied; records, masks and the pair's own intensity ranges are replicated per chunk.  The
    `keep` lowest are refined together by `iters` iterations of ONE rigid AffineMISolver (each with its own record and theta; optimizer, lr), and
    init = T0_k Tr(c) Theta_best Tr(-c) of the candidate whose best loss is lowest, c = the target's centre of mass (a caller's candidates: its geometric
    centre).  iters = 0: the best-scored candidate as it is.  Always rigid."""
    _require_gpu(moving, "moving")
    _require_gpu(target, "target")
    if moving.dim() not in (4, 5) or target.dim() != moving.dim() or moving.shape[1] != 1 or target.shape[1] != 1 or moving.shape[0] != target.shape[0]:
        raise ValueError(f"expected two [B,1,*spatial] tensors of one batch size, got {tuple(moving.shape)} and {tuple(target.shape)}")
    ms, ts, nd = _world_shapes(moving.shape[2:], target.shape[2:])
    B, dev, n1 = target.shape[0], target.device, nd + 1
    keep, iters = int(keep), int(iters)
    if keep < 1 or iters < 0:
        raise ValueError(f"world_search: keep must be at least 1 and iters at least 0, got {keep} and {iters}")
    Am = _world_affine(moving_affine, nd, "moving_affine", B).expand(B, n1, n1)
    At = _world_affine(target_affine, nd, "target_affine", B).expand(B, n1, n1)
    if mask is not None:
        mask = _mask_u8(mask, target)
    overlap, moving_mask = overlap_args(overlap, moving_mask, moving)
    mi = {} if mi is None else dict(mi)
    eig = None
    if isinstance(candidates, str):
        if candidates not in ("principal_axes", "search"):
            raise ValueError(f"candidates must be 'principal_axes', 'search' or a tensor of world transforms, got {candidates!r}")
        if moments is None:
            (cm, Cm), (ct, Ct) = world_moments(moving, Am, moving_mask), world_moments(target, At, mask)
        else:
            cm, Cm, ct, Ct = (torch.as_tensor(t).detach().to("cpu", torch.float64) for t in moments)
        eig = (principal_axes(Cm)[0], principal_axes(Ct)[0])
        T0 = principal_axes_candidates(Cm, cm, Ct, ct)
        if candidates == "search":
            grid = rotation_grid(nd, step)
            T0 = torch.cat([T0, torch.stack([_about(grid, ct[b], cm[b]) for b in range(B)])], dim=1)
        center = ct
    else:
        T0 = torch.as_tensor(candidates).detach().to("cpu", torch.float64)
        if T0.dim() == 3:
            T0 = T0[None].expand(B, *T0.shape)
        if T0.dim() != 4 or T0.shape[0] != B or T0.shape[1] < 1 or tuple(T0.shape[2:]) != (n1, n1):
            raise ValueError(f"candidates must be [K,{n1},{n1}] or [{B},K,{n1},{n1}], got {tuple(T0.shape)}")
        T0 = _world_affine(T0.reshape(-1, n1, n1), nd, "candidates").reshape(B, -1, n1, n1)
        center = lattice_center(ts, At).expand(B, nd)
    K = T0.shape[1]
    keep = min(keep, K)
    lib = _lib.load()
    mov, tgt = moving.detach().contiguous(), target.detach().contiguous()
    tables = base_tables(ts, dev)
    scores = torch.empty(B, K)
    kept, refined, chosen, init = torch.empty(B, keep, dtype=torch.long), torch.empty(B, keep), torch.empty(B, dtype=torch.long), torch.empty(B, n1, n1, dtype=torch.float64)
    for b in range(B):
        geo = world_geometry(ms, ts, Am[b], At[b], T0[b], center[b])               # K records of one pair
        mk_b = None if mask is None else mask[b:b + 1]
        mm_b = None if moving_mask is None else moving_mask[b:b + 1].to(dev)
        cfg1, rng1, _ = _mi_cfg(mi, tgt[b:b + 1], mov[b:b + 1], mk_b, overlap, mm_b)      # the run's own ranges: fitted once to (target, moving)
        rec = geo.record.to(dev)
        for k0 in range(0, K, SEARCH_CHUNK):
            n = min(SEARCH_CHUNK, K - k0)
            vol = _volumes(mov[b:b + 1], tgt[b:b + 1], 0, 0, ts, tables=tables)     # strides 0: every candidate reads the same two images
            vol.B = n
            rng = rng1.expand(n, 4).contiguous()
            mk = None if mk_b is None else mk_b.expand(n, *mk_b.shape[1:]).contiguous()
            mm = None if mm_b is None else mm_b.expand(n, *mm_b.shape[1:]).contiguous()
            cfg = _mi_cfg_c(cfg1.bins, cfg1.alpha, cfg1.normalized, rng, mk)
            recs = rec[k0:k0 + n].contiguous()
            mg = _moving_grid(ms, None, overlap, mm, recs)
            th = pad_theta(torch.eye(nd, n1, device=dev).repeat(n, 1, 1), nd)
            ws_bytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), cfg.bins)
            if ws_bytes == 0:
                raise _lib.TrxError(f"trx_affine_mi_workspace_bytes rejected {n} x {ts} with {cfg.bins} bins")
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            loss = torch.empty(n, device=dev)
            with torch.cuda.device(dev):
                rc = lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), _lib.ptr(th), _lib.ptr(loss), None, _lib.ptr(ws),
                                                       ws_bytes, _lib.current_stream(dev))
            _lib.check(rc, "trx_affine_mi_loss_grad_grids")
            scores[b, k0:k0 + n] = loss.cpu()             # (the copy waits for the call: its tensors may go)
        kept[b] = torch.sort(scores[b], stable=True).indices[:keep]
        if iters == 0:
            refined[b], chosen[b], init[b] = scores[b, kept[b]], kept[b, 0], T0[b, kept[b, 0]]
            continue
        sub = WorldGeometry(geo.record[kept[b]], geo.center[kept[b]], geo.init[kept[b]], geo.extent[kept[b]])
        rep = lambda t: None if t is None else t.expand(keep, *t.shape[1:])  # noqa: E731
        solver = AffineMISolver(rep(mov[b:b + 1]), rep(tgt[b:b + 1]), mode="rigid", mi=mi, optimizer=optimizer, lr=lr, init=torch.zeros(keep, 6 if nd == 3 else 3),
                                capacity=iters, mask=rep(mk_b), overlap=overlap, moving_mask=rep(mm_b), world=sub)
        solver.run(iters)
        refined[b] = solver.best_loss.cpu()
        j = int(torch.sort(refined[b], stable=True).indices[0])
        chosen[b], init[b] = kept[b, j], sub.matrix(solver.best)[j]
    return WorldSearch(init=init, center=center.clone(), candidates=T0, scores=scores, kept=kept, refined=refined, chosen=chosen, eigenvalues=eig)


_run_world_search = world_search      # (world_setup and the solvers have a keyword of the same name)
WORLD_INITS = (None, "centers", "moments", "principal_axes", "search")
SEARCH_KEYS = ("step", "keep", "iters")


def world_setup(moving, target, moving_affine, target_affine, world_init=None, mask=None, moving_mask=None, world_search=None, overlap=None, mi=None,
                search_on=None):
    """WorldGeometry of a pair of tensors [B,1,*spatial] from their headers and world_init: None (trust the headers: T0 = I, c = the target's geometric
    centre), 'centers' (T0 = the translation between the geometric centres), 'moments' (T0 = the translation between the intensity centres of mass -
    image_moments inside mask / moving_mask where given - and c = the target's centre of mass) or a world matrix [nd+1, nd+1] / [B, nd+1, nd+1].
    'principal_axes' / 'search' (DESIGN.md section 4.21): T0 = world_search(candidates=world_init).init, c = the target's centre of mass, the record in
    `.search` of the result.  world_search: dict of step / keep / iters for it; overlap, mi: the run's, handed to it.  The moments are taken on these
    (full-resolution) images; search_on = (moving, target, mask, moving_mask) are the images the candidates are scored and refined on - the first
    level of a coarse-to-fine run - and default to the images themselves."""
    ms, ts, nd = _world_shapes(moving.shape[2:], target.shape[2:])
    B = target.shape[0]
    if isinstance(world_init, str) and world_init not in WORLD_INITS:
        raise ValueError(f"world_init must be None, 'centers', 'moments', 'principal_axes', 'search' or a matrix, got {world_init!r}")
    searching = isinstance(world_init, str) and world_init in ("principal_axes", "search")
    if world_search is not None and (not searching or not isinstance(world_search, dict) or set(world_search) - set(SEARCH_KEYS)):
        raise ValueError(f"world_search is a dict of {SEARCH_KEYS} for world_init='principal_axes' / 'search', got {world_search!r} with world_init = {world_init!r}")
    Am, At = _world_affine(moving_affine, nd, "moving_affine", B), _world_affine(target_affine, nd, "target_affine", B)
    if searching:
        (cm, Cm), (ct, Ct) = world_moments(moving, Am, moving_mask), world_moments(target, At, mask)
        lm, lt, lmask, lmmask = (moving, target, mask, moving_mask) if search_on is None else search_on
        found = _run_world_search(lm, lt, level_affine(Am, ms, tuple(lm.shape[2:])), level_affine(At, ts, tuple(lt.shape[2:])), candidates=world_init, mask=lmask,
                                  moving_mask=lmmask, overlap=overlap, mi=mi, moments=(cm, Cm, ct, Ct), **(world_search or {}))
        geo = world_geometry(ms, ts, Am, At, found.init, ct)
    elif isinstance(world_init, str) and world_init == "moments":
        def com(x, A, m):
            ctr = image_moments(x, m)[1].cpu()                                       # voxel indices, the tensor's axis order: A's columns
            return (A[:, :nd, :nd] @ ctr[:, :, None])[:, :, 0] + A[:, :nd, nd]
        cm, ct = com(moving, Am, moving_mask), com(target, At, mask)
        geo = world_geometry(ms, ts, Am, At, _translation(cm - ct), ct)
    else:
        if world_init is not None and not isinstance(world_init, str):
            world_init = _world_affine(world_init, nd, "world_init", B)
        geo = world_geometry(ms, ts, Am, At, world_init)
    if geo.B not in (1, B):
        raise ValueError(f"the headers describe {geo.B} pairs, the batch has {B}")
    if geo.B != B:
        geo = WorldGeometry(*(t.expand(B, *t.shape[1:]).contiguous() for t in (geo.record, geo.center, geo.init, geo.extent)))
    if searching:
        geo.search = found
    return geo


class _GridPair:
    """B single-channel (moving, target) pairs on two lattices, described for the cross-lattice entry points (include/trx.h: trx_moving_grid):
    the Volumes carry the TARGET lattice and its base-coordinate tables, the MovingGrid the moving lattice and the scales.  _Batch keeps
    refusing differing shapes; this is the description of the pair the new path uses."""

    def __init__(self, moving, target, scale=None, moving_voxel=None, target_voxel=None):
        _require_gpu(moving, "moving")
        _require_gpu(target, "target")
        if moving.dim() not in (4, 5) or target.dim() != moving.dim():
            raise ValueError(f"expected two [B,1,H,W] or two [B,1,D,H,W] tensors, got {tuple(moving.shape)} and {tuple(target.shape)}")
        if moving.shape[1] != 1 or target.shape[1] != 1:
            raise ValueError("the mutual-information path takes single-channel volumes [B,1,...]")
        if moving.shape[0] != target.shape[0]:
            raise ValueError("moving and target batch sizes differ")
        self.moving, self.target = moving.contiguous(), target.contiguous()
        self.nd, self.B, self.C, self.device = moving.dim() - 2, moving.shape[0], 1, moving.device
        self.spatial, self.moving_spatial = tuple(target.shape[2:]), tuple(moving.shape[2:])
        if scale is None:
            scale = grid_scale(self.moving_spatial, self.spatial, moving_voxel, target_voxel)
        scale = torch.as_tensor(scale).detach().to("cpu", torch.float32)
        if tuple(scale.shape) != (self.nd, self.nd + 1):
            raise ValueError(f"expected a scale of shape {(self.nd, self.nd + 1)}, got {tuple(scale.shape)}")
        self.scale = scale                                        # what the kernels multiply by: fp32
        self.half_extent_moving = None if moving_voxel is None else _half_extents(self.moving_spatial, moving_voxel, "moving_voxel")
        self.tables = base_tables(self.spatial, self.device)

    def vol(self):
        return _volumes(self.moving, self.target, self.moving[0].numel(), self.target[0].numel(), self.spatial, tables=self.tables)

    def grid(self, overlap=False, moving_mask=None, world=None):
        return _moving_grid(self.moving_spatial, self.scale, overlap, moving_mask, world)


def _moving_grid(moving_spatial, scale=None, overlap=False, moving_mask=None, world=None):
    """trx_moving_grid of a moving lattice (the tensor's spatial shape) and a scale [nd, nd+1] (None: ones); overlap / moving_mask (uint8 on the
    device, kept alive by the caller): the overlap rule and its mask on the moving lattice; world (fp64 [B, 32] on the device, kept alive by the
    caller): the world-geometry records, in whose presence the scale is not read."""
    g = _lib.MovingGrid()
    g.overlap, g.mask = int(bool(overlap)), None if moving_mask is None else moving_mask.data_ptr()
    g.world = None if world is None else world.data_ptr()
    g.D, g.H, g.W = _dhw(tuple(moving_spatial))
    nd = len(moving_spatial)
    flat = [1.0] * (nd * (nd + 1)) if scale is None else [float(s) for s in scale.reshape(-1)]
    for k in range(PSTRIDE):
        g.scale[k] = flat[k] if k < len(flat) else 0.0
    return g


def _affine_warp_grids(lib, theta, moving, size):
    """affine_warp(..., size=) on a lattice other than moving's: trx_affine_warp_grids with scale 1 (theta is the effective one)."""
    _require_gpu(moving, "moving")
    if moving.dim() not in (4, 5) or len(size) != moving.dim() - 2 or min(size) < 1:
        raise ValueError(f"expected [B,C,H,W] or [B,C,D,H,W] and a size of as many positive entries, got {tuple(moving.shape)} and {size}")
    mov = moving.contiguous()
    B, C, nd, dev = mov.shape[0], mov.shape[1], mov.dim() - 2, mov.device
    th = pad_theta(theta.detach().to(dev).reshape(B, -1), nd)
    out = torch.empty((B, C) + size, dtype=torch.float32, device=dev)
    v = _volumes(mov, None, mov[0].numel(), 0, size, tables=base_tables(size, dev))
    mg = _moving_grid(tuple(mov.shape[2:]))
    with torch.cuda.device(dev):
        rc = lib.trx_affine_warp_grids(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), C, _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "trx_affine_warp_grids")
    return out


def _initial_theta(theta, B, nd, device=None):
    """An initial affine for the composed warp: [B,nd,nd+1] (or one [nd,nd+1] / [1,nd,nd+1] for every pair) -> [B, PSTRIDE] fp32 (on `device`)."""
    if not isinstance(theta, torch.Tensor) or theta.numel() % (nd * (nd + 1)) != 0 or theta.numel() // (nd * (nd + 1)) not in (1, B) or \
            tuple(theta.shape[-2:]) != (nd, nd + 1):
        raise ValueError(f"expected an initial theta of shape {(B, nd, nd + 1)}, got {tuple(theta.shape) if isinstance(theta, torch.Tensor) else type(theta).__name__}")
    th = theta.detach().reshape(-1, nd, nd + 1).expand(B, nd, nd + 1)
    return pad_theta(th if device is None else th.to(device), nd)


def _affine_flow_call(x, theta, flow, scale):
    """The arguments the two composed-warp entry points share: (Volumes of the TARGET lattice = flow's, MovingGrid, theta [B,PSTRIDE], flow, x), all
    contiguous and kept alive by the caller."""
    _require_gpu(x, "x")
    _require_gpu(flow, "flow")
    if x.dim() not in (4, 5) or flow.dim() != x.dim():
        raise ValueError(f"expected x [B,C,*moving spatial] and flow [B,nd,*target spatial] of 2 or 3 spatial dims, got {tuple(x.shape)} and {tuple(flow.shape)}")
    nd, B = x.dim() - 2, x.shape[0]
    if flow.shape[0] != B or flow.shape[1] != nd:
        raise ValueError(f"flow shape {tuple(flow.shape)} is not [{B},{nd},*target spatial]")
    mov, fl = x.contiguous(), flow.detach().contiguous()
    th = _initial_theta(theta, B, nd, x.device)
    if scale is not None:
        scale = torch.as_tensor(scale).detach().to("cpu", torch.float32)
        if tuple(scale.shape) != (nd, nd + 1):
            raise ValueError(f"expected a scale of shape {(nd, nd + 1)}, got {tuple(scale.shape)}")
    v = _volumes(mov, None, mov[0].numel(), 0, fl.shape[2:])      # no tables: the composed position is not an integer, the closed form serves it
    return v, _moving_grid(tuple(mov.shape[2:]), scale), th, fl, mov


def _affine_flow_forward(x, theta, flow, scale):
    lib = _lib.load()
    v, mg, th, fl, mov = _affine_flow_call(x, theta, flow, scale)
    out = torch.empty((mov.shape[0], mov.shape[1]) + tuple(fl.shape[2:]), dtype=torch.float32, device=mov.device)
    with torch.cuda.device(mov.device):
        rc = lib.trx_affine_flow_warp(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), _lib.ptr(fl), mov.shape[1], _lib.ptr(out), _lib.current_stream(mov.device))
    _lib.check(rc, "trx_affine_flow_warp")
    return out


def affine_flow_warp_backward(x, theta, flow, grad_out, scale=None):
    """dL/dflow [B,nd,*target spatial] of affine_flow_warp for dL/dout = grad_out [B,C,*target spatial] (trx_affine_flow_warp_backward): a gather per
    target voxel, the same bits on every call.  No gradient with respect to theta or x."""
    lib = _lib.load()
    v, mg, th, fl, mov = _affine_flow_call(x, theta, flow, scale)
    _require_gpu(grad_out, "grad_out")
    if tuple(grad_out.shape) != (mov.shape[0], mov.shape[1]) + tuple(fl.shape[2:]):
        raise ValueError(f"grad_out shape {tuple(grad_out.shape)} is not the warp's {(mov.shape[0], mov.shape[1]) + tuple(fl.shape[2:])}")
    go = grad_out.detach().contiguous()
    dfl = torch.empty_like(fl)
    with torch.cuda.device(mov.device):
        rc = lib.trx_affine_flow_warp_backward(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), _lib.ptr(fl), mov.shape[1], _lib.ptr(go), _lib.ptr(dfl),
                                               _lib.current_stream(mov.device))
    _lib.check(rc, "trx_affine_flow_warp_backward")
    return dfl


class _AffineFlowWarpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, theta, flow, scale):
        ctx.save_for_backward(x, theta, flow)
        ctx.scale = scale
        return _affine_flow_forward(x, theta, flow, scale)

    @staticmethod
    def backward(ctx, grad_out):
        x, theta, flow = ctx.saved_tensors
        dflow = affine_flow_warp_backward(x, theta, flow, grad_out, ctx.scale) if ctx.needs_input_grad[2] else None
        return None, None, dflow, None      # no gradient flows to the moving image or to theta on this path


def affine_flow_warp(x, theta, flow, scale=None):
    """A deformation composed with an initial affine, sampled once (extension, include/trx.h: trx_affine_flow_warp): x [B,C,*moving spatial], theta
    [B,nd,nd+1], flow [B,nd,*target spatial] in target voxels (channel i along spatial dim i), scale [nd,nd+1] (grid_scale; None = ones:
    theta is the effective one) -> [B,C,*target spatial] = grid_sample(x, theta_eff applied to the normalised positions voxel + flow,
    align_corners=False).  Differentiable with respect to flow (trx_affine_flow_warp_backward)."""
    return _AffineFlowWarpFn.apply(x, theta, flow, scale)


INTERPOLATIONS = ("nearest", "linear", "cubic")


def affine_flow_valid(moving_spatial, theta, flow, scale=None, mask=None, moving_mask=None):
    """The overlap rule at the composed warp's coordinates (extension, include/trx.h: trx_affine_flow_valid): uint8 [B,1,*target spatial], 1 where
    target voxel x counts - mask at x (target lattice, or None), the sample coordinate of affine_flow_warp(., theta, flow, scale) inside a moving
    image of `moving_spatial`, moving_mask (moving lattice, or None) non-zero at the nearest moving voxel.  flow [B,nd,*target spatial] on the GPU."""
    lib = _lib.load()
    _require_gpu(flow, "flow")
    nd, B, dev = flow.dim() - 2, flow.shape[0], flow.device
    moving_spatial = tuple(int(s) for s in moving_spatial)
    if nd not in (2, 3) or flow.shape[1] != nd or len(moving_spatial) != nd:
        raise ValueError(f"expected a flow [B,nd,*target spatial] and a moving shape of nd sizes, got {tuple(flow.shape)} and {moving_spatial}")
    spatial = tuple(flow.shape[2:])
    like_t, like_m = torch.empty((B, 1) + spatial, device=dev), torch.empty((B, 1) + moving_spatial, device=dev)      # (shapes and device for _mask_u8)
    m8 = None if mask is None else _mask_u8(mask, like_t)
    mm8 = None if moving_mask is None else _mask_u8(moving_mask, like_m)
    fl = flow.detach().contiguous().float()
    if isinstance(theta, torch.Tensor) and tuple(theta.shape) == (B, PSTRIDE):      # a solver's padded rows
        theta = theta[:, : nd * (nd + 1)].reshape(B, nd, nd + 1)
    th = _initial_theta(theta, B, nd, dev)
    v = _lib.Volumes()
    v.moving = v.target = fl.data_ptr()      # (not read: the rule needs coordinates only; the checks want non-null images)
    v.moving_stride, v.target_stride, v.ndim, v.B = math.prod(moving_spatial), math.prod(spatial), nd, B
    v.D, v.H, v.W = _dhw(spatial)
    mg = _moving_grid(moving_spatial, None if scale is None else torch.as_tensor(scale).float(), True, mm8)
    out = torch.empty((B, 1) + spatial, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.trx_affine_flow_valid(ctypes.byref(v), ctypes.byref(mg), _lib.ptr(th), _lib.ptr(fl), _lib.ptr(m8), _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "trx_affine_flow_valid")
    return out


def check_interpolation(value):
    """ValueError unless `value` is one of INTERPOLATIONS; host only."""
    if value not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be 'nearest', 'linear' or 'cubic', got {value!r}")
    return value


def spline_coefficients(x):
    """The coefficients of the interpolating cubic B-spline of x [B,C,*spatial] (fp32, GPU) with whole-sample mirror boundaries, the same shape
    (extension, include/trx.h: trx_spline_coefficients; = scipy.ndimage.spline_filter(order=3, mode='mirror') per volume).  What resample(...,
    interpolation='cubic') samples; an axis of one voxel is left alone.  Not differentiable."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError(f"expected [B,C,H,W] or [B,C,D,H,W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    _require_gpu(x, "x")
    lib = _lib.load()
    src = x.detach().contiguous()
    nd, n, dhw = src.dim() - 2, src.shape[0] * src.shape[1], _dhw(tuple(src.shape[2:]))
    nbytes = lib.trx_spline_workspace_bytes(nd, n, *dhw)
    if nbytes == ctypes.c_size_t(-1).value:
        raise ValueError(f"spline_coefficients takes 1 .. 65535 volumes (batch x channels) of 1 .. 2^31 - 1 voxels, got {tuple(src.shape)}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=src.device)
    out = torch.empty_like(src)
    with torch.cuda.device(src.device):
        rc = lib.trx_spline_coefficients(_lib.ptr(src), _lib.ptr(out), nd, n, *dhw, _lib.ptr(ws) if nbytes else None, nbytes, _lib.current_stream(src.device))
    _lib.check(rc, "trx_spline_coefficients")
    return out


def _resample_args(x, theta, flow, size, scale, interpolation):
    """What resample refuses, on the host, before any device work: returns (target spatial shape, scale as fp32 on the CPU or None)."""
    check_interpolation(interpolation)
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError(f"expected x [B,C,H,W] or [B,C,D,H,W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if theta is None and flow is None:
        raise ValueError("resample needs a transform: theta, flow or both")
    nd, B = x.dim() - 2, x.shape[0]
    if theta is not None and (not isinstance(theta, torch.Tensor) or theta.dim() != 3 or tuple(theta.shape[1:]) != (nd, nd + 1) or theta.shape[0] not in (1, B)):
        raise ValueError(f"expected theta of shape {(B, nd, nd + 1)} or {(1, nd, nd + 1)}, got {tuple(theta.shape) if isinstance(theta, torch.Tensor) else type(theta).__name__}")
    if scale is not None:
        if theta is None:
            raise ValueError("scale multiplies theta (grid_scale): it needs a theta")
        scale = torch.as_tensor(scale).detach().to("cpu", torch.float32)
        if tuple(scale.shape) != (nd, nd + 1):
            raise ValueError(f"expected a scale of shape {(nd, nd + 1)}, got {tuple(scale.shape)}")
    if size is not None:
        size = tuple(int(s) for s in size)
        if len(size) != nd or min(size) < 1:
            raise ValueError(f"expected a size of {nd} positive entries, got {size}")
    if flow is None:
        return (tuple(x.shape[2:]) if size is None else size), scale
    if not isinstance(flow, torch.Tensor) or flow.dim() != x.dim() or flow.shape[1] != nd or flow.shape[0] not in (1, B):
        raise ValueError(f"expected flow [{B}|1,{nd},*target spatial], got {tuple(flow.shape) if isinstance(flow, torch.Tensor) else type(flow).__name__}")
    target = tuple(flow.shape[2:])
    if size is not None and size != target:
        raise ValueError(f"size {size} is not the flow's lattice {target}")
    if theta is None and target != tuple(x.shape[2:]):
        raise ValueError(f"without theta the flow lives on x's own lattice {tuple(x.shape[2:])}, got a flow on {target}")
    return target, scale


def resample(x, *, theta=None, flow=None, size=None, scale=None, interpolation="cubic"):
    """x [B,C,*spatial] (fp32, GPU) carried through a finished transform with the interpolation of the caller's choice (extension, include/trx.h:
    trx_transform_resample) -> [B,C,*target spatial].  The transform is theta [B|1,nd,nd+1], flow [B|1,nd,*target spatial] (target voxels, channel i
    along spatial dim i) or both - the positions are those of affine_warp / flow_warp / affine_flow_warp: with flow alone x lives on the flow's
    lattice, with theta it may have a lattice of its own; size = the output lattice when only theta is given (default: x's own); scale as for
    affine_flow_warp (grid_scale; None = theta is the effective one).
    interpolation: 'nearest' - x[rint(position)], half to even, 0 where the rounded index lies outside: what carries a label map, an atlas or a
    mask without inventing values; 'linear' - the existing warps themselves, bit for bit; 'cubic' (default) - the interpolating cubic B-spline
    of x with mirror boundaries (spline_coefficients, made on every call), 0 where the position lies more than half a voxel outside x.  The cubic
    form reproduces x at lattice points and overshoots x's range near edges; nothing is clamped.
    Not differentiable ('linear' keeps what the warp it dispatches to offers).  ValueError before any device work for an unknown interpolation,
    for neither theta nor flow, and for shapes that do not fit."""
    target, scale = _resample_args(x, theta, flow, size, scale, interpolation)
    B, C, nd, dev = x.shape[0], x.shape[1], x.dim() - 2, x.device
    if flow is not None and flow.shape[0] != B:
        flow = flow.expand(B, *flow.shape[1:])
    if interpolation == "linear":
        if theta is None:
            return flow_warp(x, flow)
        if flow is not None:
            return affine_flow_warp(x, theta, flow, scale)
        th = theta.detach().to(dev, torch.float32).expand(B, nd, nd + 1)
        return affine_warp(th if scale is None else th * scale.to(dev), x, size=target)
    _require_gpu(x, "x")
    if flow is not None:
        _require_gpu(flow, "flow")
    lib = _lib.load()
    src = x.detach().contiguous()
    if interpolation == "cubic":
        src = spline_coefficients(src)
    th = None if theta is None else _initial_theta(theta, B, nd, dev)
    fl = None if flow is None else flow.detach().contiguous()
    v = _volumes(src, None, src[0].numel(), 0, target)
    mg = None if theta is None else _moving_grid(tuple(src.shape[2:]), scale)
    out = torch.empty((B, C) + target, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.trx_transform_resample(ctypes.byref(v), None if mg is None else ctypes.byref(mg), _lib.ptr(th), _lib.ptr(fl), C,
                                        3 if interpolation == "cubic" else 0, _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "trx_transform_resample")
    return out


CHAINS = {"flow_then_affine": 0, "affine_then_flow": 1}
_ORDERS = {"nearest": 0, "linear": 1, "cubic": 3}


def invert_theta(theta):
    """The effective theta [B,nd,nd+1] (or [nd,nd+1]) of the inverse map: theta maps lattice a's normalised cube to lattice b's, the result maps b's to
    a's - what resample(x_on_target, theta=invert_theta(reg.theta), size=moving_shape) and chain 'affine_then_flow' take.  fp64 on the homogeneous
    matrix, returned as fp64 on the CPU.  ValueError for a wrong shape and for a singular or non-finite matrix."""
    if not isinstance(theta, torch.Tensor) or theta.dim() not in (2, 3) or tuple(theta.shape[-2:]) not in ((2, 3), (3, 4)):
        raise ValueError(f"expected theta [B,nd,nd+1] or [nd,nd+1] with nd 2 or 3, got {tuple(theta.shape) if isinstance(theta, torch.Tensor) else type(theta).__name__}")
    nd = theta.shape[-2]
    H = _homogeneous(theta, nd)
    if not bool(torch.isfinite(H).all()):
        raise ValueError("theta has a non-finite entry: it has no inverse")
    sv = torch.linalg.svdvals(H[:, :nd, :nd])
    if bool((sv[:, -1] <= 1e-12 * sv[:, 0]).any()) or bool((sv[:, 0] == 0).any()):
        raise ValueError("theta's matrix part is singular: it has no inverse")
    inv = torch.linalg.inv(H)[:, :nd]
    return inv if theta.dim() == 3 else inv[0]


def _world_points(points, affine, name):
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] not in (2, 3):
        raise ValueError(f"expected points [B,P,nd] or [P,nd] with nd 2 or 3, got {tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    nd = points.shape[-1]
    A = _world_affine(affine, nd, name, points.shape[0] if points.dim() == 3 else 1)
    p = points.detach().to(torch.float64)
    return p, (A if p.dim() == 3 else A[0]).to(p.device), nd


def points_to_world(points, affine):
    """Voxel positions [B,P,nd] / [P,nd] in the tensor's axis order (z, y, x / y, x) -> world positions (x, y(, z)) in mm under a voxel-to-world matrix of
    optim's convention (columns in the tensor's axis order, rows world x, y(, z); [nd+1,nd+1] or [B,nd+1,nd+1]).  fp64 torch arithmetic on the points'
    device, no kernel: (points_to_world(a, A) - points_to_world(b, A)).norm(dim=-1) is a target registration error in mm."""
    p, A, nd = _world_points(points, affine, "affine")
    return p @ A[..., :nd, :nd].transpose(-1, -2) + A[..., None, :nd, nd]


def points_from_world(points, affine):
    """The inverse of points_to_world: world positions (x, y(, z)) in mm -> voxel positions in the tensor's axis order, fp64."""
    p, A, nd = _world_points(points, affine, "affine")
    Ai = torch.linalg.inv(A)
    return p @ Ai[..., :nd, :nd].transpose(-1, -2) + Ai[..., None, :nd, nd]


def _chain_theta(theta, B, nd, what):
    if not isinstance(theta, torch.Tensor) or theta.dim() != 3 or tuple(theta.shape[1:]) != (nd, nd + 1) or theta.shape[0] not in (1, B):
        raise ValueError(f"{what}: expected theta of shape {(B, nd, nd + 1)} or {(1, nd, nd + 1)}, got {tuple(theta.shape) if isinstance(theta, torch.Tensor) else type(theta).__name__}")


def _chain_shape(shape, nd, name):
    try:
        shape = tuple(int(s) for s in shape)
    except TypeError:
        raise ValueError(f"{name} must be {nd} positive sizes, got {shape!r}") from None
    if len(shape) != nd or min(shape) < 1:
        raise ValueError(f"{name} must be {nd} positive sizes, got {shape}")
    return shape


def _points_args(points, theta, flow, from_shape, to_shape, chain, padding):
    """What transform_points refuses, on the host, before any device work: returns (B, P, nd, from shape, to shape)."""
    if chain not in CHAINS:
        raise ValueError(f"chain must be 'flow_then_affine' or 'affine_then_flow', got {chain!r}")
    if padding not in _FLOW_PADDING:
        raise ValueError(f"padding must be 'border' or 'zeros', got {padding!r}")
    if not isinstance(points, torch.Tensor) or points.dim() not in (2, 3) or points.shape[-1] not in (2, 3) or points.shape[-2] < 1:
        raise ValueError(f"expected points [B,P,nd] or [P,nd] with nd 2 or 3 and P >= 1, got {tuple(points.shape) if isinstance(points, torch.Tensor) else type(points).__name__}")
    if theta is None and flow is None:
        raise ValueError("transform_points needs a transform: theta, flow or both")
    nd, P, B = points.shape[-1], points.shape[-2], (points.shape[0] if points.dim() == 3 else 1)
    if theta is not None:
        _chain_theta(theta, B, nd, "transform_points")
    lattice = None
    if flow is not None:
        if not isinstance(flow, torch.Tensor) or flow.dim() != nd + 2 or flow.shape[1] != nd or flow.shape[0] not in (1, B):
            raise ValueError(f"expected flow [{B}|1,{nd},*spatial], got {tuple(flow.shape) if isinstance(flow, torch.Tensor) else type(flow).__name__}")
        lattice = tuple(flow.shape[2:])
    # the flow lives on the start lattice in chain 0 and on the end lattice in chain 1: that shape defaults from it
    own, other = ("from_shape", "to_shape") if CHAINS[chain] == 0 else ("to_shape", "from_shape")
    shapes = {"from_shape": None if from_shape is None else _chain_shape(from_shape, nd, "from_shape"),
              "to_shape": None if to_shape is None else _chain_shape(to_shape, nd, "to_shape")}
    if lattice is not None:
        if shapes[own] is not None and shapes[own] != lattice:
            raise ValueError(f"{own} {shapes[own]} is not the flow's lattice {lattice} (chain {chain!r})")
        shapes[own] = lattice
    if theta is None:
        if shapes[other] is not None and shapes[other] != shapes[own]:
            raise ValueError(f"without theta both lattices are the flow's {shapes[own]}, got {other} {shapes[other]}")
        shapes[other] = shapes[own]
    if shapes["from_shape"] is None or shapes["to_shape"] is None:
        raise ValueError("theta acts between two lattices: give from_shape and to_shape (the flow's lattice is taken from the flow)")
    return B, P, nd, shapes["from_shape"], shapes["to_shape"]


def transform_points(points, *, theta=None, flow=None, from_shape=None, to_shape=None, chain="flow_then_affine", padding="border"):
    """Points [B,P,nd] or [P,nd] (fp32, GPU; voxel positions in the tensor's axis order) carried through an effective theta [B|1,nd,nd+1], a dense flow
    [B|1,nd,*spatial] or both (extension, include/trx.h: trx_transform_points) -> the same shape.  From the lattice from_shape to the lattice to_shape:
      chain='flow_then_affine': p' = p + S(flow, p) with the flow on from_shape, then theta between the normalised cubes - target voxels to moving
          voxels under a registration's theta_eff(p + u(p)): transform_points(p, theta=reg.initial, flow=reg.theta, to_shape=moving spatial);
      chain='affine_then_flow': theta first, then q + S(flow, q) with the flow on to_shape - the inverse map with invert_theta(theta) and
          invert_flow(flow).
    The flow's lattice is taken from the flow; without theta both lattices are that one.  padding: 'border' (default; the displacement continues past
    a face) or 'zeros' (compose_flows' pair).  A non-finite point comes back as NaN.  Not differentiable.  ValueError before any device work for an
    unknown chain or padding, neither theta nor flow, and shapes that do not fit."""
    B, P, nd, fs, ts = _points_args(points, theta, flow, from_shape, to_shape, chain, padding)
    _require_gpu(points, "points")
    if flow is not None:
        _require_gpu(flow, "flow")
    lib = _lib.load()
    dev = points.device
    pts = points.detach().reshape(B, P, nd).to(torch.float32).contiguous()
    th = None if theta is None else _initial_theta(theta, B, nd, dev)
    fl = None if flow is None else flow.detach().to(torch.float32).expand(B, *flow.shape[1:]).contiguous()
    out = torch.empty_like(pts)
    with torch.cuda.device(dev):
        rc = lib.trx_transform_points(_lib.ptr(pts), _lib.ptr(out), nd, B, P, _lib.ptr(th), _lib.ptr(fl), (ctypes.c_int * 3)(*_dhw(fs)),
                                      (ctypes.c_int * 3)(*_dhw(ts)), CHAINS[chain], _FLOW_PADDING[padding], _lib.current_stream(dev))
    _lib.check(rc, "trx_transform_points")
    return out.reshape(points.shape)


def _chain_resample_args(x, theta, flow, size, interpolation, padding):
    """What resample_affine_then_flow refuses, on the host, before any device work: returns the output lattice."""
    check_interpolation(interpolation)
    if padding not in _FLOW_PADDING:
        raise ValueError(f"padding must be 'border' or 'zeros', got {padding!r}")
    if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
        raise ValueError(f"expected x [B,C,H,W] or [B,C,D,H,W], got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if theta is None and flow is None:
        raise ValueError("resample_affine_then_flow needs a transform: theta, flow or both")
    nd, B = x.dim() - 2, x.shape[0]
    if theta is not None:
        _chain_theta(theta, B, nd, "resample_affine_then_flow")
    if flow is not None:
        if not isinstance(flow, torch.Tensor) or flow.dim() != x.dim() or flow.shape[1] != nd or flow.shape[0] not in (1, B):
            raise ValueError(f"expected flow [{B}|1,{nd},*x's spatial], got {tuple(flow.shape) if isinstance(flow, torch.Tensor) else type(flow).__name__}")
        if tuple(flow.shape[2:]) != tuple(x.shape[2:]):
            raise ValueError(f"the flow lives on x's lattice {tuple(x.shape[2:])} (the affine comes first), got a flow on {tuple(flow.shape[2:])}")
    size = _chain_shape(size, nd, "size")
    if theta is None and size != tuple(x.shape[2:]):
        raise ValueError(f"without theta the output lattice is x's own {tuple(x.shape[2:])}, got size {size}")
    return size


def resample_affine_then_flow(x, *, theta=None, flow=None, size, interpolation="cubic", padding="border"):
    """x [B,C,*spatial] (fp32, GPU) resampled onto the lattice `size` in the chain order resample() does not have: the affine first, then a flow that
    lives on x's own lattice (extension, include/trx.h: trx_affine_then_flow_resample) -> [B,C,*size].  Output voxel y samples x at q + S(flow, q),
    q = theta applied to y between the normalised cubes of `size` and of x's lattice (theta None: q = y, size = x's lattice; flow None: q itself).
    With theta = invert_theta(theta_eff) and flow = invert_flow(u) it carries an image from the target lattice of a registration run with
    optim(initial=...) back onto the moving lattice: Register.to_moving.  interpolation as for resample ('cubic' runs spline_coefficients first);
    padding is the FLOW sampler's, 'border' or 'zeros' - the image is zero padded in every interpolation.  Not differentiable."""
    size = _chain_resample_args(x, theta, flow, size, interpolation, padding)
    _require_gpu(x, "x")
    if flow is not None:
        _require_gpu(flow, "flow")
    lib = _lib.load()
    B, C, nd, dev = x.shape[0], x.shape[1], x.dim() - 2, x.device
    src = x.detach().to(torch.float32).contiguous()
    if interpolation == "cubic":
        src = spline_coefficients(src)
    th = None if theta is None else _initial_theta(theta, B, nd, dev)
    fl = None if flow is None else flow.detach().to(torch.float32).expand(B, *flow.shape[1:]).contiguous()
    out = torch.empty((B, C) + size, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.trx_affine_then_flow_resample(_lib.ptr(src), src[0].numel(), (ctypes.c_int * 3)(*_dhw(tuple(src.shape[2:]))), _lib.ptr(th), _lib.ptr(fl), nd, B, C,
                                               (ctypes.c_int * 3)(*_dhw(size)), _ORDERS[interpolation], _FLOW_PADDING[padding], _lib.ptr(out),
                                               _lib.current_stream(dev))
    _lib.check(rc, "trx_affine_then_flow_resample")
    return out


def _world_record(world, B, dev):
    """The records [B, 32] (a WorldGeometry or a tensor) as a contiguous fp64 tensor on `dev`."""
    rec = world.record if isinstance(world, WorldGeometry) else torch.as_tensor(world)
    if tuple(rec.shape) != (B, _lib.WORLD_STRIDE):
        raise ValueError(f"expected world-geometry records of shape {(B, _lib.WORLD_STRIDE)}, got {tuple(rec.shape)}")
    return rec.detach().to(device=dev, dtype=torch.float64).contiguous()


def affine_world_theta(theta, world):
    """theta_eff [B, nd, nd+1] fp32 of the UNSCALED theta [B, nd, nd+1] (on the GPU) under world-geometry records (a WorldGeometry or [B, 32]):
    trx_affine_world_theta - the device function of the fused passes, so bit for bit the theta they sample at."""
    _require_gpu(theta, "theta")
    B, nd, dev = theta.shape[0], theta.shape[-1] - 1, theta.device
    rec = _world_record(world, B, dev)
    th = pad_theta(theta.detach().reshape(B, -1), nd)
    out = torch.empty(B, PSTRIDE, device=dev)
    mg = _lib.MovingGrid()
    mg.world = rec.data_ptr()
    with torch.cuda.device(dev):
        rc = _lib.load().trx_affine_world_theta(ctypes.byref(mg), nd, B, _lib.ptr(th), _lib.ptr(out), _lib.current_stream(dev))
    _lib.check(rc, "trx_affine_world_theta")
    return out[:, : nd * (nd + 1)].reshape(B, nd, nd + 1)


def affine_mi_loss_grad(moving, target, theta, rng, bins=32, alpha=1.0, normalized=False, need_grad=True, mask=None, scale=None, overlap=None,
                        moving_mask=None, return_counts=False, world=None):
    """Mutual information of (target, affine warp of moving by theta) and its gradient with respect to theta without a warped volume (extension,
    include/trx.h: trx_affine_mi_loss_grad): moving / target [B,1,*spatial] fp32 on the GPU, theta [B,nd,nd+1], rng [B,4] (mi_range), mask (see
    _mask_u8) or None = every voxel.  Returns (loss [B], dtheta [B,nd,nd+1] or None) - what affine_warp -> mi_loss_grad -> affine_warp_backward
    give, in two passes over the pair.
    moving may live on a lattice of its own (another spatial shape), and scale [nd, nd+1] (grid_scale; None = ones) multiplies theta entry by
    entry in front of the sampler (trx_affine_mi_loss_grad_grids): theta and dtheta are the unscaled ones, the mask and the loop's voxels are
    the target's.  With moving's shape equal to target's and scale None this is the one-lattice entry point, the bits of before.
    overlap / moving_mask (overlap_args): only target voxels whose sample lies inside the moving image - and inside
    moving_mask [B,1,*moving spatial], looked up at the nearest moving voxel - count; the call then goes through the cross-lattice entry point
    whatever the shapes.  return_counts: a third result, the pairs' joint tables uint64-as-int64 [B,K,K] (2^31 units per counted voxel).
    world (a WorldGeometry or records [B, 32]; not with scale): theta_eff = (L Theta R)[:nd] instead, dtheta through the matrix
    chain rule; also the cross-lattice entry point."""
    if mask is not None:
        mask = _mask_u8(mask, target)
    overlap, moving_mask = overlap_args(overlap, moving_mask, moving)
    if world is not None and scale is not None:
        raise ValueError("world replaces scale: give one of them")
    lib = _lib.load()
    two = overlap or scale is not None or world is not None or (isinstance(moving, torch.Tensor) and isinstance(target, torch.Tensor) and moving.shape[2:] != target.shape[2:])
    pair = _GridPair(moving, target, scale) if two else _mi_pair_batch(moving, target)
    B, nd, dev = pair.B, pair.nd, pair.device
    if tuple(rng.shape) != (B, 4):
        raise ValueError(f"expected a range tensor [{B}, 4], got {tuple(rng.shape)}")
    rng = rng.detach().to(device=dev, dtype=torch.float32).contiguous()
    th = pad_theta(theta.detach().to(dev).reshape(B, -1), nd)
    mask = None if mask is None else mask.to(dev)
    moving_mask = None if moving_mask is None else moving_mask.to(dev)
    cfg = _mi_cfg_c(bins, alpha, normalized, rng, mask)
    vol = pair.vol()
    ws_bytes = lib.trx_affine_mi_workspace_bytes(ctypes.byref(vol), cfg.bins)
    if ws_bytes == 0:
        raise _lib.TrxError(f"trx_affine_mi_workspace_bytes rejected {B} x {pair.spatial} with {bins} bins")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    loss = torch.empty(B, device=dev)
    dth = torch.zeros(B, PSTRIDE, device=dev) if need_grad else None
    tail = (_lib.ptr(th), _lib.ptr(loss), _lib.ptr(dth), _lib.ptr(ws), ws_bytes, _lib.current_stream(dev))
    with torch.cuda.device(dev):
        if two:
            rec = None if world is None else _world_record(world, B, dev)
            mg = pair.grid(overlap, moving_mask, rec)
            rc = lib.trx_affine_mi_loss_grad_grids(ctypes.byref(vol), ctypes.byref(mg), ctypes.byref(cfg), *tail)
        else:
            rc = lib.trx_affine_mi_loss_grad(ctypes.byref(vol), ctypes.byref(cfg), *tail)
    _lib.check(rc, "trx_affine_mi_loss_grad_grids" if two else "trx_affine_mi_loss_grad")
    dth = dth[:, : nd * (nd + 1)].reshape(B, nd, nd + 1) if need_grad else None
    if return_counts:
        return loss, dth, ws[: B * cfg.bins * cfg.bins * 8].view(torch.int64).view(B, cfg.bins, cfg.bins).clone()
    return loss, dth


class AffineMISolver(_AffineParams):
    """Batched rigid / affine registration under the Parzen joint-histogram mutual information, the whole loop on the GPU (extension, include/trx.h:
    trx_affine_mi_run): per iteration the warp is fused into the histogram pass and into the gradient pass - no warped volume, no autograd, no
    torch optimiser, no host sync.  The B pairs are independent: each has its own parameters and its own intensity range.

    moving, target: [B,1,*spatial] fp32 on the GPU.  mode, init, optimizer, lr, capacity, betas, eps as for AffineSolver; the state tensors
    (param, theta, losses, best_theta, best_loss, best_idx, step, grad) have AffineSolver's meaning.
    mi: dict(bins=32, alpha=1.0, normalized=False, target_range=None, moving_range=None); a range of None is fitted once, here, to
    (target, moving), the moving side widened to contain 0.
    mask: a region of interest on the target lattice (see _mask_u8), one per pair, or None = every voxel: only voxels inside it enter the
    histogram and the gradient, the target's range is fitted inside it, and the solver keeps the uint8 tensor (`.mask`) alive.
    moving may live on a lattice of its own (another spatial shape), and moving_voxel / target_voxel (both or neither; the tensors' axis order,
    mm) make theta act in millimetres: the loop is trx_affine_mi_run_grids, sampling at theta * scale (grid_scale).  The state (theta, param,
    best_theta) stays the UNSCALED theta; .effective(theta) is what F.affine_grid takes, .world_matrix(theta) the map in mm.  With equal shapes
    and no voxel sizes the solver is the one-lattice one: the same entry point, the same bits.
    overlap / moving_mask (overlap_args): the overlap rule - a target voxel counts only while its sample lies inside the
    moving image (and inside moving_mask [B,1,*moving spatial], kept alive as `.moving_mask`); validity is re-decided in every pass from the
    current theta and is constant under the gradient; the moving range is the image's own (inside the mask), not widened to 0.  The loop is then
    trx_affine_mi_run_grids whatever the shapes.  valid_fraction(theta): the share of counted voxels at a theta.
    moving_affine / target_affine (both or neither, not with voxel sizes; world_geometry describes them) and world_init (None, 'centers', 'moments'
    or a world matrix; world_setup): world geometry, DESIGN.md section 4.17 - theta acts in world millimetres about a centre behind a fixed
    initial transform, whatever the origins and axis directions of the two headers.  `.world` is the WorldGeometry used (T0 = .world.init, c =
    .world.center), `.world_record` its records on the device (kept alive for the loop); world= takes a prepared WorldGeometry instead (the levels
    of a pyramid share one).  .effective(theta) then goes through trx_affine_world_theta and .world_matrix(theta) is T.
    world_init 'principal_axes' / 'search' (world_search: dict of step / keep / iters): T0 is found by world_search - principal-axes
    candidates, with 'search' also a grid of rotations, scored by this criterion and refined rigidly - for a pair whose orientation the headers do not
    give; `.world_search` is its record."""

    def __init__(self, moving, target, mode="affine", mi=None, optimizer="sgd", lr=1e-5, init=None, capacity=1000, betas=(0.9, 0.999), eps=1e-8, mask=None,
                 moving_voxel=None, target_voxel=None, overlap=None, moving_mask=None, moving_affine=None, target_affine=None, world_init=None, world=None,
                 world_search=None):
        if mask is not None:
            mask = _mask_u8(mask, target)
        self.overlap, moving_mask = overlap_args(overlap, moving_mask, moving)
        headers = moving_affine is not None or target_affine is not None
        if world_search is not None and not headers:
            raise ValueError("world_search (the settings of world_init='principal_axes' / 'search') needs moving_affine and target_affine")
        if headers and (moving_affine is None or target_affine is None):
            raise ValueError("moving_affine and target_affine go together: give both voxel-to-world matrices or neither")
        if (headers or world is not None) and (moving_voxel is not None or target_voxel is not None):
            raise ValueError("a voxel-to-world matrix carries the voxel sizes: give moving_affine / target_affine or moving_voxel / target_voxel, not both")
        if world_init is not None and not headers:
            raise ValueError("world_init needs moving_affine and target_affine")
        if headers and world is not None:
            raise ValueError("world is the prepared geometry of moving_affine / target_affine / world_init: give one or the other")
        self.lib = _lib.load()
        if headers:      # (its ValueErrors - and, for 'moments', two launches of trx_image_moments - before the solver allocates anything)
            world = world_setup(moving, target, moving_affine, target_affine, world_init, mask, moving_mask, world_search, self.overlap, mi)
        self.world = world                 # WorldGeometry (host, fp64) or None
        self.world_search = getattr(world, "search", None)      # world_init='principal_axes' / 'search': the WorldSearch behind world.init
        two = self.overlap or world is not None or moving_voxel is not None or target_voxel is not None or (
            isinstance(moving, torch.Tensor) and isinstance(target, torch.Tensor) and moving.shape[2:] != target.shape[2:])
        self.batch = _GridPair(moving, target, None, moving_voxel, target_voxel) if two else _mi_pair_batch(moving, target)
        self.moving_mask = None if moving_mask is None else moving_mask.to(self.batch.device)
        self.world_record = None if world is None else _world_record(world, self.batch.B, self.batch.device)      # kept alive: the grid points to it
        self.grid = self.batch.grid(self.overlap, self.moving_mask, self.world_record) if two else None      # trx_moving_grid, or None: one lattice
        b, nd, dev = self.batch.B, self.batch.nd, self.batch.device
        self.opt = opt_cfg(optimizer, lr, betas, eps)
        self._init_params(b, nd, dev, mode, init, capacity)
        self.mi, self.mi_range, self.mask = _mi_cfg({} if mi is None else mi, self.batch.target, self.batch.moving, mask, self.overlap, self.moving_mask)
        self.vol = self.batch.vol()
        self.ws_bytes = self.lib.trx_affine_mi_workspace_bytes(ctypes.byref(self.vol), self.mi.bins)
        if self.ws_bytes == 0:
            raise _lib.TrxError("trx_affine_mi_workspace_bytes rejected the batch geometry")
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)

    def run(self, iters):
        """Enqueue `iters` iterations on the current stream (no host sync)."""
        iters = _reserve(self, iters)
        with torch.cuda.device(self.batch.device):
            if self.grid is None:
                rc = self.lib.trx_affine_mi_run(ctypes.byref(self.vol), ctypes.byref(self.mi), ctypes.byref(self.opt), ctypes.byref(self.state), iters,
                                                _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(self.batch.device))
            else:
                rc = self.lib.trx_affine_mi_run_grids(ctypes.byref(self.vol), ctypes.byref(self.grid), ctypes.byref(self.mi), ctypes.byref(self.opt),
                                                      ctypes.byref(self.state), iters, _lib.ptr(self.workspace), self.ws_bytes,
                                                      _lib.current_stream(self.batch.device))
        _lib.check(rc, "trx_affine_mi_run" if self.grid is None else "trx_affine_mi_run_grids")

    def valid_fraction(self, theta):
        """[B] fp32: the voxels that enter the criterion at `theta` [B,nd,nd+1] (the UNSCALED theta, like the state) over the target-mask voxels
        (or N) - 1 without the overlap rule.  One extra evaluation of pass 1 whose counts are read back (each counted voxel adds exactly 2^31);
        a pair with an empty target mask has 0."""
        B, nd, dev = self.batch.B, self.nd, self.batch.device
        total = torch.full((B,), float(math.prod(self.batch.spatial)), dtype=torch.float64, device=dev) if self.mask is None else \
            self.mask.reshape(B, -1).sum(1).double()
        if self.grid is None:
            return (total > 0).float()
        th = pad_theta(theta.detach().to(dev).reshape(B, -1), nd)
        loss = torch.empty(B, device=dev)
        with torch.cuda.device(dev):
            rc = self.lib.trx_affine_mi_loss_grad_grids(ctypes.byref(self.vol), ctypes.byref(self.grid), ctypes.byref(self.mi), _lib.ptr(th), _lib.ptr(loss),
                                                        None, _lib.ptr(self.workspace), self.ws_bytes, _lib.current_stream(dev))
        _lib.check(rc, "trx_affine_mi_loss_grad_grids")
        K = self.mi.bins
        units = self.workspace[: B * K * K * 8].view(torch.int64).view(B, -1).sum(1).double()      # (the next run() zeroes the counts itself)
        return (units / 2.0 ** 31 / total.clamp(min=1.0)).float()

    @property
    def scale(self):
        """[nd, nd+1] fp32 on the solver's device: what the kernels multiply theta by (ones on one lattice)."""
        if self.grid is None:
            return torch.ones(self.nd, self.nd + 1, device=self.batch.device)
        return self.batch.scale.to(self.batch.device)

    def effective(self, theta):
        """theta * scale in fp32, as the kernels form it: the theta of F.affine_grid(., target.shape) + F.grid_sample(moving, .).  Under world
        geometry: trx_affine_world_theta, the passes' own device function."""
        if self.world is not None:
            return affine_world_theta(theta.to(device=self.batch.device, dtype=torch.float32).reshape(-1, self.nd, self.nd + 1), self.world_record).to(theta.device)
        return theta.to(torch.float32) * self.scale.to(theta.device)

    def world_matrix(self, theta):
        """[B, nd+1, nd+1] fp64, homogeneous, rows and columns in theta's order (x, y(, z)): moving_mm = M target_mm for the two volumes with
        their centres at the origin, M = [theta[:, :nd] | e_moving * theta[:, nd]].  None without voxel sizes.  Under world geometry:
        T = T0 Tr(c) Theta Tr(-c) between the two world frames (WorldGeometry.matrix), on theta's device."""
        if self.world is not None:
            return self.world.matrix(theta).to(theta.device)
        e_m = getattr(self.batch, "half_extent_moving", None)
        if e_m is None:
            return None
        nd = self.nd
        th = theta.detach().to(torch.float64).reshape(-1, nd, nd + 1)
        M = torch.zeros(th.shape[0], nd + 1, nd + 1, dtype=torch.float64, device=th.device)
        M[:, :nd, :nd] = th[:, :, :nd]
        M[:, :nd, nd] = th[:, :, nd] * e_m.to(th.device)
        M[:, nd, nd] = 1.0
        return M


def local_ncc_loss_grad(target, warped, window=9, alpha=1.0, eps=1e-5, need_grad=True):
    """Local-window NCC (extension, include/trx.h: trx_lncc_loss_grad): target / warped [B,1,*spatial] fp32 on the GPU.
    Returns (loss [B], d loss / d warped (same shape as warped) or None)."""
    lib = _lib.load()
    if not (target.is_cuda and warped.is_cuda):
        raise _lib.TrxError("local_ncc_loss_grad needs CUDA (HIP) tensors: there is no CPU fallback")
    if target.shape != warped.shape or target.dim() not in (4, 5) or target.shape[1] != 1:
        raise ValueError(f"expected two [B,1,*spatial] tensors of equal shape, got {tuple(target.shape)} and {tuple(warped.shape)}")
    nd = target.dim() - 2
    y, w = target.detach().contiguous().float(), warped.detach().contiguous().float()
    B = y.shape[0]
    D, H, W = (1, *y.shape[2:]) if nd == 2 else y.shape[2:]
    loss = torch.empty(B, device=y.device)
    grad = torch.empty_like(w) if need_grad else None
    ws_bytes = lib.trx_lncc_workspace_bytes(nd, B, D, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        rc = lib.trx_lncc_loss_grad(_lib.ptr(y), _lib.ptr(w), nd, B, D, H, W, int(window), float(alpha), float(eps), _lib.ptr(loss),
                                    _lib.ptr(grad), _lib.ptr(ws), ws_bytes, _lib.current_stream(y.device))
    _lib.check(rc, "trx_lncc_loss_grad")
    return loss, grad


def kde_series_center(signals, xis, h):
    """Centre of the value range if the series form of the PDF applies (|s - x| <= h for every pair: include/trx.h), else None.
    One host sync (the reference's get_pdf syncs twice per PDF for its .item() calls anyway, ref:utils.py:40-48)."""
    ends = torch.stack([signals.detach().amin(), signals.detach().amax(), xis.detach().amin(), xis.detach().amax()]).tolist()
    lo, hi = min(ends[0], ends[2]), max(ends[1], ends[3])
    return 0.5 * (lo + hi) if (hi - lo) <= float(h) else None


class KdeSums:
    """The power sums of a fixed set of signals [N,S] (series form about `center`), kept on the device: pdf(xis) for any number of sample
    lines costs one small kernel each instead of a pass over the samples (include/trx.h: trx_kde_pdf_series_cached)."""

    def __init__(self, signals, h, center):
        self.lib = _lib.load()
        sig = signals.detach().contiguous().float()
        self.N, self.S = sig.shape
        self.h, self.center = float(h), float(center)
        dev = sig.device
        ws_bytes = self.lib.trx_kde_series_workspace_bytes(self.N, self.S, 1)
        self.ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        x0 = torch.full((self.N, 1), self.center, device=dev)
        scratch = torch.empty(self.N, 1, device=dev)
        with torch.cuda.device(dev):
            rc = self.lib.trx_kde_pdf_series(_lib.ptr(sig), _lib.ptr(x0), self.N, self.S, 1, self.h, self.center, _lib.ptr(scratch), _lib.ptr(self.ws),
                                             ws_bytes, _lib.current_stream(dev))
        _lib.check(rc, "trx_kde_pdf_series")

    def pdf(self, xis):
        """xis [N, bins] fp32, rows may be strided (a column slice of a wider matrix is read in place)."""
        x = xis.detach()
        if x.dtype != torch.float32 or x.stride(1) != 1:
            x = x.contiguous().float()
        out = torch.empty(self.N, x.shape[1], device=x.device)
        with torch.cuda.device(x.device):
            rc = self.lib.trx_kde_pdf_series_cached(_lib.ptr(self.ws), x.data_ptr(), int(x.stride(0)), self.N, self.S, x.shape[1], self.h, self.center,
                                                    _lib.ptr(out), _lib.current_stream(x.device))
        _lib.check(rc, "trx_kde_pdf_series_cached")
        return out


def kde_pdf(signals, xis, h, center=None):
    """Parzen-window PDF (include/trx.h: trx_kde_pdf / trx_kde_pdf_series): signals [N,S], xis [N,bins] fp32 on the GPU -> pdf [N,bins].
    center: None = one exponential per (sample, bin) pair; a float = the series form about that value (see kde_series_center)."""
    lib = _lib.load()
    if not (signals.is_cuda and xis.is_cuda):
        raise _lib.TrxError("kde_pdf needs CUDA (HIP) tensors: there is no CPU fallback")
    sig, x = signals.detach().contiguous().float(), xis.detach().contiguous().float()
    N, S = sig.shape
    bins = x.shape[1]
    pdf = torch.empty(N, bins, device=sig.device)
    ws_bytes = (lib.trx_kde_workspace_bytes if center is None else lib.trx_kde_series_workspace_bytes)(N, S, bins)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=sig.device)
    with torch.cuda.device(sig.device):
        if center is None:
            rc = lib.trx_kde_pdf(_lib.ptr(sig), _lib.ptr(x), N, S, bins, float(h), _lib.ptr(pdf), _lib.ptr(ws), ws_bytes, _lib.current_stream(sig.device))
        else:
            rc = lib.trx_kde_pdf_series(_lib.ptr(sig), _lib.ptr(x), N, S, bins, float(h), float(center), _lib.ptr(pdf), _lib.ptr(ws), ws_bytes,
                                        _lib.current_stream(sig.device))
    _lib.check(rc, "trx_kde_pdf")
    return pdf


def kde_pdf_backward(signals, xis, grad_pdf, h, center=None):
    lib = _lib.load()
    sig, x, g = signals.detach().contiguous().float(), xis.detach().contiguous().float(), grad_pdf.contiguous().float()
    N, S = sig.shape
    out = torch.empty_like(sig)
    with torch.cuda.device(sig.device):
        if center is None:
            rc = lib.trx_kde_pdf_backward(_lib.ptr(sig), _lib.ptr(x), _lib.ptr(g), N, S, x.shape[1], float(h), _lib.ptr(out), _lib.current_stream(sig.device))
        else:
            ws_bytes = lib.trx_kde_series_workspace_bytes(N, S, x.shape[1])
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=sig.device)
            rc = lib.trx_kde_pdf_series_backward(_lib.ptr(sig), _lib.ptr(x), _lib.ptr(g), N, S, x.shape[1], float(h), float(center), _lib.ptr(out),
                                                 _lib.ptr(ws), ws_bytes, _lib.current_stream(sig.device))
    _lib.check(rc, "trx_kde_pdf_backward")
    return out



def nearest_lattice(spatial, size, device):
    """Source indices of F.interpolate(x[..., *spatial], size=size, mode="nearest") per axis, as int32 device tables.  Taken from
    ATen itself (an index ramp pushed through the same call), so the lattice is exactly the one the torch composition samples."""
    tabs = []
    for n_in, n_out in zip(spatial, size):
        ramp = torch.arange(int(n_in), device=device, dtype=torch.float32).view(1, 1, -1)
        tabs.append(F.interpolate(ramp, size=int(n_out), mode="nearest").view(-1).to(torch.int32).contiguous())
    return tabs


class LatticeWarp:
    """warp(moving, theta) evaluated only on a sub-lattice of the output grid and its theta-backward (include/trx.h:
    trx_affine_warp_lattice[_backward]) - what F.interpolate(get_affine_warp(theta, moving), size, mode="nearest") and the backward of
    that chain compute, without the full-volume warp, the down-sampling and the full-volume gradient."""

    def __init__(self, vol, spatial, size, device):
        """vol: the _lib.Volumes of the (moving, target) batch (single channel; its tensors must outlive this object)."""
        self.vol, self.lib = vol, _lib.load()
        dev = torch.device(device)
        nd, B = int(vol.ndim), int(vol.B)
        self.B = B
        self.size = tuple(int(v) for v in size)
        tabs = nearest_lattice(spatial, self.size, dev)
        zero = torch.zeros(1, dtype=torch.int32, device=dev)
        self.iz, self.iy, self.ix = (tabs if nd == 3 else [zero] + tabs)
        self.nz = self.size[0] if nd == 3 else 1
        self.ny, self.nx = self.size[-2], self.size[-1]
        self.n = self.nz * self.ny * self.nx
        self.ws_bytes = max(int(self.lib.trx_affine_workspace_bytes(ctypes.byref(vol))), B * 1024 * 12 * 4, B * 8192 * 2 * 4)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.dtheta = torch.zeros(B, PSTRIDE, device=dev)

    def forward(self, theta):
        out = torch.empty(self.B, self.n, device=theta.device)
        with torch.cuda.device(theta.device):
            rc = self.lib.trx_affine_warp_lattice(ctypes.byref(self.vol), _lib.ptr(theta), _lib.ptr(self.iz), self.nz, _lib.ptr(self.iy), self.ny,
                                                  _lib.ptr(self.ix), self.nx, _lib.ptr(out), _lib.current_stream(theta.device))
        _lib.check(rc, "trx_affine_warp_lattice")
        return out

    def forward_lines(self, theta, minmax_target, patches, bins):
        """forward() plus the NMI loss's two sample lines (include/trx.h: trx_nmi_lattice_lines): returns (values [B, n], xis
        [B * patches, 2 * bins]); minmax_target [B, 2] = (min, max) of the target's samples."""
        out = torch.empty(self.B, self.n, device=theta.device)
        xis = torch.empty(self.B * patches, 2 * bins, device=theta.device)
        with torch.cuda.device(theta.device):
            rc = self.lib.trx_nmi_lattice_lines(ctypes.byref(self.vol), _lib.ptr(theta), _lib.ptr(self.iz), self.nz, _lib.ptr(self.iy), self.ny,
                                                _lib.ptr(self.ix), self.nx, _lib.ptr(out), _lib.ptr(minmax_target), int(patches), int(bins), _lib.ptr(xis),
                                                None, _lib.ptr(self.ws), self.ws_bytes, _lib.current_stream(theta.device))
        _lib.check(rc, "trx_nmi_lattice_lines")
        return out, xis

    def backward(self, theta, grad_out):
        """grad_out [B, n] (contiguous fp32) -> dL/dtheta [B, PSTRIDE] (a buffer owned by this object, overwritten by the next call)."""
        with torch.cuda.device(theta.device):
            rc = self.lib.trx_affine_warp_lattice_backward(ctypes.byref(self.vol), _lib.ptr(theta), _lib.ptr(self.iz), self.nz, _lib.ptr(self.iy),
                                                           self.ny, _lib.ptr(self.ix), self.nx, _lib.ptr(grad_out), _lib.ptr(self.dtheta),
                                                           _lib.ptr(self.ws), self.ws_bytes, _lib.current_stream(theta.device))
        _lib.check(rc, "trx_affine_warp_lattice_backward")
        return self.dtheta


def nmi_from_pdfs_pooled(h1, pdf_w, pdf_t, alpha):
    """include/trx.h: trx_nmi_from_pdfs_pooled - h1 [N,bins], pdf_w [N,2 bins] (own line | pooled line), pdf_t [N,bins] (target on the pooled
    line), all contiguous fp32 on the GPU.  Returns (loss_terms [N], grad_w [N, 2 bins])."""
    lib = _lib.load()
    N, bins = h1.shape
    terms = torch.empty(N, device=h1.device)
    grad = torch.empty(N, 2 * bins, device=h1.device)
    with torch.cuda.device(h1.device):
        rc = lib.trx_nmi_from_pdfs_pooled(_lib.ptr(h1), _lib.ptr(pdf_w), _lib.ptr(pdf_t), N, bins, float(alpha), None, None, _lib.ptr(terms), _lib.ptr(grad),
                                          _lib.current_stream(h1.device))
    _lib.check(rc, "trx_nmi_from_pdfs_pooled")
    return terms, grad


def nmi_from_pdfs(h1, h2, hj, alpha, need_grad=True):
    """The NMI loss's algebra behind the three PDFs in one kernel (include/trx.h: trx_nmi_from_pdfs): h* [N,bins] fp32 on the GPU.
    Returns (nmi [N], mi [N], loss_terms [N], (g1, g2, gj) = d loss / d h* or None)."""
    lib = _lib.load()
    if not (h1.is_cuda and h2.is_cuda and hj.is_cuda):
        raise _lib.TrxError("nmi_from_pdfs needs CUDA (HIP) tensors: there is no CPU fallback")
    a, b, c = (t.detach().contiguous().float() for t in (h1, h2, hj))
    N, bins = a.shape
    out = torch.empty(3, N, device=a.device)
    grads = torch.empty(3, N, bins, device=a.device) if need_grad else None
    with torch.cuda.device(a.device):
        rc = lib.trx_nmi_from_pdfs(_lib.ptr(a), _lib.ptr(b), _lib.ptr(c), N, bins, float(alpha), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                   _lib.ptr(grads[0]) if need_grad else None, _lib.ptr(grads[1]) if need_grad else None,
                                   _lib.ptr(grads[2]) if need_grad else None, _lib.current_stream(a.device))
    _lib.check(rc, "trx_nmi_from_pdfs")
    return out[0], out[1], out[2], (tuple(grads) if need_grad else None)
