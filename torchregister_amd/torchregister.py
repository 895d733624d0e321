"""`Register` — the public façade, drop-in for ref:src/TorchRegister/torchregister.py:11-129.

Same constructor, `optim` and `__call__` signatures and the same criterion/weight branching
(ref:torchregister.py:70-106).  Extensions are keyword-only and default to reference behaviour:
optimizer ('sgd'|'adam'), honor_criterion, init, smooth_weight, flow_model ('unet' = the reference's
U-Net-generated flow, 'direct' = the flow field itself is the parameter), levels (coarse-to-fine); after `optim`,
`.losses` (the loss curve the reference only plots), `.final_theta` and `.best_idx` are available.
"""
import torch
from torch import cat

from ._engine import _bending_weight, _folding_threshold, _folding_weight, _invert_args, invert_flow, invert_theta, jacobian_determinant, resample_affine_then_flow, transform_points, _mask_u8, _squarings, affine_warp, check_interpolation, grid_scale, overlap_args, resample, world_setup, world_geometry, SEARCH_KEYS
from .gaussian import _factors, _level_sigmas, pyramid_schedule, schedule_shapes
from .pyramid import level_theta, pyramid, pyramid_masks, pyramid_shapes, upsample_flow
from .warpings import (GRIDS_SUPPORT, INITIAL_SUPPORT, MASK_SUPPORT, OVERLAP_SUPPORT, WORLD_SUPPORT, affine_register, device_loop_settings, flow_register, get_affine_warp, resolve_initial, rigid_register,
                       two_lattices)


def _per_level(value, levels, name):
    """One value for every level, or a sequence of `levels` values (coarse to fine)."""
    if isinstance(value, (list, tuple)):
        if len(value) != levels:
            raise ValueError(f"{name}: {len(value)} values for {levels} levels")
        return list(value)
    return [value] * levels


class Register():
    def __init__(self, mode='rigid', device='cpu', criterion=None, weight=None, grad_edges=False, debug=False, *,
                 optimizer='sgd', honor_criterion=False, init=None, smooth_weight=0.0, flow_model='unet', levels=1, spacing=None,
                 bending_weight=0.0, device_loop=False, diffeomorphic=False, squarings=6, folding_weight=0.0, folding_threshold=0.3,
                 shrink=None, smoothing=None, moving_shrink=None, moving_smoothing=None):
        '''
        Numerical registration on an AMD GPU (MI355X) behind the TorchRegister API.

        Parameters
        ----------
        mode : 'rigid', 'affine' or 'flow'. The default is 'rigid'.
        device : kept for signature compatibility; the tensors passed to optim()/__call__ must live on
            the GPU ('cuda'); CPU tensors raise (there is no CPU fallback).
        criterion : list of losses (nn.MSELoss, NCCLoss, SSDLoss are fused; anything else runs through
            the generic autograd path). For rigid/affine the reference ignores a user list:
            reproduced unless honor_criterion=True.
        weight : list of floats associated with criterion.
        grad_edges : must stay False (the reference's edge filter crashes when enabled).
        debug : print a one-line summary after optim (one per level with levels > 1).
        levels : (keyword-only extension) coarse-to-fine registration over a pyramid of this many levels (pyramid_shapes: each level
            halves every axis that stays >= 8 voxels).  Rigid / affine hand the final parameters of a level to the next unchanged (theta is
            in normalised coordinates); flow_model='direct' hands its final flow up through upsample_flow.  1 = single resolution.
        flow_model : (keyword-only extension) 'unet', 'direct' or 'bspline' - a cubic B-spline free-form deformation whose control lattice has
            `spacing` voxels between control points (an int or one per axis, default 8).  After optim, `.control` is the final control tensor
            (the finest level's).  With levels > 1 the spacing in voxels is the same at every level, every level starts from a zero control
            tensor and adds to base = upsample_flow(the previous level's final dense flow): multi-level FFD as a sum of levels.
        bending_weight : (keyword-only extension, flow_model='bspline' only) lambda >= 0: lambda * (bending energy of the control lattice,
            bspline_bending) joins each pair's loss; `.losses` and the early stop see the total.  With levels > 1 the same lambda applies to
            each level's own lattice: the energy is per voxel of that level, in that level's voxel coordinates, nothing is rescaled between
            levels, and the base handed up from the coarser levels is not penalised.
        diffeomorphic, squarings : (keyword-only extension, mode='flow' with flow_model='bspline' and the fused criteria only; ValueError otherwise,
            and with MILoss, here) True: the lattice parameterises a stationary VELOCITY field and the deformation is its exponential by `squarings`
            (0 .. 12, default 6) steps of scaling and squaring (svf_exp; trx_bspline_svf_run) - free of folds up to the discretisation, and
            invertible.  After optim: `.theta` is the flow of the last forward as always, `.velocity` its velocity, `.control` the lattice,
            `.inverse_flow` = exp(-velocity), and `.inverse(x)` warps x with it.  With levels > 1 the hand-over passes the VELOCITY: a level's base
            is upsample_flow(the previous level's final velocity), its velocity is base + expand(control), and the exponential is taken of the
            sum; bending_weight acts on each level's own lattice as without diffeomorphic.
        folding_weight, folding_threshold : (keyword-only extension, flow_model='bspline' only, not with diffeomorphic=True; ValueError otherwise, here)
            w >= 0 and eps: w * folding_penalty(flow, eps) = w * mean_x max(0, eps - det(x))^2 joins each pair's loss, det being the Jacobian
            determinant map of the level's TOTAL flow (jacobian_determinant: finite differences at voxel centres).  It keeps the deformation from
            folding where bending_weight only penalises curvature, on every route of the B-spline loop - fused criteria, MILoss, initial=, mask=,
            overlap=.  `.losses` hold the total.  With levels > 1 the same weight applies at every level, each on its own lattice and on the sum
            base + expand(control) handed up so far.  The default eps = 0.3 is a margin for what lies between the voxel centres.  After optim,
            `.jacobian()` is the map of `.theta`.  With initial= the whole transform's local volume change is that map times the constant
            determinant of the affine.
        device_loop : (keyword-only extension, mode='rigid' / 'affine') True: criterion must be exactly [MILoss] with a non-zero weight (ValueError
            otherwise, here) and optim runs the whole loop on the device (trx_affine_mi_run: the warp fused into the histogram and gradient passes
            of the mutual information, no host sync per iteration); honor_criterion is implied, a batch is B independent pairs, and with levels > 1
            each level fits its intensity ranges to that level's images.  False (default): every route as before.
        shrink, smoothing, moving_shrink, moving_smoothing : (keyword-only extension, levels > 1 only) the pyramid's schedule.
            All None (default): today's pyramid - every axis halved per level behind a fixed [1,4,6,4,1]/16 blur.  shrink=[...]: `levels` tuples of
            per-axis integer factors, coarsest first, the finest all ones - level k has shape ceil(S / f_k) and is the full-resolution image behind
            a Gaussian of smoothing[k] (voxels of the full image, per axis; None: f / 2 where f > 1, elastix's default) sampled at that size
            (pyramid(x, levels, shrink=, sigma=)).  The schedule is the target's and also the moving image's unless moving_shrink /
            moving_smoothing give that one its own - possible where the two images may lie on lattices of their own (mode 'rigid' / 'affine' with
            device_loop=True; the B-spline mutual-information loop, there with optim(initial=...)), ValueError elsewhere.  shrink='voxel': each image
            gets pyramid_schedule of its own shape and its own voxel sizes (optim's moving_voxel / target_voxel, or the column norms of
            moving_affine / target_affine - of a batch of matrices, their mean), so that an anisotropic CT is not shrunk along its thick slices
            while an isotropic MR is; optim raises ValueError without voxel sizes for both images.  Masks follow their image's schedule.  After
            optim, .level_schedule = ((shrink, sigma) of the target, (shrink, sigma) of the moving image), None without a schedule.
        '''
        if mode not in ('rigid', 'affine', 'flow'):
            raise ValueError("mode must be 'rigid', 'affine' or 'flow'")
        if device_loop:
            if mode == 'flow':
                raise ValueError("device_loop is the fused mutual-information loop of mode='rigid' / 'affine' (mode='flow' with MILoss alone already runs on the device)")
            device_loop_settings(criterion, weight)     # raises unless the list is exactly [MILoss] with a non-zero weight
        if not isinstance(levels, int) or isinstance(levels, bool) or levels < 1:
            raise ValueError(f"levels must be an int >= 1, got {levels!r}")
        self._init_schedule(mode, criterion, weight, flow_model, levels, device_loop, diffeomorphic, shrink, smoothing, moving_shrink, moving_smoothing)
        if levels > 1 and mode == 'flow' and flow_model not in ('direct', 'bspline'):
            raise ValueError("levels > 1 needs flow_model='direct': the U-Net is built for one image size")
        if spacing is not None and not (mode == 'flow' and flow_model == 'bspline'):
            raise ValueError("spacing is the control-point spacing of mode='flow' with flow_model='bspline'")
        if mode == 'flow' and flow_model == 'bspline':
            each = [] if spacing is None else list(spacing) if isinstance(spacing, (list, tuple)) else [spacing]
            if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in each) or len(each) > 3:
                raise ValueError(f"spacing must be an int >= 1 or one per axis, got {spacing!r}")
            if smooth_weight != 0:
                raise ValueError("flow_model='bspline' takes no smooth_weight: its regularisers are the control-point spacing and bending_weight")
        bending_weight = _bending_weight(bending_weight)
        if bending_weight != 0 and not (mode == 'flow' and flow_model == 'bspline'):
            raise ValueError("bending_weight is the bending-energy penalty of mode='flow' with flow_model='bspline'")
        folding_weight, folding_threshold = _folding_weight(folding_weight), _folding_threshold(folding_threshold)
        if folding_weight != 0 and not (mode == 'flow' and flow_model == 'bspline'):
            raise ValueError("folding_weight is the folding penalty of mode='flow' with flow_model='bspline' (autograd users have folding_penalty)")
        if folding_weight != 0 and diffeomorphic:
            raise ValueError("folding_weight is not taken with diffeomorphic=True: the exponential of a velocity field does not fold")
        self.folding_weight, self.folding_threshold = folding_weight, folding_threshold
        squarings = _squarings(squarings)
        if diffeomorphic:
            if not (mode == 'flow' and flow_model == 'bspline'):
                raise ValueError("diffeomorphic=True is the velocity-field form of mode='flow' with flow_model='bspline'")
            from .utils import MILoss
            if any(isinstance(c, MILoss) for c in (criterion or [])):
                raise ValueError("diffeomorphic=True runs the fused criteria only (nn.MSELoss, NCCLoss, SSDLoss): mutual information on a velocity field is not built")
            from .utils import NGFLoss
            if any(isinstance(c, NGFLoss) for c in (criterion or [])):
                raise ValueError("diffeomorphic=True runs the fused criteria only (nn.MSELoss, NCCLoss, SSDLoss): the normalised gradient field on a velocity field is not built")
        self.diffeomorphic, self.squarings = bool(diffeomorphic), squarings
        self.velocity = self.inverse_flow = None
        self._inverse_warp = None
        self.criterion = criterion
        self.weight = weight
        self.mode = mode
        self.warp = None if mode == 'flow' else get_affine_warp
        self.device = device
        self.debug = debug
        self.theta = None
        self.grad_edges = grad_edges
        self.optimizer = optimizer
        self.honor_criterion = honor_criterion
        self.init = init
        self.smooth_weight = smooth_weight
        self.flow_model = flow_model
        self.spacing = spacing
        self.bending_weight = bending_weight
        self.levels = levels
        self.device_loop = bool(device_loop)
        self.control = None
        self.losses = None
        self.final_theta = None
        self.best_idx = None
        self.final_pose = None      # mode='rigid' on the device paths: the pose [B,6] (3-D) / [B,3] (2-D) behind final_theta
        self.level_losses = None
        self.level_shapes = None
        self.level_schedule = None  # levels > 1 with shrink=...: ((shrink, sigma) of the target, (shrink, sigma) of the moving image), coarsest first
        self.world_matrix = None    # device_loop with voxel sizes: [B,nd+1,nd+1], the best theta as moving_mm = M target_mm (rows / columns x, y(, z))
        self.world_init = None      # optim(moving_affine=, target_affine=): T0 [B,nd+1,nd+1] fp64, the fixed world transform in front of what was optimised
        self.world_search = None    # optim(world_init='principal_axes' / 'search'): the WorldSearch record behind world_init (candidates, scores, kept, refined, chosen, eigenvalues)
        self.world_center = None    # ... and c [B,nd] fp64, the centre (world mm) theta acted about; world_matrix is then T0 Tr(c) Theta Tr(-c)
        self.target_shape = None    # the spatial shape of the lattice optim registered onto: what reg(x) returns
        self.moving_shape = None    # the spatial shape of the moving image optim ran on (the finest level's): what to_moving(x) returns
        self.initial = None         # optim(initial=...): the effective theta [B,nd,nd+1] the deformation is composed with
        self.valid_fraction = None  # optim(overlap=True / moving_mask=...): [B], N_valid / (target-mask voxels or N) at the returned transform

    def _init_schedule(self, mode, criterion, weight, flow_model, levels, device_loop, diffeomorphic, shrink, smoothing, moving_shrink, moving_smoothing):
        '''The schedule keywords of __init__: their ValueErrors (what does not need the images' number of axes), and the values as given.'''
        self.shrink, self.smoothing, self.moving_shrink, self.moving_smoothing = shrink, smoothing, moving_shrink, moving_smoothing
        rest = (smoothing, moving_shrink, moving_smoothing)
        if shrink is None and all(v is None for v in rest):
            return
        if levels == 1:
            raise ValueError("shrink / smoothing / moving_shrink / moving_smoothing describe the levels of a pyramid: they need levels > 1")
        if shrink is None:
            raise ValueError("smoothing, moving_shrink and moving_smoothing go with shrink=[...]: without it the pyramid halves every axis behind its fixed blur")
        if isinstance(shrink, str):
            if shrink != 'voxel' or any(v is not None for v in rest):
                raise ValueError(f"shrink is a list of per-level factors or 'voxel' (which takes no smoothing / moving_shrink / moving_smoothing: "
                                 f"each image's schedule comes from its own voxel sizes), got {shrink!r}")
            return
        fs = _factors(shrink, None, levels, 'shrink')
        _level_sigmas(smoothing, fs, None, levels, 'smoothing')
        if moving_shrink is None and moving_smoothing is None:
            return
        mfs = fs if moving_shrink is None else _factors(moving_shrink, None, levels, 'moving_shrink')
        _level_sigmas(moving_smoothing, mfs, None, levels, 'moving_smoothing')
        if mode == 'flow':
            from .utils import MILoss, NGFLoss
            alone = criterion is not None and weight is not None and len(criterion) == 1 and isinstance(criterion[0], (MILoss, NGFLoss))
            own = flow_model == 'bspline' and alone and not diffeomorphic       # (the loop that takes optim(initial=...))
        else:
            own = bool(device_loop)
        if not own:
            raise ValueError("moving_shrink / moving_smoothing give the moving image levels of its own shape: that needs a loop in which the two images may "
                             "lie on lattices of their own - mode 'rigid' / 'affine' with device_loop=True, or the B-spline mutual-information loop with "
                             "optim(initial=...); everywhere else both images share one lattice and one schedule")

    def _schedules(self, moving, target, moving_voxel, target_voxel, moving_affine, target_affine, initial):
        '''None without a schedule, else ((shrink, sigma) of the target, (shrink, sigma) of the moving image) for these images: host arithmetic only.'''
        if self.shrink is None or self.levels == 1:
            return None
        L, nd, ndm = self.levels, target.dim() - 2, moving.dim() - 2
        if isinstance(self.shrink, str):
            if moving_affine is not None and target_affine is not None:      # columns in the tensor's axis order: their norms are the voxel sizes
                world_geometry(moving.shape[2:], target.shape[2:], moving_affine, target_affine)      # (a malformed header: its ValueError, here)
                norms = lambda A, n: torch.as_tensor(A, dtype=torch.float64).cpu().reshape(-1, n + 1, n + 1)[:, :n, :n].norm(dim=1).mean(0).tolist()  # noqa: E731
                moving_voxel, target_voxel = norms(moving_affine, ndm), norms(target_affine, nd)
            if moving_voxel is None or target_voxel is None:
                raise ValueError("shrink='voxel' derives each image's schedule from its voxel sizes: give moving_voxel= and target_voxel=, or "
                                 "moving_affine= and target_affine=")
            return pyramid_schedule(target.shape[2:], L, target_voxel), pyramid_schedule(moving.shape[2:], L, moving_voxel)
        fs = _factors(self.shrink, nd, L, 'shrink')
        tsched = (fs, _level_sigmas(self.smoothing, fs, nd, L, 'smoothing'))
        if self.moving_shrink is None and self.moving_smoothing is None:
            return tsched, tsched
        if self.mode == 'flow' and initial is None:
            raise ValueError("moving_shrink / moving_smoothing need optim(initial=...) in mode='flow': without it both images share one lattice and one schedule")
        mfs = fs if self.moving_shrink is None else _factors(self.moving_shrink, ndm, L, 'moving_shrink')
        return tsched, (mfs, _level_sigmas(self.moving_smoothing, mfs, ndm, L, 'moving_smoothing'))

    def _flow_kw(self, n, lr, max_epochs):
        kw = dict(mode='bilinear', n=n, lr=lr, max_epochs=max_epochs, optimizer=self.optimizer, smooth_weight=self.smooth_weight,
                  flow_model=self.flow_model)
        if self.flow_model == 'bspline':
            kw.update(spacing=self.spacing, bending_weight=self.bending_weight, diffeomorphic=self.diffeomorphic, squarings=self.squarings,
                      folding_weight=self.folding_weight, folding_threshold=self.folding_threshold)
        if self.criterion is not None and self.weight is not None:           # ref:torchregister.py:71-73
            kw.update(criterions=self.criterion, weights=self.weight)
        elif self.weight is not None:                                         # ref:torchregister.py:74-76
            kw.update(weights=self.weight)
        return kw

    def _ngf_alone(self):
        '''Whether optim runs the normalised-gradient-field B-spline loop (trx_bspline_ngf_run): mode 'flow', flow_model 'bspline', NGFLoss alone.'''
        from .utils import NGFLoss
        alone = self.criterion is not None and self.weight is not None and len(self.criterion) == 1 and isinstance(self.criterion[0], NGFLoss)
        return self.mode == 'flow' and self.flow_model == 'bspline' and alone and not self.diffeomorphic

    def _level_criteria(self, full_shape, level_shape):
        '''The criterion list of a pyramid level: an NGFLoss with voxel sizes gets a copy whose voxel is the level's, v S / S_l per axis (a level keeps
        the image's field of view), so that its differences stay in millimetres on every level; everything else is passed as it is.'''
        from .utils import NGFLoss
        out = []
        for c in self.criterion:
            if isinstance(c, NGFLoss) and c.voxel is not None and len(c.voxel) == len(level_shape):
                voxel = tuple(v * s / sl for v, s, sl in zip(c.voxel, full_shape, level_shape))
                c = NGFLoss(eta=c.eta, alpha=c.alpha, voxel=voxel, target_eps=c.target_eps, moving_eps=c.moving_eps)
            out.append(c)
        return out

    def _check_mask(self, mask, target):
        '''mask=... of optim: ValueError unless the loop is one of the device-side mutual-information loops; the uint8 mask [B,1,*spatial].'''
        if self.mode == 'flow':
            from .utils import MILoss
            alone = self.criterion is not None and self.weight is not None and len(self.criterion) == 1 and isinstance(self.criterion[0], MILoss)
            ok = alone and not self.diffeomorphic and (self.flow_model == 'bspline' or (self.flow_model == 'direct' and target.dim() == 5))
            ok = ok or self._ngf_alone()
        else:
            ok = self.device_loop
        if not ok:
            raise ValueError(MASK_SUPPORT)
        return _mask_u8(mask, target)

    def _check_grids(self, moving, target, moving_voxel, target_voxel):
        '''Differing spatial shapes / voxel sizes of optim: ValueError unless the loop is the fused mutual-information loop of mode 'rigid' /
        'affine' (device_loop=True), before any device work.  Returns whether the pair takes the cross-lattice path.'''
        if not two_lattices(moving, target, moving_voxel, target_voxel):
            return False
        if self.mode == 'flow' or not self.device_loop or moving.dim() != target.dim():
            raise ValueError(GRIDS_SUPPORT)
        grid_scale(moving.shape[2:], target.shape[2:], moving_voxel, target_voxel)      # exactly one voxel size, a non-positive one: ValueError
        return True

    def _check_initial(self, initial, moving, target, moving_voxel, target_voxel):
        '''initial=... of optim: ValueError unless the loop is the B-spline mutual-information loop or the B-spline normalised-gradient-field loop
        (mode 'flow', flow_model 'bspline', MILoss or NGFLoss alone - trx_bspline_mi_run_grids / trx_bspline_ngf_run -, not diffeomorphic, no voxel sizes), before any device work.  Returns the effective theta [B,nd,nd+1].'''
        from .utils import MILoss, NGFLoss
        alone = self.criterion is not None and self.weight is not None and len(self.criterion) == 1 and isinstance(self.criterion[0], (MILoss, NGFLoss))
        if not (self.mode == 'flow' and self.flow_model == 'bspline' and alone and not self.diffeomorphic) or moving_voxel is not None or target_voxel is not None:
            raise ValueError(INITIAL_SUPPORT)
        return resolve_initial(initial, moving, target)

    def _check_overlap(self, overlap, moving_mask, moving, initial):
        '''overlap=... / moving_mask=... of optim: ValueError unless the loop is the fused rigid / affine mutual-information loop (device_loop=True) or
        the B-spline mutual-information loop composed with initial=, before any device work.  Returns (on, the uint8 moving mask or None).'''
        if not overlap and moving_mask is None:
            return False, None
        if self.mode == 'flow':
            from .utils import MILoss
            alone = self.criterion is not None and self.weight is not None and len(self.criterion) == 1 and isinstance(self.criterion[0], MILoss)
            ok = alone and self.flow_model == 'bspline' and not self.diffeomorphic and initial is not None
        else:
            ok = self.device_loop
        if not ok:
            raise ValueError(OVERLAP_SUPPORT)
        return overlap_args(overlap, moving_mask, moving)

    def _check_world(self, moving, target, moving_affine, target_affine, world_init, moving_voxel, target_voxel, mask, moving_mask, overlap=False,
                     world_search=None, sched=None):
        '''moving_affine=... / target_affine=... / world_init=... of optim: ValueError unless the loop is the fused mutual-information loop of mode
        'rigid' / 'affine' (device_loop=True) - GRIDS_SUPPORT's rule - and for every malformed header, before any device work (world_init='moments'
        then runs trx_image_moments on each image).  Returns the WorldGeometry, made once from the full-resolution headers, or None.'''
        if moving_affine is None and target_affine is None and world_init is None and world_search is None:
            return None
        if self.mode == 'flow' or not self.device_loop or moving.dim() != target.dim():
            raise ValueError(WORLD_SUPPORT)
        if moving_affine is None or target_affine is None:
            raise ValueError("moving_affine and target_affine go together: give both voxel-to-world matrices or neither")
        if moving_voxel is not None or target_voxel is not None:
            raise ValueError("a voxel-to-world matrix carries the voxel sizes: give moving_affine / target_affine or moving_voxel / target_voxel, not both")
        if not (isinstance(world_init, str) and world_init in ('principal_axes', 'search')):
            return world_setup(moving, target, moving_affine, target_affine, world_init, mask, moving_mask, world_search)
        # the candidates are scored and refined on the first level the run will use, with the run's own criterion settings
        mi = device_loop_settings(self.criterion, self.weight)
        world_geometry(moving.shape[2:], target.shape[2:], moving_affine, target_affine)      # (the headers' ValueErrors, before the pyramid touches the device)
        if world_search is not None and (not isinstance(world_search, dict) or set(world_search) - set(SEARCH_KEYS)):
            raise ValueError(f"world_search is a dict of {SEARCH_KEYS}, got {world_search!r}")
        on = None
        if self.levels > 1:
            L = self.levels
            tk, mk = ({}, {}) if sched is None else (dict(shrink=s[0], sigma=s[1]) for s in sched)      # the run's own coarsest level
            on = (pyramid(moving, L, **mk)[0], pyramid(target, L, **tk)[0], None if mask is None else pyramid_masks(mask, L, **tk)[0],
                  None if moving_mask is None else pyramid_masks(moving_mask.to(moving.device), L, **mk)[0])
        return world_setup(moving, target, moving_affine, target_affine, world_init, mask, moving_mask, world_search, overlap, mi, on)

    def _set_grids(self, grids, target, info):
        '''After a rigid / affine optim: the warp behind __call__ (two lattices: onto the target lattice, forward only) and the new attributes.'''
        self.target_shape = tuple(target.shape[2:])
        self.world_matrix = info.get('world_matrix')
        self.world_init, self.world_center = info.get('world_init'), info.get('world_center')
        self.world_search = info.get('world_search')
        size = self.target_shape
        self.warp = (lambda theta, x: affine_warp(theta, x, size=size)) if grids else get_affine_warp

    def optim(self, moving, target, lr=1E-5, max_epochs=1000, n=32, per=0.1, *, mask=None, moving_voxel=None, target_voxel=None, initial=None,
              overlap=None, moving_mask=None, moving_affine=None, target_affine=None, world_init=None, world_search=None):
        '''
        Optimisation loop: moving, target [1,1,x,y(,z)] float32 GPU tensors (a leading batch > 1 of
        independent pairs is an extension).  Sets self.theta (best theta [B,nd,nd+1], or the flow
        [B,nd,...] of the last forward in flow mode) and self.warp.  Returns None.
        With levels > 1, lr and max_epochs may each be one value for every level or a sequence of `levels` values, coarse to fine.
        A level with max_epochs 0 runs no iteration and hands its starting parameters to the next level unchanged (its entry in
        .level_losses is empty).
        mask : (keyword-only extension) a region of interest on the TARGET lattice, one per pair: bool / uint8 / numeric, [B,1,*spatial] or
            [B,*spatial], non-zero = the voxel counts.  Only those voxels enter the mutual information (histogram, normalisation, gradient) and
            the fitted target range - a couch, a coil or a lesion the moving image lacks is left out.  Supported where the loop is one of the
            device-side mutual-information loops: mode 'rigid' / 'affine' with device_loop=True, or mode 'flow' with flow_model 'direct' (3-D) or
            'bspline' and MILoss alone, or with 'bspline' and NGFLoss alone; ValueError anywhere else, before any device work.  With levels > 1 a level's mask is the float mask sent
            through the pyramid call of the target and thresholded at >= 0.5; a pair whose mask is empty at some level raises ValueError.
        moving_voxel, target_voxel : (keyword-only extension) voxel sizes in mm, in the tensors' axis order (dz, dy, dx) / (dy, dx), both or
            neither.  With them theta acts between the two volumes in millimetres (their centres coinciding, their axes aligned): mode='rigid' is
            rigid in the world whatever the voxel sizes.  moving may also have a spatial shape of its own - a CT and an MR on their own grids.
            Honoured by mode 'rigid' / 'affine' with device_loop=True; ValueError anywhere else, before any device work.  Then .theta /
            .final_theta are the EFFECTIVE thetas - F.grid_sample(moving, F.affine_grid(reg.theta, target.shape), align_corners=False) is
            reg(moving) -, reg(x) warps any [B,c,*moving spatial] onto the target lattice, .world_matrix is the best theta in mm (None without
            voxel sizes), .target_shape the lattice, .final_pose keeps its meaning and mask= stays on the target lattice.  With levels > 1 each
            image gets its own pyramid, so both fields of view and the scale are the same at every level; .level_shapes are the target's.
        initial : (keyword-only extension, mode 'flow' with flow_model='bspline' and MILoss or NGFLoss alone; ValueError anywhere else, before any device work)
            the result of the rigid / affine stage before - an effective theta [B,nd,nd+1], or a Register of mode 'rigid' / 'affine' that has run
            onto this target lattice (its .theta is used).  The deformation is composed with it and the ORIGINAL moving image, on its own lattice,
            is sampled once (affine_flow_warp; the loop runs in trx_bspline_mi_run_grids) - no resampling in between, nothing lost outside the
            target's field of view.  .theta / .final_theta / .control keep their meaning (the flow on the target lattice, in target voxels),
            reg(x) warps any [B,c,*moving spatial] onto the target lattice by one composed interpolation, .initial holds the theta used.  With
            levels > 1 moving and target get their own pyramids (align_corners=True, as flow mode does) and a level runs with
            pyramid.level_theta of the theta; .level_shapes are the target's.
        overlap, moving_mask : (keyword-only extension) overlap=True: the mutual information is taken over the overlap only - a target voxel counts
            while its sample lies inside the moving image (all corners of the interpolation in the volume), so the zero padding outside the moving
            field of view never forms an intensity class of its own (elastix / ITK / NiftyReg behaviour; partial overlap is the normal case for
            volumes on their own grids).  moving_mask: a mask on the MOVING lattice, [B,1,*moving spatial] or [B,*moving spatial], non-zero = the
            moving voxel counts, looked up at the sample's nearest voxel; it implies overlap (with an explicit overlap=False: ValueError).  The
            moving range is then the image's own min / max (inside the mask), not widened to 0; validity is re-decided in every iteration and is
            constant under the gradient.  Supported by mode 'rigid' / 'affine' with device_loop=True (one or two lattices, with or without voxel
            sizes) and by mode 'flow' with flow_model='bspline', MILoss alone and initial=; ValueError anywhere else, before any device work.
            Afterwards .valid_fraction [B] is N_valid / (target-mask voxels or N) at the returned transform (one extra evaluation; nothing is read
            back inside the loop) - there is no minimum-overlap guard: a pair that lost all overlap has loss 0, check the fraction.  With levels > 1
            the moving mask goes through pyramid_masks over the moving pyramid and every level fits its own ranges.
        moving_affine, target_affine, world_init : (keyword-only extension) the images' voxel-to-world matrices, [nd+1,nd+1]
            for every pair or [B,nd+1,nd+1]: columns in the tensor's axis order (nibabel's img.affine for get_fdata() put into [B,1,*shape]), rows
            world x, y(, z) in mm.  Both or neither, not together with voxel sizes (they carry them).  The transform is optimised in world
            millimetres about a centre c, behind a fixed world transform T0 chosen by world_init: None - trust the headers, T0 = I, c = the target's
            geometric centre; 'centers' - T0 takes the target's geometric centre to the moving image's; 'moments' - T0 is the translation between the
            intensity centres of mass (inside mask / moving_mask where given), c = the target's centre of mass; or a world matrix from anywhere
            ([nd+1,nd+1] / [B,nd+1,nd+1], p_moving = T0 p_target).  Honoured where voxel sizes are: mode 'rigid' / 'affine' with device_loop=True;
            ValueError anywhere else and for a malformed header, before any device work.  Works with mask=, overlap=, moving_mask= and levels=
            (the geometry is made once from the full-resolution headers and shared by the levels).  Afterwards .theta / .final_theta are EFFECTIVE
            thetas as with voxel sizes, .world_matrix [B,nd+1,nd+1] fp64 is T = T0 Tr(c) Theta Tr(-c) at the best theta (p_moving = T p_target),
            .world_init and .world_center are T0 and c, .final_pose keeps its meaning; ffd.optim(moving, target, initial=reg) and
            reg(x, interpolation=) work as before - they only ever see the effective theta.
            world_init='principal_axes' / 'search'  are for a pair whose orientation cannot be trusted - prone against supine, a
            specimen placed differently, a wrong header: 'principal_axes' takes the four (2-D: two) proper rotations that align the principal axes of the
            two intensity distributions (second moments inside mask / moving_mask, about the centres of mass), 'search' adds the centre-of-mass
            alignment composed with a regular grid of rotations; every candidate is scored by the mutual information of this run's criterion, the best
            few are refined by a short rigid loop, and T0 is the winner, c the target's centre of mass.  Scoring and refinement run on the coarsest level
            of `levels`.  world_search : dict of step (degrees of the grid, a divisor of 90; 45), keep (candidates refined; 8) and iters (iterations of the
            refinement; 30).  .world_search holds the record (candidates, scores, kept, refined, chosen, eigenvalues - near-equal eigenvalues mean the
            principal axes carried no information).  Always rigid, whatever the mode.
        '''
        self.valid_fraction = None
        overlap, moving_mask = self._check_overlap(overlap, moving_mask, moving, initial)
        self.moving_shape = tuple(moving.shape[2:])
        headers = moving_affine is not None or target_affine is not None or world_init is not None or world_search is not None
        if initial is not None:
            if headers:
                raise ValueError(WORLD_SUPPORT)
            initial, grids = self._check_initial(initial, moving, target, moving_voxel, target_voxel), False
        elif headers and (self.mode == 'flow' or not self.device_loop):
            raise ValueError(WORLD_SUPPORT)
        else:
            grids = self._check_grids(moving, target, moving_voxel, target_voxel) or headers
        self.initial = initial
        if mask is not None:
            mask = self._check_mask(mask, target)
        sched = self._schedules(moving, target, moving_voxel, target_voxel, moving_affine, target_affine, initial)
        world = self._check_world(moving, target, moving_affine, target_affine, world_init, moving_voxel, target_voxel, mask, moving_mask, overlap,
                                  world_search, sched) if headers else None
        if self.levels > 1:
            return self._optim_levels(moving, target, lr, max_epochs, n, per, mask, moving_voxel, target_voxel, initial, overlap, moving_mask, world,
                                      sched)
        okw = dict(overlap=True, moving_mask=moving_mask) if overlap else {}
        if self.mode == 'flow':
            flowreg = flow_register(target.shape[2:], **self._flow_kw(n, lr, max_epochs)).to(moving.device)
            flowreg.optimize(moving, target, self.device, self.debug, mask=mask, initial=initial, **okw)
            self.valid_fraction = flowreg.valid_fraction
            if initial is not None:
                self.target_shape = tuple(target.shape[2:])
            self.theta = flowreg.flow
            self.warp = flowreg.deform
            self.losses = flowreg.losses
            self.final_theta = flowreg.final_flow
            self.control = flowreg.control
            self.velocity, self.inverse_flow, self._inverse_warp = flowreg.velocity, flowreg.inverse_flow, flowreg.inverse
            return

        fn = affine_register if self.mode == 'affine' else rigid_register
        info = {}
        kw = dict(lr=lr, epochs=max_epochs, per=per, device=self.device, debug=self.debug, grad_edges=self.grad_edges,
                  honor_criterion=self.honor_criterion, optimizer=self.optimizer, init=self.init, info=info, device_loop=self.device_loop)
        if self.criterion is not None and self.weight is not None:           # ref:torchregister.py:85-87,97-99
            kw.update(criterions=self.criterion, weights=self.weight)
        elif self.weight is not None:                                         # ref:torchregister.py:88-90,100-102
            kw.update(weights=self.weight)
        if mask is not None:
            kw.update(mask=mask)
        if world is not None:
            kw.update(world=world)
        elif grids:
            kw.update(moving_voxel=moving_voxel, target_voxel=target_voxel)
        _, theta = fn(moving, target, **kw, **okw)
        self.valid_fraction = info.get('valid_fraction')
        self.theta = theta[-1]                                                # best theta (Q8)
        self.final_theta = theta[0]
        self.losses = info.get('losses')
        self.best_idx = info.get('best_idx')
        self.final_pose = info.get('final_pose')
        self._set_grids(grids, target, info)

    def _optim_levels(self, moving, target, lr, max_epochs, n, per, mask=None, moving_voxel=None, target_voxel=None, initial=None, overlap=False,
                      moving_mask=None, world=None, sched=None):
        '''Coarse-to-fine: the single-level machinery (flow_register / _affine_family) on each level of pyramid(moving) and
        pyramid(target), coarsest first; each level starts from the previous level's FINAL parameters (rigid: the pose, drawn by
        torch.rand for the coarsest level as a single-level run draws it; affine: theta; flow: upsample_flow of the flow).  Optimiser
        state starts fresh at every level.  .theta / .warp / .losses / .best_idx / .final_theta are the finest level's.
        Two lattices (rigid / affine, device_loop): moving and target each get their own pyramid, so a level halves both lattices and doubles both
        voxel sizes - the half extents, and with them the scale, are the same at every level; the theta handed up is the unscaled one.
        initial (flow, B-spline mutual information): moving and target get their own pyramids (align_corners=True) and level k runs with
        level_theta(initial, ...), the theta between the two level lattices; the flow is handed up by upsample_flow as without it.
        sched (shrink=...): the levels come from pyramid(x, L, shrink=, sigma=) with each image's own schedule and have the shapes ceil(S / f); nothing
        else changes - theta does not depend on the level, a level's voxel is v S / S_l per axis, level_theta and upsample_flow take any shapes.'''
        grids = world is not None or two_lattices(moving, target, moving_voxel, target_voxel)      # (refused by optim unless the loop is the fused mutual-information one)
        L = self.levels
        lrs, epochs = _per_level(lr, L, 'lr'), _per_level(max_epochs, L, 'max_epochs')
        tk, mk = ({}, {}) if sched is None else (dict(shrink=s[0], sigma=s[1]) for s in sched)
        shapes = pyramid_shapes(target.shape[2:], L) if sched is None else schedule_shapes(target.shape[2:], sched[0][0])
        if tuple(moving.shape[2:]) != tuple(target.shape[2:]) and not grids and initial is None:
            raise ValueError(f"moving {tuple(moving.shape)} and target {tuple(target.shape)} differ in spatial size")
        flow = self.mode == 'flow'
        movs, tgts = pyramid(moving, L, align_corners=flow, **mk), pyramid(target, L, align_corners=flow, **tk)
        masks = [None] * L if mask is None else pyramid_masks(mask, L, align_corners=flow, **tk)      # raises for a pair whose mask empties at some level
        mmasks = [None] * L if moving_mask is None else pyramid_masks(moving_mask.to(moving.device), L, align_corners=flow, **mk)      # over the MOVING pyramid's shapes
        okw = (lambda k: dict(overlap=True, moving_mask=mmasks[k])) if overlap else (lambda k: {})      # the flag goes to every level
        init = None if flow else self.init
        mshapes = None if initial is None else pyramid_shapes(moving.shape[2:], L) if sched is None else schedule_shapes(moving.shape[2:], sched[1][0])
        self.level_losses, self.level_shapes, self.level_schedule = [], shapes, sched
        for k in range(L):
            if flow:
                fkw = self._flow_kw(n, lrs[k], epochs[k])
                if 'criterions' in fkw:
                    fkw['criterions'] = self._level_criteria(target.shape[2:], shapes[k])
                reg = flow_register(shapes[k], **fkw).to(moving.device)
                up = None if init is None else upsample_flow(init, shapes[k])
                if self.flow_model == 'bspline':
                    reg.base_flow = up       # the level's lattice starts from zero and adds to what the coarser levels found
                else:
                    reg.init_flow = up
                lvl_initial = None if initial is None else level_theta(initial, target.shape[2:], shapes[k], moving.shape[2:], mshapes[k])
                reg.optimize(movs[k], tgts[k], self.device, False, mask=masks[k], initial=lvl_initial, **okw(k))
                self.valid_fraction = reg.valid_fraction
                if initial is not None:
                    self.target_shape = tuple(shapes[k])
                init = reg.final_velocity if self.diffeomorphic else reg.final_flow      # diffeomorphic: the levels add up as velocities
                self.velocity, self.inverse_flow, self._inverse_warp = reg.velocity, reg.inverse_flow, reg.inverse
                self.theta, self.warp, self.final_theta = reg.flow, reg.deform, reg.final_flow
                self.control = reg.control
                self.losses = reg.losses
            else:
                fn = affine_register if self.mode == 'affine' else rigid_register
                info = {}
                kw = dict(lr=lrs[k], epochs=epochs[k], per=per, device=self.device, debug=False, grad_edges=self.grad_edges,
                          honor_criterion=self.honor_criterion, optimizer=self.optimizer, init=init, info=info, device_loop=self.device_loop)
                if self.criterion is not None and self.weight is not None:
                    kw.update(criterions=self._level_criteria(target.shape[2:], shapes[k]), weights=self.weight)
                elif self.weight is not None:
                    kw.update(weights=self.weight)
                if masks[k] is not None:
                    kw.update(mask=masks[k])
                if world is not None:
                    kw.update(world=world)      # A . N(S) does not depend on the level (align_corners=False keeps the field of view): one record for all
                elif grids:
                    # align_corners=False keeps an image's field of view: a level's voxel is the full one times (full size / level size), per axis
                    lvl = lambda voxel, full, x: None if voxel is None else tuple(v * s / sl for v, s, sl in zip(voxel, full.shape[2:], x.shape[2:]))  # noqa: E731
                    kw.update(moving_voxel=lvl(moving_voxel, moving, movs[k]), target_voxel=lvl(target_voxel, target, tgts[k]))
                _, theta = fn(movs[k], tgts[k], **kw, **okw(k))
                self.valid_fraction = info.get('valid_fraction')
                # (a level whose two shapes happen to coincide, without voxel sizes, is a one-lattice run: its theta is unscaled as it is)
                init = info['final_pose'] if self.mode == 'rigid' else info.get('final_unscaled_theta', theta[0])
                self.theta, self.final_theta = theta[-1], theta[0]
                self.losses, self.best_idx = info.get('losses'), info.get('best_idx')
                self.final_pose = info.get('final_pose')
                self._set_grids(grids, tgts[k], info)
            self.level_losses.append(self.losses)
            if self.debug:
                ls = self.losses.detach().flatten().cpu()
                ls = ls[~torch.isnan(ls)]
                print(f"[{self.mode}] level {k + 1}/{L} {tuple(shapes[k])}: {epochs[k]} iterations, lr {lrs[k]:g}, " +
                      (f"loss {ls[0].item():.6g} -> {ls[-1].item():.6g} (min {ls.min().item():.6g})" if len(ls) else "no iterations"))

    def __call__(self, moving, interpolation='linear'):
        '''
        Warp moving [B,c,x,y(,z)] with the deformation found by optim: one fused launch for all
        channels (the reference loops over channels, ref:torchregister.py:123-128).
        interpolation (extension): 'linear' - the path above, unchanged; 'nearest' (label maps, atlases, masks) / 'cubic' (the final
        resample of an image) - resample() with the registration's own transform: theta onto .target_shape for 'rigid' / 'affine', the
        flow - composed with .initial when optim(initial=...) set one - for 'flow'.  Those two are not differentiable.
        '''
        check_interpolation(interpolation)
        if self.theta is None:
            raise RuntimeError("call optim() first")
        if self.mode == 'flow':
            return self.warp(moving) if interpolation == 'linear' else self.warp(moving, interpolation=interpolation)
        if interpolation == 'linear':
            return self.warp(self.theta.detach(), moving)
        return resample(moving, theta=self.theta.detach(), size=self.target_shape, interpolation=interpolation)

    def jacobian(self):
        '''
        The Jacobian determinant map [B,1,x,y(,z)] of the deformation in .theta (mode='flow', any flow model, after optim): jacobian_determinant of
        the flow.  det <= 0 marks a fold; reg.jacobian().amin() and (reg.jacobian() <= 0).float().mean() are the usual summaries.  With
        optim(initial=...) multiply by the constant determinant of the affine for the whole transform.
        '''
        if self.mode != 'flow':
            raise ValueError("jacobian() is the determinant map of mode='flow': a rigid / affine transform has one constant determinant, that of reg.theta[:, :, :-1]")
        if self.theta is None:
            raise RuntimeError("call optim() first")
        return jacobian_determinant(self.theta)

    def invert_flow(self, iterations=30, tol=1e-3):
        '''
        (v, residual): the inverse [B,nd,x,y(,z)] of the deformation in .theta on its own lattice (mode='flow', any flow model, after optim) by the
        fixed-point iteration of invert_flow, and each voxel's last update [B,1,x,y(,z)] - a voxel has converged exactly when residual <= tol; where
        the deformation folds (reg.jacobian() <= 0) it has no inverse and residual says so.  resample(labels_on_target, flow=v,
        interpolation='nearest') carries a label map from the target back onto the moving image.  Not with optim(initial=...): the whole
        transform's inverse lives on the moving lattice - to_moving(x), transform_points(p, inverse=True) and inverse_transform() build it.
        diffeomorphic=True has .inverse_flow, the exponential of -velocity.
        '''
        iterations, tol = _invert_args(iterations, tol)
        if self.mode != 'flow':
            raise ValueError("invert_flow() inverts the dense flow of mode='flow': a rigid / affine transform has a closed-form inverse, that of the matrix reg.theta")
        if self.theta is None:
            raise RuntimeError("call optim() first")
        if self.initial is not None:
            raise ValueError("invert_flow() is not built for optim(initial=...): the inverse of the whole transform lives on the moving lattice")
        return invert_flow(self.theta, iterations, tol, return_residual=True)

    def _whole_transform(self):
        '''(effective theta or None, flow or None, target lattice, moving lattice) of the transform optim found: T(p) = theta(p + flow(p)) takes
        target-lattice voxels to moving-lattice voxels (theta between the normalised cubes; a missing piece is the identity).'''
        if self.theta is None:
            raise RuntimeError("call optim() first")
        if self.mode == 'flow':
            flow = self.theta.detach()
            lattice = tuple(flow.shape[2:])
            return (None if self.initial is None else self.initial.detach()), flow, lattice, (self.moving_shape or lattice)
        lattice = self.target_shape or self.moving_shape
        return self.theta.detach(), None, lattice, (self.moving_shape or lattice)

    def inverse_transform(self, iterations=30, tol=1e-3):
        '''
        (theta_inv, flow_inv, residual): the pieces of the inverse of the whole transform, moving-lattice voxels to target-lattice voxels,
        T^-1(q) = r + flow_inv(r) with r = theta_inv q (chain 'affine_then_flow' of transform_points / resample_affine_then_flow).  theta_inv is
        invert_theta of reg.theta (mode 'rigid' / 'affine') or of .initial (None without one), fp64; flow_inv [B,nd,x,y(,z)] on the target lattice is
        invert_flow(reg.theta, iterations, tol) with each voxel's last update in residual [B,1,x,y(,z)] - or .inverse_flow, the exponential of
        -velocity, under diffeomorphic=True (residual None); both None for mode 'rigid' / 'affine'.  For callers who keep the pieces:
        transform_points(inverse=True) and to_moving() build them on every call.
        '''
        iterations, tol = _invert_args(iterations, tol)
        theta, flow, _, _ = self._whole_transform()
        theta_inv = None if theta is None else invert_theta(theta)
        if flow is None:
            return theta_inv, None, None
        if self.inverse_flow is not None:
            return theta_inv, self.inverse_flow.detach(), None
        flow_inv, residual = invert_flow(flow, iterations, tol, return_residual=True)
        return theta_inv, flow_inv, residual

    def transform_points(self, points, inverse=False, iterations=30, tol=1e-3):
        '''
        Points [B,P,nd] or [P,nd] (fp32, GPU; voxel positions in the tensor's axis order) through the transform optim found (transform_points).
        inverse=False: target-lattice voxels to moving-lattice voxels, T(p) = theta(p + flow(p)) - reg.theta for 'rigid' / 'affine', the flow for
        'flow', the flow and then .initial after optim(initial=...).  inverse=True: moving to target through inverse_transform(iterations, tol).
        With the headers, (points_to_world(reg.transform_points(p), A_moving) - points_to_world(q, A_moving)).norm(dim=-1) is the target
        registration error in mm of landmarks p (target) and q (moving).
        '''
        iterations, tol = _invert_args(iterations, tol)
        theta, flow, tshape, mshape = self._whole_transform()
        if not inverse:
            return transform_points(points, theta=theta, flow=flow, from_shape=tshape, to_shape=mshape, chain='flow_then_affine')
        theta_inv, flow_inv, _ = self.inverse_transform(iterations, tol)
        return transform_points(points, theta=theta_inv, flow=flow_inv, from_shape=mshape, to_shape=tshape, chain='affine_then_flow')

    def to_moving(self, x, interpolation='linear', iterations=30, tol=1e-3):
        '''
        x [B,c,*target lattice] carried onto the moving lattice (.moving_shape) through the inverse of the whole transform - a label map drawn on
        the target back onto the moving image with interpolation='nearest'.  'rigid' / 'affine': resample with invert_theta(reg.theta); 'flow':
        resample with the inverted flow; 'flow' after optim(initial=...): resample_affine_then_flow, the inverse affine first and then the inverted
        flow on the target lattice, one interpolation.  The inverted flow is inverse_transform(iterations, tol)'s.
        '''
        check_interpolation(interpolation)
        iterations, tol = _invert_args(iterations, tol)
        _, _, _, mshape = self._whole_transform()
        theta_inv, flow_inv, _ = self.inverse_transform(iterations, tol)
        if flow_inv is None:
            return resample(x, theta=theta_inv.to(torch.float32), size=mshape, interpolation=interpolation)
        if theta_inv is None:
            return resample(x, flow=flow_inv, interpolation=interpolation)
        return resample_affine_then_flow(x, theta=theta_inv, flow=flow_inv, size=mshape, interpolation=interpolation)

    def inverse(self, x, interpolation='linear'):
        '''
        Warp x [B,c,x,y(,z)] with the inverse of the deformation found by optim, exp(-velocity) (diffeomorphic=True only).
        interpolation: as for __call__.
        '''
        check_interpolation(interpolation)
        if self.inverse_flow is None:
            raise RuntimeError("inverse() needs diffeomorphic=True and optim() first")
        return self._inverse_warp(x) if interpolation == 'linear' else self._inverse_warp(x, interpolation=interpolation)
