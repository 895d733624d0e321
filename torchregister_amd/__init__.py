"""MI355X-native TorchRegister hot path (drop-in for AgamChopra/TorchRegister's Register API).

`import torchregister_amd as tr` (or `import TorchRegister as tr` through the alias package)
gives `tr.Register(mode=...).optim(moving, target, ...)` / `reg(moving)` backed by hand-written
HIP kernels in lib/libtrx.so (C ABI: include/trx.h).  There is no CPU fallback.
"""
__version__ = "0.2.3"   # = the reference package version this host layer mirrors (ref:src/TorchRegister/__init__.py:4); C ABI: trx_version()

from ._engine import (AffineMISolver, AffineSolver, BSplineSolver, FlowSolver, LossSpec, SlabFlowSolver, SlabPeers, bspline_bending, bspline_expand, bspline_grid, bspline_reduce, svf_exp, svf_exp_backward,  # noqa: F401
                      folding_penalty, folding_penalty_grad, jacobian_determinant, compose_flows, invert_flow,
                      invert_theta, points_from_world, points_to_world, resample_affine_then_flow, transform_points,
                      affine_flow_valid, affine_flow_warp, affine_flow_warp_backward, affine_mi_loss_grad, grid_scale, resample, run_slabs_lockstep, spline_coefficients,
                      WorldGeometry, affine_world_theta, image_moments, theta_from_world, world_from_theta, world_geometry, world_setup,
                      WorldSearch, image_covariance, principal_axes_candidates, rotation_grid, world_search, ngf_edge_parameters, ngf_loss_grad)
from .gaussian import gaussian_resample, gaussian_smooth, pyramid_schedule  # noqa: F401
from .metrics import SurfaceDistances, dilate_mask, distance_transform, erode_mask, label_overlap, mask_surface, signed_distance, surface_distances  # noqa: F401
from .pyramid import pyramid, pyramid_masks, pyramid_shapes, upsample_flow  # noqa: F401
from .sharding import register_sharded  # noqa: F401
from .torchregister import Register  # noqa: F401
from .utils import (EPSILON, Attention_UNet, K_gauss, LocalNCCLoss, MILoss, NCCLoss, NGFLoss, NMI, NMILoss, PDF, PDF_xis, Regressor, SpatialTransformer, SSDLoss,  # noqa: F401
                    Theta, attention_grid, get_pdf, norm, padNd)
from .warpings import OVERLAP_SUPPORT, WORLD_SUPPORT, affine_register, compose_theta, flow_register, get_affine_warp, rigid_register  # noqa: F401
