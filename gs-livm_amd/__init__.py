"""gs_livm_amd -- MI355X-native tile rasterizer for GS-LIVM's render/optimisation hot path.

Layout (only what the hot path needs):
  csrc/            hand-written HIP kernels (gfx950) + the C ABI (include/gsraster.h) + LibTorch binding
  _capi.py         ctypes binding of the C ABI (mirrors src/gs/rasterize_points.cu)
  rasterizer.py    host-side mirror of the reference operator surface (src/gs/rasterizer.cu)
  render_utils.py  Camera (rasterizer-facing part) and render() as in include/gs/gs/render_utils.cuh
  seed.py          sweep admission: the points of a LiDAR sweep a keyframe's render does not explain yet, coloured from
                   the keyframe and sized by their pixel footprint, ready for add_new_pointcloud (csrc/seed.hip)
  voxelmap.py      the sweep voxel map: a persistent device voxel table with exact moments, one oriented Gaussian per
                   matured voxel, the voxel key of every sweep point (csrc/voxel.hip)
  loss.py          fused L1 + SSIM photometric loss (SURVEY.md 8(f) "next" row 2); fused LiDAR similarity loss; the fused
                   point-to-plane loss on oriented surfels (csrc/surfel.hip); fused
                   delta-depth loss between keyframe pairs; LiDAR depth supervision (sweep z-buffer + masked depth L1,
                   its occlusion filter, Huber residual and clip);
                   per-keyframe exposure compensation fused into the photometric loss; the weighted photometric loss
                   (per-pixel weights, a silhouette gate, the exposure)
  covis.py         keyframe covisibility: visibility bitsets, their overlap counts, observation counts, the remap a prune needs
  contribution.py  per-Gaussian blend contribution of a forward: pixels touched, summed and largest blend weight
  normals.py       rendered normal maps (per-Gaussian attributes blended behind a forward, camera-facing surfel normals) and
                   the depth-normal consistency loss (csrc/normal.hip)
  metrics.py       fused evaluation pass: PSNR / SSIM / L1 of a render, 8-bit frame export, the keyframe sweep
  model.py         fused activations + Adam for the caller's leaf tensors (SURVEY.md 8(f) "next" row 1)
  synthetic.py     synthetic scenes of SURVEY.md section 8(d) for tests and bench
  multiview.py     view-parallel sharding + the two RCCL exchange steps
  build.py         hipcc / g++ build recipe

The directory is named `gs-livm_amd`; import it as `gs_livm_amd` (alias module at the repo root).
"""
from . import multiview, synthetic  # noqa: F401
from ._capi import (GsrError, LIB_PATH, NumRendered, emit_guard_trips, last_num_rendered, lib, mailbox_slow_path_last, mark_visible,
                    set_binning_capacity_hint, speculation_stats, set_near_far, set_near_far_thread, set_reference_rects_thread, async_outcomes_pending, set_near_far_hints, last_near_far, set_far_speculation, last_far_skipped, profile_enable, profile_read,  # noqa: F401
                    pose_gradient, rasterize_backward, rasterize_forward, reference_rects, set_reference_rects, state_views)
from .loss import (DeltaDepthLoss, ExposureLoss, LidarDepthLoss, RobustLidarDepthLoss, PhotometricLoss, SimilarityLoss, SurfelPlaneLoss, WeightedPhotometricLoss, delta_depth_loss, delta_pose,  # noqa: F401
                   weighted_photometric_loss,
                   apply_exposure, exposure_photometric_loss, identity_exposure, lidar_depth_image, lidar_depth_loss,
                   lidar_occlusion_filter,
                   photometric_loss, raster_K, reference_window_1d, similarity_loss, surfel_plane_loss,
                   world_to_camera)
from .covis import (KeyframeVisibility, covisibility, iou, observation_count, overlap_coefficient,  # noqa: F401
                    visibility_pack, visibility_remap)
from .contribution import Contribution, contribution, low_contribution, render_contribution  # noqa: F401
from .normals import (NormalConsistencyLoss, blend_attributes, normal_consistency_loss, render_attributes,  # noqa: F401
                      render_normals, surfel_normals)
from .metrics import depth_to_u8, evaluate_keyframes, image_metrics, psnr, side_by_side, to_u8  # noqa: F401
from .model import FusedActivations, FusedAdam, GaussianParameters, GrowableAdam, GrowableGaussians, VoxelIndex, prune_rows  # noqa: F401
from . import ply  # noqa: F401
from .seed import Admitted, admit_sweep  # noqa: F401
from .voxelmap import SweepVoxelMap, VoxelSeeds  # noqa: F401
from .rasterizer import (GaussianRasterizationSettings, GaussianRasterizer,  # noqa: F401
                         rasterize_gaussians)
from .render_utils import Camera, get_projection_matrix, render, render_full, se3_exp  # noqa: F401



def torch_ops():
    """The C++/LibTorch operator surface (csrc/torch_binding.cpp), built in-tree as _gsraster_torch.so.
    This is the code GS-LIVM itself would link; raises when it has not been built (no fallback)."""
    import importlib.util
    import os
    import torch  # noqa: F401  (libtorch must be loaded first)
    lib()  # libgsraster_hip.so must resolve before the extension that links it
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gsraster_torch.so")
    if not os.path.exists(path):
        raise RuntimeError("_gsraster_torch.so not built: run `python gs-livm_amd/build.py`")
    spec = importlib.util.spec_from_file_location("_gsraster_torch", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


__all__ = ["NormalConsistencyLoss", "blend_attributes", "normal_consistency_loss", "render_attributes", "render_normals", "surfel_normals", "Admitted", "admit_sweep", "SweepVoxelMap", "VoxelSeeds", "WeightedPhotometricLoss", "weighted_photometric_loss", "Contribution", "contribution", "render_contribution", "low_contribution", "KeyframeVisibility", "visibility_pack", "covisibility", "observation_count", "visibility_remap", "iou", "overlap_coefficient", "ExposureLoss", "exposure_photometric_loss", "apply_exposure", "identity_exposure", "LidarDepthLoss", "RobustLidarDepthLoss", "lidar_occlusion_filter", "lidar_depth_image", "lidar_depth_loss", "raster_K", "world_to_camera", "prune_rows", "image_metrics", "psnr", "to_u8", "side_by_side", "depth_to_u8", "evaluate_keyframes", "DeltaDepthLoss", "delta_depth_loss", "delta_pose", "SimilarityLoss", "similarity_loss", "SurfelPlaneLoss", "surfel_plane_loss", "VoxelIndex", "PhotometricLoss", "photometric_loss", "reference_window_1d", "FusedActivations", "FusedAdam", "GaussianParameters", "GrowableAdam", "GrowableGaussians", "ply", "GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "Camera", "render", "render_full", "se3_exp", "pose_gradient", "get_projection_matrix", "rasterize_forward",
           "rasterize_backward", "mark_visible", "state_views", "set_reference_rects", "reference_rects", "last_num_rendered", "set_binning_capacity_hint", "speculation_stats", "emit_guard_trips", "mailbox_slow_path_last", "set_near_far", "set_near_far_thread", "set_reference_rects_thread", "async_outcomes_pending", "set_near_far_hints", "last_near_far", "set_far_speculation", "last_far_skipped", "NumRendered", "lib", "torch_ops", "synthetic", "multiview", "GsrError", "LIB_PATH"]
