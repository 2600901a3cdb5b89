"""ctypes binding of the C ABI in include/gsraster.h (libgsraster_hip.so).

This is the reference-side binding a Python host would use; the C++/LibTorch operator surface
(csrc/torch_binding.cpp) goes through the same ABI.  Device memory, streams and allocation are
PyTorch-ROCm plumbing; all compute is in the HIP library.  There is NO CPU fallback: if the
library is missing or a call fails, this module raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GSR_LIB", os.path.join(_HERE, "libgsraster_hip.so"))  # GSR_LIB: A/B experiment builds

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class GeometryView(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("depths", "radii", "splats", "cov3D", "tiles_touched", "point_offsets", "clamped", "depth_order",
                 "num_rendered", "gpack")]


class BinningView(C.Structure):
    _fields_ = [("point_list", C.c_void_p)]


class ImageView(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ranges", "final_T", "n_contrib", "quad_last", "ranges_far")]


class MailboxEvent(C.Structure):
    _fields_ = [("count", C.c_uint), ("ticket_expected", C.c_uint32), ("ticket_seen_before_query", C.c_uint32),
                ("elapsed_us", C.c_double), ("ticket_seen_after_query", C.c_uint32), ("first_query_result", C.c_int),
                ("visible_at_query", C.c_int), ("queries", C.c_uint), ("longest_query_us", C.c_double),
                ("longest_poll_gap_us", C.c_double)]


class NumRendered(int):
    """num_rendered as the reference returns it (RasterizeGaussiansCUDA's first element) -- the exact instance count --
    carrying `key`: what gsr_forward returned, the capacity the binning blob was carved for (== the count after a
    synchronous forward, >= it after a speculative one).  rasterize_backward / state_views take the key from it."""

    def __new__(cls, exact, key):
        obj = super().__new__(cls, exact)
        obj.key = int(key)
        return obj


def _key(R):
    return int(getattr(R, "key", R))


_lib = None

EXPORTS = ("gsr_forward", "gsr_backward", "gsr_backward_depth", "gsr_mark_visible", "gsr_geometry_bytes", "gsr_image_bytes",
           "gsr_binning_bytes", "gsr_geometry_view_of", "gsr_binning_view_of", "gsr_image_view_of",
           "gsr_higher_msb", "gsr_last_error", "gsr_abi_version", "gsr_kernel_count", "gsr_kernel_name",
           "gsr_profile_enable", "gsr_profile_enable_only", "gsr_profile_read", "gsr_mailbox_slow_path_hits", "gsr_activate", "gsr_activate_backward", "gsr_adam_step",
           "gsr_photometric_loss", "gsr_photometric_loss_workspace", "gsr_init_gaussians", "gsr_ply_row_floats",
           "gsr_pack_ply_rows", "gsr_model_step", "gsr_set_reference_rects", "gsr_reference_rects",
           "gsr_last_num_rendered", "gsr_set_binning_capacity_hint", "gsr_speculative_forwards",
           "gsr_speculation_overflows", "gsr_emit_guard_trips", "gsr_mailbox_slow_path_last", "gsr_set_near_far", "gsr_near_far",
           "gsr_last_near_far", "gsr_set_near_far_hints", "gsr_near_far_forwards", "gsr_set_far_speculation",
           "gsr_last_far_skipped", "gsr_far_skips", "gsr_far_skip_misses", "gsr_async_far_frames",
           "gsr_near_budget_scale", "gsr_near_budget_feedback", "gsr_near_far_pause", "gsr_set_near_far_thread",
           "gsr_set_reference_rects_thread", "gsr_async_outcomes_pending", "gsr_async_outcomes_lost",
           "gsr_frame_note_misses", "gsr_similarity_loss", "gsr_similarity_loss_workspace",
           "gsr_delta_depth_loss", "gsr_delta_depth_loss_workspace", "gsr_image_metrics",
           "gsr_image_metrics_workspace", "gsr_pack_image_u8", "gsr_pack_depth_u8", "gsr_prune_workspace",
           "gsr_prune_mark", "gsr_prune_compact", "gsr_lidar_depth_image", "gsr_lidar_depth_loss",
           "gsr_lidar_depth_loss_workspace", "gsr_density_accumulate", "gsr_densify_workspace", "gsr_densify_mark",
           "gsr_densify_apply", "gsr_pose_gradient", "gsr_pose_gradient_workspace", "gsr_exposure_loss",
           "gsr_exposure_loss_workspace", "gsr_apply_exposure", "gsr_visibility_words", "gsr_visibility_pack",
           "gsr_covisibility", "gsr_observation_count", "gsr_visibility_remap", "gsr_contribution_workspace",
           "gsr_contribution", "gsr_contribution_finish", "gsr_weighted_loss", "gsr_weighted_loss_workspace",
           "gsr_sweep_admit", "gsr_sweep_admit_workspace", "gsr_lidar_occlusion_filter",
           "gsr_lidar_depth_loss_robust", "gsr_lidar_depth_loss_robust_workspace", "gsr_voxel_table_bytes",
           "gsr_voxel_sweep_workspace", "gsr_voxel_sweep", "gsr_voxel_rehash", "gsr_surfel_plane_loss",
           "gsr_surfel_plane_loss_workspace", "gsr_blend_attributes", "gsr_surfel_normals",
           "gsr_normal_consistency_workspace", "gsr_normal_consistency_loss")


def lib():
    """Loads libgsraster_hip.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libgsraster_hip.so not built: run `python gs-livm_amd/build.py` (needs hipcc). "
            "gs_livm_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, ci, cf, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    L.gsr_forward.restype = ci
    L.gsr_forward.argtypes = [ALLOC_FN, vp, ALLOC_FN, vp, ALLOC_FN, vp, ci, ci, ci, vp, ci, ci, vp, vp, vp, vp, vp, cf,
                              vp, vp, vp, vp, vp, cf, cf, ci, vp, vp, vp, vp, ci, vp]
    L.gsr_backward.restype = ci
    L.gsr_backward.argtypes = [ci, ci, ci, ci, vp, ci, ci, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp,
                               vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp]
    # gsr_backward's arguments + dL_ddepth (after dL_dacc) and dL_ddepths (after dL_drot)
    L.gsr_backward_depth.restype = ci
    L.gsr_backward_depth.argtypes = L.gsr_backward.argtypes[:25] + [vp] + L.gsr_backward.argtypes[25:34] + [vp, ci, vp]
    L.gsr_mark_visible.restype = ci
    L.gsr_mark_visible.argtypes = [ci, vp, vp, vp, vp, vp]
    L.gsr_pose_gradient_workspace.restype = sz
    L.gsr_pose_gradient_workspace.argtypes = [ci]
    L.gsr_pose_gradient.restype = ci
    L.gsr_pose_gradient.argtypes = [ci, ci, ci, vp, vp, cf, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    for n in ("gsr_geometry_bytes", "gsr_binning_bytes"):
        getattr(L, n).restype = sz
        getattr(L, n).argtypes = [ci]
    L.gsr_image_bytes.restype = sz
    L.gsr_image_bytes.argtypes = [ci, ci]
    L.gsr_geometry_view_of.argtypes = [vp, ci, C.POINTER(GeometryView)]
    L.gsr_binning_view_of.argtypes = [vp, ci, C.POINTER(BinningView)]
    L.gsr_image_view_of.argtypes = [vp, ci, ci, C.POINTER(ImageView)]
    L.gsr_higher_msb.restype = C.c_uint32
    L.gsr_higher_msb.argtypes = [C.c_uint32]
    L.gsr_last_error.restype = C.c_char_p
    L.gsr_abi_version.restype = ci
    L.gsr_kernel_count.restype = ci
    L.gsr_kernel_name.restype = C.c_char_p
    L.gsr_kernel_name.argtypes = [ci]
    L.gsr_profile_enable.argtypes = [ci]
    L.gsr_profile_enable_only.argtypes = [C.POINTER(ci), ci]
    L.gsr_set_reference_rects.restype = ci
    L.gsr_set_reference_rects.argtypes = [ci]
    L.gsr_reference_rects.restype = ci
    L.gsr_reference_rects.argtypes = []
    L.gsr_last_num_rendered.restype = ci
    L.gsr_last_num_rendered.argtypes = []
    L.gsr_set_binning_capacity_hint.restype = C.c_longlong
    L.gsr_set_binning_capacity_hint.argtypes = [C.c_longlong]
    for n in ("gsr_speculative_forwards", "gsr_speculation_overflows", "gsr_emit_guard_trips"):
        getattr(L, n).restype = C.c_ulonglong
        getattr(L, n).argtypes = []
    L.gsr_set_near_far.restype = ci
    L.gsr_set_near_far.argtypes = [ci]
    L.gsr_near_far.restype = ci
    L.gsr_near_far.argtypes = []
    L.gsr_last_near_far.restype = ci
    L.gsr_last_near_far.argtypes = [C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.gsr_set_near_far_hints.restype = None
    L.gsr_set_near_far_hints.argtypes = [C.c_longlong, C.c_longlong]
    L.gsr_near_far_forwards.restype = C.c_ulonglong
    L.gsr_near_far_forwards.argtypes = []
    L.gsr_set_far_speculation.restype = ci
    L.gsr_set_far_speculation.argtypes = [ci]
    L.gsr_last_far_skipped.restype = ci
    L.gsr_last_far_skipped.argtypes = []
    L.gsr_near_budget_scale.restype = C.c_uint
    L.gsr_near_budget_scale.argtypes = []
    L.gsr_near_budget_feedback.restype = C.c_uint
    L.gsr_near_budget_feedback.argtypes = [C.c_uint, C.c_uint, C.c_uint]
    L.gsr_near_far_pause.restype = ci
    L.gsr_near_far_pause.argtypes = [ci]
    for n in ("gsr_far_skips", "gsr_far_skip_misses", "gsr_async_far_frames", "gsr_async_outcomes_lost",
              "gsr_frame_note_misses", "gsr_similarity_loss", "gsr_similarity_loss_workspace"):
        getattr(L, n).restype = C.c_ulonglong
        getattr(L, n).argtypes = []
    for n in ("gsr_set_near_far_thread", "gsr_set_reference_rects_thread"):
        getattr(L, n).restype = ci
        getattr(L, n).argtypes = [ci]
    L.gsr_async_outcomes_pending.restype = ci
    L.gsr_async_outcomes_pending.argtypes = []
    L.gsr_mailbox_slow_path_last.restype = ci
    L.gsr_mailbox_slow_path_last.argtypes = [C.POINTER(MailboxEvent)]
    L.gsr_mailbox_slow_path_hits.restype = C.c_ulonglong
    L.gsr_mailbox_slow_path_hits.argtypes = []
    L.gsr_profile_read.restype = ci
    L.gsr_profile_read.argtypes = [ci, C.POINTER(C.c_double), C.POINTER(ci)]
    L.gsr_activate.restype = ci
    L.gsr_activate.argtypes = [ci, ci] + [vp] * 9 + [vp]
    L.gsr_activate_backward.restype = ci
    L.gsr_activate_backward.argtypes = [ci, ci] + [vp] * 12 + [vp]
    L.gsr_photometric_loss_workspace.restype = sz
    L.gsr_photometric_loss_workspace.argtypes = [ci, ci, ci]
    L.gsr_photometric_loss.restype = ci
    L.gsr_photometric_loss.argtypes = [ci, ci, ci, vp, vp, C.POINTER(cf), cf, vp, vp, vp, sz, vp]
    L.gsr_exposure_loss_workspace.restype = sz
    L.gsr_exposure_loss_workspace.argtypes = [ci, ci, ci]
    L.gsr_exposure_loss.restype = ci
    L.gsr_exposure_loss.argtypes = [ci, ci, ci, vp, vp, vp, C.POINTER(cf), cf, vp, vp, vp, vp, sz, vp]
    L.gsr_weighted_loss_workspace.restype = sz
    L.gsr_weighted_loss_workspace.argtypes = [ci, ci, ci]
    L.gsr_weighted_loss.restype = ci
    L.gsr_weighted_loss.argtypes = [ci, ci, ci, vp, vp, vp, vp, cf, vp, C.POINTER(cf), cf, vp, vp, vp, vp, sz, vp]
    L.gsr_apply_exposure.restype = ci
    L.gsr_apply_exposure.argtypes = [ci, ci, ci, vp, vp, vp, vp]
    L.gsr_similarity_loss_workspace.restype = sz
    L.gsr_similarity_loss_workspace.argtypes = [ci, ci]
    L.gsr_similarity_loss.restype = ci
    L.gsr_similarity_loss.argtypes = [ci, ci, ci, vp, vp, vp, vp, cf, vp, vp, vp, ci, vp, sz, vp]
    L.gsr_surfel_plane_loss_workspace.restype = sz
    L.gsr_surfel_plane_loss_workspace.argtypes = [ci, ci]
    L.gsr_surfel_plane_loss.restype = ci
    L.gsr_surfel_plane_loss.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, cf, cf, cf, cf, vp, vp, vp, vp, ci, vp, sz, vp]
    L.gsr_delta_depth_loss_workspace.restype = sz
    L.gsr_delta_depth_loss_workspace.argtypes = [ci, ci]
    L.gsr_delta_depth_loss.restype = ci
    L.gsr_delta_depth_loss.argtypes = [ci, ci, vp, vp, vp, vp, C.POINTER(cf), C.POINTER(cf), C.POINTER(cf), cf, vp, vp,
                                       vp, vp, vp, sz, vp]
    L.gsr_lidar_depth_image.restype = ci
    L.gsr_lidar_depth_image.argtypes = [ci, vp, C.POINTER(cf), C.POINTER(cf), ci, ci, cf, cf, vp, vp, vp]
    L.gsr_lidar_depth_loss_workspace.restype = sz
    L.gsr_lidar_depth_loss_workspace.argtypes = [ci, ci]
    L.gsr_lidar_depth_loss.restype = ci
    L.gsr_lidar_depth_loss.argtypes = [ci, ci, vp, vp, vp, cf, cf, vp, vp, vp, vp, sz, vp]
    L.gsr_lidar_occlusion_filter.restype = ci
    L.gsr_lidar_occlusion_filter.argtypes = [ci, ci, vp, ci, cf, vp, vp, vp]
    L.gsr_lidar_depth_loss_robust_workspace.restype = sz
    L.gsr_lidar_depth_loss_robust_workspace.argtypes = [ci, ci]
    L.gsr_lidar_depth_loss_robust.restype = ci
    L.gsr_lidar_depth_loss_robust.argtypes = [ci, ci, vp, vp, vp, cf, cf, cf, cf, cf, cf, vp, vp, vp, vp, sz, vp]
    L.gsr_sweep_admit_workspace.restype = sz
    L.gsr_sweep_admit_workspace.argtypes = [ci, ci, ci]
    L.gsr_sweep_admit.restype = ci
    L.gsr_sweep_admit.argtypes = [ci, vp, vp, C.POINTER(cf), C.POINTER(cf), ci, ci, cf, cf, vp, vp, cf, cf, vp, ci, cf,
                                  vp, vp, cf, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.gsr_voxel_table_bytes.restype = sz
    L.gsr_voxel_table_bytes.argtypes = [C.c_longlong]
    L.gsr_voxel_sweep_workspace.restype = sz
    L.gsr_voxel_sweep_workspace.argtypes = [ci]
    L.gsr_voxel_sweep.restype = ci
    L.gsr_voxel_sweep.argtypes = [ci, vp, vp, cf, ci, cf, cf, vp, C.c_longlong, ci] + [vp] * 11 + [vp, sz, vp]
    L.gsr_voxel_rehash.restype = ci
    L.gsr_voxel_rehash.argtypes = [vp, C.c_longlong, vp, C.c_longlong, vp]
    L.gsr_image_metrics_workspace.restype = sz
    L.gsr_image_metrics_workspace.argtypes = [ci, ci, ci]
    L.gsr_image_metrics.restype = ci
    L.gsr_image_metrics.argtypes = [ci, ci, ci, vp, vp, C.POINTER(cf), vp, vp, vp, sz, vp]
    L.gsr_pack_image_u8.restype = ci
    L.gsr_pack_image_u8.argtypes = [ci, ci, vp, ci, vp, sz, vp]
    L.gsr_pack_depth_u8.restype = ci
    L.gsr_pack_depth_u8.argtypes = [ci, ci, vp, cf, vp, sz, vp]
    L.gsr_prune_workspace.restype = sz
    L.gsr_prune_workspace.argtypes = [ci]
    L.gsr_prune_mark.restype = ci
    L.gsr_prune_mark.argtypes = [ci, vp, vp, vp, vp, vp, cf, cf, ci, vp, vp, vp, vp, sz, vp]
    L.gsr_prune_compact.restype = ci
    L.gsr_prune_compact.argtypes = [ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(ci), vp, vp, vp]
    L.gsr_density_accumulate.restype = ci
    L.gsr_density_accumulate.argtypes = [ci, vp, vp, vp, vp]
    L.gsr_densify_workspace.restype = sz
    L.gsr_densify_workspace.argtypes = [ci]
    L.gsr_densify_mark.restype = ci
    L.gsr_densify_mark.argtypes = [ci, vp, vp, cf, cf, ci, vp, vp, vp, vp, sz, vp]
    L.gsr_densify_apply.restype = ci
    L.gsr_densify_apply.argtypes = [ci, ci, ci, vp, vp, C.c_ulonglong] + [vp] * 6 + [C.POINTER(vp), C.POINTER(vp), vp, vp]
    ll = C.c_longlong
    L.gsr_visibility_words.restype = sz
    L.gsr_visibility_words.argtypes = [ci]
    L.gsr_visibility_pack.restype = ci
    L.gsr_visibility_pack.argtypes = [ci, vp, vp, vp, ci, vp]
    L.gsr_covisibility.restype = ci
    L.gsr_covisibility.argtypes = [ci, vp, ll, ci, vp, ll, ci, vp, vp, vp, vp]
    L.gsr_observation_count.restype = ci
    L.gsr_observation_count.argtypes = [ci, vp, ll, ci, ci, ci, vp, vp, vp]
    L.gsr_visibility_remap.restype = ci
    L.gsr_visibility_remap.argtypes = [ci, vp, ll, ci, vp, vp, vp, ll, ci, vp]
    L.gsr_contribution_workspace.restype = sz
    L.gsr_contribution_workspace.argtypes = [ci]
    L.gsr_contribution.restype = ci
    L.gsr_contribution.argtypes = [ci, ci, ci, ci, vp, vp, vp, vp, vp]
    L.gsr_contribution_finish.restype = ci
    L.gsr_contribution_finish.argtypes = [ci, vp, ci, cf, vp, vp, vp, vp, vp, vp]
    L.gsr_blend_attributes.restype = ci
    L.gsr_blend_attributes.argtypes = [ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]
    L.gsr_surfel_normals.restype = ci
    L.gsr_surfel_normals.argtypes = [ci, vp, vp, vp, C.POINTER(cf), vp, vp]
    L.gsr_normal_consistency_workspace.restype = sz
    L.gsr_normal_consistency_workspace.argtypes = [ci, ci]
    L.gsr_normal_consistency_loss.restype = ci
    L.gsr_normal_consistency_loss.argtypes = [ci, ci, vp, vp, vp, cf, cf, cf, cf, cf, cf, cf, cf, vp, vp, vp, vp, sz, vp]
    L.gsr_init_gaussians.restype = ci
    L.gsr_init_gaussians.argtypes = [ci, ci, vp, vp, vp, cf] + [vp] * 6 + [vp]
    L.gsr_ply_row_floats.restype = sz
    L.gsr_ply_row_floats.argtypes = [ci]
    L.gsr_pack_ply_rows.restype = ci
    L.gsr_pack_ply_rows.argtypes = [ci, ci] + [vp] * 7 + [vp]
    L.gsr_model_step.restype = ci
    L.gsr_model_step.argtypes = [ci, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)] + [vp] * 9 + \
        [C.POINTER(cf), C.c_double, C.c_double, C.c_double, ci, vp]
    L.gsr_adam_step.restype = ci
    L.gsr_adam_step.argtypes = [ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(sz),
                                C.POINTER(cf), C.c_double, C.c_double, C.c_double, ci, ci, vp]
    _lib = L
    return L


class GsrError(RuntimeError):
    pass


def _check(code):
    if code < 0:
        raise GsrError("libgsraster_hip error %d: %s" % (code, lib().gsr_last_error().decode()))
    return code


def _ptr(t):
    """Device pointer of a tensor; size-0 / None -> NULL (the reference's convention,
    src/gs/rasterizer.cu:178-193)."""
    if t is None or t.numel() == 0:
        return None
    assert t.is_cuda and t.is_contiguous(), "expects contiguous device tensors"
    return C.c_void_p(t.data_ptr())


def _rot16(t):
    """`rotations` is the one caller tensor the library reads with 16-byte loads whatever its address
    (include/gsraster.h): a misaligned one -- a view into a larger buffer -- is handed over as an aligned copy."""
    if t is not None and t.numel() and t.data_ptr() & 15:
        t = t.clone(memory_format=torch.contiguous_format)
        assert t.data_ptr() & 15 == 0
    return t


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Blob:
    """Allocator callback target: replaces resizeFunctional (src/gs/rasterize_points.cu:36-44)."""

    def __init__(self, device):
        self.device = device
        self.tensor = torch.empty(0, dtype=torch.uint8, device=device)
        self.fn = ALLOC_FN(self._alloc)

    def _alloc(self, _ctx, nbytes):
        try:
            self.tensor = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
            return self.tensor.data_ptr()
        except Exception:  # pragma: no cover - surfaces as GSR_ERR_ALLOC
            return None


def rasterize_forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                      viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                      prefiltered=False, debug=False, radii_out=True):
    """Mirror of RasterizeGaussiansCUDA (src/gs/rasterize_points.cu:46-130) over the C ABI.
    Returns (num_rendered, out_color, out_depth, out_acc, radii, geomBuffer, binningBuffer, imgBuffer)."""
    if means3D.dim() != 2 or means3D.size(1) != 3:
        raise ValueError("means3D must have dimensions (num_points, 3)")
    dev = means3D.device
    P, H, W = int(means3D.size(0)), int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=dev)
    out_color = torch.empty((3, H, W), **f32)
    out_depth = torch.empty((1, H, W), **f32)
    out_acc = torch.empty((1, H, W), **f32)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)  # the library writes every entry
    gb, bb, ib = _Blob(dev), _Blob(dev), _Blob(dev)
    M = int(sh.size(1)) if (sh is not None and sh.numel() != 0) else 0
    rotations = _rot16(rotations)
    L = lib()
    R = _check(L.gsr_forward(gb.fn, None, bb.fn, None, ib.fn, None, P, int(degree), M, _ptr(background), W, H,
                             _ptr(means3D), _ptr(sh), _ptr(colors), _ptr(opacity), _ptr(scales),
                             float(scale_modifier), _ptr(rotations), _ptr(cov3D_precomp), _ptr(viewmatrix),
                             _ptr(projmatrix), _ptr(campos), float(tan_fovx), float(tan_fovy), int(bool(prefiltered)),
                             _ptr(out_color), _ptr(out_depth), _ptr(out_acc), _ptr(radii) if radii_out else None,
                             int(bool(debug)), _stream()))
    R = NumRendered(L.gsr_last_num_rendered() if P else 0, R)
    return R, out_color, out_depth, out_acc, radii, gb.tensor, bb.tensor, ib.tensor


def rasterize_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                       viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_acc, sh, degree, campos,
                       geomBuffer, R, binningBuffer, imageBuffer, debug=False, return_conic=False, want_cov3D=True,
                       grad_depth=None):
    """Mirror of RasterizeGaussiansBackwardCUDA (src/gs/rasterize_points.cu:132-224).
    Returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    [+ dL_dconic when return_conic].  want_cov3D=False (only without cov3D_precomp): dL_dcov3D -- then an intermediate
    nobody reads -- is neither allocated nor written and comes back as None.
    grad_depth ([1,H,W] or [H,W], the gradient w.r.t. the rendered depth; an extension, the reference has none):
    gsr_backward_depth is called instead of gsr_backward and dL_ddepths [P] is appended to the result."""
    dev = means3D.device
    P = int(means3D.size(0))
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    M = int(sh.size(1)) if (sh is not None and sh.numel() != 0) else 0
    f32 = dict(dtype=torch.float32, device=dev)
    # the library overwrites every element, so torch.empty replaces the reference's nine torch::zeros
    # (rasterize_points.cu:173-181); P == 0 needs the zeros (nothing runs).
    mk = torch.zeros if P == 0 else torch.empty
    dL_dmeans3D = mk((P, 3), **f32)
    dL_dmeans2D = mk((P, 3), **f32)
    dL_dcolors = mk((P, 3), **f32)
    dL_dconic = mk((P, 2, 2), **f32)
    dL_dopacity = mk((P, 1), **f32)
    dL_dcov3D = mk((P, 6), **f32) if want_cov3D else None
    dL_dsh = mk((P, M, 3), **f32)
    dL_dscales = mk((P, 3), **f32)
    dL_drotations = mk((P, 4), **f32)
    dL_ddepths = mk((P,), **f32) if grad_depth is not None else None
    rotations = _rot16(rotations)
    if P != 0 and grad_depth is not None:
        dpix = dL_dout_color.contiguous()
        dacc = dL_dout_acc.contiguous()
        if grad_depth.dtype != torch.float32 or grad_depth.device != dev or grad_depth.numel() != H * W:
            raise ValueError("grad_depth must be a float32 tensor of H*W elements on the device of means3D")
        ddep = grad_depth.contiguous()
        _check(lib().gsr_backward_depth(P, int(degree), M, _key(R), _ptr(background), W, H, _ptr(means3D), _ptr(sh),
                                        _ptr(colors), _ptr(scales), float(scale_modifier), _ptr(rotations),
                                        _ptr(cov3D_precomp), _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos),
                                        float(tan_fovx), float(tan_fovy), _ptr(radii), _ptr(geomBuffer),
                                        _ptr(binningBuffer), _ptr(imageBuffer), _ptr(dpix), _ptr(dacc), _ptr(ddep),
                                        _ptr(dL_dmeans2D), _ptr(dL_dconic), _ptr(dL_dopacity), _ptr(dL_dcolors),
                                        _ptr(dL_dmeans3D), _ptr(dL_dcov3D), _ptr(dL_dsh), _ptr(dL_dscales),
                                        _ptr(dL_drotations), _ptr(dL_ddepths), int(bool(debug)), _stream()))
    elif P != 0:
        dpix = dL_dout_color.contiguous()
        dacc = dL_dout_acc.contiguous()
        _check(lib().gsr_backward(P, int(degree), M, _key(R), _ptr(background), W, H, _ptr(means3D), _ptr(sh),
                                  _ptr(colors), _ptr(scales), float(scale_modifier), _ptr(rotations),
                                  _ptr(cov3D_precomp), _ptr(viewmatrix), _ptr(projmatrix), _ptr(campos),
                                  float(tan_fovx), float(tan_fovy), _ptr(radii), _ptr(geomBuffer),
                                  _ptr(binningBuffer), _ptr(imageBuffer), _ptr(dpix), _ptr(dacc), _ptr(dL_dmeans2D),
                                  _ptr(dL_dconic), _ptr(dL_dopacity), _ptr(dL_dcolors), _ptr(dL_dmeans3D),
                                  _ptr(dL_dcov3D), _ptr(dL_dsh), _ptr(dL_dscales), _ptr(dL_drotations),
                                  int(bool(debug)), _stream()))
    out = (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    if return_conic:
        out = out + (dL_dconic,)
    return out + (dL_ddepths,) if grad_depth is not None else out


def pose_gradient(means3D, radii, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                  tan_fovy, image_height, image_width, dL_dmeans2D, dL_dconic, dL_dmeans3D, dL_ddepths=None,
                  workspace=None):
    """gsr_pose_gradient behind a rasterize_backward(..., return_conic=True) over the same inputs: dL/dxi [6] float32
    (device) of the left perturbation T_cw <- Exp(xi^) T_cw at xi = 0, [0:3] translation, [3:6] rotation, camera axes
    (include/gsraster.h).  dL_ddepths: that backward's last output when it was given grad_depth, else None."""
    dev = means3D.device
    P = int(means3D.size(0))
    L = lib()
    need = int(L.gsr_pose_gradient_workspace(P))
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty(6, dtype=torch.float32, device=dev)
    rotations = _rot16(rotations)
    _check(L.gsr_pose_gradient(P, int(image_width), int(image_height), _ptr(means3D), _ptr(scales),
                               float(scale_modifier), _ptr(rotations), _ptr(cov3D_precomp), _ptr(viewmatrix),
                               _ptr(projmatrix), float(tan_fovx), float(tan_fovy), _ptr(radii), _ptr(dL_dmeans2D),
                               _ptr(dL_dconic), _ptr(dL_ddepths), _ptr(dL_dmeans3D), _ptr(out), _ptr(workspace),
                               workspace.numel(), _stream()))
    return out


def last_num_rendered():
    """Exact instance count of the calling thread's last forward (no device access)."""
    return int(lib().gsr_last_num_rendered())


def set_binning_capacity_hint(capacity):
    """Test / tuning hook (include/gsraster.h): the calling thread's NEXT forward allocates its binning blob for
    `capacity` instances (smaller than the frame's count forces the overflow path); 0 = forget the history (next
    forward synchronous); None = no override."""
    return int(lib().gsr_set_binning_capacity_hint(-1 if capacity is None else int(capacity)))


def speculation_stats():
    L = lib()
    return dict(speculative_forwards=int(L.gsr_speculative_forwards()), overflows=int(L.gsr_speculation_overflows()),
                near_far_forwards=int(L.gsr_near_far_forwards()), far_skips=int(L.gsr_far_skips()),
                far_skip_misses=int(L.gsr_far_skip_misses()), async_far_frames=int(L.gsr_async_far_frames()),
                async_outcomes_lost=int(L.gsr_async_outcomes_lost()), frame_note_misses=int(L.gsr_frame_note_misses()),
                near_budget_scale_q8=int(L.gsr_near_budget_scale()),
                mailbox_slow_path_hits=int(L.gsr_mailbox_slow_path_hits()))


def emit_guard_trips():
    """Emit chunks whose chunk-table entries the emitters refused (include/gsraster.h, gsr_emit_guard_trips): 0 unless
    binning has a defect.  Reads device memory, so -- unlike speculation_stats, which bench.py reads around its timed
    region -- it waits for the work enqueued so far."""
    return int(lib().gsr_emit_guard_trips())


def mailbox_slow_path_last():
    ev = MailboxEvent()
    _check(lib().gsr_mailbox_slow_path_last(C.byref(ev)))
    return {n: getattr(ev, n) for n, _ in MailboxEvent._fields_}


def set_near_far(on):
    """Near/far frames (include/gsraster.h): speculative forwards of dense scenes bin the nearest Gaussians first and
    the rest only where a tile is still unfinished.  Returns the previous setting."""
    return bool(lib().gsr_set_near_far(int(bool(on))))


def set_near_far_thread(mode):
    """The same switch for the CALLING THREAD's forwards only: True / False, None = follow the process-wide value.
    Returns the thread's previous setting (None = none)."""
    prev = int(lib().gsr_set_near_far_thread(-1 if mode is None else int(bool(mode))))
    return None if prev < 0 else bool(prev)


def async_outcomes_pending():
    """Asynchronous frames of the calling thread whose far-chain outcome has not reached the host yet (never waits)."""
    return int(lib().gsr_async_outcomes_pending())


def set_near_far_hints(near_entries_per_tile=None, far_capacity=None):
    """Test / tuning hook: near budget in list entries per tile and the far capacity of the calling thread's next
    near/far forward (None = default / from history)."""
    lib().gsr_set_near_far_hints(-1 if near_entries_per_tile is None else int(near_entries_per_tile),
                                 -1 if far_capacity is None else int(far_capacity))


def set_far_speculation(mode):
    """Test / tuning hook (include/gsraster.h): True = the calling thread's next split forward does not enqueue its far
    chain until it has seen the live-tile count, False = never, None = automatic.  Returns the previous override."""
    return int(lib().gsr_set_far_speculation(-1 if mode is None else int(bool(mode))))


def last_far_skipped():
    return bool(lib().gsr_last_far_skipped())


def last_near_far():
    """(was the calling thread's last forward binned near/far, near instances, far instances)"""
    a, b = C.c_uint(0), C.c_uint(0)
    split = bool(lib().gsr_last_near_far(C.byref(a), C.byref(b)))
    return split, int(a.value), int(b.value)


def set_reference_rects(on):
    """Binning mode (include/gsraster.h): True = the reference's full 3-sigma tile squares (auxiliary.h:39-46), so that
    tiles_touched / num_rendered / point_list / ranges / n_contrib are the reference's own; False (default) = the
    footprint-culled rectangles.  Returns the previous setting."""
    return bool(lib().gsr_set_reference_rects(int(bool(on))))


def set_reference_rects_thread(mode):
    """Binning mode of the CALLING THREAD's forwards only: True / False, None = follow the process-wide value.  Returns
    the thread's previous setting (None = none)."""
    prev = int(lib().gsr_set_reference_rects_thread(-1 if mode is None else int(bool(mode))))
    return None if prev < 0 else bool(prev)


def reference_rects():
    return bool(lib().gsr_reference_rects())


def mark_visible(means3D, viewmatrix, projmatrix):
    """Mirror of markVisible (src/gs/rasterize_points.cu:226-241)."""
    P = int(means3D.size(0))
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P:
        _check(lib().gsr_mark_visible(P, _ptr(means3D), _ptr(viewmatrix), _ptr(projmatrix),
                                      C.c_void_p(present.data_ptr()), _stream()))
    return present


def _sub(blob, ptr, count, dtype):
    if not ptr or count == 0:
        return None
    off = int(ptr) - blob.data_ptr()
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    return blob[off:off + nbytes].view(dtype)


def state_views(geomBuffer, binningBuffer, imageBuffer, P, R, W, H):
    """Typed tensor views into the three opaque blobs (tests / tooling)."""
    L = lib()
    gv, bv, iv = GeometryView(), BinningView(), ImageView()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    out = {}
    if P:
        _check(L.gsr_geometry_view_of(_ptr(geomBuffer), P, C.byref(gv)))
        splats = _sub(geomBuffer, gv.splats, P * 12, torch.float32).view(P, 12)
        gpack = _sub(geomBuffer, gv.gpack, P * 2, torch.int32).view(P, 2)
        out.update(depths=splats[:, 9],  # (culled Gaussians have no record: compare where radii > 0)
                   radii=_sub(geomBuffer, gv.radii, P, torch.int32),  # valid only if the forward got no radii array
                   splats=splats,
                   cov3D=_sub(geomBuffer, gv.cov3D, P * 6, torch.float32).view(P, 6),  # debug forwards only
                   tiles_touched=gpack[:, 0],
                   point_offsets=_sub(geomBuffer, gv.point_offsets, P, torch.int32),
                   clamped=_sub(geomBuffer, gv.clamped, P, torch.uint8),
                   depth_order=_sub(geomBuffer, gv.depth_order, P, torch.int32))
        _check(L.gsr_image_view_of(_ptr(imageBuffer), W, H, C.byref(iv)))
        out.update(ranges=_sub(imageBuffer, iv.ranges, T * 2, torch.int32).view(T, 2),
                   final_T=_sub(imageBuffer, iv.final_T, W * H, torch.float32).view(H, W),
                   n_contrib=_sub(imageBuffer, iv.n_contrib, W * H, torch.int32).view(H, W),
                   quad_last=_sub(imageBuffer, iv.quad_last, T * 4, torch.int32).view(T, 4))
        counters = _sub(geomBuffer, gv.num_rendered, 16, torch.int32).cpu().tolist()  # the forward's device counters
        split = counters[12] == 1
        exact = counters[6] + counters[8] if split else counters[0]
        out.update(num_rendered=exact, near_far=split, counters=counters)
        key = _key(R)
        if exact:
            _check(L.gsr_binning_view_of(_ptr(binningBuffer), key, C.byref(bv)))
            raw = _sub(binningBuffer, bv.point_list, key, torch.int32)
            # A tile's list = its near segment followed by its far segment (near/far frames; the far ranges are (0, 0)
            # otherwise).  The views present it as the reference does: ONE list per tile, lists back to back in tile
            # order, `ranges` indexing into `point_list`.
            ra = out["ranges"].long()
            rb = _sub(imageBuffer, iv.ranges_far, T * 2, torch.int32).view(T, 2).long()
            seg_start = torch.stack([ra[:, 0], rb[:, 0]], 1).reshape(-1)
            seg_len = torch.stack([ra[:, 1] - ra[:, 0], rb[:, 1] - rb[:, 0]], 1).reshape(-1)
            total = int(seg_len.sum())
            excl = torch.cumsum(seg_len, 0) - seg_len
            idx = torch.repeat_interleave(seg_start - excl, seg_len) + torch.arange(total, device=ra.device)
            point_list = raw[idx]
            ln = seg_len.view(T, 2).sum(1)
            ends = torch.cumsum(ln, 0)
            ranges = torch.stack([ends - ln, ends], 1)
            ranges[ln == 0] = 0  # the reference's memset leaves (0, 0) for tiles without instances
            out.update(ranges_near=out["ranges"], ranges_far=rb.int(), ranges=ranges.int())
            tile_ids = torch.repeat_interleave(torch.arange(T, device=ra.device), ln)
            # the reference's 64-bit sorted keys, recomposed: (tile << 32) | bits(depth of the instance's Gaussian)
            dbits = out["depths"].view(torch.int32)[point_list.long()].long() & 0xFFFFFFFF
            out.update(tile_ids=tile_ids, point_list=point_list, keys=(tile_ids.long() << 32) | dbits)
    return out


def profile_enable(on=True, only=None):
    """Start / stop recording a hipEvent pair around every kernel launch (bench.py's roofline line).
    `only`: iterable of kernel names -- record just those (each recorded launch costs a few us of GPU idle)."""
    L = lib()
    if on and only is not None:
        names = [L.gsr_kernel_name(i).decode() for i in range(L.gsr_kernel_count())]
        ids = [names.index(k) for k in only]
        _check(L.gsr_profile_enable_only((C.c_int * len(ids))(*ids), len(ids)))
    else:
        _check(L.gsr_profile_enable(int(bool(on))))


def profile_read():
    """{kernel name: (total_ms, launches)} since the last read; synchronises the recorded events."""
    L = lib()
    n = L.gsr_kernel_count()
    ms = (C.c_double * n)()
    cnt = (C.c_int * n)()
    _check(L.gsr_profile_read(n, ms, cnt))
    return {L.gsr_kernel_name(i).decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}


# ---- "next" row: fused activations + Adam (include/gsraster.h; csrc/optimizer.hip) ----
def activate(scaling_raw, rotation_raw, opacity_raw, features_dc, features_rest):
    """GaussianModel's getters in one launch (include/gs/gs/gaussian.cuh:40-54):
    returns (scales [P,3], rotations [P,4], opacities [P,1], shs [P,M,3])."""
    P = int(scaling_raw.size(0))
    M = 1 + (int(features_rest.size(1)) if features_rest is not None and features_rest.numel() else 0)
    f32 = dict(dtype=torch.float32, device=scaling_raw.device)
    scales, rot = torch.empty((P, 3), **f32), torch.empty((P, 4), **f32)
    opac, shs = torch.empty((P, 1), **f32), torch.empty((P, M, 3), **f32)
    _check(lib().gsr_activate(P, M, _ptr(scaling_raw), _ptr(rotation_raw), _ptr(opacity_raw), _ptr(features_dc),
                              _ptr(features_rest), _ptr(scales), _ptr(rot), _ptr(opac), _ptr(shs), _stream()))
    return scales, rot, opac, shs


def activate_backward(rotation_raw, scales, opacities, g_scales, g_rot, g_opac, g_shs):
    """Chain rule of `activate`; returns grads w.r.t. (_scaling, _rotation, _opacity, _features_dc, _features_rest)."""
    P, M = int(scales.size(0)), int(g_shs.size(1))
    f32 = dict(dtype=torch.float32, device=scales.device)
    gs, gr, go = torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 1), **f32)
    gdc, grest = torch.empty((P, 1, 3), **f32), torch.empty((P, M - 1, 3), **f32)
    _check(lib().gsr_activate_backward(P, M, _ptr(rotation_raw), _ptr(scales), _ptr(opacities), _ptr(g_scales),
                                       _ptr(g_rot), _ptr(g_opac), _ptr(g_shs), _ptr(gs), _ptr(gr), _ptr(go),
                                       _ptr(gdc), _ptr(grest), _stream()))
    return gs, gr, go, gdc, grest


def adam_step(params, grads, exp_avg, exp_avg_sq, lrs, beta1, beta2, eps, step, zero_grads=True):
    """torch::optim::Adam::step for up to 8 tensors in one launch (in place)."""
    n = len(params)
    VP = C.c_void_p * n
    arr = lambda ts: VP(*[t.data_ptr() if t.numel() else None for t in ts])  # noqa: E731
    numel = (C.c_size_t * n)(*[int(t.numel()) for t in params])
    lr = (C.c_float * n)(*[float(x) for x in lrs])
    for t in list(params) + list(grads) + list(exp_avg) + list(exp_avg_sq):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
    _check(lib().gsr_adam_step(n, arr(params), arr(grads), arr(exp_avg), arr(exp_avg_sq), numel, lr, float(beta1),
                               float(beta2), float(eps), int(step), int(bool(zero_grads)), _stream()))


def photometric_loss(img, gt, window11, lambda_dssim, want_grad=True):
    """(1 - lambda) * L1 + lambda * (1 - SSIM) in three launches (include/gsraster.h).
    Returns (out3 = [loss, l1, ssim] device tensor, dL_dimg or None)."""
    assert img.dim() == 3 and img.shape == gt.shape and img.is_cuda
    Cn, H, W = (int(x) for x in img.shape)
    img, gt = img.contiguous(), gt.contiguous()
    nbytes = int(lib().gsr_photometric_loss_workspace(Cn, H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    out3 = torch.empty(3, dtype=torch.float32, device=img.device)
    grad = torch.empty_like(img) if want_grad else None
    win = (C.c_float * 11)(*[float(x) for x in window11])
    _check(lib().gsr_photometric_loss(Cn, H, W, _ptr(img), _ptr(gt), win, float(lambda_dssim), _ptr(out3), _ptr(grad),
                                      _ptr(ws), nbytes, _stream()))
    return out3, grad


def exposure_loss(img, gt, exposure, window11, lambda_dssim, want_grad=True):
    """The photometric loss on x' = fma(g_c, img, b_c) in three launches (include/gsraster.h, gsr_exposure_loss).
    exposure: [C,2] f32 on the device.  Returns (out3 = [loss, l1, ssim] device tensor, dL_dimg or None,
    dL_dexposure [C,2] or None)."""
    assert img.dim() == 3 and img.shape == gt.shape and img.is_cuda
    Cn, H, W = (int(x) for x in img.shape)
    assert exposure.is_cuda and exposure.dtype == torch.float32 and tuple(exposure.shape) == (Cn, 2)
    img, gt, exposure = img.contiguous(), gt.contiguous(), exposure.contiguous()
    nbytes = int(lib().gsr_exposure_loss_workspace(Cn, H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=img.device)
    out3 = torch.empty(3, dtype=torch.float32, device=img.device)
    grad = torch.empty_like(img) if want_grad else None
    grad_e = torch.empty_like(exposure) if want_grad else None
    win = (C.c_float * 11)(*[float(x) for x in window11])
    _check(lib().gsr_exposure_loss(Cn, H, W, _ptr(img), _ptr(gt), _ptr(exposure), win, float(lambda_dssim), _ptr(out3),
                                   _ptr(grad), _ptr(grad_e), _ptr(ws), nbytes, _stream()))
    return out3, grad, grad_e


def weighted_loss(img, gt, weights, acc, acc_min, exposure, window11, lambda_dssim, want_grad=True, out=None):
    """The photometric loss under per-pixel weights w = weights * [acc >= acc_min], normalised by their sum
    (include/gsraster.h, gsr_weighted_loss).  weights, acc: [H,W] f32 on the device or None; exposure: [C,2] or None.
    out: a contiguous device f32 [6] to write, or None.  Returns (out6 = [loss, l1, ssim, S, mse, psnr] device tensor,
    dL_dimg or None, dL_dexposure [C,2] or None)."""
    assert img.dim() == 3 and img.shape == gt.shape and img.is_cuda and img.dtype == torch.float32 == gt.dtype
    Cn, H, W = (int(x) for x in img.shape)
    img, gt = img.contiguous(), gt.contiguous()
    planes = []
    for t in (weights, acc):
        if t is not None:
            assert t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (H, W), "weights / acc: [H,W] float32"
            t = t.contiguous()
        planes.append(t)
    if exposure is not None:
        assert exposure.is_cuda and exposure.dtype == torch.float32 and tuple(exposure.shape) == (Cn, 2)
        exposure = exposure.contiguous()
    nbytes = int(lib().gsr_weighted_loss_workspace(Cn, H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=img.device)
    if out is None:
        out = torch.empty(6, dtype=torch.float32, device=img.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() == 6 and out.is_contiguous()
    grad = torch.empty_like(img) if want_grad else None
    grad_e = torch.empty_like(exposure) if want_grad and exposure is not None else None
    win = (C.c_float * 11)(*[float(x) for x in window11])
    _check(lib().gsr_weighted_loss(Cn, H, W, _ptr(img), _ptr(gt), _ptr(planes[0]), _ptr(planes[1]), float(acc_min),
                                   _ptr(exposure), win, float(lambda_dssim), _ptr(out), _ptr(grad), _ptr(grad_e),
                                   _ptr(ws), nbytes, _stream()))
    return out, grad, grad_e


def apply_exposure(img, exposure, out=None):
    """out = fma(g_c, img, b_c) in one launch (include/gsraster.h, gsr_apply_exposure).  img: [C,H,W] f32 on the device,
    contiguous; exposure: [C,2]; out: a contiguous tensor of img's shape (img itself is allowed) or None = a new one."""
    assert img.dim() == 3 and img.is_cuda and img.dtype == torch.float32 and img.is_contiguous()
    Cn, H, W = (int(x) for x in img.shape)
    assert exposure.is_cuda and exposure.dtype == torch.float32 and tuple(exposure.shape) == (Cn, 2)
    if out is None:
        out = torch.empty_like(img)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == img.shape
    _check(lib().gsr_apply_exposure(Cn, H, W, _ptr(img), _ptr(exposure.contiguous()), _ptr(out), _stream()))
    return out


def similarity_loss(points, sel, xyz, scaling, lambda_, grad_xyz=None, grad_scaling=None, accumulate=False):
    """lambda * mean_i max(min_j |p_i - xyz[sel_j]| - mean(scaling[sel]), 0) in three launches (include/gsraster.h,
    gsr_similarity_loss).  points [m,3] f32, sel [n] int32 (ascending, unique, < P), xyz / scaling [P,3] f32, all on
    the device.  grad_xyz / grad_scaling: [P,3] buffers whose selected rows are written (accumulate=False) or added to
    (accumulate=True); None = not wanted.  Returns out3 = [loss, mean clamped distance, r] (device tensor)."""
    P, m, n = int(xyz.size(0)), int(points.size(0)), int(sel.size(0))
    assert xyz.is_cuda and xyz.shape == (P, 3) and scaling.shape == (P, 3) and points.shape == (m, 3)
    assert sel.dtype == torch.int32 and sel.dim() == 1
    for t in (points, xyz, scaling, grad_xyz, grad_scaling):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32)
    assert sel.is_cuda and sel.is_contiguous()
    for g in (grad_xyz, grad_scaling):
        assert g is None or g.shape == (P, 3)
    nbytes = int(lib().gsr_similarity_loss_workspace(m, n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xyz.device)
    out3 = torch.empty(3, dtype=torch.float32, device=xyz.device)
    _check(lib().gsr_similarity_loss(P, m, n, _ptr(points), _ptr(sel), _ptr(xyz), _ptr(scaling), float(lambda_),
                                     _ptr(out3), _ptr(grad_xyz), _ptr(grad_scaling), int(bool(accumulate)), _ptr(ws),
                                     nbytes, _stream()))
    return out3


def surfel_plane_loss(points, sel, xyz, scaling, rotation, lambda_, huber=0.0, max_dist=float("inf"), lambda_flat=0.0,
                      grad_xyz=None, grad_scaling=None, grad_rotation=None, accumulate=False):
    """The point-to-plane loss of LiDAR points against the thinnest axis of their nearest selected Gaussian, plus the
    flatness prior, in three launches (include/gsraster.h, gsr_surfel_plane_loss).  points [m,3] f32, sel [n] int32
    (ascending, unique, < P), xyz / scaling [P,3] and rotation [P,4] f32 (scaling and rotation ACTIVATED), all on the
    device.  grad_xyz / grad_scaling [P,3], grad_rotation [P,4]: buffers whose selected rows are written
    (accumulate=False) or added to (accumulate=True); None = not wanted.  Returns out4 = [loss, mean rho, mean
    thinnest scale, share of points inside max_dist] (device tensor)."""
    P, m, n = int(xyz.size(0)), int(points.size(0)), int(sel.size(0))
    assert xyz.is_cuda and xyz.shape == (P, 3) and scaling.shape == (P, 3) and rotation.shape == (P, 4)
    assert points.shape == (m, 3) and sel.dtype == torch.int32 and sel.dim() == 1
    for t in (points, xyz, scaling, rotation, grad_xyz, grad_scaling, grad_rotation):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32)
    assert sel.is_cuda and sel.is_contiguous()
    for g, width in ((grad_xyz, 3), (grad_scaling, 3), (grad_rotation, 4)):
        assert g is None or g.shape == (P, width)
    nbytes = int(lib().gsr_surfel_plane_loss_workspace(m, n))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=xyz.device)
    out4 = torch.empty(4, dtype=torch.float32, device=xyz.device)
    _check(lib().gsr_surfel_plane_loss(P, m, n, _ptr(points), _ptr(sel), _ptr(xyz), _ptr(scaling), _ptr(rotation),
                                       float(lambda_), float(huber), float(max_dist), float(lambda_flat), _ptr(out4),
                                       _ptr(grad_xyz), _ptr(grad_scaling), _ptr(grad_rotation),
                                       int(bool(accumulate)), _ptr(ws), nbytes, _stream()))
    return out4


def _host_floats(m, n):
    """n floats of a small host matrix (tensor, array or nested list) as a ctypes array, row-major."""
    t = torch.as_tensor(m, dtype=torch.float64).reshape(-1)
    assert t.numel() == n, "expected %d elements" % n
    return (C.c_float * n)(*[float(x) for x in t.tolist()])


def delta_depth_loss(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel, lambda_, want_warped=False,
                     want_grad_src=True, want_grad_ref=True):
    """The delta-depth term of a keyframe pair in four launches (include/gsraster.h, gsr_delta_depth_loss).
    depth_* / acc_*: [H,W] or [1,H,W] f32 on the device; inv_K_src, K_ref (3x3) and T_rel (3x4 or 4x4, loss.delta_pose)
    on the host.  Returns (out3 = [loss, mean gap, share of unmasked pixels] device tensor, warped or None,
    dL/ddepth_src or None, dL/ddepth_ref or None), the images shaped like depth_src."""
    H, W = int(depth_src.shape[-2]), int(depth_src.shape[-1])
    for t in (depth_src, acc_src, depth_ref, acc_ref):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == H * W
    T = torch.as_tensor(T_rel, dtype=torch.float64).reshape(-1, 4)[:3]
    kin, kref, trel = _host_floats(inv_K_src, 9), _host_floats(K_ref, 9), _host_floats(T, 12)
    nbytes = int(lib().gsr_delta_depth_loss_workspace(H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=depth_src.device)
    out3 = torch.empty(3, dtype=torch.float32, device=depth_src.device)
    warped = torch.empty_like(depth_src) if want_warped else None
    gs = torch.empty_like(depth_src) if want_grad_src else None
    gr = torch.empty_like(depth_ref) if want_grad_ref else None
    _check(lib().gsr_delta_depth_loss(H, W, _ptr(depth_src), _ptr(acc_src), _ptr(depth_ref), _ptr(acc_ref), kin, kref,
                                      trel, float(lambda_), _ptr(out3), _ptr(warped), _ptr(gs), _ptr(gr), _ptr(ws),
                                      nbytes, _stream()))
    return out3, warped, gs, gr


def lidar_depth_image(points_world, T_cw, K, height, width, min_depth=0.2, max_depth=float("inf"), want_counts=False):
    """The z-buffer of a LiDAR sweep in a keyframe's view in three launches (include/gsraster.h,
    gsr_lidar_depth_image).  points_world: [n,3] f32 on the device (n == 0 is legal); T_cw (3x4 or 4x4, [R | t] with
    x_c = R x_w + t) and K (3x3) on the host.  Returns the [H,W] f32 image -- the smallest z per pixel, 0 where no
    point lands -- and, with want_counts, an int32 device tensor {points kept, pixels hit} beside it."""
    assert points_world.is_cuda and points_world.dtype == torch.float32 and points_world.is_contiguous()
    assert points_world.dim() == 2 and points_world.size(1) == 3
    n, H, W = int(points_world.size(0)), int(height), int(width)
    T = torch.as_tensor(T_cw, dtype=torch.float64).reshape(-1, 4)[:3]
    tcw, k9 = _host_floats(T, 12), _host_floats(K, 9)
    dev = points_world.device
    image = torch.empty((max(H, 0), max(W, 0)), dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev) if want_counts else None
    _check(lib().gsr_lidar_depth_image(n, _ptr(points_world), tcw, k9, H, W, float(min_depth), float(max_depth),
                                       _ptr(image), _ptr(counts), _stream()))
    return (image, counts) if want_counts else image


def lidar_depth_loss(depth, acc, lidar_depth, acc_min, lambda_, want_grad_depth=True, want_grad_acc=True):
    """The masked depth L1 of a render against a LiDAR depth image in three launches (include/gsraster.h,
    gsr_lidar_depth_loss).  depth / acc: the rasterizer's second and third outputs, [H,W] or [1,H,W] f32 on the device;
    lidar_depth: what lidar_depth_image returns.  Returns (out3 = [loss, mean |depth error| in metres, supervised
    share] device tensor, dL/ddepth or None, dL/dacc or None), the gradients shaped like depth and acc."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    for t in (depth, acc, lidar_depth):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == H * W
    nbytes = int(lib().gsr_lidar_depth_loss_workspace(H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=depth.device)
    out3 = torch.empty(3, dtype=torch.float32, device=depth.device)
    gd = torch.empty_like(depth) if want_grad_depth else None
    ga = torch.empty_like(acc) if want_grad_acc else None
    _check(lib().gsr_lidar_depth_loss(H, W, _ptr(depth), _ptr(acc), _ptr(lidar_depth), float(acc_min), float(lambda_),
                                      _ptr(out3), _ptr(gd), _ptr(ga), _ptr(ws), nbytes, _stream()))
    return out3, gd, ga


def lidar_occlusion_filter(lidar_depth, radius, tol, want_counts=False):
    """The occlusion filter of a LiDAR depth image in one launch (include/gsraster.h, gsr_lidar_occlusion_filter).
    lidar_depth: [H,W] or [1,H,W] f32 on the device.  Returns a new image of the same shape -- the input's bits, or 0
    where the pixel is empty or a return nearer by more than tol * z lies within radius pixels -- and, with
    want_counts, an int32 device tensor {pixels kept, pixels removed} beside it."""
    assert lidar_depth.is_cuda and lidar_depth.dtype == torch.float32 and lidar_depth.is_contiguous()
    assert lidar_depth.dim() >= 2
    H, W = int(lidar_depth.shape[-2]), int(lidar_depth.shape[-1])
    assert lidar_depth.numel() == H * W
    out = torch.empty_like(lidar_depth)
    counts = torch.empty(2, dtype=torch.int32, device=lidar_depth.device) if want_counts else None
    _check(lib().gsr_lidar_occlusion_filter(H, W, _ptr(lidar_depth), int(radius), float(tol), _ptr(out), _ptr(counts),
                                            _stream()))
    return (out, counts) if want_counts else out


def lidar_depth_loss_robust(depth, acc, lidar_depth, acc_min, lambda_, huber_abs, huber_rel, clip_abs, clip_rel,
                            want_grad_depth=True, want_grad_acc=True, out4=None):
    """The depth loss with a Huber residual and a clip in three launches (include/gsraster.h,
    gsr_lidar_depth_loss_robust); the operands of lidar_depth_loss.  Returns (out4 = [loss, mean |depth error| in
    metres over the supervised pixels, supervised share, clipped share] device tensor, dL/ddepth or None, dL/dacc or
    None).  out4: a contiguous f32 [4] device view to write into (a row of a caller's result buffer)."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    for t in (depth, acc, lidar_depth):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == H * W
    nbytes = int(lib().gsr_lidar_depth_loss_robust_workspace(H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=depth.device)
    if out4 is None:
        out4 = torch.empty(4, dtype=torch.float32, device=depth.device)
    assert out4.is_cuda and out4.is_contiguous() and out4.dtype == torch.float32 and out4.numel() == 4
    gd = torch.empty_like(depth) if want_grad_depth else None
    ga = torch.empty_like(acc) if want_grad_acc else None
    _check(lib().gsr_lidar_depth_loss_robust(H, W, _ptr(depth), _ptr(acc), _ptr(lidar_depth), float(acc_min),
                                             float(lambda_), float(huber_abs), float(huber_rel), float(clip_abs),
                                             float(clip_rel), _ptr(out4), _ptr(gd), _ptr(ga), _ptr(ws), nbytes,
                                             _stream()))
    return out4, gd, ga


def sweep_admit(points_world, T_cw, K, height, width, depth_tol, occlusion_tol, depth=None, acc=None, image=None,
                lidar_depth=None, covs=None, exposure=None, acc_min=0.5, occlusion_radius=1, footprint=1.0,
                min_depth=0.2, max_depth=float("inf"), one_per_pixel=True, want_reasons=False, out=None, workspace=None):
    """Sweep admission in five launches (include/gsraster.h, gsr_sweep_admit).  points_world: [n,3] f32 on the device
    (n == 0 is legal); T_cw (3x4 or 4x4) and K (3x3) on the host; depth / acc / lidar_depth: [H,W] or [1,H,W]; image:
    [3,H,W]; covs: [n,3,3] or [n,9]; exposure: [3,2] rows (g, b); all f32 on the device or None.  out: a dict of
    contiguous device tensors of max(n, 1) rows to write (xyz [n,3], covs [n,9], rgb [n,3], index, pixel int32 [n], z [n]) or
    None = new ones; workspace: a uint8 device tensor of at least the queried size or None.  No host wait.  Returns
    (the dict with FULL-length outputs -- rows at and behind counts[0] are not written -- counts int32 [6] on the
    device, reasons uint8 [n] or None)."""
    assert points_world.is_cuda and points_world.dtype == torch.float32 and points_world.is_contiguous()
    assert points_world.dim() == 2 and points_world.size(1) == 3
    n, H, W = int(points_world.size(0)), int(height), int(width)
    dev = points_world.device
    T = torch.as_tensor(T_cw, dtype=torch.float64).reshape(-1, 4)[:3]
    tcw, k9 = _host_floats(T, 12), _host_floats(K, 9)
    for t in (depth, acc, lidar_depth):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == H * W)
    assert image is None or (image.is_cuda and image.is_contiguous() and image.dtype == torch.float32
                             and tuple(image.shape) == (3, H, W))
    assert covs is None or (covs.is_cuda and covs.is_contiguous() and covs.dtype == torch.float32
                            and covs.numel() == 9 * n)
    assert exposure is None or (exposure.is_cuda and exposure.is_contiguous() and exposure.dtype == torch.float32
                                and tuple(exposure.shape) == (3, 2))
    if out is None:
        r = max(n, 1)   # (at least one row: the library refuses a null output even when n == 0)
        out = dict(xyz=torch.empty((r, 3), dtype=torch.float32, device=dev),
                   covs=torch.empty((r, 9), dtype=torch.float32, device=dev),
                   rgb=torch.empty((r, 3), dtype=torch.float32, device=dev) if image is not None else None,
                   index=torch.empty(r, dtype=torch.int32, device=dev),
                   pixel=torch.empty(r, dtype=torch.int32, device=dev),
                   z=torch.empty(r, dtype=torch.float32, device=dev))
    nbytes = int(lib().gsr_sweep_admit_workspace(n, H, W))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(6, dtype=torch.int32, device=dev)
    reasons = torch.empty(n, dtype=torch.uint8, device=dev) if want_reasons else None
    _check(lib().gsr_sweep_admit(n, _ptr(points_world), _ptr(covs), tcw, k9, H, W, float(min_depth), float(max_depth),
                                 _ptr(depth), _ptr(acc), float(acc_min), float(depth_tol), _ptr(lidar_depth),
                                 int(occlusion_radius), float(occlusion_tol), _ptr(image), _ptr(exposure),
                                 float(footprint), int(bool(one_per_pixel)), _out_ptr(out["xyz"]), _out_ptr(out["covs"]),
                                 _out_ptr(out.get("rgb")), _out_ptr(out["index"]), _out_ptr(out.get("pixel")),
                                 _out_ptr(out.get("z")), _ptr(reasons), C.c_void_p(counts.data_ptr()),
                                 C.c_void_p(workspace.data_ptr()) if nbytes else None, min(nbytes, workspace.numel()),
                                 _stream()))
    return out, counts, reasons


def _out_ptr(t):
    """Device pointer of an output of sweep_admit (None -> NULL)."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


def voxel_table(capacity, device):
    """A zeroed voxel table of `capacity` slots (a power of two): int64 [capacity, 16] on `device`."""
    nbytes = int(lib().gsr_voxel_table_bytes(int(capacity)))
    if nbytes == 0:
        raise GsrError("voxel_table: capacity %r is not a power of two up to 2^26" % (capacity,))
    return torch.zeros((nbytes // 128, 16), dtype=torch.int64, device=device)


def voxel_sweep(points, colors, grid, min_points, min_sigma, scale_factor, table, live_before, out=None,
                workspace=None):
    """One sweep into the voxel table in four launches (include/gsraster.h, gsr_voxel_sweep).  points: [n,3] f32 on the
    device (n == 0 is legal); colors: [n,3] f32 (0..255) or None; table: int64 [capacity,16] (voxel_table), changed in
    place; live_before: the live keys the previous call reported.  out: a dict of contiguous device tensors of max(n, 1)
    rows to write (status uint8 [n], point_keys int64 [n], xyz [n,3], covs [n,9], rgb [n,3], keys int64 [n], points
    int32 [n], scaling [n,3], rotation [n,4], normal [n,3]) or None = new ones.  No host wait.  Returns (the dict with
    FULL-length outputs -- seed rows at and behind counts[4] are not written -- and counts int32 [6] on the device)."""
    assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous()
    assert points.dim() == 2 and points.size(1) == 3
    n, dev = int(points.size(0)), points.device
    assert colors is None or (colors.is_cuda and colors.is_contiguous() and colors.dtype == torch.float32
                              and tuple(colors.shape) == (n, 3))
    assert table.is_cuda and table.is_contiguous() and table.dtype == torch.int64 and table.dim() == 2 \
        and table.size(1) == 16
    if out is None:
        r = max(n, 1)
        f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        out = dict(status=torch.empty(r, dtype=torch.uint8, device=dev),
                   point_keys=torch.empty(r, dtype=torch.int64, device=dev), xyz=f(r, 3), covs=f(r, 9),
                   rgb=f(r, 3) if colors is not None else None, keys=torch.empty(r, dtype=torch.int64, device=dev),
                   points=torch.empty(r, dtype=torch.int32, device=dev), scaling=f(r, 3), rotation=f(r, 4),
                   normal=f(r, 3))
    nbytes = int(lib().gsr_voxel_sweep_workspace(n))
    if workspace is None:
        workspace = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(6, dtype=torch.int32, device=dev)
    _check(lib().gsr_voxel_sweep(n, _ptr(points), _ptr(colors), float(grid), int(min_points), float(min_sigma),
                                 float(scale_factor), C.c_void_p(table.data_ptr()), int(table.size(0)),
                                 int(live_before), _out_ptr(out["status"]), _out_ptr(out["point_keys"]),
                                 _out_ptr(out["xyz"]), _out_ptr(out["covs"]), _out_ptr(out.get("rgb")),
                                 _out_ptr(out["keys"]), _out_ptr(out["points"]), _out_ptr(out["scaling"]),
                                 _out_ptr(out["rotation"]), _out_ptr(out["normal"]), C.c_void_p(counts.data_ptr()),
                                 C.c_void_p(workspace.data_ptr()) if nbytes else None, min(nbytes, workspace.numel()),
                                 _stream()))
    return out, counts


def voxel_rehash(src, dst):
    """Every record of the voxel table src into the zeroed, not smaller table dst (gsr_voxel_rehash): one launch."""
    for t in (src, dst):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and t.dim() == 2 and t.size(1) == 16
    _check(lib().gsr_voxel_rehash(C.c_void_p(src.data_ptr()), int(src.size(0)), C.c_void_p(dst.data_ptr()),
                                  int(dst.size(0)), _stream()))
    return dst


def image_metrics(img, gt, window11, out=None, totals=None):
    """{psnr, ssim, l1, mse} of img against gt ([C,H,W] f32 on the device) in two launches (include/gsraster.h,
    gsr_image_metrics).  out: a contiguous device f32 [4] to write (a row of a larger tensor); totals: a device float64
    [4] the call adds {psnr, ssim, l1, 1} to.  Returns out (a new tensor when none is given)."""
    assert img.dim() == 3 and img.shape == gt.shape and img.is_cuda and img.dtype == torch.float32 == gt.dtype
    Cn, H, W = (int(x) for x in img.shape)
    img, gt = img.contiguous(), gt.contiguous()
    if out is None:
        out = torch.empty(4, dtype=torch.float32, device=img.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.numel() == 4 and out.is_contiguous()
    if totals is not None:
        assert totals.is_cuda and totals.dtype == torch.float64 and totals.numel() == 4 and totals.is_contiguous()
    nbytes = int(lib().gsr_image_metrics_workspace(Cn, H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=img.device)
    win = (C.c_float * 11)(*[float(x) for x in window11])
    _check(lib().gsr_image_metrics(Cn, H, W, _ptr(img), _ptr(gt), win, _ptr(out), _ptr(totals), _ptr(ws), nbytes,
                                   _stream()))
    return out


def _rows_u8(out, shape, dev):
    """(out, pitch): `out` -- a uint8 device tensor of `shape` whose elements of a row are adjacent, e.g. a column slice
    of a wider image -- or a new one."""
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != tuple(shape):
        raise ValueError("out must be a uint8 tensor of shape %s on the device of the image" % (tuple(shape),))
    row = shape[1] * (shape[2] if len(shape) == 3 else 1)   # bytes of a row
    want = (None, shape[2], 1) if len(shape) == 3 else (None, 1)
    pitch = int(out.stride(0)) if shape[0] > 1 else row
    if any(shape[d] > 1 and out.stride(d) != want[d] for d in range(1, len(shape))) or pitch < row:
        raise ValueError("out: the bytes of a row must be adjacent and rows must not overlap")
    return out, pitch


def pack_image_u8(img, bgr=True, out=None):
    """[3,H,W] f32 -> interleaved uint8 [H,W,3] (include/gsraster.h, gsr_pack_image_u8), written into `out` if given."""
    assert img.dim() == 3 and img.size(0) == 3 and img.is_cuda and img.dtype == torch.float32
    H, W = int(img.size(1)), int(img.size(2))
    img = img.contiguous()
    out, pitch = _rows_u8(out, (H, W, 3), img.device)
    _check(lib().gsr_pack_image_u8(H, W, _ptr(img), int(bool(bgr)), C.c_void_p(out.data_ptr()), pitch, _stream()))
    return out


def pack_depth_u8(depth, max_depth, out=None):
    """[H,W] or [1,H,W] f32 -> uint8 [H,W] (include/gsraster.h, gsr_pack_depth_u8), written into `out` if given."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    assert depth.is_cuda and depth.dtype == torch.float32 and depth.numel() == H * W
    depth = depth.contiguous()
    out, pitch = _rows_u8(out, (H, W), depth.device)
    _check(lib().gsr_pack_depth_u8(H, W, _ptr(depth), float(max_depth), C.c_void_p(out.data_ptr()), pitch, _stream()))
    return out


# ---- "next" row 4: map growth and PLY export (include/gsraster.h; csrc/growth.hip) ----
def init_gaussians(xyz, covs, rgbs, scale_factor, out_xyz, out_features_dc, out_features_rest, out_scaling,
                   out_rotation, out_opacity):
    """GaussianModel::addNewPointcloud's arithmetic (src/gs/gaussian.cu:241-313) for n new points, written in
    place into the given (contiguous, n-row) output views -- normally the tail rows of capacity buffers."""
    n = int(xyz.size(0))
    M = 1 + (int(out_features_rest.size(1)) if out_features_rest is not None and out_features_rest.numel() else 0)
    for t in (xyz, covs, rgbs, out_xyz, out_features_dc, out_scaling, out_rotation, out_opacity):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
    assert covs.shape == (n, 3, 3) and rgbs.shape == (n, 3)
    _check(lib().gsr_init_gaussians(n, M, _ptr(xyz), _ptr(covs), _ptr(rgbs), float(scale_factor), _ptr(out_xyz),
                                    _ptr(out_features_dc), _ptr(out_features_rest), _ptr(out_scaling),
                                    _ptr(out_rotation), _ptr(out_opacity), _stream()))


def pack_ply_rows(xyz, features_dc, features_rest, opacity, scaling, rotation):
    """[P, 14 + 3M] f32 device tensor: the vertex rows of the reference's PLY export (one coalesced pass)."""
    P = int(xyz.size(0))
    M = 1 + (int(features_rest.size(1)) if features_rest is not None and features_rest.numel() else 0)
    rf = int(lib().gsr_ply_row_floats(M))
    rows = torch.empty((P, rf), dtype=torch.float32, device=xyz.device)
    args = [t.contiguous() for t in (xyz, features_dc, features_rest, opacity, scaling, rotation)]
    _check(lib().gsr_pack_ply_rows(P, M, *[_ptr(t) for t in args], _ptr(rows), _stream()))
    return rows


def model_step(params6, exp_avg6, exp_avg_sq6, g_xyz, g_scales, g_rot, g_opac, g_shs, lrs6, beta1, beta2, eps, step,
               want_activated=True):
    """Chain rule of the activations + Adam on the six groups + activations of the updated parameters, one launch
    (include/gsraster.h, gsr_model_step).  params6 in the order xyz, features_dc, features_rest, scaling, rotation,
    opacity.  Returns (scales, rotations, opacities [P,1], shs) of the UPDATED model, or None."""
    xyz, fdc, frest = params6[0], params6[1], params6[2]
    P = int(xyz.size(0))
    M = 1 + (int(frest.size(1)) if frest.numel() else 0)
    for t in list(params6) + list(exp_avg6) + list(exp_avg_sq6) + [g_xyz, g_scales, g_rot, g_opac, g_shs]:
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
    outs = None
    if want_activated:
        f32 = dict(dtype=torch.float32, device=xyz.device)
        outs = (torch.empty((P, 3), **f32), torch.empty((P, 4), **f32), torch.empty((P, 1), **f32),
                torch.empty((P, M, 3), **f32))
    VP = C.c_void_p * 6
    arr = lambda ts: VP(*[t.data_ptr() if t.numel() else None for t in ts])  # noqa: E731
    lr = (C.c_float * 6)(*[float(x) for x in lrs6])
    o = outs if outs is not None else (None, None, None, None)
    _check(lib().gsr_model_step(P, M, arr(params6), arr(exp_avg6), arr(exp_avg_sq6), _ptr(g_xyz), _ptr(g_scales),
                                _ptr(g_rot), _ptr(g_opac), _ptr(g_shs), _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _ptr(o[3]), lr,
                                float(beta1), float(beta2), float(eps), int(step), _stream()))
    return outs


# ---- in-place pruning (include/gsraster.h; csrc/prune.hip) ----
def prune_mark(xyz, scaling_raw, rotation_raw, opacity_raw, min_opacity=1.0 / 255.0, max_scale=0.3,
               drop_nonfinite=True, drop=None, packed=False):
    """The drop rule and the row map of the stable compaction, three launches (include/gsraster.h, gsr_prune_mark).
    The raw leaves [P,3], [P,3], [P,4], [P,1] on the device; drop: an optional [P] bool / uint8 mask of the caller's.
    Returns (reasons [P] uint8, row_map [P+1] int32, counts [5] int32 = {P', opacity, scale, non-finite, mask}),
    device tensors; nothing waits for the device.  row_map and counts are views of ONE int32 [P+6] buffer, which
    packed=True appends to the result: a host that wants both fetches them with one copy."""
    P = int(xyz.size(0))
    dev = xyz.device
    for t in (xyz, scaling_raw, rotation_raw, opacity_raw):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and int(t.size(0)) == P
    if drop is not None:
        if drop.dtype == torch.bool:
            drop = drop.view(torch.uint8)
        assert drop.is_cuda and drop.is_contiguous() and drop.dtype == torch.uint8 and drop.numel() == P
    reasons = torch.empty((P,), dtype=torch.uint8, device=dev)
    both = torch.empty((P + 6,), dtype=torch.int32, device=dev)
    row_map, counts = both[:P + 1], both[P + 1:]
    nbytes = int(lib().gsr_prune_workspace(P))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _check(lib().gsr_prune_mark(P, _ptr(xyz), _ptr(scaling_raw), _ptr(rotation_raw), _ptr(opacity_raw), _ptr(drop),
                                float(min_opacity), float(max_scale), int(bool(drop_nonfinite)), _ptr(reasons),
                                C.c_void_p(row_map.data_ptr()), C.c_void_p(counts.data_ptr()), _ptr(ws), nbytes,
                                _stream()))
    return (reasons, row_map, counts, both) if packed else (reasons, row_map, counts)


def prune_compact(src, dst, reasons, row_map):
    """dst[k][row_map[i]] = src[k][i] for the rows with reasons[i] == 0, up to 18 tensors in ONE launch
    (include/gsraster.h, gsr_prune_compact).  src[k]: [P, ...] f32; dst[k]: a buffer of its own with the same row shape
    and at least row_map[P] rows, whose further rows are not written."""
    n = len(src)
    assert n == len(dst)
    P = int(reasons.numel())
    widths = []
    for s, d in zip(src, dst):
        assert s.is_cuda and s.is_contiguous() and s.dtype == torch.float32 and int(s.size(0)) == P
        assert d.is_cuda and d.is_contiguous() and d.dtype == torch.float32 and d.shape[1:] == s.shape[1:]
        assert s.numel() == 0 or d.numel() == 0 or s.data_ptr() != d.data_ptr()
        widths.append(int(s[0].numel()) if P else 0)
    assert reasons.is_cuda and reasons.dtype == torch.uint8 and reasons.is_contiguous()
    assert row_map.is_cuda and row_map.dtype == torch.int32 and row_map.is_contiguous() and row_map.numel() == P + 1
    VP = C.c_void_p * max(n, 1)
    arr = lambda ts: VP(*[t.data_ptr() if t.numel() else None for t in ts])  # noqa: E731
    _check(lib().gsr_prune_compact(P, n, arr(src), arr(dst), (C.c_int * max(n, 1))(*widths), _ptr(reasons),
                                   C.c_void_p(row_map.data_ptr()), _stream()))


# ---- per-Gaussian blend contribution (include/gsraster.h; csrc/contrib.hip, the walk in csrc/render.hip) ----
def contribution_rows(P, R, W, H, geomBuffer, binningBuffer, imageBuffer, out=None):
    """The integer frame rows of a completed forward, the zero fill plus one launch (gsr_contribution): [P, 2] int64 on
    the device, row i = {wsum_fx, pixels | wmax_bits << 32}.  R: what rasterize_forward returned (its key is used).
    out: a contiguous int64 device tensor [P, 2] to write instead of a new one."""
    P = int(P)
    if out is None:
        out = torch.empty((P, 2), dtype=torch.int64, device=geomBuffer.device)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.numel() == 2 * P
    _check(lib().gsr_contribution(P, _key(R), int(W), int(H), _ptr(geomBuffer), _ptr(binningBuffer), _ptr(imageBuffer),
                                  _ptr(out), _stream()))
    return out


def contribution_finish(rows, min_pixels=1, min_weight=0.0, n_touched=None, weight_sum=None, weight_max=None,
                        mask=None, stats=None):
    """One launch over the frame rows (gsr_contribution_finish): writes the given outputs -- n_touched [P] int32,
    weight_sum / weight_max [P] f32, mask [P] uint8, contiguous device tensors -- and folds the view into
    stats [P, 3] f32 = {weight_sum_total, views, weight_max} in place; None = not wanted."""
    P = int(rows.numel()) // 2
    assert rows.is_cuda and rows.dtype == torch.int64 and rows.is_contiguous()
    for t, dt, n in ((n_touched, torch.int32, P), (weight_sum, torch.float32, P), (weight_max, torch.float32, P),
                     (mask, torch.uint8, P), (stats, torch.float32, 3 * P)):
        assert t is None or (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == n)
    _check(lib().gsr_contribution_finish(P, _ptr(rows), int(min_pixels), float(min_weight), _ptr(n_touched),
                                         _ptr(weight_sum), _ptr(weight_max), _ptr(mask), _ptr(stats), _stream()))


# ---- rendered normal maps and the depth-normal consistency loss (include/gsraster.h; csrc/normal.hip) ----
def blend_attributes(P, R, W, H, attributes, geomBuffer, binningBuffer, imageBuffer, out=None):
    """Per-Gaussian attributes blended into an image behind a completed forward, one launch (gsr_blend_attributes; the
    walk is csrc/render.hip's k_attribute_tile).  attributes: [P, C] (or [P], C = 1) f32 on the device, C in 1..4.
    R: what rasterize_forward returned (its key is used).  out: a contiguous f32 device tensor of C * H * W elements to
    write instead of a new one.  Returns [C, H, W]."""
    P, W, H = int(P), int(W), int(H)
    assert attributes.is_cuda and attributes.is_contiguous() and attributes.dtype == torch.float32
    assert attributes.dim() in (1, 2) and int(attributes.shape[0]) == P
    ch = int(attributes.shape[1]) if attributes.dim() == 2 else 1
    if out is None:
        out = torch.empty((ch, H, W), dtype=torch.float32, device=attributes.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == ch * H * W
    _check(lib().gsr_blend_attributes(P, _key(R), W, H, ch, _ptr(attributes), _ptr(geomBuffer), _ptr(binningBuffer),
                                      _ptr(imageBuffer), _ptr(out), _stream()))
    return out


def surfel_normals(xyz, scaling, rotation, T_cw, out=None):
    """Camera-facing normals of the surfels' thin axes, one launch (gsr_surfel_normals).  xyz, scaling [P,3] and
    rotation [P,4]: the ACTIVATED values, f32 on the device; T_cw: [R | t] (3x4 or 4x4) on the host.  Returns [P,3]."""
    P = int(xyz.shape[0])
    for t, w in ((xyz, 3), (scaling, 3), (rotation, 4)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (P, w)
    if out is None:
        out = torch.empty((P, 3), dtype=torch.float32, device=xyz.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == 3 * P
    tcw = (C.c_float * 12)(*[float(v) for v in torch.as_tensor(T_cw).detach().cpu().double()[:3, :4].reshape(-1)])
    _check(lib().gsr_surfel_normals(P, _ptr(xyz), _ptr(scaling), _ptr(rotation), tcw, _ptr(out), _stream()))
    return out


def normal_consistency_loss(depth, acc, normals, fx, fy, cx, cy, acc_min, normal_min, jump_rel, lambda_,
                            want_grad_depth=True, want_grad_acc=True):
    """The depth-normal consistency loss in three launches, two without gradients (include/gsraster.h,
    gsr_normal_consistency_loss).  depth / acc: the rasterizer's second and third outputs, [H,W] or [1,H,W] f32 on the
    device; normals: [3,H,W], un-normalised.  Returns (out3 = [loss, mean rho, supervised share] device tensor,
    dL/ddepth or None, dL/dacc or None), the gradients shaped like depth and acc."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    for t, n in ((depth, H * W), (acc, H * W), (normals, 3 * H * W)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and t.numel() == n
    nbytes = int(lib().gsr_normal_consistency_workspace(H, W))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=depth.device)
    out3 = torch.empty(3, dtype=torch.float32, device=depth.device)
    gd = torch.empty_like(depth) if want_grad_depth else None
    ga = torch.empty_like(acc) if want_grad_acc else None
    _check(lib().gsr_normal_consistency_loss(H, W, _ptr(depth), _ptr(acc), _ptr(normals), float(fx), float(fy),
                                             float(cx), float(cy), float(acc_min), float(normal_min), float(jump_rel),
                                             float(lambda_), _ptr(out3), _ptr(gd), _ptr(ga), _ptr(ws), nbytes,
                                             _stream()))
    return out3, gd, ga


# ---- adaptive density control (include/gsraster.h; csrc/densify.hip) ----
def density_accumulate(radii, dL_dmean2D, stats):
    """One view's statistics, one launch (include/gsraster.h, gsr_density_accumulate): radii [P] int32 (the forward's),
    dL_dmean2D [P,3] f32 (the backward's, unscaled), stats [P,3] f32 = {grad_sum, views, max_radius}, updated in place
    for the visible rows with a finite gradient norm."""
    P = int(radii.numel())
    assert radii.is_cuda and radii.is_contiguous() and radii.dtype == torch.int32
    assert dL_dmean2D.is_cuda and dL_dmean2D.is_contiguous() and dL_dmean2D.dtype == torch.float32
    assert stats.is_cuda and stats.is_contiguous() and stats.dtype == torch.float32
    assert tuple(dL_dmean2D.shape) == (P, 3) and tuple(stats.shape) == (P, 3)
    _check(lib().gsr_density_accumulate(P, _ptr(radii), _ptr(dL_dmean2D), _ptr(stats), _stream()))


def densify_mark(stats, scaling_raw, grad_threshold, size_threshold, max_new=None, packed=False):
    """The clone / split rule, three launches (include/gsraster.h, gsr_densify_mark).  stats / scaling_raw: [P,3] f32.
    Returns (kinds [P] uint8: 0 none, 1 clone, 2 split; offsets [P+1] int32; counts [3] int32 = {n_new, clones,
    splits}), device tensors; nothing waits for the device.  offsets and counts are views of ONE int32 [P+4] buffer,
    which packed=True appends to the result."""
    P = int(stats.size(0))
    dev = stats.device
    for t in (stats, scaling_raw):
        assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape) == (P, 3)
    kinds = torch.empty((P,), dtype=torch.uint8, device=dev)
    both = torch.empty((P + 4,), dtype=torch.int32, device=dev)
    offsets, counts = both[:P + 1], both[P + 1:]
    nbytes = int(lib().gsr_densify_workspace(P))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _check(lib().gsr_densify_mark(P, _ptr(stats), _ptr(scaling_raw), float(grad_threshold), float(size_threshold),
                                  -1 if max_new is None else int(max_new), _ptr(kinds),
                                  C.c_void_p(offsets.data_ptr()), C.c_void_p(counts.data_ptr()), _ptr(ws), nbytes,
                                  _stream()))
    return (kinds, offsets, counts, both) if packed else (kinds, offsets, counts)


def densify_apply(P, n_new, kinds, offsets, seed, params6, exp_avg6=None, exp_avg_sq6=None, stats=None):
    """Clone and split in place, one launch (include/gsraster.h, gsr_densify_apply).  params6: the six raw leaves in
    the order xyz, features_dc, features_rest, scaling, rotation, opacity as CAPACITY buffers of at least P + n_new
    rows; exp_avg6 / exp_avg_sq6 (six buffers each, or None) and stats ([., 3] or None) likewise."""
    P, n_new = int(P), int(n_new)
    frest = params6[2]
    M = 1 + (int(frest.size(1)) if frest.numel() else 0)
    groups = [params6] + [g for g in (exp_avg6, exp_avg_sq6) if g is not None]
    for g in groups:
        assert len(g) == 6
        for t in g:
            assert t.is_cuda and t.is_contiguous() and t.dtype == torch.float32
            assert t.numel() == 0 or int(t.size(0)) >= P + n_new, "densify_apply: a buffer holds fewer than P + n_new rows"
    if stats is not None:
        assert stats.is_cuda and stats.is_contiguous() and stats.dtype == torch.float32
        assert stats.dim() == 2 and stats.size(1) == 3 and int(stats.size(0)) >= P + n_new
    assert kinds.is_cuda and kinds.dtype == torch.uint8 and kinds.is_contiguous() and kinds.numel() == P
    assert offsets.is_cuda and offsets.dtype == torch.int32 and offsets.is_contiguous() and offsets.numel() == P + 1
    VP = C.c_void_p * 6
    arr = lambda ts: None if ts is None else VP(*[t.data_ptr() if t.numel() else None for t in ts])  # noqa: E731
    _check(lib().gsr_densify_apply(P, M, n_new, _ptr(kinds), C.c_void_p(offsets.data_ptr()),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, *[_ptr(t) for t in params6], arr(exp_avg6),
                                   arr(exp_avg_sq6), _ptr(stats), _stream()))
