// gsr_torch_next.hpp -- C++/LibTorch hosts of the rows either side of the rasterizer (SURVEY.md 8(f) "next" rows 1, 2
// and 4), for GS-LIVM's own translation units: what src/liw/lioOptimization.cpp and src/gs/gaussian.cu call instead of
// the Torch-op sequences they run today.  Definitions: torch_next.cpp (plain C++, links libgsraster_hip.so through the
// C ABI of include/gsraster.h).  The reference has no declarations for these -- its versions are header-inline Torch
// code (loss_utils.cuh) or private members of GaussianModel -- so this header is what a maintainer includes;
// INTEGRATION.md section 3 shows the call sites.  oracle/ref_link/caller.cpp odr-uses every entry point next to the
// reference's own headers (`make -C oracle ref_link`).
#pragma once
#include <torch/torch.h>

#include <cstddef>
#include <cstdint>
#include <array>
#include <limits>
#include <string>
#include <tuple>
#include <unordered_map>
#include <utility>
#include <vector>

namespace gsr_torch {

// ---- row 2: photometric loss ------------------------------------------------------------------------------------
// gaussian_splatting::gaussian(window_size, sigma) (include/gs/gs/loss_utils.cuh:24-31), bug for bug: the exponent
// uses floor((x - window_size) / 2), so the window is not the centred Gaussian.  CPU f32 [window_size].
torch::Tensor reference_window_1d(int window_size = 11, float sigma = 1.5f);

// (1 - lambda_dssim) * l1_loss(image, gt) + lambda_dssim * (1 - ssim(image, gt, create_window(11, C), 11, C))
// (loss_utils.cuh:11-13, 43-70; src/liw/lioOptimization.cpp:1705-1710) as ONE autograd node on the fused kernels of
// csrc/loss.hip.  image, gt: [C, H, W] f32 on the device; gradient w.r.t. image only.  window1d: 11 taps (CPU or
// device), undefined = reference_window_1d().  Returns the 0-dim loss.
torch::Tensor photometric_loss(const torch::Tensor& image, const torch::Tensor& gt, float lambda_dssim = 0.2f,
                               const torch::Tensor& window1d = torch::Tensor());
// [loss, l1, ssim] of the same evaluation, no graph (the reference logs PSNR / SSIM every 50 iterations)
torch::Tensor photometric_loss_parts(const torch::Tensor& image, const torch::Tensor& gt, float lambda_dssim = 0.2f,
                                     const torch::Tensor& window1d = torch::Tensor());

// ---- per-keyframe exposure compensation (an extension; csrc/exposure.hip) -------------------------------------------
// photometric_loss on x' = g_c * image + b_c as ONE autograd node, the compensated image never reaching memory:
// exposure is [C,2] rows (g_c, b_c) or [2] shared by the channels (f32 on the device, typically a leaf per keyframe
// beside its pose leaf); log_gain reads column 0 as log g (exp on C numbers, in Torch).  Gradients w.r.t. image and
// exposure.  Returns the 0-dim loss.
// (Like image_metrics, these two are not part of the oracle/ref_link link check, which stays as it is.)
torch::Tensor exposure_photometric_loss(const torch::Tensor& image, const torch::Tensor& gt,
                                        const torch::Tensor& exposure, float lambda_dssim = 0.2f,
                                        const torch::Tensor& window1d = torch::Tensor(), bool log_gain = false);
// g_c * image + b_c (one fused multiply-add per element, no graph) for evaluation and export; out: a contiguous tensor
// of the image's shape to write (the image itself is allowed), undefined = a new one.
torch::Tensor apply_exposure(const torch::Tensor& image, const torch::Tensor& exposure,
                             const torch::Tensor& out = torch::Tensor());

// ---- the weighted photometric loss (an extension; csrc/weighted.hip) -------------------------------------------------
// photometric_loss / exposure_photometric_loss over the pixels that carry a measurement, as ONE autograd node:
// w = weights * [acc >= acc_min], L1, SSIM and the squared error weighted per pixel and divided by the weight sum.
// weights (finite, >= 0: an undistortion border, a sky or dynamic-object mask) and acc (e.g. the render's silhouette;
// detached, the gate has no gradient): [H,W] or [1,H,W] f32 on the device, undefined = absent.  exposure: as in
// exposure_photometric_loss, undefined = none.  The SSIM windows see the whole images: a zero weight does not shield a
// non-finite pixel from its neighbours.  Gradients w.r.t. image and exposure.  Returns the 0-dim loss.
// (Like image_metrics, these two are not part of the oracle/ref_link link check, which stays as it is.)
torch::Tensor weighted_photometric_loss(const torch::Tensor& image, const torch::Tensor& gt,
                                        const torch::Tensor& weights = torch::Tensor(),
                                        const torch::Tensor& acc = torch::Tensor(), float acc_min = 0.5f,
                                        const torch::Tensor& exposure = torch::Tensor(), float lambda_dssim = 0.2f,
                                        const torch::Tensor& window1d = torch::Tensor(), bool log_gain = false);
// [loss, l1, ssim, weight sum, mse, psnr] of the same evaluation, no graph
torch::Tensor weighted_photometric_loss_parts(const torch::Tensor& image, const torch::Tensor& gt,
                                              const torch::Tensor& weights = torch::Tensor(),
                                              const torch::Tensor& acc = torch::Tensor(), float acc_min = 0.5f,
                                              const torch::Tensor& exposure = torch::Tensor(),
                                              float lambda_dssim = 0.2f,
                                              const torch::Tensor& window1d = torch::Tensor(), bool log_gain = false);

// ---- the LiDAR similarity loss (optimize_vis step 3) ---------------------------------------------------------------
// lambda * compute_min_distance(points, Get_xyz()[sel], Get_scaling()[sel]) (src/gs/gaussian.cu:87-114, 230-237) as ONE
// autograd node on the kernels of csrc/simi.hip: points [m,3] f32 and sel [n] int32 (ascending unique rows) on the
// device, from VoxelIndex::select; xyz = the model's _xyz [P,3]; scaling = its ACTIVATED scales [P,3].  Gradients
// w.r.t. xyz and scaling, dense and zero outside the selection.  Returns the 0-dim loss.
torch::Tensor similarity_loss(const torch::Tensor& points, const torch::Tensor& sel, const torch::Tensor& xyz,
                              const torch::Tensor& scaling, float lambda = 0.2f);

// ---- the point-to-plane LiDAR loss on oriented surfels (an extension; csrc/surfel.hip) -------------------------------
// lambda * mean_i [d_i <= max_dist] rho(n_j . (p_i - xyz_j)) + lambda_flat * mean_j min_k scaling[j][k] as ONE autograd
// node: every point against the thinnest axis n_j (a column of R(rotation_j)) of its nearest selected Gaussian j; rho is
// |e| for huber = 0 and the Huber function otherwise (include/gsraster.h, gsr_surfel_plane_loss).  points, sel, xyz as
// similarity_loss; scaling [P,3] and rotation [P,4] ACTIVATED.  Gradients w.r.t. xyz, scaling and rotation, dense and
// zero outside the selection.  lambda has no default: the term has no reference value.  Returns the 0-dim loss.
torch::Tensor surfel_plane_loss(const torch::Tensor& points, const torch::Tensor& sel, const torch::Tensor& xyz,
                                const torch::Tensor& scaling, const torch::Tensor& rotation, float lambda,
                                float huber = 0.f, float max_dist = std::numeric_limits<float>::infinity(),
                                float lambda_flat = 0.f);

// ---- the delta-depth loss between a history keyframe and its successor (optimize_vis step 5) ------------------------
// The body of the loop at src/liw/lioOptimization.cpp:1780-1801 -- calcDeltaSimi (src/gs/gaussian.cu:116-199), the two
// inv_depth, the masks, lambda * mean -- as ONE autograd node on the kernels of csrc/delta.hip.  depth_* / acc_*: the
// rendered depth and silhouette (depth_sol) of the two views, [H,W] or [1,H,W] f32 on the device; inv_K_src, K_ref:
// 3x3, T_rel: 3x4 or 4x4 ([R_rel | t_rel] = T_ref T_src^-1 as calcDeltaSimi composes it, i.e. with Get_R() transposed,
// gaussian.cu:138-162), on the host or anywhere (they are read as 9 + 9 + 12 host floats).  Gradients w.r.t. the two
// depth images only.  Returns the 0-dim loss.  (Not part of the oracle/ref_link link check, which stays as it is.)
torch::Tensor delta_depth_loss(const torch::Tensor& depth_src, const torch::Tensor& acc_src,
                               const torch::Tensor& depth_ref, const torch::Tensor& acc_ref,
                               const torch::Tensor& inv_K_src, const torch::Tensor& K_ref, const torch::Tensor& T_rel,
                               float lambda = 0.2f);

// ---- LiDAR depth supervision (an extension; csrc/lidar.hip) ----------------------------------------------------------
// lidar_depth_image: the z-buffer of a sweep in a keyframe's view, built once when gsAddCamera makes the keyframe:
// points_world [n,3] f32 on the device (n == 0 is legal), T_cw 3x4 or 4x4 ([R | t], x_c = R x_w + t) and K 3x3 on the
// host or anywhere (read as 12 + 9 host floats) -> [H,W] f32, the smallest z per pixel, 0 where no point lands.
// counts (optional): receives an int32 device tensor {points kept, pixels hit}.
torch::Tensor lidar_depth_image(const torch::Tensor& points_world, const torch::Tensor& T_cw, const torch::Tensor& K,
                                int64_t height, int64_t width, float min_depth = 0.2f,
                                float max_depth = std::numeric_limits<float>::infinity(),
                                torch::Tensor* counts = nullptr);
// lidar_depth_loss: lambda * mean over the supervised pixels (lidar_depth > 0 and acc >= acc_min) of
// |depth / acc - lidar_depth| as ONE autograd node; depth / acc: the rasterizer's second and third outputs, [H,W] or
// [1,H,W] f32 on the device.  Gradients w.r.t. depth and acc only.  Returns the 0-dim loss.
// (Like delta_depth_loss, these two are not part of the oracle/ref_link link check, which stays as it is.)
torch::Tensor lidar_depth_loss(const torch::Tensor& depth, const torch::Tensor& acc, const torch::Tensor& lidar_depth,
                               float acc_min = 0.5f, float lambda = 1.0f);
// lidar_occlusion_filter: the LiDAR depth image ([H,W] or [1,H,W] f32 on the device) without the returns seen through
// the gaps of a nearer surface (gsr_lidar_occlusion_filter: sweep admission's OCCLUDED rule on the supervision image);
// called once per keyframe behind lidar_depth_image.  radius (0..3) and tol have no default: the caller's policy.
// Returns a new image; counts (optional) receives an int32 device tensor {pixels kept, pixels removed}.
torch::Tensor lidar_occlusion_filter(const torch::Tensor& lidar_depth, int64_t radius, float tol,
                                     torch::Tensor* counts = nullptr);
// lidar_depth_loss_robust: lidar_depth_loss with a Huber residual (quadratic below huber_abs + huber_rel z_L) and a
// clip (|depth error| above clip_abs + clip_rel z_L is not supervised; clip_abs = +inf: no clip) as ONE autograd node
// (gsr_lidar_depth_loss_robust).  At huber_abs = huber_rel = clip_rel = 0 and clip_abs = +inf it returns
// lidar_depth_loss's bits.  (Like the two above, these are not part of the oracle/ref_link link check, which stays as
// it is: that check links the reference's own callers, and the reference has no LiDAR depth term.)
torch::Tensor lidar_depth_loss_robust(const torch::Tensor& depth, const torch::Tensor& acc,
                                      const torch::Tensor& lidar_depth, float acc_min, float lambda, float huber_abs,
                                      float huber_rel, float clip_abs, float clip_rel);

// ---- sweep admission (an extension; csrc/seed.hip, gsr_sweep_admit) ----------------------------------------------------
// The points of a sweep that a keyframe's render does not explain yet, compacted in input order and ready for
// GrowableGaussians::add_new_pointcloud: coloured from the keyframe's image (bilinear, the exposure inverted, times
// 255) and sized by their pixel footprint unless covs is given.  An undefined tensor stands for an absent optional
// input (depth and acc go together).  One host wait: the read of the counts.  The returned tensors are views of the
// first `admitted` rows.  (Like delta_depth_loss, not part of the oracle/ref_link link check, which stays as it is.)
struct SweepAdmitOptions {
  float acc_min = 0.5f;
  int occlusion_radius = 1;
  float footprint = 1.0f;
  float min_depth = 0.2f;
  float max_depth = std::numeric_limits<float>::infinity();
  bool one_per_pixel = true;
  bool want_reasons = false;
};
struct Admitted {
  torch::Tensor xyz, covs, rgbs, index, pixel, z;  // [m,3], [m,3,3], [m,3] or undefined, int32 [m], int32 [m], [m]
  std::array<int64_t, 6> counts;                   // admitted, out, occluded, explained, behind, duplicate
  torch::Tensor reasons;                           // uint8 [n] on the device (want_reasons) or undefined
};
Admitted admit_sweep(const torch::Tensor& points_world, const torch::Tensor& T_cw, const torch::Tensor& K,
                     int64_t height, int64_t width, float depth_tol, float occlusion_tol,
                     const torch::Tensor& depth = torch::Tensor(), const torch::Tensor& acc = torch::Tensor(),
                     const torch::Tensor& image = torch::Tensor(), const torch::Tensor& lidar_depth = torch::Tensor(),
                     const torch::Tensor& covs = torch::Tensor(), const torch::Tensor& exposure = torch::Tensor(),
                     const SweepAdmitOptions& options = SweepAdmitOptions());

// ---- the sweep voxel map (an extension; csrc/voxel.hip, gsr_voxel_sweep) -----------------------------------------------
// A persistent voxel table on the device with exact, order-independent per-voxel moments, and one oriented Gaussian per
// voxel that matures: what stands between admit_sweep and GrowableGaussians::add_new_pointcloud, where the reference
// walks an unordered_map on the host (GpMap::splitPointsIntoCell / dividePointsIntoCellInitMap, src/gp3d/map.cpp).
// grid, min_points and min_sigma have no default: the caller's policy.  voxel_sweep doubles the table BEFORE the launch
// while live + n > capacity / 2, so no point is ever FULL; one host wait: the read of the counts.  The seed tensors
// are views of the first `matured` rows, in the order of first appearance; status / point_keys have one entry per
// point.  (Like admit_sweep, not part of the oracle/ref_link link check, which stays as it is.)
struct VoxelMap {
  torch::Tensor table;  // int64 [capacity,16] on the device: voxel_table()
  int64_t live = 0;     // the keys it holds
  float grid = 0.f, min_sigma = 0.f;
  int64_t min_points = 0;
};
struct VoxelSeeds {
  torch::Tensor xyz, covs, rgbs, keys, points, scaling_raw, rotation, normal;  // [v,3] [v,3,3] [v,3]|undefined i64[v] i32[v] [v,3] [v,4] [v,3]
  torch::Tensor status, point_keys;                                           // uint8 [n], int64 [n]
  std::array<int64_t, 6> counts;                                               // accumulated, seeded, out, full, matured, live keys
};
torch::Tensor voxel_table(int64_t capacity, const torch::Tensor& like);  // zeroed; capacity a power of two
// every record of `table` in a new zeroed table of `capacity` slots (gsr_voxel_rehash)
torch::Tensor voxel_rehash(const torch::Tensor& table, int64_t capacity);
VoxelSeeds voxel_sweep(VoxelMap& map, const torch::Tensor& points, const torch::Tensor& colors = torch::Tensor(),
                       float scale_factor = 1.0f);

// ---- the evaluation pass (saveRender, src/liw/lioOptimization.cpp:2182-2245; the status line of optimize_vis) ------
// [psnr, ssim, l1, mse] of image against gt ([C,H,W] f32 on the device) on the kernels of csrc/metrics.hip, a device
// tensor, no graph: gaussian_splatting::psnr (loss_utils.cuh:89-93, the mean of the per-channel PSNRs, +inf where a
// channel is identical) and ::ssim (:43-70) of :2203-2207 in two launches.  totals: a device float64 [4] that
// {psnr, ssim, l1, 1} is added to -- psnr_value, ssim_value and count of :2184-2231 without an .item() per frame.
// (Like delta_depth_loss, not part of the oracle/ref_link link check, which keeps its twenty entry points.)
// weights: [H,W] f32 on the device (finite, >= 0): the four numbers are then weighted_photometric_loss's, every sum
// weighted per pixel and divided by the weight sum; undefined = today's call.
torch::Tensor image_metrics(const torch::Tensor& image, const torch::Tensor& gt,
                            const torch::Tensor& window1d = torch::Tensor(),
                            const torch::Tensor& totals = torch::Tensor(),
                            const torch::Tensor& weights = torch::Tensor());
torch::Tensor psnr(const torch::Tensor& image, const torch::Tensor& gt);  // image_metrics(...)[0], 0-dim
// tensor2CvMat3X (:2113-2136) on the device: [3,H,W] f32 -> uint8 [H,W,3] (x * 255, clamp, truncate; NaN -> 0), BGR
// for cv::imwrite unless bgr = false.  out: a uint8 [H,W,3] view to write into, e.g. a column slice of the [H,2W,3]
// image that replaces cv::hconcat (:2219-2220); undefined = a new tensor.
torch::Tensor to_u8(const torch::Tensor& image, bool bgr = true, torch::Tensor out = torch::Tensor());
// tensor2CvMat2X (:2150-2164) up to cv::applyColorMap: [H,W] or [1,H,W] f32 -> uint8 [H,W],
// round_half_even(depth * (255 / max_depth)) saturated, NaN -> 0.
torch::Tensor depth_to_u8(const torch::Tensor& depth, float max_depth = 50.0f, torch::Tensor out = torch::Tensor());

// gs_hash_indexes_ (voxel key -> rows of its Gaussians, gaussian.cu:257-263) kept as ranges -- the reference's row
// vectors are an iota from the running model size (src/liw/lioOptimization.cpp:1268-1279) -- and the selection of
// calcSimiLoss (gaussian.cu:201-228) on them.
class VoxelIndex {
 public:
  // The voxels `keys` contributed counts[i] consecutive rows each, from first_row on (pcd.hash_posi_s / pcd.indexes).
  // Returns the row after the last.  A key that is known already, or given twice, throws and registers nothing (the
  // reference ends the program there, gaussian.cu:258-262); a count of 0 registers a key without rows.
  int64_t add(const std::vector<std::size_t>& keys, const std::vector<int64_t>& counts, int64_t first_row);
  // Steps 1-2 of calcSimiLoss for GSLIVM::GsForLosses::_losses ({key: [k,3] f32 CPU}): the points of every known key
  // (ascending key order), cut to exactly max_points by torch::randperm when there are that many or more
  // (MAX_SIMI, include/gs/gp3d/gp_types.h:15), and the ascending unique rows of those keys as int32, both copied to
  // `device` without waiting.  false where the reference returns false (no point left; also: no row to compare with).
  bool select(const std::unordered_map<std::size_t, torch::Tensor>& losses, torch::Tensor& points, torch::Tensor& sel,
              int64_t max_points = 500, torch::Device device = torch::kCUDA) const;
  // Follows a stable compaction of the model's rows (prune_mark / FusedAdam::prune): row_map_cpu [P+1] integers on the
  // host, the exclusive prefix sum of "kept".  (first, count) becomes (row_map[first], row_map[first + count] -
  // row_map[first]); a voxel that loses all its rows stays registered with count 0, so adding its key again still
  // throws.  Throws, and changes nothing, when a range ends beyond P.
  void remap(const torch::Tensor& row_map_cpu);
  // (first_row, count) of a key; false when the key is unknown
  bool get(std::size_t key, int64_t& first_row, int64_t& count) const;
  std::size_t size() const { return ranges_.size(); }
  bool contains(std::size_t key) const { return ranges_.count(key) > 0; }

 private:
  std::unordered_map<std::size_t, std::pair<int64_t, int64_t>> ranges_;  // key -> (first_row, count)
};

// ---- row 1: activations + Adam ----------------------------------------------------------------------------------
// The five getters of GaussianModel (include/gs/gs/gaussian.cuh:40-54) as one autograd node:
//   scaling = exp(_scaling), rotation = normalize(_rotation), opacity = sigmoid(_opacity),
//   features = cat({_features_dc, _features_rest}, 1)
struct Activated {
  torch::Tensor scaling, rotation, opacity, features;
};
Activated activate(const torch::Tensor& scaling_raw, const torch::Tensor& rotation_raw, const torch::Tensor& opacity_raw,
                   const torch::Tensor& features_dc, const torch::Tensor& features_rest);

// torch::optim::Adam as GaussianModel::Training_setup configures it (src/gs/gaussian.cu:396-428: one group per leaf,
// betas (0.9, 0.999), eps 1e-15, no weight decay / amsgrad) with _optimizer->step() + zero_grad()
// (lioOptimization.cpp:1831-1832) in one launch per eight tensors.  The moments are owned here.
class FusedAdam {
 public:
  // params / lrs in the reference's group order: _xyz, _features_dc, _features_rest, _scaling, _rotation, _opacity
  FusedAdam(std::vector<torch::Tensor> params, std::vector<double> lrs, double beta1 = 0.9, double beta2 = 0.999,
            double eps = 1e-15);
  // every param with a defined .grad() is stepped; zero_grad: the gradients are cleared by the same kernel
  void step(bool zero_grad = true);
  // The whole optimiser tail in ONE launch (k_model_step): chain rule of the activations applied to the gradients
  // w.r.t. the ACTIVATED tensors (what the rasterizer's backward returns), Adam on the six groups, and the activated
  // values of the updated parameters for the next forward.  g_xyz [P,3], g_scaling [P,3], g_rotation [P,4],
  // g_opacity [P,1], g_features [P,M,3].  Needs exactly the six leaves of a GaussianModel in the order above.
  Activated step_model(const torch::Tensor& g_xyz, const torch::Tensor& g_scaling, const torch::Tensor& g_rotation,
                       const torch::Tensor& g_opacity, const torch::Tensor& g_features);
  // GaussianModel::cat_tensors_to_optimizer (gaussian.cu:451-472): the leaf at `index` was replaced by a longer tensor
  // whose first rows are the old ones; its moments grow by zero rows
  void replace_param(size_t index, torch::Tensor new_param);
  // GaussianModel::prune_optimizer (gaussian.cu:430-449) for all groups in ONE launch: every parameter and both of
  // its moments are replaced by their compacted tensors -- the rows with reasons[i] == 0, in order, P_new of them
  // (reasons, row_map: from prune_mark; P_new = row_map[P], which the caller has fetched).  The new parameters are
  // fresh leaves that require grad as the old ones did; step_count() is unchanged.
  void prune(const torch::Tensor& reasons, const torch::Tensor& row_map, int64_t P_new);
  int64_t step_count() const { return step_; }
  const std::vector<torch::Tensor>& params() const { return params_; }
  const std::vector<torch::Tensor>& exp_avg() const { return m_; }
  const std::vector<torch::Tensor>& exp_avg_sq() const { return v_; }

 private:
  std::vector<torch::Tensor> params_, m_, v_;
  std::vector<double> lrs_;
  double beta1_, beta2_, eps_;
  int64_t step_ = 0;
};

// ---- in-place pruning (an extension: the reference carries prune_optimizer and never calls it) ------------------------
// The drop rule and the row map of the stable compaction on the kernels of csrc/prune.hip (include/gsraster.h,
// gsr_prune_mark): a row leaves when sigmoid(_opacity) < min_opacity, any exp(_scaling) > max_scale, (drop_nonfinite) any
// of the four tensors is NaN / +-Inf, or drop ([P] bool / uint8 on the device, may be undefined) marks it.  All device
// tensors, nothing waits: reasons [P] uint8 (0 = keep), row_map [P+1] int32 (row_map[P] = P'), counts [5] int32 =
// {P', opacity, scale, non-finite, mask}.  (Like delta_depth_loss and image_metrics, these entry points are not part of
// the oracle/ref_link link check, which keeps its twenty entry points.)
struct PruneMarks {
  torch::Tensor reasons, row_map, counts;
};
PruneMarks prune_mark(const torch::Tensor& xyz, const torch::Tensor& scaling_raw, const torch::Tensor& rotation_raw,
                      const torch::Tensor& opacity_raw, float min_opacity = 1.0f / 255.0f, float max_scale = 0.3f,
                      bool drop_nonfinite = true, const torch::Tensor& drop = torch::Tensor());
// tensors[k][reasons == 0] for up to any number of [P, ...] f32 device tensors, eighteen per launch: new [P_new, ...]
// tensors
std::vector<torch::Tensor> prune_rows(const std::vector<torch::Tensor>& tensors, const torch::Tensor& reasons,
                                      const torch::Tensor& row_map, int64_t P_new);

// ---- adaptive density control (an extension: the reference carries densification_postfix and never runs the loop) ------
// Thin tensor-level hosts of csrc/densify.hip; include/gsraster.h has the contract (the rule, the generator, what is
// written and what is not).  All device tensors, nothing waits.  (Not part of the oracle/ref_link link check either.)
// stats [P,3] f32 {grad_sum, views, max_radius} is updated in place from one view's radii [P] int32 and dL_dmean2D [P,3].
void density_accumulate(const torch::Tensor& radii, const torch::Tensor& dL_dmean2D, torch::Tensor stats);
struct DensifyMarks {
  torch::Tensor kinds, offsets, counts;  // [P] uint8 (0 none, 1 clone, 2 split), [P+1] int32, [3] int32 {n_new, clones, splits}
};
DensifyMarks densify_mark(const torch::Tensor& stats, const torch::Tensor& scaling_raw, float grad_threshold,
                          float size_threshold, int64_t max_new = -1);
// In place on capacity buffers of at least P + n_new rows: params6 in the order xyz, features_dc, features_rest, scaling,
// rotation, opacity; exp_avg6 / exp_avg_sq6 six buffers each or empty vectors; stats [., 3] or undefined.  n_new =
// offsets[P], which the caller has fetched.
void densify_apply(int64_t P, int64_t n_new, const torch::Tensor& kinds, const torch::Tensor& offsets, uint64_t seed,
                   const std::vector<torch::Tensor>& params6, const std::vector<torch::Tensor>& exp_avg6,
                   const std::vector<torch::Tensor>& exp_avg_sq6, const torch::Tensor& stats = torch::Tensor());

// ---- keyframe covisibility (an extension: the reference draws its training views blindly) -----------------------------
// Thin tensor-level hosts of csrc/covis.hip; include/gsraster.h has the contract.  A visibility row is int64 words, bit
// i % 64 of word i / 64 = model row i; a slab is a 2-D int64 device tensor with contiguous rows, its stride(0) the pitch
// (a 1-D tensor is one row).  All device tensors, nothing waits.  (Not part of the oracle/ref_link link check either.)
// source: a forward's radii ([P] int32, seen = radii > 0) or a bool / uint8 mask (markVisible's).  words: 0 = ceil(P / 64);
// all `words` words are written, bits at and beyond P are zero.
torch::Tensor visibility_pack(const torch::Tensor& source, int64_t words = 0);
struct Covisibility {
  torch::Tensor inter, q_count, k_count;  // [Q,K], [Q], [K] int32; the counts undefined when not asked for
};
// inter[q][k] = popcount(q row & k row) over `words` words (0 = all that both hold); k_bits undefined = q_bits.
Covisibility covisibility(const torch::Tensor& q_bits, const torch::Tensor& k_bits = torch::Tensor(), int64_t words = 0,
                          bool counts = true);
struct ObservationCount {
  torch::Tensor count, drop;  // [P] int32, [P] uint8 (i >= first_row && count < min_count); undefined when not asked for
};
ObservationCount observation_count(const torch::Tensor& bits, int64_t P, int64_t first_row = 0, int64_t min_count = 0,
                                   bool want_count = true, bool want_drop = false);
// The rows of `src` after the stable compaction of prune_mark's (reasons, row_map): a new [K, dst_words] slab
// (dst_words: 0 = ceil(P / 64), which always suffices).
torch::Tensor visibility_remap(const torch::Tensor& src, const torch::Tensor& reasons, const torch::Tensor& row_map,
                               int64_t dst_words = 0);

// ---- per-Gaussian blend contribution (an extension: the reference's rasterizer has no such output) ---------------------
// Thin tensor-level hosts of gsr_contribution / gsr_contribution_finish; include/gsraster.h has the contract.  geom,
// binning, img: the three blobs of a completed forward (RasterizeGaussiansCUDA's last three results), R: its first.
// Returns the integer frame rows, [P, 2] int64 = {wsum_fx, pixels | wmax_bits << 32}.  Nothing waits.
torch::Tensor contribution(const torch::Tensor& geom, const torch::Tensor& binning, const torch::Tensor& img, int64_t P,
                           int64_t R, int64_t W, int64_t H);
struct Contribution {
  torch::Tensor n_touched, weight_sum, weight_max, mask;  // [P] int32, f32, f32, uint8; undefined when not asked for
};
// stats (optional): [P, 3] f32 {weight_sum_total, views, weight_max}, updated in place.
Contribution contribution_finish(const torch::Tensor& rows, int64_t min_pixels = 1, double min_weight = 0.0,
                                 bool want_n_touched = true, bool want_weight_sum = true, bool want_weight_max = true,
                                 bool want_mask = true, const torch::Tensor& stats = torch::Tensor());

// ---- rendered normal maps and the depth-normal consistency loss (an extension; csrc/normal.hip) -------------------------
// Thin tensor-level hosts of gsr_blend_attributes / gsr_surfel_normals / gsr_normal_consistency_loss;
// include/gsraster.h has the contracts.  blend_attributes: attributes [P, C] (or [P]) f32 on the device, C in 1..4,
// blended behind the completed forward whose blobs and R are given -> [C, H, W].  surfel_normals: the ACTIVATED xyz
// [P,3], scaling [P,3], rotation [P,4] and T_cw = [R | t] (3x4 or 4x4, any device) -> the camera-facing thin axes [P,3].
// Neither builds an autograd graph; nothing waits.
torch::Tensor blend_attributes(const torch::Tensor& geom, const torch::Tensor& binning, const torch::Tensor& img,
                               const torch::Tensor& attributes, int64_t R, int64_t W, int64_t H);
torch::Tensor surfel_normals(const torch::Tensor& xyz, const torch::Tensor& scaling, const torch::Tensor& rotation,
                             const torch::Tensor& T_cw);
// normal_consistency_loss: lambda * mean over the supervised pixels of 1 - n_r . n_d as ONE autograd node; depth / acc:
// the rasterizer's second and third outputs, normals: blend_attributes of surfel_normals ([3,H,W], data), K: the 3x3
// pinhole of the render.  Gradients w.r.t. depth and acc only.  lambda and normal_min have no default, on purpose.
torch::Tensor normal_consistency_loss(const torch::Tensor& depth, const torch::Tensor& acc,
                                      const torch::Tensor& normals, const torch::Tensor& K, float acc_min, float lambda,
                                      float normal_min, float jump_rel = std::numeric_limits<float>::infinity());

// ---- row 4: map growth and PLY export ---------------------------------------------------------------------------
// The tensor construction of GaussianModel::addNewPointcloud (src/gs/gaussian.cu:241-313) for n new points -- xyz
// [n,3], covs [n,3,3], rgbs [n,3] in 0..255 -- written IN PLACE into n-row views (normally the tail rows of capacity
// buffers): scaling = log(sqrt(diag(cov) * scale_factor)), rotation = (1,0,0,0), opacity = inverse_sigmoid(0.5) = 0,
// features_dc = RGB2SH(rgb / 255), features_rest = 0.
void init_gaussians(const torch::Tensor& xyz, const torch::Tensor& covs, const torch::Tensor& rgbs, float scale_factor,
                    torch::Tensor xyz_out, torch::Tensor features_dc_out, torch::Tensor features_rest_out,
                    torch::Tensor scaling_out, torch::Tensor rotation_out, torch::Tensor opacity_out);

// Vertex rows of GaussianModel::Save_ply (gaussian.cu:494-522) interleaved on the device: [P, 14 + 3 M] f32 in the
// order of construct_list_of_attributes (:474-492).
torch::Tensor pack_ply_rows(const torch::Tensor& xyz, const torch::Tensor& features_dc,
                            const torch::Tensor& features_rest, const torch::Tensor& opacity,
                            const torch::Tensor& scaling, const torch::Tensor& rotation);
// Write_output_ply (gaussian.cu:542-573) without tinyply: one D2H copy of the packed rows behind a header that is byte
// for byte what the reference's vendored tinyply writes (tests/golden/ply_*.ply).  Returns the bytes written.
size_t write_ply(const std::string& file_path, const torch::Tensor& xyz, const torch::Tensor& features_dc,
                 const torch::Tensor& features_rest, const torch::Tensor& opacity, const torch::Tensor& scaling,
                 const torch::Tensor& rotation);
std::vector<std::string> ply_attribute_names(int M);  // construct_list_of_attributes

// ---- depth gradient (torch_binding.cpp; an extension, the reference's backward ignores the depth output's gradient) ----
// The reference's GaussianRasterizationSettings cannot grow a field (torch_binding.cpp is compiled against the
// reference's own header too), so the opt-in is a switch of the calling thread: a forward of _RasterizeGaussians
// captures it, and that render's backward then uses the gradient of its depth output when one arrives (a depth L1
// against a LiDAR depth image, the delta-depth term of lioOptimization.cpp:1780-1814, depth regularisers).
// Off by default.  Returns the previous value.
bool set_depth_gradient(bool on);

// ---- camera pose gradient (torch_next.cpp; an extension, the reference's poses are constants) ---------------------------
// gsr_pose_gradient with tensors: dL/dxi [6] f32 of the left perturbation T_cw <- Exp(xi^) T_cw at xi = 0 ([0:3]
// translation, [3:6] rotation, camera axes; include/gsraster.h has the convention), from what a backward was given and
// wrote.  scales / rotations or cov3D_precomp: size-0 or undefined = not provided; dL_ddepths undefined = none.  All
// device tensors, nothing waits.
torch::Tensor pose_gradient(const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& scales,
                            const torch::Tensor& rotations, float scale_modifier, const torch::Tensor& cov3D_precomp,
                            const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, float tan_fovx,
                            float tan_fovy, int image_height, int image_width, const torch::Tensor& dL_dmeans2D,
                            const torch::Tensor& dL_dconic, const torch::Tensor& dL_dmeans3D,
                            const torch::Tensor& dL_ddepths = torch::Tensor());
// T_cw <- Exp(xi^) T_cw IN PLACE in a camera's device tensors (world_view_transform, full_proj_transform, camera_center;
// `projection` is read), then xi <- 0: the addresses stay, which keeps the library's per-view history.  Composed in
// float64 on the device and rounded once; no host wait.
void retract_camera(torch::Tensor view, torch::Tensor full_proj, torch::Tensor centre, const torch::Tensor& projection,
                    torch::Tensor xi);
torch::Tensor se3_exp(const torch::Tensor& xi);  // Exp(xi^) [4,4] in xi's dtype, on its device

}  // namespace gsr_torch

// RasterizeGaussiansBackwardCUDA with the gradient of the depth output (gsr_backward_depth): the same arguments plus
// dL_dout_depth ([1,H,W]) after dL_dout_acc; the same eight gradients plus dL_ddepths [P] (dL/d view-space depth).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardDepthCUDA(const torch::Tensor& background, const torch::Tensor& means3D,
                                    const torch::Tensor& radii, const torch::Tensor& colors, const torch::Tensor& scales,
                                    const torch::Tensor& rotations, const float scale_modifier,
                                    const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                    const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                    const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_acc,
                                    const torch::Tensor& dL_dout_depth, const torch::Tensor& sh, const int degree,
                                    const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                                    const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                    const bool debug);

// The backward and the camera pose gradient behind it (gsr_pose_gradient), for a C++ host: the arguments of
// RasterizeGaussiansBackwardDepthCUDA -- an undefined dL_dout_depth selects the plain backward, dL_ddepths then comes back
// undefined -- and its nine tensors plus dL_dpose [6].
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansBackwardPoseCUDA(const torch::Tensor& background, const torch::Tensor& means3D,
                                   const torch::Tensor& radii, const torch::Tensor& colors, const torch::Tensor& scales,
                                   const torch::Tensor& rotations, const float scale_modifier,
                                   const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                                   const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                                   const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_acc,
                                   const torch::Tensor& dL_dout_depth, const torch::Tensor& sh, const int degree,
                                   const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                                   const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                                   const bool debug);
