// torch_next.cpp -- definitions of gsr_torch_next.hpp: the C++/LibTorch hosts of the rows either side of the
// rasterizer, over the C ABI of libgsraster_hip.so (include/gsraster.h).  Plain C++ (no device code); PyTorch-ROCm
// supplies tensors, autograd and the current HIP stream.  Python mirrors with the same semantics: gs-livm_amd/loss.py,
// model.py, ply.py (the GPU tests compare the two routes bit for bit through the pybind11 module of torch_binding.cpp).
//
// Replaces, at their call sites:
//   gaussian_splatting::l1_loss + ssim + the loss line     include/gs/gs/loss_utils.cuh:11-13,43-70,
//                                                           src/liw/lioOptimization.cpp:1705-1710
//   GaussianModel's getters                                include/gs/gs/gaussian.cuh:40-54
//   _optimizer->step() / zero_grad()                       src/gs/gaussian.cu:396-428, lioOptimization.cpp:1831-1832
//   the tensor construction of addNewPointcloud            src/gs/gaussian.cu:241-313
//   Save_ply / Write_output_ply                            src/gs/gaussian.cu:494-573
//   compute_min_distance + the selection of calcSimiLoss   src/gs/gaussian.cu:87-114, 201-239
//   calcDeltaSimi + the loop body around it                src/gs/gaussian.cu:116-199, lioOptimization.cpp:1780-1801
//   prune_optimizer (carried, never called there)          src/gs/gaussian.cu:430-449
//   psnr + ssim + tensor2CvMat3X / 2X of saveRender        loss_utils.cuh:89-93, lioOptimization.cpp:2113-2164, 2198-2231
#include "gsr_torch_next.hpp"

#include <c10/hip/HIPStream.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <unordered_set>

#include "gsraster.h"

namespace gsr_torch {
namespace {

void* current_stream() { return static_cast<void*>(c10::hip::getCurrentHIPStream().stream()); }

void check(int code, const char* what) {
  if (code < 0) throw std::runtime_error(std::string(what) + ": " + gsr_last_error());
}

float* fp(const torch::Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }

torch::Tensor dev_f32(const torch::Tensor& t, const char* name) {
  if (!t.defined() || !t.is_cuda() || t.scalar_type() != torch::kFloat32)
    throw std::invalid_argument(std::string(name) + ": expected a float32 tensor on the device");
  return t.contiguous();
}

int coefficients(const torch::Tensor& features_rest) {  // M = SH coefficients per channel
  return 1 + (features_rest.defined() && features_rest.numel() ? static_cast<int>(features_rest.size(1)) : 0);
}

// a byte workspace on the device of `like`; never empty, so that an entry point that needs no bytes gets a pointer too
torch::Tensor workspace(size_t nbytes, const torch::Tensor& like) {
  return torch::empty({static_cast<long long>(nbytes ? nbytes : 1)}, like.options().dtype(torch::kByte));
}

// the first three rows of a 2-d matrix (3x3, 3x4 or 4x4; any device, any float type) as float32 on the host
torch::Tensor host_rows3(const torch::Tensor& t, const char* name) {
  if (!t.defined() || t.dim() != 2 || t.size(0) < 3)
    throw std::invalid_argument(std::string(name) + ": a 2-d matrix of at least three rows");
  return t.to(torch::kCPU, torch::kFloat64).slice(0, 0, 3).to(torch::kFloat32).contiguous();
}

// a loss node's backward: the gradient saved by its forward times the upstream scalar, or undefined where the forward
// saved none (an empty tensor stands for "none")
torch::Tensor scaled(const torch::Tensor& saved, const torch::Tensor& upstream) {
  return saved.numel() ? saved * upstream : torch::Tensor();
}

void window_taps(const torch::Tensor& window1d, float out[11]) {
  const torch::Tensor w = (window1d.defined() ? window1d : reference_window_1d()).to(torch::kCPU, torch::kFloat32).contiguous();
  if (w.numel() != 11) throw std::invalid_argument("photometric_loss: the window has 11 taps");
  for (int k = 0; k < 11; k++) out[k] = w.data_ptr<float>()[k];
}

// one evaluation of the fused loss: out3 = [loss, l1, ssim], grad = dL/dimage (or undefined)
std::pair<torch::Tensor, torch::Tensor> run_loss(const torch::Tensor& image, const torch::Tensor& gt, float lambda,
                                                 const torch::Tensor& window1d, bool want_grad) {
  const torch::Tensor img = dev_f32(image, "image"), ref = dev_f32(gt, "gt");
  if (img.dim() != 3 || img.sizes() != ref.sizes()) throw std::invalid_argument("photometric_loss: [C,H,W] images of one shape");
  const int C = img.size(0), H = img.size(1), W = img.size(2);
  float taps[11];
  window_taps(window1d, taps);
  const size_t nbytes = gsr_photometric_loss_workspace(C, H, W);
  torch::Tensor ws = workspace(nbytes, img);
  torch::Tensor out3 = torch::empty({3}, img.options());
  torch::Tensor grad = want_grad ? torch::empty_like(img) : torch::Tensor();
  check(gsr_photometric_loss(C, H, W, fp(img), fp(ref), taps, lambda, out3.data_ptr<float>(), fp(grad),
                             reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
        "gsr_photometric_loss");
  return {out3, grad};
}

struct PhotometricLossFn : public torch::autograd::Function<PhotometricLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor image, torch::Tensor gt,
                               double lambda, torch::Tensor window1d) {
    auto r = run_loss(image, gt, static_cast<float>(lambda), window1d, image.requires_grad());
    ctx->save_for_backward({r.second.defined() ? r.second : torch::empty({0}, image.options())});
    return r.first[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const torch::Tensor grad = ctx->get_saved_variables()[0];
    return {scaled(grad, grad_outputs[0]), torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

// [C,2] rows (g_c, b_c) from [C,2] or a shared [2] (expanded: autograd sums its gradient); log_gain: g = exp(column 0)
torch::Tensor per_channel_exposure(const torch::Tensor& exposure, int64_t channels, bool log_gain) {
  if (!exposure.defined() || !((exposure.dim() == 1 && exposure.size(0) == 2) ||
                               (exposure.dim() == 2 && exposure.size(0) == channels && exposure.size(1) == 2)))
    throw std::invalid_argument("exposure: [C,2] rows (gain, bias), or [2] shared by the channels");
  torch::Tensor e = exposure.dim() == 1 ? exposure.expand({channels, 2}) : exposure;
  if (log_gain) e = torch::stack({torch::exp(e.select(1, 0)), e.select(1, 1)}, 1);
  return e;
}

struct ExposureLossFn : public torch::autograd::Function<ExposureLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor image, torch::Tensor gt,
                               torch::Tensor exposure, double lambda, torch::Tensor window1d) {
    const torch::Tensor img = dev_f32(image, "image"), ref = dev_f32(gt, "gt"), e = dev_f32(exposure, "exposure");
    if (img.dim() != 3 || img.sizes() != ref.sizes())
      throw std::invalid_argument("exposure_photometric_loss: [C,H,W] images of one shape");
    const int C = img.size(0), H = img.size(1), W = img.size(2);
    float taps[11];
    window_taps(window1d, taps);
    const bool want = image.requires_grad() || exposure.requires_grad();
    const size_t nbytes = gsr_exposure_loss_workspace(C, H, W);
    torch::Tensor ws = workspace(nbytes, img);
    torch::Tensor out3 = torch::empty({3}, img.options());
    torch::Tensor grad = want ? torch::empty_like(img) : torch::Tensor();
    torch::Tensor grad_e = want ? torch::empty_like(e) : torch::Tensor();
    check(gsr_exposure_loss(C, H, W, fp(img), fp(ref), fp(e), taps, static_cast<float>(lambda), out3.data_ptr<float>(),
                            fp(grad), fp(grad_e), reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_exposure_loss");
    ctx->save_for_backward({image.requires_grad() ? grad : torch::empty({0}, img.options()),
                            exposure.requires_grad() ? grad_e : torch::empty({0}, img.options())});
    return out3[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    return {scaled(saved[0], grad_outputs[0]), torch::Tensor(), scaled(saved[1], grad_outputs[0]), torch::Tensor(),
            torch::Tensor()};
  }
};

// an [H,W] plane (weights, acc: [H,W] or [1,H,W]) of the image's size as a contiguous float32 device tensor; undefined
// stays undefined
torch::Tensor plane_of(const torch::Tensor& t, int64_t H, int64_t W, const char* what) {
  if (!t.defined() || t.numel() == 0) return torch::Tensor();
  if (t.numel() != H * W) throw std::invalid_argument(std::string(what) + ": one value per pixel, [H,W]");
  return dev_f32(t.detach().reshape({H, W}), what);
}

// one evaluation of the weighted loss: out6 = [loss, l1, ssim, S, mse, psnr], dL/dimage and dL/dexposure (or undefined)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> run_weighted(const torch::Tensor& image, const torch::Tensor& gt,
                                                                     const torch::Tensor& weights, const torch::Tensor& acc,
                                                                     float acc_min, const torch::Tensor& exposure,
                                                                     float lambda, const torch::Tensor& window1d,
                                                                     bool want_grad) {
  const torch::Tensor img = dev_f32(image, "image"), ref = dev_f32(gt, "gt");
  if (img.dim() != 3 || img.sizes() != ref.sizes())
    throw std::invalid_argument("weighted_photometric_loss: [C,H,W] images of one shape");
  const int C = img.size(0), H = img.size(1), W = img.size(2);
  const torch::Tensor w = plane_of(weights, H, W, "weights"), a = plane_of(acc, H, W, "acc");
  const torch::Tensor e = exposure.defined() && exposure.numel() ? dev_f32(exposure, "exposure") : torch::Tensor();
  float taps[11];
  window_taps(window1d, taps);
  const size_t nbytes = gsr_weighted_loss_workspace(C, H, W);
  torch::Tensor ws = workspace(nbytes, img);
  torch::Tensor out6 = torch::empty({6}, img.options());
  torch::Tensor grad = want_grad ? torch::empty_like(img) : torch::Tensor();
  torch::Tensor grad_e = want_grad && e.defined() ? torch::empty_like(e) : torch::Tensor();
  check(gsr_weighted_loss(C, H, W, fp(img), fp(ref), fp(w), fp(a), acc_min, fp(e), taps, lambda, out6.data_ptr<float>(),
                          fp(grad), fp(grad_e), reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
        "gsr_weighted_loss");
  return {out6, grad, grad_e};
}

struct WeightedLossFn : public torch::autograd::Function<WeightedLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor image, torch::Tensor gt,
                               torch::Tensor weights, torch::Tensor acc, double acc_min, torch::Tensor exposure,
                               double lambda, torch::Tensor window1d) {
    const bool need_i = image.requires_grad(), need_e = exposure.numel() && exposure.requires_grad();
    auto r = run_weighted(image, gt, weights, acc, static_cast<float>(acc_min), exposure, static_cast<float>(lambda),
                          window1d, need_i || need_e);
    const torch::Tensor none = torch::empty({0}, std::get<0>(r).options());
    ctx->save_for_backward({need_i ? std::get<1>(r) : none, need_e ? std::get<2>(r) : none});
    return std::get<0>(r)[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    return {scaled(saved[0], grad_outputs[0]), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(),
            scaled(saved[1], grad_outputs[0]), torch::Tensor(), torch::Tensor()};
  }
};

// the selection of operator `op` (the terms on selected Gaussians), as the library reads it
torch::Tensor selection_rows(const torch::Tensor& sel, const char* op) {
  if (!sel.defined() || !sel.is_cuda() || sel.scalar_type() != torch::kInt32 || sel.dim() != 1)
    throw std::invalid_argument(std::string(op) + ": sel is a 1-d int32 tensor on the device");
  return sel.contiguous();
}

struct SimilarityLossFn : public torch::autograd::Function<SimilarityLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor points, torch::Tensor sel,
                               torch::Tensor xyz, torch::Tensor scaling, double lambda) {
    const torch::Tensor p = dev_f32(points, "points"), x = dev_f32(xyz, "xyz"), s = dev_f32(scaling, "scaling");
    const torch::Tensor rows = selection_rows(sel, "similarity_loss");
    if (p.dim() != 2 || p.size(1) != 3 || x.dim() != 2 || x.size(1) != 3 || s.sizes() != x.sizes())
      throw std::invalid_argument("similarity_loss: points [m,3], xyz [P,3], scaling [P,3]");
    const int P = x.size(0), m = p.size(0), n = rows.size(0);
    torch::Tensor gx = xyz.requires_grad() ? torch::zeros_like(x) : torch::Tensor();
    torch::Tensor gs = scaling.requires_grad() ? torch::zeros_like(s) : torch::Tensor();
    const size_t nbytes = gsr_similarity_loss_workspace(m, n);
    torch::Tensor ws = workspace(nbytes, x);
    torch::Tensor out3 = torch::empty({3}, x.options());
    check(gsr_similarity_loss(P, m, n, fp(p), n ? rows.data_ptr<int>() : nullptr, fp(x), fp(s),
                              static_cast<float>(lambda), out3.data_ptr<float>(), fp(gx), fp(gs), 0,
                              reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_similarity_loss");
    ctx->save_for_backward({gx.defined() ? gx : torch::empty({0}, x.options()),
                            gs.defined() ? gs : torch::empty({0}, x.options())});
    return out3[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor gx = saved[0], gs = saved[1], g = grad_outputs[0];
    return {torch::Tensor(), torch::Tensor(), scaled(gx, g), scaled(gs, g), torch::Tensor()};
  }
};

struct SurfelPlaneLossFn : public torch::autograd::Function<SurfelPlaneLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor points, torch::Tensor sel,
                               torch::Tensor xyz, torch::Tensor scaling, torch::Tensor rotation, double lambda,
                               double huber, double max_dist, double lambda_flat) {
    const torch::Tensor p = dev_f32(points, "points"), x = dev_f32(xyz, "xyz"), s = dev_f32(scaling, "scaling"),
                        q = dev_f32(rotation, "rotation");
    const torch::Tensor rows = selection_rows(sel, "surfel_plane_loss");
    if (p.dim() != 2 || p.size(1) != 3 || x.dim() != 2 || x.size(1) != 3 || s.sizes() != x.sizes() || q.dim() != 2 ||
        q.size(0) != x.size(0) || q.size(1) != 4)
      throw std::invalid_argument("surfel_plane_loss: points [m,3], xyz [P,3], scaling [P,3], rotation [P,4]");
    const int P = x.size(0), m = p.size(0), n = rows.size(0);
    torch::Tensor gx = xyz.requires_grad() ? torch::zeros_like(x) : torch::Tensor();
    torch::Tensor gs = scaling.requires_grad() ? torch::zeros_like(s) : torch::Tensor();
    torch::Tensor gq = rotation.requires_grad() ? torch::zeros_like(q) : torch::Tensor();
    const size_t nbytes = gsr_surfel_plane_loss_workspace(m, n);
    torch::Tensor ws = workspace(nbytes, x);
    torch::Tensor out4 = torch::empty({4}, x.options());
    check(gsr_surfel_plane_loss(P, m, n, fp(p), n ? rows.data_ptr<int>() : nullptr, fp(x), fp(s), fp(q),
                                static_cast<float>(lambda), static_cast<float>(huber), static_cast<float>(max_dist),
                                static_cast<float>(lambda_flat), out4.data_ptr<float>(), fp(gx), fp(gs), fp(gq), 0,
                                reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_surfel_plane_loss");
    const torch::Tensor none = torch::empty({0}, x.options());
    ctx->save_for_backward({gx.defined() ? gx : none, gs.defined() ? gs : none, gq.defined() ? gq : none});
    return out4[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor g = grad_outputs[0];
    return {torch::Tensor(), torch::Tensor(), scaled(saved[0], g), scaled(saved[1], g), scaled(saved[2], g),
            torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

struct DeltaDepthLossFn : public torch::autograd::Function<DeltaDepthLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth_src, torch::Tensor acc_src,
                               torch::Tensor depth_ref, torch::Tensor acc_ref, torch::Tensor inv_K_src,
                               torch::Tensor K_ref, torch::Tensor T_rel, double lambda) {
    const torch::Tensor ds = dev_f32(depth_src, "depth_src"), as = dev_f32(acc_src, "acc_src"),
                        dr = dev_f32(depth_ref, "depth_ref"), ar = dev_f32(acc_ref, "acc_ref");
    if (ds.dim() < 2) throw std::invalid_argument("delta_depth_loss: [H,W] or [1,H,W] images");
    const int64_t H = ds.size(-2), W = ds.size(-1);
    if (ds.numel() != H * W || as.numel() != H * W || dr.numel() != H * W || ar.numel() != H * W)
      throw std::invalid_argument("delta_depth_loss: four images of one shape [H,W] or [1,H,W]");
    const torch::Tensor ki = host_rows3(inv_K_src, "inv_K_src"), kr = host_rows3(K_ref, "K_ref"),
                        tr = host_rows3(T_rel, "T_rel");
    if (ki.numel() != 9 || kr.numel() != 9 || tr.numel() != 12)
      throw std::invalid_argument("delta_depth_loss: inv_K_src and K_ref are 3x3, T_rel is 3x4 or 4x4");
    torch::Tensor gs = depth_src.requires_grad() ? torch::empty_like(ds) : torch::Tensor();
    torch::Tensor gr = depth_ref.requires_grad() ? torch::empty_like(dr) : torch::Tensor();
    const size_t nbytes = gsr_delta_depth_loss_workspace(static_cast<int>(H), static_cast<int>(W));
    torch::Tensor ws = workspace(nbytes, ds);
    torch::Tensor out3 = torch::empty({3}, ds.options());
    check(gsr_delta_depth_loss(static_cast<int>(H), static_cast<int>(W), fp(ds), fp(as), fp(dr), fp(ar),
                               ki.data_ptr<float>(), kr.data_ptr<float>(), tr.data_ptr<float>(),
                               static_cast<float>(lambda), out3.data_ptr<float>(), nullptr, fp(gs), fp(gr),
                               reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_delta_depth_loss");
    ctx->save_for_backward({gs.defined() ? gs : torch::empty({0}, ds.options()),
                            gr.defined() ? gr : torch::empty({0}, ds.options())});
    return out3[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor gs = saved[0], gr = saved[1], g = grad_outputs[0];
    return {scaled(gs, g), torch::Tensor(), scaled(gr, g), torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor(), torch::Tensor()};
  }
};

struct LidarDepthLossFn : public torch::autograd::Function<LidarDepthLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth, torch::Tensor acc,
                               torch::Tensor lidar_depth, double acc_min, double lambda) {
    const torch::Tensor d = dev_f32(depth, "depth"), a = dev_f32(acc, "acc"), zl = dev_f32(lidar_depth, "lidar_depth");
    if (d.dim() < 2) throw std::invalid_argument("lidar_depth_loss: [H,W] or [1,H,W] images");
    const int64_t H = d.size(-2), W = d.size(-1);
    if (d.numel() != H * W || a.numel() != H * W || zl.numel() != H * W)
      throw std::invalid_argument("lidar_depth_loss: three images of one shape [H,W] or [1,H,W]");
    torch::Tensor gd = depth.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    torch::Tensor ga = acc.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    const size_t nbytes = gsr_lidar_depth_loss_workspace(static_cast<int>(H), static_cast<int>(W));
    torch::Tensor ws = workspace(nbytes, d);
    torch::Tensor out3 = torch::empty({3}, d.options());
    check(gsr_lidar_depth_loss(static_cast<int>(H), static_cast<int>(W), fp(d), fp(a), fp(zl),
                               static_cast<float>(acc_min), static_cast<float>(lambda), out3.data_ptr<float>(), fp(gd),
                               fp(ga), reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_lidar_depth_loss");
    ctx->save_for_backward({gd.defined() ? gd : torch::empty({0}, d.options()),
                            ga.defined() ? ga.view_as(acc) : torch::empty({0}, d.options())});
    return out3[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor gd = saved[0], ga = saved[1], g = grad_outputs[0];
    return {scaled(gd, g), scaled(ga, g), torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

struct NormalConsistencyLossFn : public torch::autograd::Function<NormalConsistencyLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth, torch::Tensor acc,
                               torch::Tensor normals, double fx, double fy, double cx, double cy, double acc_min,
                               double normal_min, double jump_rel, double lambda) {
    const torch::Tensor d = dev_f32(depth, "depth"), a = dev_f32(acc, "acc"), nr = dev_f32(normals, "normals");
    if (d.dim() < 2) throw std::invalid_argument("normal_consistency_loss: [H,W] or [1,H,W] images");
    const int64_t H = d.size(-2), W = d.size(-1);
    if (d.numel() != H * W || a.numel() != H * W || nr.numel() != 3 * H * W)
      throw std::invalid_argument("normal_consistency_loss: depth and acc [H,W] or [1,H,W], normals [3,H,W]");
    torch::Tensor gd = depth.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    torch::Tensor ga = acc.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    const size_t nbytes = gsr_normal_consistency_workspace(static_cast<int>(H), static_cast<int>(W));
    torch::Tensor ws = workspace(nbytes, d);
    torch::Tensor out3 = torch::empty({3}, d.options());
    check(gsr_normal_consistency_loss(static_cast<int>(H), static_cast<int>(W), fp(d), fp(a), fp(nr),
                                      static_cast<float>(fx), static_cast<float>(fy), static_cast<float>(cx),
                                      static_cast<float>(cy), static_cast<float>(acc_min),
                                      static_cast<float>(normal_min), static_cast<float>(jump_rel),
                                      static_cast<float>(lambda), out3.data_ptr<float>(), fp(gd), fp(ga),
                                      reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
          "gsr_normal_consistency_loss");
    ctx->save_for_backward({gd.defined() ? gd : torch::empty({0}, d.options()),
                            ga.defined() ? ga.view_as(acc) : torch::empty({0}, d.options())});
    return out3[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor gd = saved[0], ga = saved[1], g = grad_outputs[0];
    return {scaled(gd, g), scaled(ga, g), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

struct RobustLidarDepthLossFn : public torch::autograd::Function<RobustLidarDepthLossFn> {
  static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth, torch::Tensor acc,
                               torch::Tensor lidar_depth, double acc_min, double lambda, double huber_abs,
                               double huber_rel, double clip_abs, double clip_rel) {
    const torch::Tensor d = dev_f32(depth, "depth"), a = dev_f32(acc, "acc"), zl = dev_f32(lidar_depth, "lidar_depth");
    if (d.dim() < 2) throw std::invalid_argument("lidar_depth_loss_robust: [H,W] or [1,H,W] images");
    const int64_t H = d.size(-2), W = d.size(-1);
    if (d.numel() != H * W || a.numel() != H * W || zl.numel() != H * W)
      throw std::invalid_argument("lidar_depth_loss_robust: three images of one shape [H,W] or [1,H,W]");
    torch::Tensor gd = depth.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    torch::Tensor ga = acc.requires_grad() ? torch::empty_like(d) : torch::Tensor();
    const size_t nbytes = gsr_lidar_depth_loss_robust_workspace(static_cast<int>(H), static_cast<int>(W));
    torch::Tensor ws = workspace(nbytes, d);
    torch::Tensor out4 = torch::empty({4}, d.options());
    check(gsr_lidar_depth_loss_robust(static_cast<int>(H), static_cast<int>(W), fp(d), fp(a), fp(zl),
                                      static_cast<float>(acc_min), static_cast<float>(lambda),
                                      static_cast<float>(huber_abs), static_cast<float>(huber_rel),
                                      static_cast<float>(clip_abs), static_cast<float>(clip_rel),
                                      out4.data_ptr<float>(), fp(gd), fp(ga), reinterpret_cast<char*>(ws.data_ptr()),
                                      nbytes, current_stream()),
          "gsr_lidar_depth_loss_robust");
    ctx->save_for_backward({gd.defined() ? gd : torch::empty({0}, d.options()),
                            ga.defined() ? ga.view_as(acc) : torch::empty({0}, d.options())});
    return out4[0];
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list grad_outputs) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor gd = saved[0], ga = saved[1], g = grad_outputs[0];
    return {scaled(gd, g), scaled(ga, g), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(),
            torch::Tensor(), torch::Tensor(), torch::Tensor()};
  }
};

struct ActivateFn : public torch::autograd::Function<ActivateFn> {
  static torch::autograd::tensor_list forward(torch::autograd::AutogradContext* ctx, torch::Tensor scaling_raw,
                                              torch::Tensor rotation_raw, torch::Tensor opacity_raw,
                                              torch::Tensor features_dc, torch::Tensor features_rest) {
    const torch::Tensor s = dev_f32(scaling_raw, "_scaling"), r = dev_f32(rotation_raw, "_rotation"),
                        o = dev_f32(opacity_raw, "_opacity"), dc = dev_f32(features_dc, "_features_dc"),
                        rest = dev_f32(features_rest, "_features_rest");
    const int P = s.size(0), M = coefficients(rest);
    torch::Tensor scales = torch::empty({P, 3}, s.options()), rot = torch::empty({P, 4}, s.options()),
                  opac = torch::empty({P, 1}, s.options()), shs = torch::empty({P, M, 3}, s.options());
    check(gsr_activate(P, M, fp(s), fp(r), fp(o), fp(dc), fp(rest), fp(scales), fp(rot), fp(opac), fp(shs),
                       current_stream()),
          "gsr_activate");
    ctx->save_for_backward({r, scales, opac});
    ctx->saved_data["M"] = M;
    return {scales, rot, opac, shs};
  }
  static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
                                               torch::autograd::tensor_list g) {
    const auto saved = ctx->get_saved_variables();
    const torch::Tensor rotation_raw = saved[0], scales = saved[1], opac = saved[2];
    const int P = scales.size(0), M = ctx->saved_data["M"].toInt();
    auto or_zero = [&](const torch::Tensor& t, std::initializer_list<int64_t> shape) {
      return t.defined() ? t.contiguous() : torch::zeros(shape, scales.options());
    };
    const torch::Tensor gs = or_zero(g[0], {P, 3}), gr = or_zero(g[1], {P, 4}), go = or_zero(g[2], {P, 1}),
                        gsh = or_zero(g[3], {P, M, 3});
    torch::Tensor d_s = torch::empty({P, 3}, scales.options()), d_r = torch::empty({P, 4}, scales.options()),
                  d_o = torch::empty({P, 1}, scales.options()), d_dc = torch::empty({P, 1, 3}, scales.options()),
                  d_rest = torch::empty({P, M - 1, 3}, scales.options());
    check(gsr_activate_backward(P, M, fp(rotation_raw), fp(scales), fp(opac), fp(gs), fp(gr), fp(go), fp(gsh), fp(d_s),
                                fp(d_r), fp(d_o), fp(d_dc), fp(d_rest), current_stream()),
          "gsr_activate_backward");
    return {d_s, d_r, d_o, d_dc, d_rest};
  }
};

}  // namespace

torch::Tensor reference_window_1d(int window_size, float sigma) {
  torch::Tensor g = torch::empty({window_size}, torch::kFloat32);
  for (int x = 0; x < window_size; ++x)  // loss_utils.cuh:27 (floor of the halved OFFSET: the reference's quirk)
    g[x] = std::exp(-(std::pow(std::floor(static_cast<float>(x - window_size) / 2.f), 2)) / (2.f * sigma * sigma));
  return g / g.sum();
}

torch::Tensor photometric_loss(const torch::Tensor& image, const torch::Tensor& gt, float lambda_dssim,
                               const torch::Tensor& window1d) {
  return PhotometricLossFn::apply(image, gt, static_cast<double>(lambda_dssim),
                                  window1d.defined() ? window1d : reference_window_1d());
}

torch::Tensor photometric_loss_parts(const torch::Tensor& image, const torch::Tensor& gt, float lambda_dssim,
                                     const torch::Tensor& window1d) {
  torch::NoGradGuard no_grad;
  return run_loss(image, gt, lambda_dssim, window1d, false).first;
}

torch::Tensor exposure_photometric_loss(const torch::Tensor& image, const torch::Tensor& gt,
                                        const torch::Tensor& exposure, float lambda_dssim,
                                        const torch::Tensor& window1d, bool log_gain) {
  if (!image.defined() || image.dim() != 3) throw std::invalid_argument("exposure_photometric_loss: image is [C,H,W]");
  return ExposureLossFn::apply(image, gt, per_channel_exposure(exposure, image.size(0), log_gain),
                               static_cast<double>(lambda_dssim), window1d.defined() ? window1d : reference_window_1d());
}

torch::Tensor weighted_photometric_loss(const torch::Tensor& image, const torch::Tensor& gt, const torch::Tensor& weights,
                                        const torch::Tensor& acc, float acc_min, const torch::Tensor& exposure,
                                        float lambda_dssim, const torch::Tensor& window1d, bool log_gain) {
  if (!image.defined() || image.dim() != 3) throw std::invalid_argument("weighted_photometric_loss: image is [C,H,W]");
  // (an absent operand travels through apply() as an empty tensor: an undefined one has no device to guard)
  const torch::Tensor none = torch::empty({0}, image.options());
  const torch::Tensor e = exposure.defined() ? per_channel_exposure(exposure, image.size(0), log_gain) : none;
  return WeightedLossFn::apply(image, gt, weights.defined() ? weights.detach() : none,
                               acc.defined() ? acc.detach() : none, static_cast<double>(acc_min), e,
                               static_cast<double>(lambda_dssim), window1d.defined() ? window1d : reference_window_1d());
}

torch::Tensor weighted_photometric_loss_parts(const torch::Tensor& image, const torch::Tensor& gt,
                                              const torch::Tensor& weights, const torch::Tensor& acc, float acc_min,
                                              const torch::Tensor& exposure, float lambda_dssim,
                                              const torch::Tensor& window1d, bool log_gain) {
  torch::NoGradGuard no_grad;
  if (!image.defined() || image.dim() != 3) throw std::invalid_argument("weighted_photometric_loss: image is [C,H,W]");
  const torch::Tensor e = exposure.defined() ? per_channel_exposure(exposure, image.size(0), log_gain) : exposure;
  return std::get<0>(run_weighted(image, gt, weights, acc, acc_min, e, lambda_dssim, window1d, false));
}

torch::Tensor apply_exposure(const torch::Tensor& image, const torch::Tensor& exposure, const torch::Tensor& out) {
  torch::NoGradGuard no_grad;
  const torch::Tensor img = dev_f32(image.detach(), "image");
  if (img.dim() != 3) throw std::invalid_argument("apply_exposure: image is [C,H,W]");
  const torch::Tensor e = dev_f32(per_channel_exposure(exposure.detach(), img.size(0), false), "exposure");
  torch::Tensor dst = out.defined() ? out : torch::empty_like(img);
  if (!dst.is_cuda() || dst.scalar_type() != torch::kFloat32 || !dst.is_contiguous() || dst.sizes() != img.sizes())
    throw std::invalid_argument("apply_exposure: out is a contiguous float32 device tensor of the image's shape");
  check(gsr_apply_exposure(static_cast<int>(img.size(0)), static_cast<int>(img.size(1)), static_cast<int>(img.size(2)),
                           fp(img), fp(e), fp(dst), current_stream()),
        "gsr_apply_exposure");
  return dst;
}

torch::Tensor similarity_loss(const torch::Tensor& points, const torch::Tensor& sel, const torch::Tensor& xyz,
                              const torch::Tensor& scaling, float lambda) {
  return SimilarityLossFn::apply(points, sel, xyz, scaling, static_cast<double>(lambda));
}

torch::Tensor surfel_plane_loss(const torch::Tensor& points, const torch::Tensor& sel, const torch::Tensor& xyz,
                                const torch::Tensor& scaling, const torch::Tensor& rotation, float lambda, float huber,
                                float max_dist, float lambda_flat) {
  return SurfelPlaneLossFn::apply(points, sel, xyz, scaling, rotation, static_cast<double>(lambda),
                                  static_cast<double>(huber), static_cast<double>(max_dist),
                                  static_cast<double>(lambda_flat));
}

torch::Tensor delta_depth_loss(const torch::Tensor& depth_src, const torch::Tensor& acc_src,
                               const torch::Tensor& depth_ref, const torch::Tensor& acc_ref,
                               const torch::Tensor& inv_K_src, const torch::Tensor& K_ref, const torch::Tensor& T_rel,
                               float lambda) {
  return DeltaDepthLossFn::apply(depth_src, acc_src, depth_ref, acc_ref, inv_K_src, K_ref, T_rel,
                                 static_cast<double>(lambda));
}

torch::Tensor lidar_depth_image(const torch::Tensor& points_world, const torch::Tensor& T_cw, const torch::Tensor& K,
                                int64_t height, int64_t width, float min_depth, float max_depth,
                                torch::Tensor* counts) {
  torch::NoGradGuard no_grad;
  const torch::Tensor p = dev_f32(points_world, "points_world");
  if (p.dim() != 2 || p.size(1) != 3) throw std::invalid_argument("lidar_depth_image: points_world is [n,3]");
  const torch::Tensor tcw = host_rows3(T_cw, "T_cw"), k = host_rows3(K, "K");
  if (tcw.numel() != 12 || k.numel() != 9) throw std::invalid_argument("lidar_depth_image: T_cw is 3x4 or 4x4, K is 3x3");
  torch::Tensor image = torch::empty({std::max<int64_t>(height, 0), std::max<int64_t>(width, 0)}, p.options());
  torch::Tensor c2 = counts ? torch::empty({2}, p.options().dtype(torch::kInt32)) : torch::Tensor();
  check(gsr_lidar_depth_image(static_cast<int>(p.size(0)), fp(p), tcw.data_ptr<float>(), k.data_ptr<float>(),
                              static_cast<int>(height), static_cast<int>(width), min_depth, max_depth, fp(image),
                              counts ? c2.data_ptr<int>() : nullptr, current_stream()),
        "gsr_lidar_depth_image");
  if (counts) *counts = c2;
  return image;
}

torch::Tensor lidar_depth_loss(const torch::Tensor& depth, const torch::Tensor& acc, const torch::Tensor& lidar_depth,
                               float acc_min, float lambda) {
  return LidarDepthLossFn::apply(depth, acc, lidar_depth, static_cast<double>(acc_min), static_cast<double>(lambda));
}

torch::Tensor lidar_occlusion_filter(const torch::Tensor& lidar_depth, int64_t radius, float tol,
                                     torch::Tensor* counts) {
  torch::NoGradGuard no_grad;
  const torch::Tensor zl = dev_f32(lidar_depth.detach(), "lidar_depth");
  if (zl.dim() < 2) throw std::invalid_argument("lidar_occlusion_filter: an [H,W] or [1,H,W] image");
  const int64_t H = zl.size(-2), W = zl.size(-1);
  if (zl.numel() != H * W) throw std::invalid_argument("lidar_occlusion_filter: an [H,W] or [1,H,W] image");
  torch::Tensor out = torch::empty_like(zl);
  torch::Tensor c2 = counts ? torch::empty({2}, zl.options().dtype(torch::kInt32)) : torch::Tensor();
  check(gsr_lidar_occlusion_filter(static_cast<int>(H), static_cast<int>(W), fp(zl),
                                   static_cast<int>(std::max<int64_t>(std::min<int64_t>(radius, 1 << 20), -1)), tol,
                                   fp(out), counts ? c2.data_ptr<int>() : nullptr, current_stream()),
        "gsr_lidar_occlusion_filter");
  if (counts) *counts = c2;
  return out;
}

torch::Tensor lidar_depth_loss_robust(const torch::Tensor& depth, const torch::Tensor& acc,
                                      const torch::Tensor& lidar_depth, float acc_min, float lambda, float huber_abs,
                                      float huber_rel, float clip_abs, float clip_rel) {
  return RobustLidarDepthLossFn::apply(depth, acc, lidar_depth, static_cast<double>(acc_min),
                                       static_cast<double>(lambda), static_cast<double>(huber_abs),
                                       static_cast<double>(huber_rel), static_cast<double>(clip_abs),
                                       static_cast<double>(clip_rel));
}

Admitted admit_sweep(const torch::Tensor& points_world, const torch::Tensor& T_cw, const torch::Tensor& K,
                     int64_t height, int64_t width, float depth_tol, float occlusion_tol, const torch::Tensor& depth,
                     const torch::Tensor& acc, const torch::Tensor& image, const torch::Tensor& lidar_depth,
                     const torch::Tensor& covs, const torch::Tensor& exposure, const SweepAdmitOptions& o) {
  torch::NoGradGuard no_grad;
  const torch::Tensor p = dev_f32(points_world, "points_world");
  if (p.dim() != 2 || p.size(1) != 3) throw std::invalid_argument("admit_sweep: points_world is [n,3]");
  const torch::Tensor tcw = host_rows3(T_cw, "T_cw"), k = host_rows3(K, "K");
  if (tcw.numel() != 12 || k.numel() != 9) throw std::invalid_argument("admit_sweep: T_cw is 3x4 or 4x4, K is 3x3");
  const int64_t n = p.size(0), HW = std::max<int64_t>(height, 0) * std::max<int64_t>(width, 0);
  auto plane = [&](const torch::Tensor& t, const char* name, int64_t numel) {
    if (!t.defined()) return torch::Tensor();
    const torch::Tensor c = dev_f32(t.detach(), name);
    if (c.numel() != numel) throw std::invalid_argument(std::string("admit_sweep: bad shape of ") + name);
    return c;
  };
  const torch::Tensor d = plane(depth, "depth", HW), a = plane(acc, "acc", HW), zl = plane(lidar_depth, "lidar_depth", HW),
                      img = plane(image, "image", 3 * HW), cv = plane(covs, "covs", 9 * n), e = plane(exposure, "exposure", 6);
  const int64_t rows = std::max<int64_t>(n, 1);  // (at least one row: a null output is refused even when n == 0)
  const auto i32 = p.options().dtype(torch::kInt32);
  torch::Tensor xyz = torch::empty({rows, 3}, p.options()), cov = torch::empty({rows, 9}, p.options()),
                rgb = img.defined() ? torch::empty({rows, 3}, p.options()) : torch::Tensor(),
                index = torch::empty({rows}, i32), pixel = torch::empty({rows}, i32), z = torch::empty({rows}, p.options()),
                counts = torch::empty({6}, i32),
                reasons = o.want_reasons ? torch::empty({n}, p.options().dtype(torch::kByte)) : torch::Tensor();
  const size_t nbytes = gsr_sweep_admit_workspace(static_cast<int>(n), static_cast<int>(height), static_cast<int>(width));
  torch::Tensor ws = workspace(nbytes, p);
  check(gsr_sweep_admit(static_cast<int>(n), fp(p), fp(cv), tcw.data_ptr<float>(), k.data_ptr<float>(),
                        static_cast<int>(height), static_cast<int>(width), o.min_depth, o.max_depth, fp(d), fp(a),
                        o.acc_min, depth_tol, fp(zl), o.occlusion_radius, occlusion_tol, fp(img), fp(e), o.footprint,
                        o.one_per_pixel ? 1 : 0, xyz.data_ptr<float>(), cov.data_ptr<float>(), fp(rgb),
                        index.data_ptr<int>(), pixel.data_ptr<int>(), z.data_ptr<float>(),
                        reasons.defined() && n ? reasons.data_ptr<uint8_t>() : nullptr, counts.data_ptr<int>(),
                        reinterpret_cast<char*>(ws.data_ptr<uint8_t>()), nbytes, current_stream()),
        "gsr_sweep_admit");
  Admitted out;
  const torch::Tensor host = counts.to(torch::kCPU);  // the one host wait
  for (int q = 0; q < 6; q++) out.counts[q] = host.data_ptr<int>()[q];
  const int64_t m = out.counts[0];
  out.xyz = xyz.slice(0, 0, m);
  out.covs = cov.slice(0, 0, m).view({m, 3, 3});
  if (rgb.defined()) out.rgbs = rgb.slice(0, 0, m);
  out.index = index.slice(0, 0, m);
  out.pixel = pixel.slice(0, 0, m);
  out.z = z.slice(0, 0, m);
  out.reasons = reasons;
  return out;
}

torch::Tensor voxel_table(int64_t capacity, const torch::Tensor& like) {
  const size_t nbytes = gsr_voxel_table_bytes(capacity);
  if (!nbytes) throw std::invalid_argument("voxel_table: the capacity is a power of two up to 2^26");
  return torch::zeros({capacity, 16}, like.options().dtype(torch::kInt64));
}

torch::Tensor voxel_rehash(const torch::Tensor& table, int64_t capacity) {
  if (!table.defined() || !table.is_cuda() || table.scalar_type() != torch::kInt64 || table.dim() != 2 ||
      table.size(1) != 16 || !table.is_contiguous())
    throw std::invalid_argument("voxel_rehash: the table is a contiguous int64 [capacity,16] tensor on the device");
  torch::Tensor dst = voxel_table(capacity, table);
  check(gsr_voxel_rehash(reinterpret_cast<const long long*>(table.data_ptr<int64_t>()), table.size(0),
                         reinterpret_cast<long long*>(dst.data_ptr<int64_t>()), capacity, current_stream()),
        "gsr_voxel_rehash");
  return dst;
}

VoxelSeeds voxel_sweep(VoxelMap& map, const torch::Tensor& points, const torch::Tensor& colors, float scale_factor) {
  torch::NoGradGuard no_grad;
  const torch::Tensor p = dev_f32(points.detach(), "points");
  if (p.dim() != 2 || p.size(1) != 3) throw std::invalid_argument("voxel_sweep: points is [n,3]");
  const int64_t n = p.size(0);
  torch::Tensor c;
  if (colors.defined()) {
    c = dev_f32(colors.detach(), "colors");
    if (c.dim() != 2 || c.size(0) != n || c.size(1) != 3) throw std::invalid_argument("voxel_sweep: colors is [n,3]");
  }
  if (!map.table.defined() || map.table.scalar_type() != torch::kInt64 || map.table.dim() != 2 ||
      map.table.size(1) != 16 || !map.table.is_contiguous() || map.table.device() != p.device())
    throw std::invalid_argument("voxel_sweep: the table is a contiguous int64 [capacity,16] tensor on the points' device");
  while (2 * (map.live + n) > map.table.size(0)) map.table = voxel_rehash(map.table, 2 * map.table.size(0));
  const int64_t rows = std::max<int64_t>(n, 1);
  const auto i32 = p.options().dtype(torch::kInt32), i64 = p.options().dtype(torch::kInt64);
  torch::Tensor status = torch::empty({rows}, p.options().dtype(torch::kByte)), point_keys = torch::empty({rows}, i64),
                xyz = torch::empty({rows, 3}, p.options()), cov = torch::empty({rows, 9}, p.options()),
                rgb = c.defined() ? torch::empty({rows, 3}, p.options()) : torch::Tensor(),
                keys = torch::empty({rows}, i64), pts = torch::empty({rows}, i32),
                scaling = torch::empty({rows, 3}, p.options()), rotation = torch::empty({rows, 4}, p.options()),
                normal = torch::empty({rows, 3}, p.options()), counts = torch::empty({6}, i32);
  const size_t nbytes = gsr_voxel_sweep_workspace(static_cast<int>(n));
  torch::Tensor ws = workspace(nbytes, p);
  check(gsr_voxel_sweep(static_cast<int>(n), fp(p), fp(c), map.grid, static_cast<int>(map.min_points), map.min_sigma,
                        scale_factor, reinterpret_cast<long long*>(map.table.data_ptr<int64_t>()), map.table.size(0),
                        static_cast<int>(map.live), status.data_ptr<uint8_t>(),
                        reinterpret_cast<long long*>(point_keys.data_ptr<int64_t>()), xyz.data_ptr<float>(),
                        cov.data_ptr<float>(), fp(rgb), reinterpret_cast<long long*>(keys.data_ptr<int64_t>()),
                        pts.data_ptr<int>(), scaling.data_ptr<float>(), rotation.data_ptr<float>(),
                        normal.data_ptr<float>(), counts.data_ptr<int>(), reinterpret_cast<char*>(ws.data_ptr<uint8_t>()),
                        nbytes, current_stream()),
        "gsr_voxel_sweep");
  VoxelSeeds out;
  const torch::Tensor host = counts.to(torch::kCPU);  // the one host wait
  for (int q = 0; q < 6; q++) out.counts[q] = host.data_ptr<int>()[q];
  const int64_t v = out.counts[4];
  map.live = out.counts[5];
  out.xyz = xyz.slice(0, 0, v);
  out.covs = cov.slice(0, 0, v).view({v, 3, 3});
  if (rgb.defined()) out.rgbs = rgb.slice(0, 0, v);
  out.keys = keys.slice(0, 0, v);
  out.points = pts.slice(0, 0, v);
  out.scaling_raw = scaling.slice(0, 0, v);
  out.rotation = rotation.slice(0, 0, v);
  out.normal = normal.slice(0, 0, v);
  out.status = status.slice(0, 0, n);
  out.point_keys = point_keys.slice(0, 0, n);
  return out;
}

torch::Tensor image_metrics(const torch::Tensor& image, const torch::Tensor& gt, const torch::Tensor& window1d,
                            const torch::Tensor& totals, const torch::Tensor& weights) {
  torch::NoGradGuard no_grad;
  const torch::Tensor img = dev_f32(image, "image"), ref = dev_f32(gt, "gt");
  if (img.dim() != 3 || img.sizes() != ref.sizes()) throw std::invalid_argument("image_metrics: [C,H,W] images of one shape");
  if (totals.defined() && (!totals.is_cuda() || totals.scalar_type() != torch::kFloat64 || totals.numel() != 4 ||
                           !totals.is_contiguous()))
    throw std::invalid_argument("image_metrics: totals is a contiguous float64 tensor of 4 elements on the device");
  if (weights.defined()) {  // the forward and finish of csrc/weighted.hip: {psnr, ssim, l1, mse} out of its six
    const torch::Tensor out6 = std::get<0>(run_weighted(img, ref, weights, torch::Tensor(), 0.f, torch::Tensor(), 0.f,
                                                        window1d, false));
    const torch::Tensor out4 = out6.index({torch::tensor({5, 2, 1, 4}, torch::kLong).to(out6.device())});
    if (totals.defined()) {
      totals.slice(0, 0, 3) += out4.slice(0, 0, 3).to(torch::kFloat64);
      totals.slice(0, 3, 4) += 1.0;
    }
    return out4;
  }
  const int C = img.size(0), H = img.size(1), W = img.size(2);
  float taps[11];
  window_taps(window1d, taps);
  const size_t nbytes = gsr_image_metrics_workspace(C, H, W);
  torch::Tensor ws = workspace(nbytes, img);
  torch::Tensor out4 = torch::empty({4}, img.options());
  check(gsr_image_metrics(C, H, W, fp(img), fp(ref), taps, out4.data_ptr<float>(),
                          totals.defined() ? totals.data_ptr<double>() : nullptr,
                          reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
        "gsr_image_metrics");
  return out4;
}

torch::Tensor psnr(const torch::Tensor& image, const torch::Tensor& gt) { return image_metrics(image, gt)[0]; }

namespace {
// `out` (or a new tensor) as rows of adjacent bytes: its pitch in bytes
size_t rows_u8(torch::Tensor& out, std::vector<int64_t> shape, const torch::Tensor& like, const char* what) {
  if (!out.defined()) out = torch::empty(shape, like.options().dtype(torch::kByte));
  const int64_t row = shape[1] * (shape.size() == 3 ? shape[2] : 1);
  bool ok = out.scalar_type() == torch::kByte && out.device() == like.device() && out.sizes().vec() == shape;
  for (size_t d = 1; ok && d < shape.size(); d++)
    ok = shape[d] <= 1 || out.stride(d) == (d + 1 < shape.size() ? shape[d + 1] : 1);
  const int64_t pitch = shape[0] > 1 && ok ? out.stride(0) : row;
  if (!ok || pitch < row)
    throw std::invalid_argument(std::string(what) + ": out is a uint8 device tensor of the image's shape whose rows are adjacent bytes");
  return static_cast<size_t>(pitch);
}
}  // namespace

torch::Tensor to_u8(const torch::Tensor& image, bool bgr, torch::Tensor out) {
  torch::NoGradGuard no_grad;
  const torch::Tensor img = dev_f32(image, "image");
  if (img.dim() != 3 || img.size(0) != 3) throw std::invalid_argument("to_u8: a [3,H,W] image");
  const int64_t H = img.size(1), W = img.size(2);
  const size_t pitch = rows_u8(out, {H, W, 3}, img, "to_u8");
  check(gsr_pack_image_u8(static_cast<int>(H), static_cast<int>(W), fp(img), bgr ? 1 : 0,
                          static_cast<unsigned char*>(out.data_ptr()), pitch, current_stream()),
        "gsr_pack_image_u8");
  return out;
}

torch::Tensor depth_to_u8(const torch::Tensor& depth, float max_depth, torch::Tensor out) {
  torch::NoGradGuard no_grad;
  const torch::Tensor d = dev_f32(depth, "depth");
  if (d.dim() < 2 || d.numel() != d.size(-2) * d.size(-1)) throw std::invalid_argument("depth_to_u8: [H,W] or [1,H,W]");
  const int64_t H = d.size(-2), W = d.size(-1);
  const size_t pitch = rows_u8(out, {H, W}, d, "depth_to_u8");
  check(gsr_pack_depth_u8(static_cast<int>(H), static_cast<int>(W), fp(d), max_depth,
                          static_cast<unsigned char*>(out.data_ptr()), pitch, current_stream()),
        "gsr_pack_depth_u8");
  return out;
}

int64_t VoxelIndex::add(const std::vector<std::size_t>& keys, const std::vector<int64_t>& counts, int64_t first_row) {
  if (keys.size() != counts.size()) throw std::invalid_argument("VoxelIndex::add: one count per key");
  std::unordered_set<std::size_t> seen;
  for (size_t i = 0; i < keys.size(); i++) {
    if (counts[i] < 0) throw std::invalid_argument("VoxelIndex::add: negative count");
    if (ranges_.count(keys[i]) || !seen.insert(keys[i]).second)
      throw std::invalid_argument("VoxelIndex::add: voxel key " + std::to_string(keys[i]) + " duplicated");
  }
  int64_t row = first_row;
  for (size_t i = 0; i < keys.size(); i++) {
    ranges_.emplace(keys[i], std::make_pair(row, counts[i]));
    row += counts[i];
  }
  return row;
}

void VoxelIndex::remap(const torch::Tensor& row_map_cpu) {
  if (!row_map_cpu.defined() || row_map_cpu.numel() == 0)
    throw std::invalid_argument("VoxelIndex::remap: row_map has P + 1 entries");
  const torch::Tensor rm = row_map_cpu.to(torch::kCPU, torch::kInt64).reshape({-1}).contiguous();
  const int64_t* m = rm.data_ptr<int64_t>();
  const int64_t P = rm.numel() - 1;
  for (const auto& kv : ranges_)
    if (kv.second.first < 0 || kv.second.first + kv.second.second > P)
      throw std::invalid_argument("VoxelIndex::remap: a voxel's rows end at " +
                                  std::to_string(kv.second.first + kv.second.second) + ", row_map covers " +
                                  std::to_string(P) + " rows");
  for (auto& kv : ranges_) {
    const int64_t first = m[kv.second.first], end = m[kv.second.first + kv.second.second];
    kv.second = std::make_pair(first, end - first);
  }
}

bool VoxelIndex::get(std::size_t key, int64_t& first_row, int64_t& count) const {
  const auto it = ranges_.find(key);
  if (it == ranges_.end()) return false;
  first_row = it->second.first;
  count = it->second.second;
  return true;
}

bool VoxelIndex::select(const std::unordered_map<std::size_t, torch::Tensor>& losses, torch::Tensor& points,
                        torch::Tensor& sel, int64_t max_points, torch::Device device) const {
  std::vector<std::size_t> hit;
  for (const auto& kv : losses)
    if (ranges_.count(kv.first)) hit.push_back(kv.first);
  if (hit.empty()) return false;
  std::sort(hit.begin(), hit.end());
  std::vector<torch::Tensor> pts;
  std::vector<std::pair<int64_t, int64_t>> rng;
  int64_t n = 0;
  for (const std::size_t k : hit) {
    pts.push_back(losses.at(k).to(torch::kCPU, torch::kFloat32).reshape({-1, 3}));
    const auto r = ranges_.at(k);
    if (r.second > 0) { rng.push_back(r); n += r.second; }
  }
  torch::Tensor p = torch::cat(pts, 0);
  const int64_t m = p.size(0);
  if (m == 0 || n == 0) return false;
  std::sort(rng.begin(), rng.end());
  torch::Tensor rows = torch::empty({n}, torch::kInt32);
  int* out = rows.data_ptr<int>();
  int64_t w = 0, next = -1;  // `next`: the first row no earlier range has written (ranges may overlap: rows stay unique)
  for (const auto& r : rng)
    for (int64_t row = std::max(r.first, next); row < r.first + r.second; row++) { out[w++] = static_cast<int>(row); next = row + 1; }
  rows = rows.narrow(0, 0, w);
  if (m >= max_points) p = p.index_select(0, torch::randperm(m).slice(0, 0, max_points));
  p = p.contiguous();
  if (device.is_cuda()) { p = p.pin_memory(); rows = rows.contiguous().pin_memory(); }
  points = p.to(device, /*non_blocking=*/true);
  sel = rows.to(device, /*non_blocking=*/true);
  return true;
}

Activated activate(const torch::Tensor& scaling_raw, const torch::Tensor& rotation_raw, const torch::Tensor& opacity_raw,
                   const torch::Tensor& features_dc, const torch::Tensor& features_rest) {
  auto r = ActivateFn::apply(scaling_raw, rotation_raw, opacity_raw, features_dc, features_rest);
  return Activated{r[0], r[1], r[2], r[3]};
}

FusedAdam::FusedAdam(std::vector<torch::Tensor> params, std::vector<double> lrs, double beta1, double beta2, double eps)
    : params_(std::move(params)), lrs_(std::move(lrs)), beta1_(beta1), beta2_(beta2), eps_(eps) {
  if (params_.size() != lrs_.size()) throw std::invalid_argument("FusedAdam: one learning rate per parameter tensor");
  for (const auto& p : params_) {
    if (!p.is_cuda() || p.scalar_type() != torch::kFloat32 || !p.is_contiguous())
      throw std::invalid_argument("FusedAdam: contiguous float32 device tensors");
    m_.push_back(torch::zeros_like(p));
    v_.push_back(torch::zeros_like(p));
  }
}

void FusedAdam::step(bool zero_grad) {
  torch::NoGradGuard no_grad;
  std::vector<size_t> idx;
  for (size_t k = 0; k < params_.size(); k++)
    if (params_[k].numel() && params_[k].grad().defined()) idx.push_back(k);
  ++step_;
  for (size_t b = 0; b < idx.size(); b += 8) {
    float *p[8], *g[8], *m[8], *v[8];
    size_t numel[8];
    float lr[8];
    std::vector<torch::Tensor> keep;
    const int n = static_cast<int>(std::min<size_t>(8, idx.size() - b));
    for (int j = 0; j < n; j++) {
      const size_t k = idx[b + j];
      torch::Tensor grad = params_[k].grad();
      if (!grad.is_contiguous()) throw std::invalid_argument("FusedAdam: non-contiguous gradient");
      p[j] = params_[k].data_ptr<float>(); g[j] = grad.data_ptr<float>();
      m[j] = m_[k].data_ptr<float>(); v[j] = v_[k].data_ptr<float>();
      numel[j] = static_cast<size_t>(params_[k].numel());
      lr[j] = static_cast<float>(lrs_[k]);
    }
    check(gsr_adam_step(n, p, g, m, v, numel, lr, beta1_, beta2_, eps_, static_cast<int>(step_), zero_grad ? 1 : 0,
                        current_stream()),
          "gsr_adam_step");
  }
}

Activated FusedAdam::step_model(const torch::Tensor& g_xyz, const torch::Tensor& g_scaling,
                                const torch::Tensor& g_rotation, const torch::Tensor& g_opacity,
                                const torch::Tensor& g_features) {
  torch::NoGradGuard no_grad;
  if (params_.size() != 6) throw std::invalid_argument("FusedAdam::step_model: the six leaves of a GaussianModel");
  const int P = params_[0].size(0), M = coefficients(params_[2]);
  const torch::Tensor gx = dev_f32(g_xyz, "g_xyz"), gs = dev_f32(g_scaling, "g_scaling"),
                      gr = dev_f32(g_rotation, "g_rotation"), go = dev_f32(g_opacity, "g_opacity"),
                      gf = dev_f32(g_features, "g_features");
  float *p[6], *m[6], *v[6], lr[6];
  for (int k = 0; k < 6; k++) {
    p[k] = fp(params_[k]); m[k] = fp(m_[k]); v[k] = fp(v_[k]);
    lr[k] = static_cast<float>(lrs_[k]);
  }
  const auto o = params_[0].options();
  Activated a{torch::empty({P, 3}, o), torch::empty({P, 4}, o), torch::empty({P, 1}, o), torch::empty({P, M, 3}, o)};
  ++step_;
  check(gsr_model_step(P, M, p, m, v, fp(gx), fp(gs), fp(gr), fp(go), fp(gf), fp(a.scaling), fp(a.rotation),
                       fp(a.opacity), fp(a.features), lr, beta1_, beta2_, eps_, static_cast<int>(step_),
                       current_stream()),
        "gsr_model_step");
  return a;
}

void FusedAdam::replace_param(size_t index, torch::Tensor new_param) {
  torch::NoGradGuard no_grad;
  if (index >= params_.size()) throw std::out_of_range("FusedAdam::replace_param");
  const int64_t old_rows = params_[index].size(0), new_rows = new_param.size(0);
  if (new_rows < old_rows) throw std::invalid_argument("FusedAdam::replace_param: the tensor shrank");
  auto grow = [&](torch::Tensor& mom) {  // cat({old, zeros_like(extension)}), gaussian.cu:462-466
    torch::Tensor t = torch::zeros_like(new_param);
    if (old_rows) t.narrow(0, 0, old_rows).copy_(mom);
    mom = t;
  };
  grow(m_[index]);
  grow(v_[index]);
  params_[index] = std::move(new_param);
}

PruneMarks prune_mark(const torch::Tensor& xyz, const torch::Tensor& scaling_raw, const torch::Tensor& rotation_raw,
                      const torch::Tensor& opacity_raw, float min_opacity, float max_scale, bool drop_nonfinite,
                      const torch::Tensor& drop) {
  torch::NoGradGuard no_grad;
  const torch::Tensor x = dev_f32(xyz, "xyz"), s = dev_f32(scaling_raw, "_scaling"), r = dev_f32(rotation_raw, "_rotation"),
                      o = dev_f32(opacity_raw, "_opacity");
  const int64_t P = x.size(0);
  if (x.numel() != 3 * P || s.numel() != 3 * P || r.numel() != 4 * P || o.numel() != P)
    throw std::invalid_argument("prune_mark: xyz [P,3], scaling [P,3], rotation [P,4], opacity [P,1]");
  torch::Tensor mask;
  if (drop.defined()) {
    if (!drop.is_cuda() || (drop.scalar_type() != torch::kBool && drop.scalar_type() != torch::kByte) || drop.numel() != P)
      throw std::invalid_argument("prune_mark: drop is a bool or uint8 device tensor of P entries");
    mask = drop.contiguous();
  }
  const auto bytes = x.options().dtype(torch::kByte), ints = x.options().dtype(torch::kInt32);
  PruneMarks out{torch::empty({P}, bytes), torch::empty({P + 1}, ints), torch::empty({5}, ints)};
  const size_t nbytes = gsr_prune_workspace(static_cast<int>(P));
  torch::Tensor ws = workspace(nbytes, x);
  check(gsr_prune_mark(static_cast<int>(P), fp(x), fp(s), fp(r), fp(o),
                       mask.defined() && P ? static_cast<const unsigned char*>(mask.data_ptr()) : nullptr, min_opacity,
                       max_scale, drop_nonfinite ? 1 : 0, P ? out.reasons.data_ptr<unsigned char>() : nullptr,
                       out.row_map.data_ptr<int>(), out.counts.data_ptr<int>(), reinterpret_cast<char*>(ws.data_ptr()),
                       nbytes, current_stream()),
        "gsr_prune_mark");
  return out;
}

void density_accumulate(const torch::Tensor& radii, const torch::Tensor& dL_dmean2D, torch::Tensor stats) {
  torch::NoGradGuard no_grad;
  const int64_t P = radii.numel();
  if (!radii.is_cuda() || radii.scalar_type() != torch::kInt32 || !radii.is_contiguous())
    throw std::invalid_argument("density_accumulate: radii is a contiguous int32 device tensor");
  const torch::Tensor g = dev_f32(dL_dmean2D, "dL_dmean2D");
  if (!stats.defined() || !stats.is_cuda() || stats.scalar_type() != torch::kFloat32 || !stats.is_contiguous() ||
      stats.numel() != 3 * P || g.numel() != 3 * P)
    throw std::invalid_argument("density_accumulate: dL_dmean2D [P,3], stats [P,3] contiguous f32 on the device");
  check(gsr_density_accumulate(static_cast<int>(P), P ? radii.data_ptr<int>() : nullptr, fp(g), fp(stats),
                               current_stream()),
        "gsr_density_accumulate");
}

DensifyMarks densify_mark(const torch::Tensor& stats, const torch::Tensor& scaling_raw, float grad_threshold,
                          float size_threshold, int64_t max_new) {
  torch::NoGradGuard no_grad;
  const torch::Tensor st = dev_f32(stats, "stats"), s = dev_f32(scaling_raw, "_scaling");
  const int64_t P = st.size(0);
  if (st.numel() != 3 * P || s.numel() != 3 * P) throw std::invalid_argument("densify_mark: stats [P,3], scaling [P,3]");
  const auto bytes = st.options().dtype(torch::kByte), ints = st.options().dtype(torch::kInt32);
  DensifyMarks out{torch::empty({P}, bytes), torch::empty({P + 1}, ints), torch::empty({3}, ints)};
  const size_t nbytes = gsr_densify_workspace(static_cast<int>(P));
  torch::Tensor ws = workspace(nbytes, st);
  check(gsr_densify_mark(static_cast<int>(P), fp(st), fp(s), grad_threshold, size_threshold,
                         max_new < 0 ? -1 : static_cast<int>(std::min<int64_t>(max_new, 0x7fffffff)),
                         P ? out.kinds.data_ptr<unsigned char>() : nullptr, out.offsets.data_ptr<int>(),
                         out.counts.data_ptr<int>(), reinterpret_cast<char*>(ws.data_ptr()), nbytes, current_stream()),
        "gsr_densify_mark");
  return out;
}

void densify_apply(int64_t P, int64_t n_new, const torch::Tensor& kinds, const torch::Tensor& offsets, uint64_t seed,
                   const std::vector<torch::Tensor>& params6, const std::vector<torch::Tensor>& exp_avg6,
                   const std::vector<torch::Tensor>& exp_avg_sq6, const torch::Tensor& stats) {
  torch::NoGradGuard no_grad;
  if (P < 0 || n_new < 0 || P + n_new > GSR_PRUNE_MAX_ROWS) throw std::invalid_argument("densify_apply: bad P / n_new");
  if (!kinds.is_cuda() || kinds.scalar_type() != torch::kByte || !kinds.is_contiguous() || kinds.numel() != P ||
      !offsets.is_cuda() || offsets.scalar_type() != torch::kInt32 || !offsets.is_contiguous() || offsets.numel() != P + 1)
    throw std::invalid_argument("densify_apply: kinds [P] uint8 and offsets [P+1] int32 on the device, from densify_mark");
  if (params6.size() != 6 || (!exp_avg6.empty() && exp_avg6.size() != 6) ||
      (!exp_avg_sq6.empty() && exp_avg_sq6.size() != 6))
    throw std::invalid_argument("densify_apply: six leaves; six moments of a kind or none");
  // the surgery is in place: a buffer is taken as it is, never copied
  auto buffer = [&](const torch::Tensor& t) {
    if (!t.defined() || !t.is_cuda() || t.scalar_type() != torch::kFloat32 || !t.is_contiguous() ||
        (t.numel() && t.size(0) < P + n_new))
      throw std::invalid_argument("densify_apply: expected contiguous float32 device buffers of at least P + n_new rows");
    return fp(t);
  };
  float *p[6], *m[6], *v[6];
  for (int k = 0; k < 6; k++) {
    p[k] = buffer(params6[k]);
    m[k] = exp_avg6.empty() ? nullptr : buffer(exp_avg6[k]);
    v[k] = exp_avg_sq6.empty() ? nullptr : buffer(exp_avg_sq6[k]);
  }
  const int M = 1 + static_cast<int>(params6[2].numel() ? params6[2].size(1) : 0);
  check(gsr_densify_apply(static_cast<int>(P), M, static_cast<int>(n_new), P ? kinds.data_ptr<unsigned char>() : nullptr,
                          offsets.data_ptr<int>(), seed, p[0], p[1], p[2], p[3], p[4], p[5],
                          exp_avg6.empty() ? nullptr : m, exp_avg_sq6.empty() ? nullptr : v,
                          stats.defined() ? buffer(stats) : nullptr, current_stream()),
        "gsr_densify_apply");
}

namespace {
// A slab of visibility rows: a 2-D int64 device tensor with contiguous rows (a 1-D tensor is one row); the pitch is its
// row stride in words.
struct Slab {
  torch::Tensor t;
  int64_t rows, pitch;
  unsigned long long* ptr() const { return reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>()); }
};
Slab slab(const torch::Tensor& bits, const char* what) {
  torch::Tensor t = bits.defined() && bits.dim() == 1 ? bits.unsqueeze(0) : bits;
  if (!t.defined() || !t.is_cuda() || t.scalar_type() != torch::kInt64 || t.dim() != 2 || t.size(0) < 1 || t.size(1) < 1 ||
      (t.size(1) > 1 && t.stride(1) != 1))
    throw std::invalid_argument(std::string(what) + ": expected an int64 device tensor [rows, words] with contiguous rows");
  const int64_t pitch = t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(t.stride(0), t.size(1));
  return Slab{t, t.size(0), pitch};
}
int64_t words_of(int64_t P) { return (P + 63) / 64; }
}  // namespace

torch::Tensor visibility_pack(const torch::Tensor& source, int64_t words) {
  torch::NoGradGuard no_grad;
  if (!source.defined() || !source.is_cuda())
    throw std::invalid_argument("visibility_pack: int32 radii or a bool / uint8 mask on the device");
  const torch::Tensor src = source.reshape({-1}).contiguous();
  const int64_t P = src.numel();
  const int* radii = nullptr;
  const unsigned char* mask = nullptr;
  if (src.scalar_type() == torch::kInt32) radii = P ? src.data_ptr<int>() : nullptr;
  else if (src.scalar_type() == torch::kBool || src.scalar_type() == torch::kByte)
    mask = P ? static_cast<const unsigned char*>(src.data_ptr()) : nullptr;
  else throw std::invalid_argument("visibility_pack: int32 radii or a bool / uint8 mask on the device");
  if (words <= 0) words = words_of(P);
  torch::Tensor out = torch::empty({words}, src.options().dtype(torch::kInt64));
  check(gsr_visibility_pack(static_cast<int>(P), radii, mask, reinterpret_cast<unsigned long long*>(out.data_ptr<int64_t>()),
                            static_cast<int>(std::min<int64_t>(words, 0x7fffffff)), current_stream()),
        "gsr_visibility_pack");
  return out;
}

Covisibility covisibility(const torch::Tensor& q_bits, const torch::Tensor& k_bits, int64_t words, bool counts) {
  torch::NoGradGuard no_grad;
  const Slab q = slab(q_bits, "covisibility");
  const Slab k = k_bits.defined() ? slab(k_bits, "covisibility") : q;
  if (words <= 0) words = std::min(q.t.size(1), k.t.size(1));
  if (words > q.t.size(1) || words > k.t.size(1)) throw std::invalid_argument("covisibility: a row holds fewer words");
  const auto ints = q.t.options().dtype(torch::kInt32);
  Covisibility out;
  out.inter = torch::empty({q.rows, k.rows}, ints);
  if (counts) {
    out.q_count = torch::empty({q.rows}, ints);
    out.k_count = torch::empty({k.rows}, ints);
  }
  check(gsr_covisibility(static_cast<int>(q.rows), q.ptr(), q.pitch, static_cast<int>(k.rows), k.ptr(), k.pitch,
                         static_cast<int>(std::min<int64_t>(words, 0x7fffffff)), out.inter.data_ptr<int>(),
                         counts ? out.q_count.data_ptr<int>() : nullptr, counts ? out.k_count.data_ptr<int>() : nullptr,
                         current_stream()),
        "gsr_covisibility");
  return out;
}

ObservationCount observation_count(const torch::Tensor& bits, int64_t P, int64_t first_row, int64_t min_count,
                                   bool want_count, bool want_drop) {
  torch::NoGradGuard no_grad;
  const Slab b = slab(bits, "observation_count");
  const auto int32 = [](int64_t v) { return v >= -0x7fffffffLL && v <= 0x7fffffffLL; };
  if (P < 0 || !int32(P) || !int32(first_row) || !int32(min_count))
    throw std::invalid_argument("observation_count: P, first_row and min_count are int32, P is not negative");
  if (b.t.size(1) < words_of(P)) throw std::invalid_argument("observation_count: the rows hold fewer than ceil(P / 64) words");
  ObservationCount out;
  if (want_count) out.count = torch::empty({P}, b.t.options().dtype(torch::kInt32));
  if (want_drop) out.drop = torch::empty({P}, b.t.options().dtype(torch::kByte));
  check(gsr_observation_count(static_cast<int>(b.rows), b.ptr(), b.pitch, static_cast<int>(P), static_cast<int>(first_row),
                              static_cast<int>(min_count), want_count && P ? out.count.data_ptr<int>() : nullptr,
                              want_drop && P ? out.drop.data_ptr<unsigned char>() : nullptr, current_stream()),
        "gsr_observation_count");
  return out;
}

torch::Tensor visibility_remap(const torch::Tensor& src, const torch::Tensor& reasons, const torch::Tensor& row_map,
                               int64_t dst_words) {
  torch::NoGradGuard no_grad;
  const Slab s = slab(src, "visibility_remap");
  const int64_t P = reasons.defined() ? reasons.numel() : 0;
  if (!reasons.defined() || !reasons.is_cuda() || reasons.scalar_type() != torch::kByte || !reasons.is_contiguous() ||
      !row_map.defined() || !row_map.is_cuda() || row_map.scalar_type() != torch::kInt32 || !row_map.is_contiguous() ||
      row_map.numel() != P + 1)
    throw std::invalid_argument("visibility_remap: reasons [P] uint8 and row_map [P+1] int32 on the device, from prune_mark");
  if (s.t.size(1) < words_of(P)) throw std::invalid_argument("visibility_remap: the source rows hold fewer than ceil(P / 64) words");
  if (dst_words <= 0) dst_words = words_of(P);
  torch::Tensor dst = torch::empty({s.rows, dst_words}, s.t.options());
  check(gsr_visibility_remap(static_cast<int>(s.rows), s.ptr(), s.pitch, static_cast<int>(P),
                             P ? reasons.data_ptr<unsigned char>() : nullptr, row_map.data_ptr<int>(),
                             reinterpret_cast<unsigned long long*>(dst.numel() ? dst.data_ptr<int64_t>() : nullptr),
                             dst_words, static_cast<int>(std::min<int64_t>(dst_words, 0x7fffffff)), current_stream()),
        "gsr_visibility_remap");
  return dst;
}

torch::Tensor contribution(const torch::Tensor& geom, const torch::Tensor& binning, const torch::Tensor& img, int64_t P,
                           int64_t R, int64_t W, int64_t H) {
  torch::NoGradGuard no_grad;
  const auto int32 = [](int64_t v) { return v >= 0 && v <= 0x7fffffffLL; };
  if (!int32(P) || !int32(R) || !int32(W) || !int32(H))
    throw std::invalid_argument("contribution: P, R, W and H are non-negative int32");
  for (const torch::Tensor* t : {&geom, &binning, &img})
    if (!t->defined() || !t->is_cuda() || !t->is_contiguous())
      throw std::invalid_argument("contribution: the forward's three blobs, contiguous on the device");
  const auto blob = [](const torch::Tensor& t) { return t.numel() ? static_cast<const char*>(t.data_ptr()) : nullptr; };
  torch::Tensor rows = torch::empty({P, 2}, geom.options().dtype(torch::kInt64));
  check(gsr_contribution(static_cast<int>(P), static_cast<int>(R), static_cast<int>(W), static_cast<int>(H), blob(geom),
                         blob(binning), blob(img), P ? static_cast<char*>(rows.data_ptr()) : nullptr, current_stream()),
        "gsr_contribution");
  return rows;
}

Contribution contribution_finish(const torch::Tensor& rows, int64_t min_pixels, double min_weight, bool want_n_touched,
                                 bool want_weight_sum, bool want_weight_max, bool want_mask, const torch::Tensor& stats) {
  torch::NoGradGuard no_grad;
  if (!rows.defined() || !rows.is_cuda() || rows.scalar_type() != torch::kInt64 || !rows.is_contiguous() ||
      rows.dim() != 2 || rows.size(1) != 2)
    throw std::invalid_argument("contribution_finish: rows is what contribution returned, [P, 2] int64 on the device");
  const int64_t P = rows.size(0);
  if (stats.defined() && (!stats.is_cuda() || stats.scalar_type() != torch::kFloat32 || !stats.is_contiguous() ||
                          stats.dim() != 2 || stats.size(0) != P || stats.size(1) != 3))
    throw std::invalid_argument("contribution_finish: stats is a contiguous [P, 3] float32 device tensor");
  if (min_pixels < -0x7fffffffLL || min_pixels > 0x7fffffffLL)
    throw std::invalid_argument("contribution_finish: min_pixels is int32");
  Contribution out;
  if (want_n_touched) out.n_touched = torch::empty({P}, rows.options().dtype(torch::kInt32));
  if (want_weight_sum) out.weight_sum = torch::empty({P}, rows.options().dtype(torch::kFloat32));
  if (want_weight_max) out.weight_max = torch::empty({P}, rows.options().dtype(torch::kFloat32));
  if (want_mask) out.mask = torch::empty({P}, rows.options().dtype(torch::kByte));
  if (P == 0) return out;  // (an empty model: empty outputs, nothing to launch)
  check(gsr_contribution_finish(static_cast<int>(P), static_cast<const char*>(rows.data_ptr()),
                                static_cast<int>(min_pixels), static_cast<float>(min_weight),
                                want_n_touched ? out.n_touched.data_ptr<int>() : nullptr,
                                want_weight_sum ? out.weight_sum.data_ptr<float>() : nullptr,
                                want_weight_max ? out.weight_max.data_ptr<float>() : nullptr,
                                want_mask ? out.mask.data_ptr<unsigned char>() : nullptr,
                                stats.defined() ? stats.data_ptr<float>() : nullptr, current_stream()),
        "gsr_contribution_finish");
  return out;
}

torch::Tensor blend_attributes(const torch::Tensor& geom, const torch::Tensor& binning, const torch::Tensor& img,
                               const torch::Tensor& attributes, int64_t R, int64_t W, int64_t H) {
  torch::NoGradGuard no_grad;
  torch::Tensor at = dev_f32(attributes.detach(), "attributes");
  if (at.dim() == 1) at = at.unsqueeze(1);
  if (at.dim() != 2 || at.size(1) < 1 || at.size(1) > 4)
    throw std::invalid_argument("blend_attributes: attributes is [P, C] with C in 1..4");
  const int64_t P = at.size(0), C = at.size(1);
  const auto int32 = [](int64_t v) { return v >= 0 && v <= 0x7fffffffLL; };
  if (!int32(P) || !int32(R) || !int32(W) || !int32(H))
    throw std::invalid_argument("blend_attributes: P, R, W and H are non-negative int32");
  for (const torch::Tensor* t : {&geom, &binning, &img})
    if (!t->defined() || !t->is_cuda() || !t->is_contiguous())
      throw std::invalid_argument("blend_attributes: the forward's three blobs, contiguous on the device");
  const auto blob = [](const torch::Tensor& t) { return t.numel() ? static_cast<const char*>(t.data_ptr()) : nullptr; };
  torch::Tensor out = torch::empty({C, H, W}, at.options());
  check(gsr_blend_attributes(static_cast<int>(P), static_cast<int>(R), static_cast<int>(W), static_cast<int>(H),
                             static_cast<int>(C), fp(at), blob(geom), blob(binning), blob(img), fp(out),
                             current_stream()),
        "gsr_blend_attributes");
  return out;
}

torch::Tensor surfel_normals(const torch::Tensor& xyz, const torch::Tensor& scaling, const torch::Tensor& rotation,
                             const torch::Tensor& T_cw) {
  torch::NoGradGuard no_grad;
  const torch::Tensor x = dev_f32(xyz.detach(), "xyz"), sc = dev_f32(scaling.detach(), "scaling"),
                      q = dev_f32(rotation.detach(), "rotation");
  const int64_t P = x.dim() == 2 ? x.size(0) : -1;
  if (P < 0 || x.size(1) != 3 || sc.dim() != 2 || sc.size(0) != P || sc.size(1) != 3 || q.dim() != 2 ||
      q.size(0) != P || q.size(1) != 4)
    throw std::invalid_argument("surfel_normals: xyz [P,3], scaling [P,3], rotation [P,4]");
  const torch::Tensor tcw = host_rows3(T_cw, "T_cw");
  if (tcw.numel() != 12) throw std::invalid_argument("surfel_normals: T_cw is 3x4 or 4x4");
  torch::Tensor out = torch::empty({P, 3}, x.options());
  check(gsr_surfel_normals(static_cast<int>(P), fp(x), fp(sc), fp(q), tcw.data_ptr<float>(), fp(out), current_stream()),
        "gsr_surfel_normals");
  return out;
}

torch::Tensor normal_consistency_loss(const torch::Tensor& depth, const torch::Tensor& acc,
                                      const torch::Tensor& normals, const torch::Tensor& K, float acc_min, float lambda,
                                      float normal_min, float jump_rel) {
  const torch::Tensor k = host_rows3(K, "K");
  if (k.numel() != 9) throw std::invalid_argument("normal_consistency_loss: K is 3x3");
  const float* const kp = k.data_ptr<float>();
  return NormalConsistencyLossFn::apply(depth, acc, normals.detach(), static_cast<double>(kp[0]),
                                        static_cast<double>(kp[4]), static_cast<double>(kp[2]),
                                        static_cast<double>(kp[5]), static_cast<double>(acc_min),
                                        static_cast<double>(normal_min), static_cast<double>(jump_rel),
                                        static_cast<double>(lambda));
}

namespace {
// dst[k][row_map[i]] = src[k][i] where reasons[i] == 0, at most eighteen tensors: one launch
void compact18(const std::vector<torch::Tensor>& src, const std::vector<torch::Tensor>& dst, const torch::Tensor& reasons,
               const torch::Tensor& row_map) {
  const int64_t P = reasons.numel();
  if (!reasons.is_cuda() || reasons.scalar_type() != torch::kByte || !reasons.is_contiguous() || !row_map.is_cuda() ||
      row_map.scalar_type() != torch::kInt32 || !row_map.is_contiguous() || row_map.numel() != P + 1)
    throw std::invalid_argument("prune: reasons [P] uint8 and row_map [P+1] int32 on the device, from prune_mark");
  const float* s[18];
  float* d[18];
  int w[18];
  const int n = static_cast<int>(src.size());
  for (int k = 0; k < n; k++) {
    if (src[k].size(0) != P) throw std::invalid_argument("prune: a tensor does not have P rows");
    s[k] = fp(src[k]); d[k] = fp(dst[k]);
    w[k] = P ? static_cast<int>(src[k].numel() / P) : 0;
  }
  check(gsr_prune_compact(static_cast<int>(P), n, s, d, w, P ? reasons.data_ptr<unsigned char>() : nullptr,
                          row_map.data_ptr<int>(), current_stream()),
        "gsr_prune_compact");
}

torch::Tensor rows_like(const torch::Tensor& t, int64_t rows) {
  std::vector<int64_t> shape = t.sizes().vec();
  shape[0] = rows;
  return torch::empty(shape, t.options().requires_grad(false));
}
}  // namespace

std::vector<torch::Tensor> prune_rows(const std::vector<torch::Tensor>& tensors, const torch::Tensor& reasons,
                                      const torch::Tensor& row_map, int64_t P_new) {
  torch::NoGradGuard no_grad;
  std::vector<torch::Tensor> out;
  for (size_t b = 0; b < tensors.size(); b += 18) {
    std::vector<torch::Tensor> src, dst;
    for (size_t k = b; k < std::min(tensors.size(), b + 18); k++) {
      src.push_back(dev_f32(tensors[k], "tensor").detach());
      dst.push_back(rows_like(src.back(), P_new));
    }
    compact18(src, dst, reasons, row_map);
    out.insert(out.end(), dst.begin(), dst.end());
  }
  return out;
}

void FusedAdam::prune(const torch::Tensor& reasons, const torch::Tensor& row_map, int64_t P_new) {
  torch::NoGradGuard no_grad;
  if (3 * params_.size() > 18) throw std::invalid_argument("FusedAdam::prune: at most six parameter tensors");
  std::vector<torch::Tensor> src;
  for (size_t k = 0; k < params_.size(); k++) {
    src.push_back(params_[k]);
    src.push_back(m_[k]);
    src.push_back(v_[k]);
  }
  const std::vector<torch::Tensor> dst = prune_rows(src, reasons, row_map, P_new);
  for (size_t k = 0; k < params_.size(); k++) {
    const bool rg = params_[k].requires_grad();
    params_[k] = dst[3 * k];
    params_[k].set_requires_grad(rg);
    m_[k] = dst[3 * k + 1];
    v_[k] = dst[3 * k + 2];
  }
}

void init_gaussians(const torch::Tensor& xyz, const torch::Tensor& covs, const torch::Tensor& rgbs, float scale_factor,
                    torch::Tensor xyz_out, torch::Tensor features_dc_out, torch::Tensor features_rest_out,
                    torch::Tensor scaling_out, torch::Tensor rotation_out, torch::Tensor opacity_out) {
  torch::NoGradGuard no_grad;
  const torch::Tensor x = dev_f32(xyz, "xyz"), c = dev_f32(covs, "covs"), rgb = dev_f32(rgbs, "rgbs");
  const int n = x.size(0), M = coefficients(features_rest_out);
  if (c.dim() != 3 || c.size(0) != n || c.size(1) != 3 || c.size(2) != 3 || rgb.size(0) != n)
    throw std::invalid_argument("init_gaussians: xyz [n,3], covs [n,3,3], rgbs [n,3]");
  for (const torch::Tensor* t : {&xyz_out, &features_dc_out, &scaling_out, &rotation_out, &opacity_out})
    if (!t->is_cuda() || !t->is_contiguous() || t->size(0) != n)
      throw std::invalid_argument("init_gaussians: outputs are contiguous n-row device views");
  if (M > 1 && (!features_rest_out.is_contiguous() || features_rest_out.size(0) != n))
    throw std::invalid_argument("init_gaussians: features_rest output");
  check(gsr_init_gaussians(n, M, fp(x), fp(c), fp(rgb), scale_factor, fp(xyz_out), fp(features_dc_out),
                           fp(features_rest_out), fp(scaling_out), fp(rotation_out), fp(opacity_out), current_stream()),
        "gsr_init_gaussians");
}

torch::Tensor pack_ply_rows(const torch::Tensor& xyz, const torch::Tensor& features_dc,
                            const torch::Tensor& features_rest, const torch::Tensor& opacity,
                            const torch::Tensor& scaling, const torch::Tensor& rotation) {
  torch::NoGradGuard no_grad;
  const torch::Tensor x = dev_f32(xyz, "xyz"), dc = dev_f32(features_dc, "features_dc"),
                      rest = dev_f32(features_rest, "features_rest"), o = dev_f32(opacity, "opacity"),
                      s = dev_f32(scaling, "scaling"), r = dev_f32(rotation, "rotation");
  const int P = x.size(0), M = coefficients(rest);
  torch::Tensor rows = torch::empty({P, static_cast<long long>(gsr_ply_row_floats(M))}, x.options());
  check(gsr_pack_ply_rows(P, M, fp(x), fp(dc), fp(rest), fp(o), fp(s), fp(r), fp(rows), current_stream()),
        "gsr_pack_ply_rows");
  return rows;
}

std::vector<std::string> ply_attribute_names(int M) {  // construct_list_of_attributes, gaussian.cu:474-492
  std::vector<std::string> names = {"x", "y", "z", "nx", "ny", "nz"};
  for (int i = 0; i < 3; i++) names.push_back("f_dc_" + std::to_string(i));
  for (int i = 0; i < 3 * (M - 1); i++) names.push_back("f_rest_" + std::to_string(i));
  names.push_back("opacity");
  for (int i = 0; i < 3; i++) names.push_back("scale_" + std::to_string(i));
  for (int i = 0; i < 4; i++) names.push_back("rot_" + std::to_string(i));
  return names;
}

size_t write_ply(const std::string& file_path, const torch::Tensor& xyz, const torch::Tensor& features_dc,
                 const torch::Tensor& features_rest, const torch::Tensor& opacity, const torch::Tensor& scaling,
                 const torch::Tensor& rotation) {
  const torch::Tensor rows = pack_ply_rows(xyz, features_dc, features_rest, opacity, scaling, rotation).cpu();  // ONE D2H copy
  const int M = coefficients(features_rest);
  std::string header = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(rows.size(0)) + "\n";
  for (const auto& n : ply_attribute_names(M)) header += "property float " + n + "\n";
  header += "end_header\n";
  FILE* f = std::fopen(file_path.c_str(), "wb");
  if (!f) throw std::runtime_error("write_ply: cannot open " + file_path);
  const size_t nbytes = static_cast<size_t>(rows.numel()) * sizeof(float);
  const bool ok = std::fwrite(header.data(), 1, header.size(), f) == header.size() &&
                  (nbytes == 0 || std::fwrite(rows.data_ptr<float>(), 1, nbytes, f) == nbytes);
  if (std::fclose(f) != 0 || !ok) throw std::runtime_error("write_ply: short write to " + file_path);
  return header.size() + nbytes;
}

// ---- camera pose gradient ------------------------------------------------------------------------------------------
torch::Tensor pose_gradient(const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& scales,
                            const torch::Tensor& rotations, float scale_modifier, const torch::Tensor& cov3D_precomp,
                            const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, float tan_fovx,
                            float tan_fovy, int image_height, int image_width, const torch::Tensor& dL_dmeans2D,
                            const torch::Tensor& dL_dconic, const torch::Tensor& dL_dmeans3D,
                            const torch::Tensor& dL_ddepths) {
  const torch::Tensor m3 = dev_f32(means3D, "means3D");
  const int64_t P = m3.size(0);
  auto given = [](const torch::Tensor& t) { return t.defined() && t.numel() != 0; };
  auto c = [&](const torch::Tensor& t) { return given(t) ? t.contiguous() : torch::Tensor(); };
  const torch::Tensor sc = c(scales), cov = c(cov3D_precomp), view = c(viewmatrix), proj = c(projmatrix), rad = c(radii),
                      g2 = c(dL_dmeans2D), gc = c(dL_dconic), g3 = c(dL_dmeans3D), gz = c(dL_ddepths);
  torch::Tensor rot = c(rotations);
  if (given(rot) && (reinterpret_cast<uintptr_t>(rot.data_ptr()) & 15u) != 0) rot = rot.clone();  // read as float4
  if (given(rad) && rad.scalar_type() != torch::kInt32) throw std::invalid_argument("pose_gradient: radii is int32");
  const size_t nbytes = gsr_pose_gradient_workspace(static_cast<int>(P));
  torch::Tensor ws = workspace(nbytes, m3);
  torch::Tensor out = torch::empty({6}, m3.options());
  check(gsr_pose_gradient(static_cast<int>(P), image_width, image_height, fp(m3), fp(sc), scale_modifier, fp(rot), fp(cov),
                          fp(view), fp(proj), tan_fovx, tan_fovy, given(rad) ? rad.data_ptr<int>() : nullptr, fp(g2),
                          fp(gc), fp(gz), fp(g3), out.data_ptr<float>(), reinterpret_cast<char*>(ws.data_ptr()), nbytes,
                          current_stream()),
        "gsr_pose_gradient");
  return out;
}

// Exp(xi^) = [[R, V rho], [0, 1]]: below |phi| = 0.5 the three coefficients by their series in |phi|^2 (no cancellation,
// analytic at 0), above it in closed form; tensor ops only, so nothing waits (render_utils.py: se3_exp, the same terms).
torch::Tensor se3_exp(const torch::Tensor& xi) {
  if (xi.dim() != 1 || xi.size(0) != 6) throw std::invalid_argument("se3_exp: xi is a tensor of shape (6,)");
  const torch::Tensor rho = xi.slice(0, 0, 3), phi = xi.slice(0, 3, 6);
  const torch::Tensor t2 = (phi * phi).sum();
  const torch::Tensor one = torch::ones_like(t2);
  const torch::Tensor big = t2 > 0.25;
  const torch::Tensor t = torch::sqrt(torch::where(big, t2, one));
  const torch::Tensor h = torch::sin(0.5 * t) / (0.5 * t);
  const torch::Tensor sA = 1.0 + t2 * (-1.0 / 6.0 + t2 * (1.0 / 120.0 + t2 * (-1.0 / 5040.0 + t2 * (1.0 / 362880.0 + t2 * (-1.0 / 39916800.0 + t2 * (1.0 / 6227020800.0))))));
  const torch::Tensor sB = 0.5 + t2 * (-1.0 / 24.0 + t2 * (1.0 / 720.0 + t2 * (-1.0 / 40320.0 + t2 * (1.0 / 3628800.0 + t2 * (-1.0 / 479001600.0 + t2 * (1.0 / 87178291200.0))))));
  const torch::Tensor sC = 1.0 / 6.0 + t2 * (-1.0 / 120.0 + t2 * (1.0 / 5040.0 + t2 * (-1.0 / 362880.0 + t2 * (1.0 / 39916800.0 + t2 * (-1.0 / 6227020800.0)))));
  const torch::Tensor A = torch::where(big, torch::sin(t) / t, sA);
  const torch::Tensor B = torch::where(big, 0.5 * h * h, sB);
  const torch::Tensor C = torch::where(big, (t - torch::sin(t)) / (t * t * t), sC);
  const torch::Tensor z = torch::zeros_like(t2);
  const torch::Tensor K = torch::stack({torch::stack({z, -phi[2], phi[1]}), torch::stack({phi[2], z, -phi[0]}),
                                        torch::stack({-phi[1], phi[0], z})});
  const torch::Tensor K2 = torch::matmul(K, K);
  const torch::Tensor eye = torch::eye(3, xi.options());
  const torch::Tensor Rm = eye + A * K + B * K2, V = eye + B * K + C * K2;
  const torch::Tensor top = torch::cat({Rm, torch::matmul(V, rho).unsqueeze(1)}, 1);
  const torch::Tensor bottom = torch::cat({z.expand({3}), one.unsqueeze(0)}).unsqueeze(0);
  return torch::cat({top, bottom}, 0);
}

void retract_camera(torch::Tensor view, torch::Tensor full_proj, torch::Tensor centre, const torch::Tensor& projection,
                    torch::Tensor xi) {
  torch::NoGradGuard no_grad;
  const torch::Tensor E = se3_exp(xi.detach().to(view.device(), torch::kFloat64));
  const torch::Tensor v64 = torch::matmul(view.to(torch::kFloat64), E.t());   // view = T_cw^T: (E T_cw)^T = view E^T
  view.copy_(v64);
  full_proj.copy_(torch::matmul(v64, projection.to(torch::kFloat64)));
  centre.copy_(-torch::matmul(v64.slice(0, 0, 3).slice(1, 0, 3), v64[3].slice(0, 0, 3)));
  xi.zero_();
}

}  // namespace gsr_torch
