// torch_binding.cpp -- the LibTorch operator surface GS-LIVM links against, re-pointed at the C ABI of
// libgsraster_hip.so (include/gsraster.h).  Plain C++ (no device code): PyTorch-ROCm is used only for
// tensors, the caching allocator, autograd and the current HIP stream.
//
// Same names, argument order/meaning and return shapes as the reference:
//   GaussianRasterizationSettings, GaussianRasterizer, _RasterizeGaussians   include/gs/gs/rasterizer.cuh:8-80,
//                                                                          src/gs/rasterizer.cu
//   RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA / markVisible  include/gs/gs/rasterize_points.cuh:18-73,
//                                                                          src/gs/rasterize_points.cu
// A maintainer drops this file in place of src/gs/rasterize_points.cu + src/gs/rasterizer.cu (see
// INTEGRATION.md); the pybind11 module at the bottom exists so the Python test-suite can drive the very
// same C++ code path.
//
// Deliberate differences from the reference, all behind the same signatures:
//   * errors from the device library are thrown as std::runtime_error (a C ABI cannot throw);
//   * the reference calls exit(1) when shs / scales / rotations are undefined (rasterizer.cu:173-190);
//     here that is a std::invalid_argument -- the precomputed-colour / covariance inputs are supported;
//   * scalars are boxed into CPU tensors, so _RasterizeGaussians::forward's seven .item() calls
//     (rasterizer.cu:27-33) no longer synchronise the device;
//   * the nine gradient tensors are torch::empty (the library overwrites every element), saving the
//     ~120 B/Gaussian of memset the reference's torch::zeros cost per backward (rasterize_points.cu:173-181).
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>

#include "gsraster.h"
#include "gsr_torch_next.hpp"  // the hosts of the rows either side of the rasterizer (torch_next.cpp): bound below

// The declarations this file implements.  In the GS-LIVM tree they are the reference's OWN headers, untouched
// (-DGSR_REFERENCE_HEADER='"gs/rasterizer.cuh"', which pulls in gs/rasterize_points.cuh); standalone (this repo, the
// GPU box) the same declarations come from gsr_torch_surface.hpp.  Either way the members below are defined out of
// line, as strong symbols, exactly where src/gs/rasterizer.cu and src/gs/rasterize_points.cu defined them.
#ifdef GSR_REFERENCE_HEADER
#include GSR_REFERENCE_HEADER
#else
#include "gsr_torch_surface.hpp"
#endif

namespace {

void* current_stream() { return static_cast<void*>(c10::hip::getCurrentHIPStream().stream()); }

// size-0 tensor == "not provided" (rasterizer.cu:178-193)
const float* fptr(const torch::Tensor& t) { return t.defined() && t.numel() ? t.data_ptr<float>() : nullptr; }

void check(int code, const char* what) {
  if (code < 0) throw std::runtime_error(std::string(what) + ": " + gsr_last_error());
}

// Allocator callback: replaces resizeFunctional (rasterize_points.cu:36-44).
// The binning blob's callback can come a second time within one forward (gsr_forward, speculative path, when the
// predicted capacity was too small): the tensor is then replaced, not resized -- resize_ would copy the old contents.
char* resize_blob(void* ctx, size_t bytes) {
  auto* t = static_cast<torch::Tensor*>(ctx);
  if (t->numel() != 0)
    *t = torch::empty({static_cast<long long>(bytes)}, t->options());
  else
    t->resize_({static_cast<long long>(bytes)});
  return reinterpret_cast<char*>(t->data_ptr());
}

// `rotations` is the one caller tensor the library reads with 16-byte loads whatever its address (include/gsraster.h):
// a misaligned one -- a view into a larger buffer -- is handed over as an aligned copy.
torch::Tensor aligned16(const torch::Tensor& t) {
  if (t.defined() && t.numel() != 0 && (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15u) != 0) return t.clone();
  return t;
}

thread_local bool t_depth_gradient = false;  // gsr_torch::set_depth_gradient

}  // namespace

bool gsr_torch::set_depth_gradient(bool on) {
  const bool prev = t_depth_gradient;
  t_depth_gradient = on;
  return prev;
}

std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
RasterizeGaussiansCUDA(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors,
                       const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                       const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                       const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                       const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                       const torch::Tensor& campos, const bool prefiltered, const bool debug) {
  if (means3D.ndimension() != 2 || means3D.size(1) != 3) {
    AT_ERROR("means3D must have dimensions (num_points, 3)");
  }
  const int P = means3D.size(0);
  const int H = image_height;
  const int W = image_width;
  auto float_opts = means3D.options().dtype(torch::kFloat32);
  // fully written by the library (zero-filled by it when P == 0)
  torch::Tensor out_color = torch::empty({3, H, W}, float_opts);
  torch::Tensor out_depth = torch::empty({1, H, W}, float_opts);
  torch::Tensor out_acc = torch::empty({1, H, W}, float_opts);
  torch::Tensor radii = P ? torch::empty({P}, means3D.options().dtype(torch::kInt32))  // every entry is written
                          : torch::zeros({0}, means3D.options().dtype(torch::kInt32));
  auto byte_opts = means3D.options().dtype(torch::kByte);
  torch::Tensor geomBuffer = torch::empty({0}, byte_opts);
  torch::Tensor binningBuffer = torch::empty({0}, byte_opts);
  torch::Tensor imgBuffer = torch::empty({0}, byte_opts);

  int M = 0;
  if (sh.defined() && sh.numel() != 0) M = sh.size(1);
  auto bg = background.contiguous(), m3 = means3D.contiguous(), shc = sh.contiguous(), col = colors.contiguous(),
       op = opacity.contiguous(), sc = scales.contiguous(), rot = aligned16(rotations.contiguous()),
       cov = cov3D_precomp.contiguous(), view = viewmatrix.contiguous(), proj = projmatrix.contiguous(),
       cam = campos.contiguous();
  const int rendered = gsr_forward(
      resize_blob, &geomBuffer, resize_blob, &binningBuffer, resize_blob, &imgBuffer, P, degree, M, fptr(bg), W, H,
      fptr(m3), fptr(shc), fptr(col), fptr(op), fptr(sc), scale_modifier, fptr(rot), fptr(cov), fptr(view), fptr(proj),
      fptr(cam), tan_fovx, tan_fovy, prefiltered ? 1 : 0, out_color.data_ptr<float>(), out_depth.data_ptr<float>(),
      out_acc.data_ptr<float>(), P ? radii.data_ptr<int>() : nullptr, debug ? 1 : 0, current_stream());
  check(rendered, "gsr_forward");
  return std::make_tuple(rendered, out_color, out_depth, out_acc, radii, geomBuffer, binningBuffer, imgBuffer);
}

// want_cov3D = false (the autograd node, when the covariance comes from scales and rotations): dL_dcov3D is an
// intermediate nobody reads -- it is neither allocated nor written (24 of the 218 bytes per Gaussian the per-Gaussian
// backward moves) and comes back undefined.  The public entry point always returns it, as the reference does.
// dL_dout_depth defined: gsr_backward_depth instead of gsr_backward, and dL_ddepths [P] comes back as the ninth tensor
// (undefined otherwise).
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                  torch::Tensor, torch::Tensor>
rasterize_backward_impl(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                        const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                        const float scale_modifier, const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix,
                        const torch::Tensor& projmatrix, const float tan_fovx, const float tan_fovy,
                        const torch::Tensor& dL_dout_color, const torch::Tensor& dL_dout_acc, const torch::Tensor& sh,
                        const int degree, const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                        const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug,
                        const bool want_cov3D, const torch::Tensor& dL_dout_depth = torch::Tensor(),
                        torch::Tensor* dL_dconic_out = nullptr) {
  const int P = means3D.size(0);
  const int H = dL_dout_color.size(1);
  const int W = dL_dout_color.size(2);
  int M = 0;
  if (sh.defined() && sh.numel() != 0) M = sh.size(1);
  auto o = means3D.options();
  auto mk = [&](std::initializer_list<int64_t> shape) { return P ? torch::empty(shape, o) : torch::zeros(shape, o); };
  torch::Tensor dL_dmeans3D = mk({P, 3});
  torch::Tensor dL_dmeans2D = mk({P, 3});
  torch::Tensor dL_dcolors = mk({P, 3});
  torch::Tensor dL_dconic = mk({P, 2, 2});
  torch::Tensor dL_dopacity = mk({P, 1});
  torch::Tensor dL_dcov3D = want_cov3D ? mk({P, 6}) : torch::Tensor();
  torch::Tensor dL_dsh = mk({P, M, 3});
  torch::Tensor dL_dscales = mk({P, 3});
  torch::Tensor dL_drotations = mk({P, 4});
  const bool with_depth = dL_dout_depth.defined();
  torch::Tensor dL_ddepths = with_depth ? mk({P}) : torch::Tensor();
  if (with_depth && dL_dout_depth.numel() != static_cast<int64_t>(H) * W) {
    AT_ERROR("dL_dout_depth must have H*W elements");
  }
  if (P != 0) {
    auto bg = background.contiguous(), m3 = means3D.contiguous(), shc = sh.contiguous(), col = colors.contiguous(),
         sc = scales.contiguous(), rot = aligned16(rotations.contiguous()), cov = cov3D_precomp.contiguous(),
         view = viewmatrix.contiguous(), proj = projmatrix.contiguous(), cam = campos.contiguous(),
         dpix = dL_dout_color.contiguous(), dacc = dL_dout_acc.contiguous(), rad = radii.contiguous();
    if (with_depth) {
      auto ddep = dL_dout_depth.contiguous();
      check(gsr_backward_depth(P, degree, M, R, fptr(bg), W, H, fptr(m3), fptr(shc), fptr(col), fptr(sc), scale_modifier,
                               fptr(rot), fptr(cov), fptr(view), fptr(proj), fptr(cam), tan_fovx, tan_fovy,
                               rad.data_ptr<int>(), reinterpret_cast<char*>(geomBuffer.data_ptr()),
                               reinterpret_cast<char*>(binningBuffer.data_ptr()),
                               reinterpret_cast<char*>(imageBuffer.data_ptr()), fptr(dpix), fptr(dacc), fptr(ddep),
                               dL_dmeans2D.data_ptr<float>(), dL_dconic.data_ptr<float>(),
                               dL_dopacity.data_ptr<float>(), dL_dcolors.data_ptr<float>(),
                               dL_dmeans3D.data_ptr<float>(),
                               dL_dcov3D.defined() ? dL_dcov3D.data_ptr<float>() : nullptr,
                               M ? dL_dsh.data_ptr<float>() : nullptr, dL_dscales.data_ptr<float>(),
                               dL_drotations.data_ptr<float>(), dL_ddepths.data_ptr<float>(), debug ? 1 : 0,
                               current_stream()),
            "gsr_backward_depth");
    } else
    check(gsr_backward(P, degree, M, R, fptr(bg), W, H, fptr(m3), fptr(shc), fptr(col), fptr(sc), scale_modifier,
                       fptr(rot), fptr(cov), fptr(view), fptr(proj), fptr(cam), tan_fovx, tan_fovy,
                       rad.data_ptr<int>(), reinterpret_cast<char*>(geomBuffer.data_ptr()),
                       reinterpret_cast<char*>(binningBuffer.data_ptr()),
                       reinterpret_cast<char*>(imageBuffer.data_ptr()), fptr(dpix), fptr(dacc),
                       dL_dmeans2D.data_ptr<float>(), dL_dconic.data_ptr<float>(), dL_dopacity.data_ptr<float>(),
                       dL_dcolors.data_ptr<float>(), dL_dmeans3D.data_ptr<float>(),
                       dL_dcov3D.defined() ? dL_dcov3D.data_ptr<float>() : nullptr,
                       M ? dL_dsh.data_ptr<float>() : nullptr, dL_dscales.data_ptr<float>(),
                       dL_drotations.data_ptr<float>(), debug ? 1 : 0, current_stream()),
          "gsr_backward");
  }
  if (dL_dconic_out) *dL_dconic_out = dL_dconic;  // (an intermediate of the reference's surface: the pose gradient reads it)
  return std::make_tuple(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
                         dL_drotations, dL_ddepths);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor>
RasterizeGaussiansBackwardCUDA(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii,
                               const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations,
                               const float scale_modifier, const torch::Tensor& cov3D_precomp,
                               const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const float tan_fovx,
                               const float tan_fovy, const torch::Tensor& dL_dout_color,
                               const torch::Tensor& dL_dout_acc, const torch::Tensor& sh, const int degree,
                               const torch::Tensor& campos, const torch::Tensor& geomBuffer, const int R,
                               const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer, const bool debug) {
  auto [g0, g1, g2, g3, g4, g5, g6, g7, unused] =
      rasterize_backward_impl(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                              viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_acc, sh, degree, campos,
                              geomBuffer, R, binningBuffer, imageBuffer, debug, /*want_cov3D=*/true);
  (void)unused;
  return std::make_tuple(g0, g1, g2, g3, g4, g5, g6, g7);
}

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
                                    const bool debug) {
  if (!dL_dout_depth.defined()) AT_ERROR("dL_dout_depth must be defined");
  return rasterize_backward_impl(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_acc, sh, degree, campos,
                                 geomBuffer, R, binningBuffer, imageBuffer, debug, /*want_cov3D=*/true, dL_dout_depth);
}

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
                                   const bool debug) {
  torch::Tensor conic;
  auto [g0, g1, g2, g3, g4, g5, g6, g7, g8] =
      rasterize_backward_impl(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                              viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_acc, sh, degree, campos,
                              geomBuffer, R, binningBuffer, imageBuffer, debug, /*want_cov3D=*/true, dL_dout_depth, &conic);
  const torch::Tensor pose =
      gsr_torch::pose_gradient(means3D, radii, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                               tan_fovx, tan_fovy, static_cast<int>(dL_dout_color.size(1)),
                               static_cast<int>(dL_dout_color.size(2)), g0, conic, g3, g8);
  return std::make_tuple(g0, g1, g2, g3, g4, g5, g6, g7, g8, pose);
}

torch::Tensor markVisible(torch::Tensor& means3D, torch::Tensor& viewmatrix, torch::Tensor& projmatrix) {
  const int P = means3D.size(0);
  torch::Tensor present = torch::full({P}, false, means3D.options().dtype(at::kBool));
  if (P != 0) {
    auto m3 = means3D.contiguous(), view = viewmatrix.contiguous(), proj = projmatrix.contiguous();
    check(gsr_mark_visible(P, fptr(m3), fptr(view), fptr(proj),
                           reinterpret_cast<unsigned char*>(present.data_ptr<bool>()), current_stream()),
          "gsr_mark_visible");
  }
  return present;
}

// ------------------------------- src/gs/rasterizer.cu ---------------------------------------------
// Out-of-line definitions of the five members include/gs/gs/rasterizer.cuh:22-80 declares without bodies -- the
// strong symbols render_utils.cuh and lioOptimization.cpp link against once src/gs/rasterizer.cu is gone.
torch::autograd::tensor_list _RasterizeGaussians::forward(
    torch::autograd::AutogradContext* ctx, torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh,
    torch::Tensor colors_precomp, torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
    torch::Tensor cov3Ds_precomp, torch::Tensor image_height, torch::Tensor image_width, torch::Tensor tanfovx,
    torch::Tensor tanfovy, torch::Tensor bg, torch::Tensor scale_modifier, torch::Tensor viewmatrix,
    torch::Tensor projmatrix, torch::Tensor sh_degree, torch::Tensor camera_center, torch::Tensor prefiltered) {
  // host-resident 0-dim tensors (see rasterize_gaussians below): these reads do not touch the device
  const int image_height_val = image_height.item<int>();
  const int image_width_val = image_width.item<int>();
  const float tanfovx_val = tanfovx.item<float>();
  const float tanfovy_val = tanfovy.item<float>();
  const float scale_modifier_val = scale_modifier.item<float>();
  const int sh_degree_val = sh_degree.item<int>();
  const bool prefiltered_val = prefiltered.item<bool>();
  auto [num_rendered, color, out_depth, out_acc, radii, geomBuffer, binningBuffer, imgBuffer] =
      RasterizeGaussiansCUDA(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier_val,
                             cov3Ds_precomp, viewmatrix, projmatrix, tanfovx_val, tanfovy_val, image_height_val,
                             image_width_val, sh, sh_degree_val, camera_center, prefiltered_val, false);
  ctx->save_for_backward(
      {colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer});
  ctx->saved_data["num_rendered"] = num_rendered;
  ctx->saved_data["background"] = bg;
  ctx->saved_data["scale_modifier"] = scale_modifier_val;
  ctx->saved_data["viewmatrix"] = viewmatrix;
  ctx->saved_data["projmatrix"] = projmatrix;
  ctx->saved_data["tanfovx"] = tanfovx_val;
  ctx->saved_data["tanfovy"] = tanfovy_val;
  ctx->saved_data["image_height"] = image_height_val;
  ctx->saved_data["image_width"] = image_width_val;
  ctx->saved_data["sh_degree"] = sh_degree_val;
  ctx->saved_data["camera_center"] = camera_center;
  ctx->saved_data["prefiltered"] = prefiltered_val;
  ctx->saved_data["depth_gradient"] = t_depth_gradient;  // gsr_torch::set_depth_gradient, as it stands at forward time
  ctx->mark_non_differentiable({radii});
  ctx->set_materialize_grads(false);  // no zero images for the outputs nobody differentiates (depth)
  return {color, radii, out_depth, out_acc};
}

torch::autograd::tensor_list _RasterizeGaussians::backward(torch::autograd::AutogradContext* ctx,
                                                           torch::autograd::tensor_list grad_outputs) {
  auto grad_out_color = grad_outputs[0];
  // grad_outputs[1] (radii) and [2] (depth) are ignored, exactly as the reference (rasterizer.cu:78-79) -- the depth
  // gradient unless the forward ran under gsr_torch::set_depth_gradient(true) and one arrives
  auto grad_acc = grad_outputs[3];
  const torch::Tensor grad_depth = ctx->saved_data["depth_gradient"].toBool() ? grad_outputs[2] : torch::Tensor();
  const int num_rendered = ctx->saved_data["num_rendered"].to<int>();
  auto saved = ctx->get_saved_variables();
  auto colors_precomp = saved[0], means3D = saved[1], scales = saved[2], rotations = saved[3],
       cov3Ds_precomp = saved[4], radii = saved[5], sh = saved[6], geomBuffer = saved[7], binningBuffer = saved[8],
       imgBuffer = saved[9];
  const int H = ctx->saved_data["image_height"].to<int>(), W = ctx->saved_data["image_width"].to<int>();
  if (!grad_out_color.defined()) grad_out_color = torch::zeros({3, H, W}, means3D.options());
  if (!grad_acc.defined()) grad_acc = torch::zeros({1, H, W}, means3D.options());
  auto [grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
        grad_rotations, grad_depths] =
      rasterize_backward_impl(
          ctx->saved_data["background"].to<torch::Tensor>(), means3D, radii, colors_precomp, scales, rotations,
          ctx->saved_data["scale_modifier"].to<double>(), cov3Ds_precomp,
          ctx->saved_data["viewmatrix"].to<torch::Tensor>(), ctx->saved_data["projmatrix"].to<torch::Tensor>(),
          ctx->saved_data["tanfovx"].to<double>(), ctx->saved_data["tanfovy"].to<double>(), grad_out_color, grad_acc,
          sh, ctx->saved_data["sh_degree"].to<int>(), ctx->saved_data["camera_center"].to<torch::Tensor>(),
          geomBuffer, num_rendered, binningBuffer, imgBuffer, false, /*want_cov3D=*/cov3Ds_precomp.numel() != 0,
          grad_depth);
  (void)grad_depths;  // dL/d view-space depth: already carried into grad_means3D
  auto opt = [](const torch::Tensor& g, const torch::Tensor& x) { return x.numel() ? g : torch::Tensor(); };
  return {grad_means3D,
          grad_means2D,
          opt(grad_sh, sh),
          opt(grad_colors_precomp, colors_precomp),
          grad_opacities,
          opt(grad_scales, scales),
          opt(grad_rotations, rotations),
          opt(grad_cov3Ds_precomp, cov3Ds_precomp),
          torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(),
          torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
}

torch::Tensor GaussianRasterizer::mark_visible(torch::Tensor positions) {
  torch::NoGradGuard no_grad;
  return markVisible(positions, raster_settings_.viewmatrix, raster_settings_.projmatrix);
}

torch::autograd::tensor_list GaussianRasterizer::rasterize_gaussians(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp,
    torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3Ds_precomp,
    GaussianRasterizationSettings raster_settings) {
  torch::Device device = means3D.is_cuda() ? means3D.device() : torch::Device(torch::kCUDA);
  // scalars stay on the host: the reference's 0-dim CUDA tensors cost seven D2H syncs per render
  auto image_height = torch::tensor(raster_settings.image_height);
  auto image_width = torch::tensor(raster_settings.image_width);
  auto tanfovx = torch::tensor(raster_settings.tanfovx);
  auto tanfovy = torch::tensor(raster_settings.tanfovy);
  auto scale_modifier = torch::tensor(raster_settings.scale_modifier);
  auto sh_degree = torch::tensor(raster_settings.sh_degree);
  auto prefiltered = torch::tensor(raster_settings.prefiltered);
  auto mv = [&](torch::Tensor t) { return (t.defined() && t.device() != device) ? t.to(device) : t; };
  return _RasterizeGaussians::apply(mv(means3D), mv(means2D), mv(sh), mv(colors_precomp), mv(opacities), mv(scales),
                                    mv(rotations), mv(cov3Ds_precomp), image_height, image_width, tanfovx, tanfovy,
                                    mv(raster_settings.bg), scale_modifier, mv(raster_settings.viewmatrix),
                                    mv(raster_settings.projmatrix), sh_degree, mv(raster_settings.camera_center),
                                    prefiltered);
}

// (the default arguments live on the declaration)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> GaussianRasterizer::forward(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities, torch::Tensor shs,
    torch::Tensor colors_precomp, torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3D_precomp) {
  if ((shs.defined() && colors_precomp.defined()) || (!shs.defined() && !colors_precomp.defined())) {
    throw std::invalid_argument("Please provide exactly one of either SHs or precomputed colors!");
  }
  if (((scales.defined() || rotations.defined()) && cov3D_precomp.defined()) ||
      (!scales.defined() && !rotations.defined() && !cov3D_precomp.defined())) {
    throw std::invalid_argument(
        "Please provide exactly one of either scale/rotation pair or "
        "precomputed 3D covariance!");
  }
  if ((scales.defined() != rotations.defined()) && !cov3D_precomp.defined()) {
    throw std::invalid_argument("scales and rotations must be provided together");
  }
  auto empty = [&]() { return torch::empty({0}, means3D.options().dtype(torch::kFloat32)); };
  if (!shs.defined()) shs = empty();
  if (!colors_precomp.defined()) colors_precomp = empty();
  if (!scales.defined()) scales = empty();
  if (!rotations.defined()) rotations = empty();
  if (!cov3D_precomp.defined()) cov3D_precomp = empty();
  auto result = rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                    cov3D_precomp, raster_settings_);
  return {result[0], result[1], result[2], result[3]};
}

// ------------------------- pybind11 exposure (tests drive the C++ surface) -------------------------
#ifndef GSR_NO_PYBIND
namespace py = pybind11;

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "C++/LibTorch operator surface of gs_livm_amd (mirror of GS-LIVM's src/gs/rasterizer.cu)";
  m.def("RasterizeGaussiansCUDA", &RasterizeGaussiansCUDA);
  m.def("RasterizeGaussiansBackwardCUDA", &RasterizeGaussiansBackwardCUDA);
  m.def("RasterizeGaussiansBackwardDepthCUDA", &RasterizeGaussiansBackwardDepthCUDA);
  m.def("RasterizeGaussiansBackwardPoseCUDA",
        [](torch::Tensor bg, torch::Tensor means3D, torch::Tensor radii, torch::Tensor colors, torch::Tensor scales,
           torch::Tensor rotations, float scale_modifier, torch::Tensor cov3D_precomp, torch::Tensor viewmatrix,
           torch::Tensor projmatrix, float tan_fovx, float tan_fovy, torch::Tensor dL_dout_color,
           torch::Tensor dL_dout_acc, const py::object& dL_dout_depth, torch::Tensor sh, int degree, torch::Tensor campos,
           torch::Tensor geomBuffer, int R, torch::Tensor binningBuffer, torch::Tensor imageBuffer, bool debug) {
          return RasterizeGaussiansBackwardPoseCUDA(
              bg, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
              tan_fovx, tan_fovy, dL_dout_color, dL_dout_acc,
              dL_dout_depth.is_none() ? torch::Tensor() : dL_dout_depth.cast<torch::Tensor>(), sh, degree, campos,
              geomBuffer, R, binningBuffer, imageBuffer, debug);
        });
  m.def("set_depth_gradient", &gsr_torch::set_depth_gradient, py::arg("on"));
  m.def("markVisible", [](torch::Tensor a, torch::Tensor b, torch::Tensor c) { return markVisible(a, b, c); });
  // exact instance count of this thread's last forward (RasterizeGaussiansCUDA's first element is the binning key:
  // the capacity the binning blob was carved for -- equal to the count after a synchronous forward)
  m.def("last_num_rendered", []() { return gsr_last_num_rendered(); });
  py::class_<GaussianRasterizationSettings>(m, "GaussianRasterizationSettings")
      .def(py::init([](int h, int w, float tx, float ty, torch::Tensor bg, float sm, torch::Tensor view,
                       torch::Tensor proj, int deg, torch::Tensor cam, bool pre) {
             return GaussianRasterizationSettings{h, w, tx, ty, bg, sm, view, proj, deg, cam, pre};
           }),
           py::arg("image_height"), py::arg("image_width"), py::arg("tanfovx"), py::arg("tanfovy"), py::arg("bg"),
           py::arg("scale_modifier"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("sh_degree"),
           py::arg("camera_center"), py::arg("prefiltered") = false);
  auto opt = [](const py::object& o) { return o.is_none() ? torch::Tensor() : o.cast<torch::Tensor>(); };
  // GaussianRasterizer inherits torch::nn::Module privately (as in the reference), which pybind11 cannot
  // hold directly: the Python handle owns one by composition.
  struct PyRasterizer {
    GaussianRasterizer impl;
    explicit PyRasterizer(GaussianRasterizationSettings s) : impl(std::move(s)) {}
  };
  py::class_<PyRasterizer>(m, "GaussianRasterizer")
      .def(py::init<GaussianRasterizationSettings>())
      .def("mark_visible", [](PyRasterizer& self, torch::Tensor p) { return self.impl.mark_visible(p); })
      .def("forward",
           [opt](PyRasterizer& self, torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities,
                 py::object shs, py::object colors_precomp, py::object scales, py::object rotations,
                 py::object cov3D_precomp) {
             const torch::Tensor a = opt(shs), b = opt(colors_precomp), c = opt(scales), d = opt(rotations),
                                 e = opt(cov3D_precomp);
             // (no Python object is touched from here on: other rendering threads of the interpreter may run -- the
             // reference's rendering threads are C++ threads and never meet a GIL)
             py::gil_scoped_release unlocked;
             return self.impl.forward(means3D, means2D, opacities, a, b, c, d, e);
           },
           py::arg("means3D"), py::arg("means2D"), py::arg("opacities"), py::arg("shs") = py::none(),
           py::arg("colors_precomp") = py::none(), py::arg("scales") = py::none(), py::arg("rotations") = py::none(),
           py::arg("cov3D_precomp") = py::none());

  // ---- gsr_torch_next.hpp: the C++ hosts of the "next" rows, so that the tests can hold them against the Python route
  namespace nx = gsr_torch;
  auto n = m.def_submodule("next", "C++/LibTorch hosts of the fused loss, activations + Adam, growth and PLY export");
  n.def("reference_window_1d", &nx::reference_window_1d, py::arg("window_size") = 11, py::arg("sigma") = 1.5f);
  n.def("photometric_loss",
        [opt](torch::Tensor image, torch::Tensor gt, float lambda_dssim, py::object window) {
          return nx::photometric_loss(image, gt, lambda_dssim, opt(window));
        },
        py::arg("image"), py::arg("gt"), py::arg("lambda_dssim") = 0.2f, py::arg("window1d") = py::none());
  n.def("photometric_loss_parts",
        [opt](torch::Tensor image, torch::Tensor gt, float lambda_dssim, py::object window) {
          return nx::photometric_loss_parts(image, gt, lambda_dssim, opt(window));
        },
        py::arg("image"), py::arg("gt"), py::arg("lambda_dssim") = 0.2f, py::arg("window1d") = py::none());
  n.def("similarity_loss", &nx::similarity_loss, py::arg("points"), py::arg("sel"), py::arg("xyz"), py::arg("scaling"),
        py::arg("lambda_") = 0.2f);
  n.def("surfel_plane_loss", &nx::surfel_plane_loss, py::arg("points"), py::arg("sel"), py::arg("xyz"),
        py::arg("scaling"), py::arg("rotation"), py::arg("lambda_"), py::arg("huber") = 0.f,
        py::arg("max_dist") = std::numeric_limits<float>::infinity(), py::arg("lambda_flat") = 0.f);
  n.def("delta_depth_loss", &nx::delta_depth_loss, py::arg("depth_src"), py::arg("acc_src"), py::arg("depth_ref"),
        py::arg("acc_ref"), py::arg("inv_K_src"), py::arg("K_ref"), py::arg("T_rel"), py::arg("lambda_") = 0.2f);
  n.def("lidar_depth_image",
        [](torch::Tensor points_world, torch::Tensor T_cw, torch::Tensor K, int64_t height, int64_t width,
           float min_depth, float max_depth, bool want_counts) -> py::object {
          torch::Tensor counts;
          torch::Tensor image = nx::lidar_depth_image(points_world, T_cw, K, height, width, min_depth, max_depth,
                                                      want_counts ? &counts : nullptr);
          if (!want_counts) return py::cast(image);
          return py::make_tuple(image, counts);
        },
        py::arg("points_world"), py::arg("T_cw"), py::arg("K"), py::arg("height"), py::arg("width"),
        py::arg("min_depth") = 0.2f, py::arg("max_depth") = std::numeric_limits<float>::infinity(),
        py::arg("want_counts") = false);
  n.def("lidar_depth_loss", &nx::lidar_depth_loss, py::arg("depth"), py::arg("acc"), py::arg("lidar_depth"),
        py::arg("acc_min") = 0.5f, py::arg("lambda_") = 1.0f);
  n.def("lidar_occlusion_filter",
        [](torch::Tensor lidar_depth, int64_t radius, float tol, bool want_counts) -> py::object {
          torch::Tensor counts;
          torch::Tensor out = nx::lidar_occlusion_filter(lidar_depth, radius, tol, want_counts ? &counts : nullptr);
          if (!want_counts) return py::cast(out);
          return py::make_tuple(out, counts);
        },
        py::arg("lidar_depth"), py::arg("radius"), py::arg("tol"), py::arg("want_counts") = false);
  n.def("lidar_depth_loss_robust", &nx::lidar_depth_loss_robust, py::arg("depth"), py::arg("acc"),
        py::arg("lidar_depth"), py::arg("acc_min"), py::arg("lambda_"), py::arg("huber_abs"), py::arg("huber_rel"),
        py::arg("clip_abs"), py::arg("clip_rel"));
  n.def("admit_sweep",
        [opt](torch::Tensor points_world, torch::Tensor T_cw, torch::Tensor K, int64_t height, int64_t width,
              float depth_tol, float occlusion_tol, py::object depth, py::object acc, py::object image,
              py::object lidar_depth, py::object covs, py::object exposure, float acc_min, int occlusion_radius,
              float footprint, float min_depth, float max_depth, bool one_per_pixel, bool want_reasons) {
          nx::SweepAdmitOptions o;
          o.acc_min = acc_min; o.occlusion_radius = occlusion_radius; o.footprint = footprint;
          o.min_depth = min_depth; o.max_depth = max_depth; o.one_per_pixel = one_per_pixel;
          o.want_reasons = want_reasons;
          const nx::Admitted a = nx::admit_sweep(points_world, T_cw, K, height, width, depth_tol, occlusion_tol,
                                                 opt(depth), opt(acc), opt(image), opt(lidar_depth), opt(covs),
                                                 opt(exposure), o);
          auto none_or = [](const torch::Tensor& t) -> py::object { return t.defined() ? py::cast(t) : py::none(); };
          py::list counts;
          for (int64_t c : a.counts) counts.append(c);
          return py::make_tuple(a.xyz, a.covs, none_or(a.rgbs), a.index, a.pixel, a.z, py::tuple(counts),
                                none_or(a.reasons));
        },
        py::arg("points_world"), py::arg("T_cw"), py::arg("K"), py::arg("height"), py::arg("width"),
        py::arg("depth_tol"), py::arg("occlusion_tol"), py::arg("depth") = py::none(), py::arg("acc") = py::none(),
        py::arg("image") = py::none(), py::arg("lidar_depth") = py::none(), py::arg("covs") = py::none(),
        py::arg("exposure") = py::none(), py::arg("acc_min") = 0.5f, py::arg("occlusion_radius") = 1,
        py::arg("footprint") = 1.0f, py::arg("min_depth") = 0.2f,
        py::arg("max_depth") = std::numeric_limits<float>::infinity(), py::arg("one_per_pixel") = true,
        py::arg("want_reasons") = false);
  n.def("voxel_table", &nx::voxel_table, py::arg("capacity"), py::arg("like"));
  n.def("voxel_rehash", &nx::voxel_rehash, py::arg("table"), py::arg("capacity"));
  n.def("voxel_sweep",
        [opt](torch::Tensor table, int64_t live, torch::Tensor points, py::object colors, float grid,
              int64_t min_points, float min_sigma, float scale_factor) {
          nx::VoxelMap map;
          map.table = table; map.live = live; map.grid = grid; map.min_points = min_points; map.min_sigma = min_sigma;
          const nx::VoxelSeeds v = nx::voxel_sweep(map, points, opt(colors), scale_factor);
          auto none_or = [](const torch::Tensor& t) -> py::object { return t.defined() ? py::cast(t) : py::none(); };
          py::list counts;
          for (int64_t c : v.counts) counts.append(c);
          return py::make_tuple(py::make_tuple(v.xyz, v.covs, none_or(v.rgbs), v.keys, v.points, v.scaling_raw,
                                               v.rotation, v.normal, v.status, v.point_keys, py::tuple(counts)),
                                map.table, map.live);
        },
        py::arg("table"), py::arg("live"), py::arg("points"), py::arg("colors"), py::arg("grid"),
        py::arg("min_points"), py::arg("min_sigma"), py::arg("scale_factor") = 1.0f);
  n.def("image_metrics",
        [opt](torch::Tensor image, torch::Tensor gt, py::object window, py::object totals, py::object weights) {
          return nx::image_metrics(image, gt, opt(window), opt(totals), opt(weights));
        },
        py::arg("image"), py::arg("gt"), py::arg("window1d") = py::none(), py::arg("totals") = py::none(),
        py::arg("weights") = py::none());
  n.def("weighted_photometric_loss",
        [opt](torch::Tensor image, torch::Tensor gt, py::object weights, py::object acc, float acc_min,
              py::object exposure, float lambda_dssim, py::object window, bool log_gain) {
          return nx::weighted_photometric_loss(image, gt, opt(weights), opt(acc), acc_min, opt(exposure), lambda_dssim,
                                               opt(window), log_gain);
        },
        py::arg("image"), py::arg("gt"), py::arg("weights") = py::none(), py::arg("acc") = py::none(),
        py::arg("acc_min") = 0.5f, py::arg("exposure") = py::none(), py::arg("lambda_dssim") = 0.2f,
        py::arg("window1d") = py::none(), py::arg("log_gain") = false);
  n.def("weighted_photometric_loss_parts",
        [opt](torch::Tensor image, torch::Tensor gt, py::object weights, py::object acc, float acc_min,
              py::object exposure, float lambda_dssim, py::object window, bool log_gain) {
          return nx::weighted_photometric_loss_parts(image, gt, opt(weights), opt(acc), acc_min, opt(exposure),
                                                     lambda_dssim, opt(window), log_gain);
        },
        py::arg("image"), py::arg("gt"), py::arg("weights") = py::none(), py::arg("acc") = py::none(),
        py::arg("acc_min") = 0.5f, py::arg("exposure") = py::none(), py::arg("lambda_dssim") = 0.2f,
        py::arg("window1d") = py::none(), py::arg("log_gain") = false);
  n.def("psnr", &nx::psnr, py::arg("image"), py::arg("gt"));
  n.def("exposure_photometric_loss",
        [opt](torch::Tensor image, torch::Tensor gt, torch::Tensor exposure, float lambda_dssim, py::object window,
              bool log_gain) {
          return nx::exposure_photometric_loss(image, gt, exposure, lambda_dssim, opt(window), log_gain);
        },
        py::arg("image"), py::arg("gt"), py::arg("exposure"), py::arg("lambda_dssim") = 0.2f,
        py::arg("window1d") = py::none(), py::arg("log_gain") = false);
  n.def("apply_exposure",
        [opt](torch::Tensor image, torch::Tensor exposure, py::object out) {
          return nx::apply_exposure(image, exposure, opt(out));
        },
        py::arg("image"), py::arg("exposure"), py::arg("out") = py::none());
  n.def("to_u8", [opt](torch::Tensor image, bool bgr, py::object out) { return nx::to_u8(image, bgr, opt(out)); },
        py::arg("image"), py::arg("bgr") = true, py::arg("out") = py::none());
  n.def("depth_to_u8",
        [opt](torch::Tensor depth, float max_depth, py::object out) { return nx::depth_to_u8(depth, max_depth, opt(out)); },
        py::arg("depth"), py::arg("max_depth") = 50.0f, py::arg("out") = py::none());
  py::class_<nx::VoxelIndex>(n, "VoxelIndex")
      .def(py::init<>())
      .def("add", &nx::VoxelIndex::add, py::arg("keys"), py::arg("counts"), py::arg("first_row"))
      .def("select",
           [](const nx::VoxelIndex& self, const std::unordered_map<std::size_t, torch::Tensor>& losses,
              int64_t max_points, const std::string& device) -> py::object {
             torch::Tensor points, sel;
             if (!self.select(losses, points, sel, max_points, torch::Device(device))) return py::none();
             return py::make_tuple(points, sel);
           },
           py::arg("losses"), py::arg("max_points") = 500, py::arg("device") = "cuda")
      .def("remap", &nx::VoxelIndex::remap, py::arg("row_map"))
      .def("get",
           [](const nx::VoxelIndex& self, std::size_t key) -> py::object {
             int64_t first = 0, count = 0;
             if (!self.get(key, first, count)) return py::none();
             return py::make_tuple(first, count);
           })
      .def("__len__", &nx::VoxelIndex::size)
      .def("__contains__", &nx::VoxelIndex::contains);
  n.def("activate", [](torch::Tensor s, torch::Tensor r, torch::Tensor o, torch::Tensor dc, torch::Tensor rest) {
    const nx::Activated a = nx::activate(s, r, o, dc, rest);
    return std::make_tuple(a.scaling, a.rotation, a.opacity, a.features);
  });
  py::class_<nx::FusedAdam>(n, "FusedAdam")
      .def(py::init<std::vector<torch::Tensor>, std::vector<double>, double, double, double>(), py::arg("params"),
           py::arg("lrs"), py::arg("beta1") = 0.9, py::arg("beta2") = 0.999, py::arg("eps") = 1e-15)
      .def("step", &nx::FusedAdam::step, py::arg("zero_grad") = true)
      .def("step_model",
           [](nx::FusedAdam& self, torch::Tensor gx, torch::Tensor gs, torch::Tensor gr, torch::Tensor go,
              torch::Tensor gf) {
             const nx::Activated a = self.step_model(gx, gs, gr, go, gf);
             return std::make_tuple(a.scaling, a.rotation, a.opacity, a.features);
           })
      .def("replace_param", &nx::FusedAdam::replace_param)
      .def("prune", &nx::FusedAdam::prune, py::arg("reasons"), py::arg("row_map"), py::arg("P_new"))
      .def("step_count", &nx::FusedAdam::step_count)
      .def("params", &nx::FusedAdam::params)
      .def("exp_avg", &nx::FusedAdam::exp_avg)
      .def("exp_avg_sq", &nx::FusedAdam::exp_avg_sq);
  n.def("prune_mark",
        [opt](torch::Tensor xyz, torch::Tensor s, torch::Tensor r, torch::Tensor o, float min_opacity, float max_scale,
              bool drop_nonfinite, py::object drop) {
          const nx::PruneMarks p = nx::prune_mark(xyz, s, r, o, min_opacity, max_scale, drop_nonfinite, opt(drop));
          return std::make_tuple(p.reasons, p.row_map, p.counts);
        },
        py::arg("xyz"), py::arg("scaling_raw"), py::arg("rotation_raw"), py::arg("opacity_raw"),
        py::arg("min_opacity") = 1.0f / 255.0f, py::arg("max_scale") = 0.3f, py::arg("drop_nonfinite") = true,
        py::arg("drop") = py::none());
  n.def("prune_rows", &nx::prune_rows, py::arg("tensors"), py::arg("reasons"), py::arg("row_map"), py::arg("P_new"));
  n.def("pose_gradient",
        [opt](torch::Tensor means3D, torch::Tensor radii, py::object scales, py::object rotations, float scale_modifier,
              py::object cov3D_precomp, torch::Tensor viewmatrix, torch::Tensor projmatrix, float tan_fovx, float tan_fovy,
              int image_height, int image_width, torch::Tensor dL_dmeans2D, torch::Tensor dL_dconic,
              torch::Tensor dL_dmeans3D, py::object dL_ddepths) {
          return nx::pose_gradient(means3D, radii, opt(scales), opt(rotations), scale_modifier, opt(cov3D_precomp),
                                   viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, dL_dmeans2D,
                                   dL_dconic, dL_dmeans3D, opt(dL_ddepths));
        },
        py::arg("means3D"), py::arg("radii"), py::arg("scales"), py::arg("rotations"), py::arg("scale_modifier"),
        py::arg("cov3D_precomp"), py::arg("viewmatrix"), py::arg("projmatrix"), py::arg("tan_fovx"), py::arg("tan_fovy"),
        py::arg("image_height"), py::arg("image_width"), py::arg("dL_dmeans2D"), py::arg("dL_dconic"),
        py::arg("dL_dmeans3D"), py::arg("dL_ddepths") = py::none());
  n.def("retract_camera", &nx::retract_camera, py::arg("view"), py::arg("full_proj"), py::arg("centre"),
        py::arg("projection"), py::arg("xi"));
  n.def("se3_exp", &nx::se3_exp, py::arg("xi"));
  n.def("density_accumulate", &nx::density_accumulate, py::arg("radii"), py::arg("dL_dmean2D"), py::arg("stats"));
  n.def("densify_mark",
        [](torch::Tensor stats, torch::Tensor s, float grad_threshold, float size_threshold, int64_t max_new) {
          const nx::DensifyMarks d = nx::densify_mark(stats, s, grad_threshold, size_threshold, max_new);
          return std::make_tuple(d.kinds, d.offsets, d.counts);
        },
        py::arg("stats"), py::arg("scaling_raw"), py::arg("grad_threshold"), py::arg("size_threshold"),
        py::arg("max_new") = -1);
  n.def("densify_apply",
        [opt](int64_t P, int64_t n_new, torch::Tensor kinds, torch::Tensor offsets, uint64_t seed,
              std::vector<torch::Tensor> params6, std::vector<torch::Tensor> exp_avg6,
              std::vector<torch::Tensor> exp_avg_sq6, py::object stats) {
          nx::densify_apply(P, n_new, kinds, offsets, seed, params6, exp_avg6, exp_avg_sq6, opt(stats));
        },
        py::arg("P"), py::arg("n_new"), py::arg("kinds"), py::arg("offsets"), py::arg("seed"), py::arg("params6"),
        py::arg("exp_avg6") = std::vector<torch::Tensor>(), py::arg("exp_avg_sq6") = std::vector<torch::Tensor>(),
        py::arg("stats") = py::none());
  n.def("visibility_pack", &nx::visibility_pack, py::arg("source"), py::arg("words") = 0);
  n.def("covisibility",
        [opt](torch::Tensor q_bits, py::object k_bits, int64_t words, bool counts) {
          const nx::Covisibility c = nx::covisibility(q_bits, opt(k_bits), words, counts);
          return std::make_tuple(c.inter, c.q_count, c.k_count);
        },
        py::arg("q_bits"), py::arg("k_bits") = py::none(), py::arg("words") = 0, py::arg("counts") = true);
  n.def("observation_count",
        [](torch::Tensor bits, int64_t P, int64_t first_row, int64_t min_count, bool want_count, bool want_drop) {
          const nx::ObservationCount c = nx::observation_count(bits, P, first_row, min_count, want_count, want_drop);
          return std::make_tuple(c.count, c.drop);
        },
        py::arg("bits"), py::arg("P"), py::arg("first_row") = 0, py::arg("min_count") = 0, py::arg("want_count") = true,
        py::arg("want_drop") = false);
  n.def("visibility_remap", &nx::visibility_remap, py::arg("src"), py::arg("reasons"), py::arg("row_map"),
        py::arg("dst_words") = 0);
  n.def("contribution", &nx::contribution, py::arg("geom"), py::arg("binning"), py::arg("img"), py::arg("P"), py::arg("R"),
        py::arg("W"), py::arg("H"));
  n.def("contribution_finish",
        [opt](torch::Tensor rows, int64_t min_pixels, double min_weight, bool want_n_touched, bool want_weight_sum,
              bool want_weight_max, bool want_mask, py::object stats) {
          const nx::Contribution c = nx::contribution_finish(rows, min_pixels, min_weight, want_n_touched, want_weight_sum,
                                                             want_weight_max, want_mask, opt(stats));
          return std::make_tuple(c.n_touched, c.weight_sum, c.weight_max, c.mask);
        },
        py::arg("rows"), py::arg("min_pixels") = 1, py::arg("min_weight") = 0.0, py::arg("want_n_touched") = true,
        py::arg("want_weight_sum") = true, py::arg("want_weight_max") = true, py::arg("want_mask") = true,
        py::arg("stats") = py::none());
  n.def("blend_attributes", &nx::blend_attributes, py::arg("geom"), py::arg("binning"), py::arg("img"),
        py::arg("attributes"), py::arg("R"), py::arg("W"), py::arg("H"));
  n.def("surfel_normals", &nx::surfel_normals, py::arg("xyz"), py::arg("scaling"), py::arg("rotation"), py::arg("T_cw"));
  n.def("normal_consistency_loss", &nx::normal_consistency_loss, py::arg("depth"), py::arg("acc"), py::arg("normals"),
        py::arg("K"), py::arg("acc_min"), py::arg("lambda_"), py::arg("normal_min"),
        py::arg("jump_rel") = std::numeric_limits<float>::infinity());
  n.def("init_gaussians", &nx::init_gaussians);
  n.def("pack_ply_rows", &nx::pack_ply_rows);
  n.def("write_ply", &nx::write_ply);
  n.def("ply_attribute_names", &nx::ply_attribute_names);
}
#endif  // GSR_NO_PYBIND
