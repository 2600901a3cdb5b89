// gsr_surfel_axis.hpp -- a surfel's thin axis, written once for the two units that must agree on it: surfel.hip (the
// point-to-plane loss) and normal.hip (the camera-facing normals of the rendered normal map).
//   k* = index of the smallest activated scale (strict < from index 0: the lowest index wins a tie)
//   n  = column k* of R(q), q = (w, x, y, z) as given (NOT renormalised, as the rasterizer uses it),
//        R = [[1-2(y^2+z^2), 2(xy-wz), 2(xz+wy)], [2(xy+wz), 1-2(x^2+z^2), 2(yz-wx)], [2(xz-wy), 2(yz+wx), 1-2(x^2+y^2)]]
//        (column k is the axis of scaling[.][k]: Sigma = R S^2 R^T, cov3d_from_scale_rot in preprocess.hip)
// The sums of products are plain expressions: both including units are built with -ffp-contract=off (build.py), so
// the column has the same bits in either.
#pragma once
#include <hip/hip_runtime.h>

namespace gsr {

// k* of (s0, s1, s2); smin receives the smallest scale.
__device__ __forceinline__ int surfel_thin_index(const float s0, const float s1, const float s2, float& smin) {
  smin = s0;
  int ks = 0;
  if (s1 < smin) { smin = s1; ks = 1; }
  if (s2 < smin) { smin = s2; ks = 2; }
  return ks;
}

// Column k of R(q), q = (w, x, y, z) as given.
__device__ __forceinline__ void surfel_axis(const int k, const float w, const float x, const float y, const float z,
                                            float& n0, float& n1, float& n2) {
  if (k == 0) {
    n0 = 1.f - 2.f * (y * y + z * z); n1 = 2.f * (x * y + w * z); n2 = 2.f * (x * z - w * y);
  } else if (k == 1) {
    n0 = 2.f * (x * y - w * z); n1 = 1.f - 2.f * (x * x + z * z); n2 = 2.f * (y * z + w * x);
  } else {
    n0 = 2.f * (x * z + w * y); n1 = 2.f * (y * z - w * x); n2 = 1.f - 2.f * (x * x + y * y);
  }
}

}  // namespace gsr
