// gsr_lidar_project.hpp -- the projection of a LiDAR point into a keyframe's view, written once for the two units
// that must agree on it bit for bit: lidar.hip (the sweep's z-buffer) and seed.hip (sweep admission).
//   p = R x + t, z = p.z                              [R | t] = T_cw, x_c = R x_w + t
//   (X, Y) = (K p).xy / (K p).z                       N = M (x, 1) with M = K [R | t] composed on the host in double and
//                                                     rounded once (lidar_compose)
//   (ix, iy) = (floor(X + 0.5), floor(Y + 0.5))       pixel u covers [u - 0.5, u + 0.5): the rasterizer's ndc2Pix
// Every multiply-add is an explicit __builtin_fmaf and nothing else can contract, so the bits do not depend on the
// including unit's -ffp-contract setting.
#pragma once
#include <hip/hip_runtime.h>

#include "gsr_workgroup.hpp"

namespace gsr {

struct LidarCam {   // composed on the host in double, rounded once
  float m[12];      // M = K [R | t], row-major 3 x 4
  float r2[3];      // third row of R
  float tz;
};

inline LidarCam lidar_compose(const float* T_cw12, const float* K9) {
  LidarCam cam;
  for (int r = 0; r < 3; r++)
    for (int q = 0; q < 4; q++) {
      double v = 0.0;
      for (int k = 0; k < 3; k++) v += (double)K9[3 * r + k] * (double)T_cw12[4 * k + q];
      cam.m[4 * r + q] = (float)v;
    }
  for (int q = 0; q < 3; q++) cam.r2[q] = T_cw12[8 + q];
  cam.tz = T_cw12[11];
  return cam;
}

struct LidarHit {
  float z, X, Y;
  int ix, iy;       // valid only when lidar_project returns true: 0 <= ix < W, 0 <= iy < H
};

// false = dropped: a coordinate of the point, z, X or Y not finite; z <= min_depth; z > max_depth; |X| or |Y| beyond
// 2^30 (tested before any conversion to an integer); the pixel outside the image.
__device__ __forceinline__ bool lidar_project(const LidarCam& cam, const float x, const float y, const float w,
                                              const float min_depth, const float max_depth, const int W, const int H,
                                              LidarHit& h) {
  const float z = __builtin_fmaf(cam.r2[0], x, __builtin_fmaf(cam.r2[1], y, __builtin_fmaf(cam.r2[2], w, cam.tz)));
  const float nx = __builtin_fmaf(cam.m[0], x, __builtin_fmaf(cam.m[1], y, __builtin_fmaf(cam.m[2], w, cam.m[3])));
  const float ny = __builtin_fmaf(cam.m[4], x, __builtin_fmaf(cam.m[5], y, __builtin_fmaf(cam.m[6], w, cam.m[7])));
  const float nz = __builtin_fmaf(cam.m[8], x, __builtin_fmaf(cam.m[9], y, __builtin_fmaf(cam.m[10], w, cam.m[11])));
  const float X = nx / nz, Y = ny / nz;
  h.z = z; h.X = X; h.Y = Y; h.ix = 0; h.iy = 0;
  // every comparison is false for NaN; z <= max_depth with z finite (max_depth may be +inf)
  const bool fin = fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(w) < INFINITY && fabsf(z) < INFINITY;
  if (!(fin && z > min_depth && z <= max_depth && fabsf(X) <= COORD_MAX_ && fabsf(Y) <= COORD_MAX_)) return false;
  const int ix = (int)floorf(X + 0.5f), iy = (int)floorf(Y + 0.5f);
  if (!(ix >= 0 && ix < W && iy >= 0 && iy < H)) return false;
  h.ix = ix; h.iy = iy;
  return true;
}

}  // namespace gsr
