// gsr_api.hpp -- what the extern "C" entry points of every translation unit share: the thread's last error
// (gsr_last_error; the buffer itself is api.hip's), HIP_TRY and the input checks several families repeat.
// Host only; not part of the public ABI (include/gsraster.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/gsraster.h"

namespace gsr {

// Formats the calling thread's last error and returns `code` (api.hip).
int fail(int code, const char* fmt, ...);
// Empties the calling thread's last error: the first statement of an entry point that can fail.
void clear_error();

// Input checks that several entry points share: GSR_OK, or the error as fail() left it.
// H W >= limit: the pixel offsets (0x7fffffff) or pixel indices (0x80000000) of a plane are 32-bit.
inline bool plane_fits(int height, int width, unsigned long long limit) {
  return (unsigned long long)height * (unsigned long long)width < limit;
}
inline int check_plane(int height, int width, unsigned long long limit) {
  if (!plane_fits(height, width, limit)) return fail(GSR_ERR_INVALID_ARGUMENT, "image plane too large");
  return GSR_OK;
}
inline int check_workspace(size_t workspace_bytes, size_t need) {
  if (workspace_bytes < need) return fail(GSR_ERR_INVALID_ARGUMENT, "workspace too small: need %zu bytes", need);
  return GSR_OK;
}
constexpr const char* kMisaligned = "misaligned pointer: float and int32 arrays need 4-byte alignment";
// bits: the OR of the pointers
inline int check_aligned4(uintptr_t bits) {
  if (bits & 3u) return fail(GSR_ERR_INVALID_ARGUMENT, "%s", kMisaligned);
  return GSR_OK;
}

}  // namespace gsr

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return gsr::fail(GSR_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
  } while (0)
