// The order-preserving 32-bit key of an fp32 score that the walk-decision kernel (gnm_decision.hip) and the cover rounds
// (gnm_cover.hip) compare candidates on (include/gnm.h, "walk decisions"):
//
//   key(x) = 0 if x is NaN, else u ^ ((u >> 31) ? 0xFFFFFFFF : 0x80000000),  u = bits(x == -0 ? +0 : x)
//
// -0 and +0 tie, a denormal keeps its bits, -inf has the lowest key a number takes (0x007FFFFF) and 0 -- the image of no number --
// is given to every NaN.
#pragma once
#include <hip/hip_runtime.h>

namespace gnm {

__device__ __forceinline__ unsigned dec_key_(float x) {
  unsigned u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0u;       // NaN: below every number
  if (u == 0x80000000u) u = 0u;                         // -0 -> +0
  return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

}  // namespace gnm
