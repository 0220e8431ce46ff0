// The Gaussian sample of the augmentation kernels (aug_pixel.h): Box-Muller over two values of the counter
// hash, a pure function of (seed, plane, element): plane p uses sites 2p and 2p + 1.  The planes in use are tabled in
// draws.h.  tests/img_augment_ref.py `gauss` restates it in float64.
#pragma once
#include <hip/hip_runtime.h>

#include "draws.h"

namespace igi {

// ln(u1) of u1 = (k + 1/2) 2^-24, k < 2^24.  k + 1/2 is exact in fp32 below 2^23; above it 2^24 - (k + 1/2) is, and
// log1pf of the exact distance from 1 keeps z accurate where u1 -> 1 (z -> 0).
__device__ __forceinline__ float aug_log_u1(unsigned int k) {
  if (k < (1u << 23)) return logf(((float)k + 0.5f) * 0x1p-24f);
  return log1pf(-(((float)(0xFFFFFFu - k) + 0.5f) * 0x1p-24f));
}

__device__ __forceinline__ float aug_gauss(unsigned long long seed, unsigned int plane, unsigned int e) {
  const unsigned int h1 = tok_hash(seed, 2u * plane, e), h2 = tok_hash(seed, 2u * plane + 1u, e);
  return sqrtf(-2.0f * aug_log_u1(h1 >> 8)) * cosf(6.283185307179586f * draw_u(h2));
}

}  // namespace igi
