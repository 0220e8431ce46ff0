// Counter-based hash shared by the kernels that draw random numbers without stored state: a value is a pure function
// of (seed, site, element), so a backward pass or a second call regenerates it.  token_encoder.h thresholds it for the
// dropout masks; draws.h holds the conventions of the augmentation kernels' draws.  oracle/token_dropout.py restates it on
// the host.  Compiles in a plain host C++ translation unit too (tools/draws_check.cpp).
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#define __forceinline__ inline
#endif

namespace igi {

__host__ __device__ __forceinline__ unsigned int tok_hash(unsigned long long seed, unsigned int site, unsigned int idx) {
  unsigned int x = idx * 0x9E3779B1u ^ (unsigned int)seed ^ (site * 0x85EBCA77u);
  x ^= x >> 16; x *= 0x7FEB352Du;
  x ^= x >> 15; x *= 0x846CA68Bu;
  x ^= x >> 16;
  x += (unsigned int)(seed >> 32);
  x ^= x >> 15; x *= 0x2C1B3C6Du;
  x ^= x >> 12; x *= 0x297A2D39u;
  x ^= x >> 15;
  return x;
}

}  // namespace igi
