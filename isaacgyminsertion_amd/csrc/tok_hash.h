// Counter-based hash shared by the kernels that draw random numbers without stored state: a value is a pure function
// of (seed, site, element), so a backward pass or a second call regenerates it.  token_encoder.h thresholds it for the
// dropout masks; augment.h turns two of them into a Gaussian sample.  oracle/token_dropout.py restates it on the host.
#pragma once
#include <hip/hip_runtime.h>

namespace igi {

__device__ __forceinline__ unsigned int tok_hash(unsigned long long seed, unsigned int site, unsigned int idx) {
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
