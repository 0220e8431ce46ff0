// The one home of the draw conventions of the augmentation kernels: every random number they use is the counter hash of
// tok_hash.h, a pure function of (seed, site, element).  Here: the table of Gaussian planes and sites -- ONE flat
// namespace -- and the helpers that turn a hash into an event, a uniform value or an index.  What a header's own draws
// mean (element numbering, arithmetic, which seed) is tabled in that header.  isaacgyminsertion_amd/draws.py restates
// this file for the host; tests/test_draws_cpu.py compares the two and tools/draws_check.cpp prints this one.
// (The token encoder's dropout sites, 4 l + k under the encoder's own seed, are a different namespace: token_math.h.)
//
// To add a site: one constant and one row below, one line in draws.py, one in the test reference that restates the draw.
// Compiles in a plain host C++ translation unit.
#pragma once
#include "tok_hash.h"

namespace igi {

// Gaussian planes (aug_gauss.h): plane p occupies sites 2p and 2p + 1.
constexpr unsigned int IMG_PLANE_DEPTH = 0, IMG_PLANE_MASK = 1;    // augment.h, augment_seeded.h: the noise plane is `which`
constexpr unsigned int TAC_NOISE_PLANE = 2;                        // tactile_augment.h, tactile_augment_seeded.h
constexpr unsigned int PCL_PLANE_PN = 3, PCL_PLANE_JITTER = 4, PCL_PLANE_FREE = 5, PCL_PLANE_CONTOUR = 6;   // pcl_augment.h
// Sites.
constexpr unsigned int PCL_SITE_HIT = 14, PCL_SITE_ANGLE = 15, PCL_SITE_AXIS = 16, PCL_SITE_MASK = 17,
                       PCL_SITE_CONTOUR = 18, PCL_SITE_SIDE = 19, PCL_SITE_INDEX = 20, PCL_SITE_EXEMPT = 21,
                       PCL_SITE_DROP = 22;                         // pcl_augment.h
constexpr unsigned int TAC_SITE_JITTER = 23, TAC_SITE_BRIGHT = 24, TAC_SITE_CONTRAST = 25, TAC_SITE_ROTATE = 26,
                       TAC_SITE_ANGLE = 27, TAC_SITE_KEEP = 28;    // tactile_augment_seeded.h
constexpr unsigned int IMG_SITE_ANGLE = 29, IMG_SITE_KEEP = 30;    // augment_seeded.h

struct DrawName { const char* name; unsigned int number; };
#define IGI_DRAW_ROW(name) {#name, name}
constexpr DrawName DRAW_PLANES[] = {
    IGI_DRAW_ROW(IMG_PLANE_DEPTH), IGI_DRAW_ROW(IMG_PLANE_MASK), IGI_DRAW_ROW(TAC_NOISE_PLANE), IGI_DRAW_ROW(PCL_PLANE_PN),
    IGI_DRAW_ROW(PCL_PLANE_JITTER), IGI_DRAW_ROW(PCL_PLANE_FREE), IGI_DRAW_ROW(PCL_PLANE_CONTOUR)};
constexpr DrawName DRAW_SITES[] = {
    IGI_DRAW_ROW(PCL_SITE_HIT), IGI_DRAW_ROW(PCL_SITE_ANGLE), IGI_DRAW_ROW(PCL_SITE_AXIS), IGI_DRAW_ROW(PCL_SITE_MASK),
    IGI_DRAW_ROW(PCL_SITE_CONTOUR), IGI_DRAW_ROW(PCL_SITE_SIDE), IGI_DRAW_ROW(PCL_SITE_INDEX), IGI_DRAW_ROW(PCL_SITE_EXEMPT),
    IGI_DRAW_ROW(PCL_SITE_DROP), IGI_DRAW_ROW(TAC_SITE_JITTER), IGI_DRAW_ROW(TAC_SITE_BRIGHT), IGI_DRAW_ROW(TAC_SITE_CONTRAST),
    IGI_DRAW_ROW(TAC_SITE_ROTATE), IGI_DRAW_ROW(TAC_SITE_ANGLE), IGI_DRAW_ROW(TAC_SITE_KEEP), IGI_DRAW_ROW(IMG_SITE_ANGLE),
    IGI_DRAW_ROW(IMG_SITE_KEEP)};
#undef IGI_DRAW_ROW

// The N numbers of `v` are pairwise distinct and fill [first, first + N): N numbers set N bits only if none clashes and
// none lies outside.
template <unsigned int N>
constexpr bool draw_numbers_fill(const DrawName (&v)[N], unsigned int first) {
  unsigned long long seen = 0;
  for (const DrawName& r : v) seen |= r.number - first < N ? 1ull << (r.number - first) : 0ull;
  return seen == (1ull << N) - 1;
}
static_assert(draw_numbers_fill(DRAW_PLANES, 0), "Gaussian planes: pairwise distinct, 0 .. n - 1");
static_assert(draw_numbers_fill(DRAW_SITES, 2 * sizeof(DRAW_PLANES) / sizeof(DrawName)),
              "sites: pairwise distinct, contiguous, the first at twice the number of Gaussian planes");

// A Bernoulli event of probability p is the integer comparison  tok_hash(...) < draw_threshold(p):  p rounded to fp32, times
// 2^32, truncated (oracle/token_dropout.py `threshold`), kept in 64 bits so that p = 1 -> 2^32 is "always".  fp32 and
// float64 restatements agree on every event.
inline unsigned long long draw_threshold(double p) {
  return p > 0 ? (unsigned long long)((double)(float)p * 4294967296.0) : 0ull;
}

inline bool draw_is_prob(double p) { return p >= 0 && p <= 1; }

// u = (h >> 8) 2^-24 in [0, 1): exact in fp32.
__host__ __device__ __forceinline__ float draw_u(unsigned int h) { return (float)(h >> 8) * 0x1p-24f; }

// 2u - 1 in [-1, 1): exact in fp32.
__host__ __device__ __forceinline__ float draw_unit(unsigned int h) { return 2.0f * draw_u(h) - 1.0f; }

// floor(u n), an index in [0, n) for 0 < n < 2^32.
__host__ __device__ __forceinline__ unsigned int draw_index(unsigned int h, unsigned long long n) {
  return (unsigned int)(((unsigned long long)(h >> 8) * n) >> 24);
}

}  // namespace igi
