// Train-time augmentation of the tactile images of the ONLINE student, in the distillation step (algo/ext_adapt:
// offline_train.tactile_augment_online; the reference has the call and comments it out, runner.py:402):
//   k_tactile_augment_seeded : gather the minibatch's rows from the StudentBuffer's time-major arena and run the whole chain
//                              of tactile_augment.h -- ONE launch that reads the arena [T*N rows][planes][Hs][Ws] in place
//                              and writes [B][planes][out_h][out_w].  The arena is never written.
// The chain of an image is tac_image of tactile_augment.h, the one k_tactile_augment runs -- jitter about the image's mean
// (the same LDS window, the same fixed summation order), rotation, noise on plane 2, patch mask, store -- with the window at
// (0, 0).  What differs is where the parameters come from: nothing crosses from the host but ONE seed per call.  Every
// per-image parameter is the counter hash of tok_hash.h evaluated by the workgroup itself (uniform over it), and the
// image's keep grid is built in LDS by the workgroup before the chain reads it.
//
// Draws (the numbers of the plane and the sites, and u / 2u - 1 / thr: draws.h).  image = b * planes + plane (mod 2^32),
// u(h) = (h >> 8) 2^-24, thr(p) = draw_threshold(p), computed on the host once; every event is an integer comparison, so
// fp32 and a float64 restatement agree on all of them.  2u - 1 is exact in fp32, and each factor below is ONE rounding of
// exact operands (the fmaf is explicit): float64 arithmetic rounded once to fp32 gives the same bits.
//
//   site / plane    element                  draw
//   plane 2 (4,5)   out's linear index       noise z
//   site 23         image                    jitter flag: h < thr(0.3)
//   site 24         image                    brightness b = fmaf(2u - 1, 0.1f, 1.0f); 1 where the flag is off
//   site 25         image                    contrast c, likewise
//   site 26         image                    rotate flag: h < thr(0.5)
//   site 27         image                    angle = (2u - 1) * (float)(3 pi / 180) radians; 0 where the flag is off
//   site 28         image * gh*gw + cell     patch kept iff h >= thr(masking_prob)
// An image with both flags off passes bit for bit, without the LDS window or the clamp.  `draws` (optional): one lane per
// workgroup writes the image's record in the layout of TAC_PARAM_WORDS -- 0, 0, flag, bits of b, c, angle.
// No atomics, no workspace: the output is a pure function of the arguments.  tests/tactile_online_ref.py restates the draws.
#pragma once
#include "draws.h"
#include "tactile_augment.h"

namespace igi {

constexpr float TAC_JITTER = 0.1f;                       // TactileAugment.JITTER
constexpr float TAC_ROTATE_RAD = (float)(3.0 * 3.141592653589793 / 180.0);   // TactileAugment.ROTATE_DEG, in radians

struct TactileSeededArgs {
  AugShape c;                    // rows: flat arena rows; N = T * N; keep null, patch / gh / gw set where `masked`
  const float* src;              // arena [T*N][planes][Hs][Ws]
  float* dst;                    // [B][planes][out_h][out_w]
  int* draws;                    // [B*planes][TAC_PARAM_WORDS] or null
  int planes, masked;
  unsigned long long thr_jitter, thr_rotate, thr_keep;
};

// grid (images = B * planes)
__global__ __launch_bounds__(256) void k_tactile_augment_seeded(const TactileSeededArgs a) {
  __shared__ float win[TAC_MAX_PIXELS];
  __shared__ float wave_sum[4];
  __shared__ unsigned char keep[TAC_MAX_PIXELS];      // at most one cell per pixel (patch 1)
  const AugShape& c = a.c;
  const long long image = blockIdx.x;                  // b * planes + plane
  const long long b = image / a.planes;
  const int plane = (int)(image - b * a.planes);
  const int tid = (int)threadIdx.x;
  const unsigned int im = (unsigned int)image;
  // per-image parameters: uniform over the workgroup
  const bool jit = tok_hash(c.seed, TAC_SITE_JITTER, im) < a.thr_jitter;
  const bool rot = tok_hash(c.seed, TAC_SITE_ROTATE, im) < a.thr_rotate;
  const float jb = jit ? __fmaf_rn(draw_unit(tok_hash(c.seed, TAC_SITE_BRIGHT, im)), TAC_JITTER, 1.0f) : 1.0f;
  const float jc = jit ? __fmaf_rn(draw_unit(tok_hash(c.seed, TAC_SITE_CONTRAST, im)), TAC_JITTER, 1.0f) : 1.0f;
  const float ang = rot ? draw_unit(tok_hash(c.seed, TAC_SITE_ANGLE, im)) * TAC_ROTATE_RAD : 0.0f;
  if (a.draws && tid == 0) {
    int* __restrict__ d = a.draws + image * TAC_PARAM_WORDS;
    d[0] = 0; d[1] = 0; d[2] = jit ? 1 : 0;
    d[3] = __float_as_int(jb); d[4] = __float_as_int(jc); d[5] = __float_as_int(ang);
  }
  if (a.masked) {
    const unsigned int cells = (unsigned int)(c.gh * c.gw);
    for (unsigned int k = (unsigned int)tid; k < cells; k += 256u)
      keep[k] = tok_hash(c.seed, TAC_SITE_KEEP, im * cells + k) >= a.thr_keep ? 1 : 0;
    __syncthreads();
  }
  const long long row = c.rows[b];
  const bool live = row >= 0 && row < c.N;
  const float* __restrict__ src = a.src + (live ? row * a.planes + plane : 0) * ((long long)c.Hs * c.Ws);
  tac_image(c, src, live, a.dst, image, 0, 0, jit, jb, jc, ang, a.masked != 0, win, wave_sum,
            [&](int cell) { return (float)keep[cell]; });
}

static int tactile_augment_seeded(const float* arena, int64_t n, int planes, int hs, int ws, const int64_t* rows, int64_t b,
                                  int out_h, int out_w, int patch, float noise_std, double masking_prob, uint64_t seed,
                                  float* out, int32_t* draws, hipStream_t s) {
  if (!arena || !out || arena == out) return IGI_E_BADARG;
  if (!draw_is_prob(masking_prob) || (masking_prob > 0 && patch < 1)) return IGI_E_BADARG;
  TactileSeededArgs a;
  if (int rc = aug_shape(a.c, n, planes, hs, ws, rows, b, nullptr, out_h, out_w, 1, noise_std, seed, aligned16(out)))
    return rc;
  if ((long long)out_h * out_w > TAC_MAX_PIXELS) return IGI_E_UNSUPPORTED;              // the LDS window
  a.masked = masking_prob > 0 && out_h / patch > 0 && out_w / patch > 0;
  if (a.masked) { a.c.patch = patch; a.c.gh = out_h / patch; a.c.gw = out_w / patch; }
  a.src = arena; a.dst = out; a.draws = draws; a.planes = planes;
  a.thr_jitter = draw_threshold(0.3); a.thr_rotate = draw_threshold(0.5); a.thr_keep = draw_threshold(masking_prob);
  hipLaunchKernelGGL(k_tactile_augment_seeded, dim3((unsigned)(b * planes)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
