// Train-time augmentation of the camera pair (depth frames + segmentation masks) of the ONLINE student, in the distillation
// step (algo/ext_adapt: offline_train.img_augment_online; the reference has the call and comments it out, runner.py:421-422):
//   k_image_pair_augment_seeded : gather the minibatch's rows from the StudentBuffer's two time-major arenas and run the chain
//                                 of augment.h -- ONE launch that reads the arenas [horizon*envs rows][T][Hs][Ws] in place and
//                                 writes the two [B][T][Hs][Ws] inputs of predict.  The arenas are never written.
// A plane is (b, t, which) with which 0 = depth and 1 = mask, and a workgroup owns a band of AUG_BAND groups of four pixels of
// one plane, as in k_image_pair_augment; the chain of a pixel is aug_rows_keep of aug_pixel.h, unchanged -- rotate, noise,
// mask, store -- with the window at (0, 0) and the output at the stored size: there is no crop online.  Either arena may be
// absent: its planes are not launched, and the draws of the other do not depend on it.  What differs from augment.h is where
// the parameters come from: nothing crosses from the host but ONE seed per call.  The angle of a plane is the counter hash of
// tok_hash.h evaluated by the workgroup itself (uniform over it), and the keep cells its band covers are hashed into LDS
// behind one barrier before the chain reads them -- a pure function of (seed, frame, cell), whichever band asks.
//
// Draws (the numbers of the planes and the sites, and u / 2u - 1 / thr: draws.h).  b = the position in the minibatch (not the
// arena row), u(h) = (h >> 8) 2^-24, thr(p) = draw_threshold(p), computed on the host once; every event is an integer
// comparison.  2u - 1 is exact in fp32 (draw_unit) and the angle is ONE fp32 multiply of exact operands: a float64 product
// rounded once to fp32 gives the same bits.  max_rad is rotation_deg * pi / 180 formed in double on the host and rounded
// once to fp32; max_rad == 0 evaluates no hash and takes the angle-0 copy path of aug_window_pos.
//
//   site / plane    element (mod 2^32)          draw
//   plane 0 (0,1)   depth output's linear index noise z
//   plane 1 (2,3)   mask output's linear index  noise z
//   site 29         2*b + which                 angle = (2u - 1) * max_rad radians: one per (sample, tensor), shared by its T frames
//   site 30         (b*T + t) * gh*gw + cell    depth patch kept iff h >= thr(masking_prob)
// Only the depth frames are patch-masked; both tensors are rotated and noised (the chains of define_img_transforms).  With
// everything off a plane is the gathered frame bit for bit.  `draws` (optional): int32 [B][2], the bits of the two angles of
// sample b, both written by one lane of the band-0 workgroup of frame t = 0 of the first launched tensor.
// No atomics, no workspace: the outputs are a pure function of the arguments.  tests/img_online_ref.py restates the draws.
#pragma once
#include "augment.h"
#include "draws.h"

namespace igi {

static_assert(IMG_PLANE_DEPTH == 0 && IMG_PLANE_MASK == 1, "the noise plane of a tensor is its `which`");
constexpr int IMG_MAX_CELLS = 8192;   // keep cells per frame: one byte of LDS each

struct ImagePairSeededArgs {
  AugShape c;                    // rows: flat arena rows; N = horizon * envs; keep null, patch / gh / gw set where `masked`
  const float* src[2];           // depth, mask arenas [N][T][Hs][Ws]; null: absent
  float* dst[2];                 // [B][T][Hs][Ws]
  int* draws;                    // [B][2] or null
  int T, masked;
  int first, count;              // the launched tensors: which = first + plane % count
  float max_rad;
  unsigned long long thr_keep;
};

__device__ __forceinline__ float img_angle(const ImagePairSeededArgs& a, long long b, int which) {
  if (a.max_rad == 0.f) return 0.f;
  return draw_unit(tok_hash(a.c.seed, IMG_SITE_ANGLE, (unsigned int)(2 * b + which))) * a.max_rad;
}

// grid (planes = B*T*count, bands): a workgroup owns AUG_BAND groups of four consecutive pixels of one output plane
__global__ __launch_bounds__(256) void k_image_pair_augment_seeded(const ImagePairSeededArgs a) {
  __shared__ unsigned char keep[IMG_MAX_CELLS];
  const AugShape& c = a.c;
  const long long plane = blockIdx.x;                  // (b*T + t)*count + (which - first)
  const long long bt = plane / a.count;
  const int lane_t = (int)(plane - bt * a.count);
  const int which = a.first + lane_t;
  const long long b = bt / a.T;
  const int t = (int)(bt - b * a.T);
  const int W = c.out_w, H = c.out_h;
  const int tid = (int)threadIdx.x;
  // per-plane parameters: uniform over the workgroup
  const long long row = c.rows[b];
  const bool live = row >= 0 && row < c.N;
  const float ang = img_angle(a, b, which);
  if (a.draws && t == 0 && lane_t == 0 && blockIdx.y == 0 && tid == 0) {
    a.draws[2 * b + which] = __float_as_int(ang);
    a.draws[2 * b + (which ^ 1)] = __float_as_int(img_angle(a, b, which ^ 1));
  }
  const AugRot r = aug_rot(ang, W, H);
  const float* __restrict__ src = a.src[which] + (live ? row * a.T + t : 0) * ((long long)c.Hs * c.Ws);

  const int nq = H * c.qpr;
  const int q0 = blockIdx.y * AUG_BAND;
  const int q1 = q0 + AUG_BAND < nq ? q0 + AUG_BAND : nq;
  const bool masked = a.masked != 0 && which == 0;
  if (masked) {                                        // the cell rows this band's pixel rows fall into
    const int cy0 = (q0 / c.qpr) / c.patch;
    int cy1 = ((q1 - 1) / c.qpr) / c.patch + 1;
    cy1 = cy1 < c.gh ? cy1 : c.gh;
    const unsigned int cells = (unsigned int)(c.gh * c.gw);
    const unsigned int base = (unsigned int)bt * cells;
    for (int k = cy0 * c.gw + tid; k < cy1 * c.gw; k += 256)
      keep[k] = tok_hash(c.seed, IMG_SITE_KEEP, base + (unsigned int)k) >= a.thr_keep ? 1 : 0;
    __syncthreads();
  }
  aug_rows_keep(c, a.dst[which], bt, masked, (unsigned int)which, q0 + tid, q1,
                [&](int x, int y) {
                  int wx, wy;
                  const bool in = aug_window_pos(r, W, H, x, y, wx, wy);
                  return aug_frame_read(src, c, live && in, wy, wx);
                },
                [&](int cell) { return (float)keep[cell]; });
}

static int image_pair_augment_seeded(const float* img, const float* seg, int64_t n, int t, int hs, int ws,
                                     const int64_t* rows, int64_t b, int patch, float noise_std, double masking_prob,
                                     float max_rad, uint64_t seed, float* out_img, float* out_seg, int32_t* draws,
                                     hipStream_t s) {
  if ((!img && !seg) || (img && !out_img) || (seg && !out_seg)) return IGI_E_BADARG;
  if ((out_img && (out_img == img || out_img == seg || out_img == out_seg)) || (out_seg && (out_seg == img || out_seg == seg)))
    return IGI_E_BADARG;                                                                // an arena is never written
  if (!draw_is_prob(masking_prob) || (masking_prob > 0 && patch < 1) || !(max_rad >= 0.f)) return IGI_E_BADARG;
  if ((long long)hs * ws > (1ll << 24)) return IGI_E_BADARG;                            // grid.y and int pixel numbers
  ImagePairSeededArgs a;
  if (int rc = aug_shape(a.c, n, t, hs, ws, rows, b, nullptr, hs, ws, 1, noise_std, seed,
                         (!img || aligned16(out_img)) && (!seg || aligned16(out_seg))))
    return rc;
  const bool cells = masking_prob > 0 && hs / patch > 0 && ws / patch > 0;
  if (cells && (long long)(hs / patch) * (ws / patch) > IMG_MAX_CELLS) return IGI_E_UNSUPPORTED;   // the LDS grid
  a.masked = cells && img;
  if (a.masked) { a.c.patch = patch; a.c.gh = hs / patch; a.c.gw = ws / patch; }
  a.src[0] = img; a.src[1] = seg; a.dst[0] = out_img; a.dst[1] = out_seg;
  a.draws = draws; a.T = t;
  a.first = img ? 0 : 1; a.count = (img && seg) ? 2 : 1;
  a.max_rad = max_rad; a.thr_keep = draw_threshold(masking_prob);
  if (b * t * a.count > (1ll << 30)) return IGI_E_BADARG;
  const long long nq = (long long)hs * a.c.qpr;
  hipLaunchKernelGGL(k_image_pair_augment_seeded,
                     dim3((unsigned)(b * t * a.count), (unsigned)((nq + AUG_BAND - 1) / AUG_BAND)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
