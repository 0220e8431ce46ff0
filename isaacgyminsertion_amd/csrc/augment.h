// Train-time augmentation of the camera pair (depth frames + segmentation masks) of the offline student, straight from
// the resident arenas (algo/models/transformer/utils.py:85-128, 280-322 as called from data.py:366-367):
//   k_image_pair_augment : gather the minibatch's samples, crop both tensors with one window per sample, rotate each by its
//                          own angle (nearest resampling, zero fill), add Gaussian noise to both, zero whole patches of the
//                          depth frame -- ONE launch that reads the two arenas and writes the two batch tensors.
// Every output pixel goes through the chain of aug_pixel.h -- crop, rotate, noise, mask, store -- in the reference's order.
// This kernel's own: a plane is (sample b, frame t, which: 0 = depth, 1 = mask); the window is the sample's, the angle the
// sample's for that tensor, the noise plane is `which`, and only the depth frame has a keep grid, keep[b*T + t].
// No LDS, no atomics, no workspace: the outputs are a pure function of the arguments.
#pragma once
#include "aug_pixel.h"

namespace igi {

constexpr int AUG_BAND = 1024;   // groups of four pixels per workgroup: four per thread

struct ImagePairArgs {
  AugShape c;                    // keep: [B*T][gh][gw]
  const float* src[2];           // depth, mask arenas [N][T][Hs][Ws]
  float* dst[2];                 // [B][T][out_h][out_w]
  const int* offsets;            // [B][2] top, left
  const float* angles;           // [B][2] radians: depth, mask
  int T;
};

// grid (planes = B*T*2, bands): a workgroup owns AUG_BAND groups of four consecutive pixels of one output plane
__global__ __launch_bounds__(256) void k_image_pair_augment(const ImagePairArgs a) {
  const AugShape& c = a.c;
  const long long plane = blockIdx.x;                  // (b*T + t)*2 + which
  const int which = (int)(plane & 1);
  const long long bt = plane >> 1;
  const long long b = bt / a.T;
  const int t = (int)(bt - b * a.T);
  const int W = c.out_w, H = c.out_h;
  // per-sample parameters: uniform over the workgroup
  const long long row = c.rows[b];
  const bool live = row >= 0 && row < c.N;
  const long long top = a.offsets[2 * b], left = a.offsets[2 * b + 1];
  const AugRot r = aug_rot(a.angles[2 * b + which], W, H);
  const float* __restrict__ src = a.src[which] + (live ? row * a.T + t : 0) * ((long long)c.Hs * c.Ws);

  const int nq = H * c.qpr;
  const int q0 = blockIdx.y * AUG_BAND;
  const int q1 = q0 + AUG_BAND < nq ? q0 + AUG_BAND : nq;
  aug_rows(c, a.dst[which], bt, which == 0, (unsigned int)which, q0 + (int)threadIdx.x, q1, [&](int x, int y) {
    int wx, wy;
    const bool in = aug_window_pos(r, W, H, x, y, wx, wy);
    return aug_frame_read(src, c, live && in, wy + top, wx + left);
  });
}

static int image_pair_augment(const float* img, const float* seg, int64_t n, int t, int hs, int ws, const int64_t* rows,
                              int64_t b, const int32_t* offsets, const float* angles, const uint8_t* keep, int out_h,
                              int out_w, int patch, float noise_std, uint64_t seed, float* out_img, float* out_seg,
                              hipStream_t s) {
  if (!img || !seg || !offsets || !angles || !out_img || !out_seg) return IGI_E_BADARG;
  if ((long long)hs * ws > (1ll << 24)) return IGI_E_BADARG;                           // grid.y and int pixel numbers
  ImagePairArgs a;
  if (int rc = aug_shape(a.c, n, t, hs, ws, rows, b, keep, out_h, out_w, patch, noise_std, seed,
                         aligned16(out_img) && aligned16(out_seg)))
    return rc;
  a.src[0] = img; a.src[1] = seg; a.dst[0] = out_img; a.dst[1] = out_seg;
  a.offsets = offsets; a.angles = angles; a.T = t;
  const long long nq = (long long)out_h * a.c.qpr;
  hipLaunchKernelGGL(k_image_pair_augment, dim3((unsigned)(b * t * 2), (unsigned)((nq + AUG_BAND - 1) / AUG_BAND)),
                     dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
