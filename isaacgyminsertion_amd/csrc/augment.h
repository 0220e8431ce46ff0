// Train-time augmentation of the camera pair (depth frames + segmentation masks) of the offline student, straight from
// the resident arenas (algo/models/transformer/utils.py:85-128, 280-322 as called from data.py:366-367):
//   k_image_pair_augment : gather the minibatch's samples, crop both tensors with one window per sample, rotate each by its
//                          own angle (nearest resampling, zero fill), add Gaussian noise to both, zero whole patches of the
//                          depth frame -- ONE launch that reads the two arenas and writes the two batch tensors.
// Per output pixel, in the reference's order:
//   1. crop     window [top, top+out_h) x [left, left+out_w) of frame rows[b]; a read outside the frame gives 0
//   2. rotate   about the window's centre; the source coordinate is that of F.affine_grid / F.grid_sample(nearest, zeros,
//               align_corners=False) with theta = [[cos, -sin*H/W, 0], [sin*W/H, cos, 0]], which in pixel units is
//                 sx = cos*xc - sin*yc + (W/2 - 1/2),  sy = sin*xc + cos*yc + (H/2 - 1/2),  xc = x + 1/2 - W/2, yc likewise
//               rounded to nearest-even; a source outside the WINDOW gives 0 (the reference rotates the cropped tensor).
//               Angle 0 copies the window without this arithmetic; the angle is uniform over a workgroup
//   3. noise    + noise_std * z,  z = sqrt(-2 ln u1) cos(2 pi u2),  u1 = ((h1 >> 8) + 1/2) 2^-24,  u2 = (h2 >> 8) 2^-24,
//               h1 = tok_hash(seed, 2*plane, e), h2 = tok_hash(seed, 2*plane + 1, e); plane 0 = depth, 1 = mask; e = the
//               element's linear index in its output tensor (mod 2^32)
//   4. mask     depth only: times keep[b*T + t][y / patch][x / patch]; rows / columns past the last whole patch are kept
// No LDS, no atomics, no workspace: the outputs are a pure function of the arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aug_gauss.h"
#include "gemm_f32.h"

namespace igi {

constexpr int AUG_BAND = 1024;   // groups of four pixels per workgroup: four per thread

struct ImagePairArgs {
  const float* src[2];           // depth, mask arenas [N][T][Hs][Ws]
  float* dst[2];                 // [B][T][out_h][out_w]
  const long long* rows;         // [B] sample numbers; outside [0, N): the frame reads as zeros
  const int* offsets;            // [B][2] top, left
  const float* angles;           // [B][2] radians: depth, mask
  const unsigned char* keep;     // [B*T][gh][gw] or null
  long long N;
  int T, Hs, Ws, out_h, out_w, patch, gh, gw;
  int qpr;                       // groups of four per output row
  int vec;                       // 1: 16-byte stores (out_w % 4 == 0, both outputs 16-byte aligned)
  float noise_std;
  unsigned long long seed;
};

// grid (planes = B*T*2, bands): a workgroup owns AUG_BAND groups of four consecutive pixels of one output plane
__global__ __launch_bounds__(256) void k_image_pair_augment(const ImagePairArgs a) {
  const long long plane = blockIdx.x;                  // (b*T + t)*2 + which
  const int which = (int)(plane & 1);
  const long long bt = plane >> 1;
  const long long b = bt / a.T;
  const int t = (int)(bt - b * a.T);
  const int W = a.out_w, H = a.out_h;
  // per-sample parameters: uniform over the workgroup
  const long long row = a.rows[b];
  const bool live = row >= 0 && row < a.N;
  const long long top = a.offsets[2 * b], left = a.offsets[2 * b + 1];
  const float ang = a.angles[2 * b + which];
  const bool rot = ang != 0.f;
  float sn = 0.f, cs = 1.f;
  if (rot) sincosf(ang, &sn, &cs);
  const float hx = 0.5f * (float)W - 0.5f, hy = 0.5f * (float)H - 0.5f;   // W/2 - 1/2: exact
  const float* __restrict__ src = a.src[which] + (live ? row * a.T + t : 0) * ((long long)a.Hs * a.Ws);
  const long long e0 = bt * ((long long)H * W);
  float* __restrict__ dst = a.dst[which] + e0;
  const unsigned char* __restrict__ keep =
      (which == 0 && a.keep) ? a.keep + bt * ((long long)a.gh * a.gw) : nullptr;
  const int mh = a.gh * a.patch, mw = a.gw * a.patch;  // the masked region (whole patches)

  const int nq = H * a.qpr;
  const int q0 = blockIdx.y * AUG_BAND;
  const int q1 = q0 + AUG_BAND < nq ? q0 + AUG_BAND : nq;
  for (int q = q0 + (int)threadIdx.x; q < q1; q += 256) {
    const int y = q / a.qpr, x0 = (q - y * a.qpr) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      v[j] = 0.f;
      if (x >= W) continue;
      int wx = x, wy = y;                              // position in the cropped window
      bool in = live;
      if (rot) {
        const float xc = (float)x - hx, yc = (float)y - hy;
        const float fx = rintf((cs * xc - sn * yc) + hx), fy = rintf((sn * xc + cs * yc) + hy);
        in = in && fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;   // false for a NaN angle too
        wx = in ? (int)fx : 0;
        wy = in ? (int)fy : 0;
      }
      const long long sy = wy + top, sx = wx + left;   // position in the stored frame
      in = in && sy >= 0 && sy < a.Hs && sx >= 0 && sx < a.Ws;
      float p = in ? src[sy * a.Ws + sx] : 0.f;
      if (a.noise_std > 0.f)
        p = p + a.noise_std * aug_gauss(a.seed, (unsigned int)which, (unsigned int)(e0 + (long long)y * W + x));
      if (keep && y < mh && x < mw) p = p * (float)keep[(y / a.patch) * a.gw + x / a.patch];
      v[j] = p;
    }
    float* o = dst + (long long)y * W + x0;
    if (a.vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) o[j] = v[j];
    }
  }
}

static int image_pair_augment(const float* img, const float* seg, int64_t n, int t, int hs, int ws, const int64_t* rows,
                              int64_t b, const int32_t* offsets, const float* angles, const uint8_t* keep, int out_h,
                              int out_w, int patch, float noise_std, uint64_t seed, float* out_img, float* out_seg,
                              hipStream_t s) {
  if (!img || !seg || !rows || !offsets || !angles || !out_img || !out_seg) return IGI_E_BADARG;
  if (n < 1 || t < 1 || hs < 1 || ws < 1 || b < 1 || out_h < 1 || out_w < 1 || out_h > hs || out_w > ws) return IGI_E_BADARG;
  if (!(noise_std >= 0.f) || (keep && patch < 1)) return IGI_E_BADARG;
  if (b * t > (1ll << 30) || (long long)hs * ws > (1ll << 24)) return IGI_E_BADARG;   // grid.x; grid.y and int pixel numbers
  ImagePairArgs a;
  a.src[0] = img; a.src[1] = seg; a.dst[0] = out_img; a.dst[1] = out_seg;
  a.rows = (const long long*)rows; a.offsets = offsets; a.angles = angles; a.keep = keep;
  a.N = n; a.T = t; a.Hs = hs; a.Ws = ws; a.out_h = out_h; a.out_w = out_w;
  a.patch = keep ? patch : 1;
  a.gh = keep ? out_h / patch : 0;
  a.gw = keep ? out_w / patch : 0;
  a.qpr = (out_w + 3) / 4;
  a.vec = (out_w % 4 == 0) && aligned16(out_img) && aligned16(out_seg);
  a.noise_std = noise_std; a.seed = seed;
  const long long nq = (long long)out_h * a.qpr;
  hipLaunchKernelGGL(k_image_pair_augment, dim3((unsigned)(b * t * 2), (unsigned)((nq + AUG_BAND - 1) / AUG_BAND)),
                     dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
