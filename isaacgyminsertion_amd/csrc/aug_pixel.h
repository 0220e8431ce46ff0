// What every output pixel of the augmentation kernels goes through (augment.h: the camera pair; tactile_augment.h and
// tactile_augment_seeded.h: the tactile images), written once.  An output plane is out_h x out_w pixels cut from a stored
// frame of Hs x Ws; per pixel:
//   crop     window [top, top+out_h) x [left, left+out_w) of the frame; a read outside the frame, and every read of a
//            sample that is not live (number outside [0, N)), gives 0                                  -- aug_frame_read
//   rotate   about the window's centre; the source coordinate is that of F.affine_grid / F.grid_sample(nearest, zeros,
//            align_corners=False) with theta = [[cos, -sin*H/W, 0], [sin*W/H, cos, 0]], which in pixel units is
//              sx = cos*xc - sin*yc + (W/2 - 1/2),  sy = sin*xc + cos*yc + (H/2 - 1/2),  xc = x + 1/2 - W/2, yc likewise
//            rounded to nearest-even; a source outside the WINDOW gives 0 (the reference rotates the cropped tensor), and
//            so does a NaN angle.  Angle 0 copies the window without this arithmetic; the angle is uniform over a
//            workgroup                                                                       -- aug_rot, aug_window_pos
//   noise    + noise_std * z,  z = sqrt(-2 ln u1) cos(2 pi u2) of aug_gauss.h at (seed, noise plane, e); e = the
//            element's linear index in its output tensor (mod 2^32)
//   mask     times keep[y / patch][x / patch] where the plane has a keep grid; rows / columns past the last whole patch
//            are kept
//   store    groups of four consecutive pixels of a row: one 16-byte store where out_w % 4 == 0 and the output is 16-byte
//            aligned, scalar stores (the last group of a row may be partial) elsewhere
// aug_rows is that chain from noise on, over a range of groups; where the window's value comes from -- the stored frame
// through the window, LDS, the stored frame unrotated -- is its `fetch` argument, and where a patch's keep value comes from
// -- the caller's grids in global memory, a grid the workgroup built in LDS -- is the `keep_of` argument of aug_rows_keep
// (aug_rows is that function over AugShape's own grids).  AugShape and aug_shape hold what the launches check and derive
// alike.  tests/img_augment_ref.py restates every step in float64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aug_gauss.h"
#include "gemm_f32.h"

namespace igi {

struct AugShape {
  const long long* rows;         // [B] sample numbers; outside [0, N): the frames read as zeros
  const unsigned char* keep;     // [images][gh][gw] or null
  long long N;
  int Hs, Ws, out_h, out_w, patch, gh, gw;
  int qpr;                       // groups of four per output row
  int vec;                       // 1: 16-byte stores (out_w % 4 == 0, every output 16-byte aligned)
  float noise_std;
  unsigned long long seed;
};

// The argument checks and derived fields both launches share; `images` per sample bounds grid.x.
static int aug_shape(AugShape& c, int64_t n, int images, int hs, int ws, const int64_t* rows, int64_t b, const uint8_t* keep,
                     int out_h, int out_w, int patch, float noise_std, uint64_t seed, bool outputs_aligned16) {
  if (!rows || n < 1 || images < 1 || hs < 1 || ws < 1 || b < 1 || out_h < 1 || out_w < 1 || out_h > hs || out_w > ws)
    return IGI_E_BADARG;
  if (!(noise_std >= 0.f) || (keep && patch < 1) || b * images > (1ll << 30)) return IGI_E_BADARG;
  c.rows = (const long long*)rows; c.keep = keep;
  c.N = n; c.Hs = hs; c.Ws = ws; c.out_h = out_h; c.out_w = out_w;
  c.patch = keep ? patch : 1;
  c.gh = keep ? out_h / patch : 0;
  c.gw = keep ? out_w / patch : 0;
  c.qpr = (out_w + 3) / 4;
  c.vec = (out_w % 4 == 0) && outputs_aligned16;
  c.noise_std = noise_std; c.seed = seed;
  return 0;
}

struct AugRot {
  bool on;                       // angle != 0
  float sn, cs, hx, hy;          // hx = W/2 - 1/2: exact
};

__device__ __forceinline__ AugRot aug_rot(float ang, int W, int H) {
  AugRot r{ang != 0.f, 0.f, 1.f, 0.5f * (float)W - 0.5f, 0.5f * (float)H - 0.5f};
  if (r.on) sincosf(ang, &r.sn, &r.cs);
  return r;
}

// Output pixel (x, y) -> its position (wx, wy) in the window; false (and position 0, 0) where that leaves the window.
__device__ __forceinline__ bool aug_window_pos(const AugRot& r, int W, int H, int x, int y, int& wx, int& wy) {
  wx = x; wy = y;
  if (!r.on) return true;
  const float xc = (float)x - r.hx, yc = (float)y - r.hy;
  const float fx = rintf((r.cs * xc - r.sn * yc) + r.hx), fy = rintf((r.sn * xc + r.cs * yc) + r.hy);
  const bool in = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;   // false for a NaN angle too
  wx = in ? (int)fx : 0;
  wy = in ? (int)fy : 0;
  return in;
}

// The stored frame `src` at (sy, sx) = window position + (top, left), 0 outside it or where `in` is false.
__device__ __forceinline__ float aug_frame_read(const float* __restrict__ src, const AugShape& c, bool in, long long sy,
                                                long long sx) {
  in = in && sy >= 0 && sy < c.Hs && sx >= 0 && sx < c.Ws;
  return in ? src[sy * c.Ws + sx] : 0.f;
}

// Groups q = q0, q0 + 256, ... < q1 of output plane number `image` (its tensor's base `out`): fetch(x, y), noise of
// `noise_plane`, times keep_of(cell) inside the c.gh x c.gw whole patches where `masked`, store.
template <class Fetch, class Keep>
__device__ __forceinline__ void aug_rows_keep(const AugShape& c, float* __restrict__ out, long long image, bool masked,
                                              unsigned int noise_plane, int q0, int q1, Fetch fetch, Keep keep_of) {
  const int W = c.out_w;
  const long long e0 = image * ((long long)c.out_h * W);
  float* __restrict__ dst = out + e0;
  const int mh = c.gh * c.patch, mw = c.gw * c.patch;  // the masked region (whole patches)
  for (int q = q0; q < q1; q += 256) {
    const int y = q / c.qpr, x0 = (q - y * c.qpr) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      v[j] = 0.f;
      if (x >= W) continue;
      float p = fetch(x, y);
      if (c.noise_std > 0.f)
        p = p + c.noise_std * aug_gauss(c.seed, noise_plane, (unsigned int)(e0 + (long long)y * W + x));
      if (masked && y < mh && x < mw) p = p * keep_of((y / c.patch) * c.gw + x / c.patch);
      v[j] = p;
    }
    float* o = dst + (long long)y * W + x0;
    if (c.vec) {
      *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < W) o[j] = v[j];
    }
  }
}

// The same with the plane's keep grid of AugShape (or none).
template <class Fetch>
__device__ __forceinline__ void aug_rows(const AugShape& c, float* __restrict__ out, long long image, bool masked,
                                         unsigned int noise_plane, int q0, int q1, Fetch fetch) {
  const unsigned char* __restrict__ keep = (masked && c.keep) ? c.keep + image * ((long long)c.gh * c.gw) : nullptr;
  aug_rows_keep(c, out, image, keep != nullptr, noise_plane, q0, q1, fetch, [&](int cell) { return (float)keep[cell]; });
}

}  // namespace igi
