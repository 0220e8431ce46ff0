// Train-time augmentation of the tactile images of the offline student, straight from the loader's resident arena
// (algo/models/transformer/utils.py: _Crop + _TrainAugment + GaussianNoise + Masking as called from data.py's loader):
//   k_tactile_augment : gather the minibatch's samples and run the whole chain -- ONE launch that reads the arena
//                       [N][T][F][Hs][Ws] and writes the batch tensor [B][T][F][out_h][out_w].
// An image is one (sample, t, finger) plane; every image has its own parameters (the reference transforms image by image).
// Per image, in the torch path's order:
//   1. crop     window [top, top+out_h) x [left, left+out_w) of frame rows[b]; a sample number outside [0, N) and a
//               position outside the stored frame read 0
//   2. jitter   flag on: x = clamp(x*b, 0, 1); m = mean of the image; x = clamp((x - m)*c + m, 0, 1) -- _TrainAugment's
//               arithmetic and order.  Flag off: the window passes bit for bit (no clamp)
//   3. rotate   about the window's centre: theta, coordinate and rounding of augment.h step 2 (nearest, zero fill outside
//               the WINDOW); angle 0 copies
//   4. noise    + noise_std * aug_gauss(seed, plane 2, e), e = the element's linear index in the output tensor (mod 2^32)
//   5. mask     times keep[image][y / patch][x / patch]; rows / columns past the last whole patch are kept
// (_TrainAugment's 5-tap Gaussian blur, sigma <= 0.1, moves no pixel by 1e-21 of the image's range: not computed.)
//
// One workgroup of 256 threads per image.  An image that is jittered or rotated goes through LDS: the window is loaded
// (thread i owns pixels i, i + 256, ...), the mean is summed in a FIXED order -- each thread its own pixels in rising
// order, a butterfly over the wave's 64 lanes, then the four waves' sums left to right -- the thread rewrites its own
// pixels, and after one barrier the rotated gather reads LDS.  No atomics, no workspace: the output is a pure function of
// the arguments.  An image with neither reads global memory directly.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aug_gauss.h"
#include "gemm_f32.h"

namespace igi {

constexpr int TAC_MAX_PIXELS = 8192;   // the LDS window: 32 KB
constexpr int TAC_PARAM_WORDS = 6;     // per image: top, left, jitter flag, bits of b, c, angle (radians)

struct TactileAugArgs {
  const float* src;              // arena [N][planes][Hs][Ws], planes = T * F
  float* dst;                    // [B][planes][out_h][out_w]
  const long long* rows;         // [B] sample numbers; outside [0, N): the frames read as zeros
  const int* params;             // [B*planes][TAC_PARAM_WORDS]
  const unsigned char* keep;     // [B*planes][gh][gw] or null
  long long N;
  int planes, Hs, Ws, out_h, out_w, patch, gh, gw;
  int qpr;                       // groups of four per output row
  int vec;                       // 1: 16-byte stores (out_w % 4 == 0, the output 16-byte aligned)
  float noise_std;
  unsigned long long seed;
};

// grid (images = B * planes)
__global__ __launch_bounds__(256) void k_tactile_augment(const TactileAugArgs a) {
  __shared__ float win[TAC_MAX_PIXELS];
  __shared__ float wave_sum[4];
  const long long image = blockIdx.x;                  // b * planes + plane
  const long long b = image / a.planes;
  const int plane = (int)(image - b * a.planes);
  const int W = a.out_w, H = a.out_h, P = H * W;
  const int tid = (int)threadIdx.x;
  // per-image parameters: uniform over the workgroup
  const int* __restrict__ prm = a.params + image * TAC_PARAM_WORDS;
  const long long top = prm[0], left = prm[1];
  const bool jit = prm[2] != 0;
  const float jb = __int_as_float(prm[3]), jc = __int_as_float(prm[4]), ang = __int_as_float(prm[5]);
  const bool rot = ang != 0.f;
  const long long row = a.rows[b];
  const bool live = row >= 0 && row < a.N;
  const float* __restrict__ src = a.src + (live ? row * a.planes + plane : 0) * ((long long)a.Hs * a.Ws);
  const long long e0 = image * (long long)P;
  float* __restrict__ dst = a.dst + e0;
  const unsigned char* __restrict__ keep = a.keep ? a.keep + image * ((long long)a.gh * a.gw) : nullptr;
  const int mh = a.gh * a.patch, mw = a.gw * a.patch;  // the masked region (whole patches)
  const bool staged = jit || rot;

  if (staged) {
    float part = 0.f;
    for (int p = tid; p < P; p += 256) {
      const int y = p / W, x = p - y * W;
      const long long sy = y + top, sx = x + left;     // position in the stored frame
      const bool in = live && sy >= 0 && sy < a.Hs && sx >= 0 && sx < a.Ws;
      float v = in ? src[sy * a.Ws + sx] : 0.f;
      if (jit) {
        v = fminf(fmaxf(v * jb, 0.f), 1.f);
        part = part + v;
      }
      win[p] = v;
    }
    if (jit) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) part = part + __shfl_xor(part, o, 64);
      if ((tid & 63) == 0) wave_sum[tid >> 6] = part;
      __syncthreads();
      const float m = (((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3]) / (float)P;
      for (int p = tid; p < P; p += 256) win[p] = fminf(fmaxf((win[p] - m) * jc + m, 0.f), 1.f);   // the thread's own pixels
    }
    __syncthreads();
  }

  float sn = 0.f, cs = 1.f;
  if (rot) sincosf(ang, &sn, &cs);
  const float hx = 0.5f * (float)W - 0.5f, hy = 0.5f * (float)H - 0.5f;   // W/2 - 1/2: exact
  const int nq = H * a.qpr;
  for (int q = tid; q < nq; q += 256) {
    const int y = q / a.qpr, x0 = (q - y * a.qpr) * 4;
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      v[j] = 0.f;
      if (x >= W) continue;
      float p;
      if (staged) {
        int wx = x, wy = y;                            // position in the cropped window
        bool in = true;
        if (rot) {
          const float xc = (float)x - hx, yc = (float)y - hy;
          const float fx = rintf((cs * xc - sn * yc) + hx), fy = rintf((sn * xc + cs * yc) + hy);
          in = fx >= 0.f && fx < (float)W && fy >= 0.f && fy < (float)H;   // false for a NaN angle too
          wx = in ? (int)fx : 0;
          wy = in ? (int)fy : 0;
        }
        p = in ? win[wy * W + wx] : 0.f;
      } else {
        const long long sy = y + top, sx = x + left;
        const bool in = live && sy >= 0 && sy < a.Hs && sx >= 0 && sx < a.Ws;
        p = in ? src[sy * a.Ws + sx] : 0.f;
      }
      if (a.noise_std > 0.f)
        p = p + a.noise_std * aug_gauss(a.seed, 2u, (unsigned int)(e0 + (long long)y * W + x));
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

static int tactile_augment(const float* arena, int64_t n, int planes, int hs, int ws, const int64_t* rows, int64_t b,
                           const int32_t* params, const uint8_t* keep, int out_h, int out_w, int patch, float noise_std,
                           uint64_t seed, float* out, hipStream_t s) {
  if (!arena || !rows || !params || !out) return IGI_E_BADARG;
  if (n < 1 || planes < 1 || hs < 1 || ws < 1 || b < 1 || out_h < 1 || out_w < 1 || out_h > hs || out_w > ws) return IGI_E_BADARG;
  if (!(noise_std >= 0.f) || (keep && patch < 1)) return IGI_E_BADARG;
  if (b * planes > (1ll << 30)) return IGI_E_BADARG;                                  // grid.x
  if ((long long)out_h * out_w > TAC_MAX_PIXELS) return IGI_E_UNSUPPORTED;              // the LDS window
  TactileAugArgs a;
  a.src = arena; a.dst = out; a.rows = (const long long*)rows; a.params = params; a.keep = keep;
  a.N = n; a.planes = planes; a.Hs = hs; a.Ws = ws; a.out_h = out_h; a.out_w = out_w;
  a.patch = keep ? patch : 1;
  a.gh = keep ? out_h / patch : 0;
  a.gw = keep ? out_w / patch : 0;
  a.qpr = (out_w + 3) / 4;
  a.vec = (out_w % 4 == 0) && aligned16(out);
  a.noise_std = noise_std; a.seed = seed;
  hipLaunchKernelGGL(k_tactile_augment, dim3((unsigned)(b * planes)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
