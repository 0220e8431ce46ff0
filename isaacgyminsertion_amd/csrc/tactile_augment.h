// Train-time augmentation of the tactile images of the offline student, straight from the loader's resident arena
// (algo/models/transformer/utils.py: _Crop + _TrainAugment + GaussianNoise + Masking as called from data.py's loader):
//   k_tactile_augment : gather the minibatch's samples and run the whole chain -- ONE launch that reads the arena
//                       [N][T][F][Hs][Ws] and writes the batch tensor [B][T][F][out_h][out_w].
// An image is one (sample, t, finger) plane; every image has its own parameters (the reference transforms image by image)
// and goes through the chain of aug_pixel.h -- crop, rotate, noise on plane 2, mask with its own keep grid, store -- with
// one step of this kernel's own between the crop and the rotation, in the torch path's order:
//   jitter   flag on: x = clamp(x*b, 0, 1); m = mean of the image; x = clamp((x - m)*c + m, 0, 1) -- _TrainAugment's
//            arithmetic and order.  Flag off: the window passes bit for bit (no clamp)
// (_TrainAugment's 5-tap Gaussian blur, sigma <= 0.1, moves no pixel by 1e-21 of the image's range: not computed.)
//
// One workgroup of 256 threads per image.  An image that is jittered or rotated goes through LDS: the window is loaded
// (thread i owns pixels i, i + 256, ...), the mean is summed in a FIXED order -- each thread its own pixels in rising
// order, a butterfly over the wave's 64 lanes, then the four waves' sums left to right -- the thread rewrites its own
// pixels, and after one barrier the rotated gather reads LDS.  No atomics, no workspace: the output is a pure function of
// the arguments.  An image with neither reads global memory directly.  That per-image body is tac_image, which
// k_tactile_augment_seeded runs too (tactile_augment_seeded.h: the online student's step, every parameter hashed from one
// seed).
#pragma once
#include "aug_pixel.h"

namespace igi {

constexpr int TAC_MAX_PIXELS = 8192;   // the LDS window: 32 KB
constexpr int TAC_PARAM_WORDS = 6;     // per image: top, left, jitter flag, bits of b, c, angle (radians)

struct TactileAugArgs {
  AugShape c;                    // keep: [B*planes][gh][gw]
  const float* src;              // arena [N][planes][Hs][Ws], planes = T * F
  float* dst;                    // [B][planes][out_h][out_w]
  const int* params;             // [B*planes][TAC_PARAM_WORDS]
  int planes;
};

// One image by the whole workgroup: the window at (top, left) of the stored plane `src` -> jitter -> rotation -> noise ->
// keep_of (where `masked`) -> output plane number `image`.  `win` is the workgroup's LDS window of TAC_MAX_PIXELS floats,
// `wave_sum` its four floats.  Every argument but the thread's number is uniform over the workgroup.
template <class Keep>
__device__ __forceinline__ void tac_image(const AugShape& c, const float* __restrict__ src, bool live, float* __restrict__ dst,
                                          long long image, long long top, long long left, bool jit, float jb, float jc,
                                          float ang, bool masked, float* __restrict__ win, float* __restrict__ wave_sum,
                                          Keep keep_of) {
  const int W = c.out_w, H = c.out_h, P = H * W;
  const int tid = (int)threadIdx.x;
  const AugRot r = aug_rot(ang, W, H);
  const int nq = H * c.qpr;

  if (!jit && !r.on) {                                 // the window of the stored frame, as it is
    aug_rows_keep(c, dst, image, masked, TAC_NOISE_PLANE, tid, nq,
                  [&](int x, int y) { return aug_frame_read(src, c, live, y + top, x + left); }, keep_of);
    return;
  }
  float part = 0.f;
  for (int p = tid; p < P; p += 256) {
    const int y = p / W, x = p - y * W;
    float v = aug_frame_read(src, c, live, y + top, x + left);
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
  aug_rows_keep(c, dst, image, masked, TAC_NOISE_PLANE, tid, nq, [&](int x, int y) {
    int wx, wy;
    return aug_window_pos(r, W, H, x, y, wx, wy) ? win[wy * W + wx] : 0.f;
  }, keep_of);
}

// grid (images = B * planes)
__global__ __launch_bounds__(256) void k_tactile_augment(const TactileAugArgs a) {
  __shared__ float win[TAC_MAX_PIXELS];
  __shared__ float wave_sum[4];
  const AugShape& c = a.c;
  const long long image = blockIdx.x;                  // b * planes + plane
  const long long b = image / a.planes;
  const int plane = (int)(image - b * a.planes);
  // per-image parameters: uniform over the workgroup
  const int* __restrict__ prm = a.params + image * TAC_PARAM_WORDS;
  const long long row = c.rows[b];
  const bool live = row >= 0 && row < c.N;
  const float* __restrict__ src = a.src + (live ? row * a.planes + plane : 0) * ((long long)c.Hs * c.Ws);
  const unsigned char* __restrict__ keep = c.keep ? c.keep + image * ((long long)c.gh * c.gw) : nullptr;
  tac_image(c, src, live, a.dst, image, prm[0], prm[1], prm[2] != 0, __int_as_float(prm[3]), __int_as_float(prm[4]),
            __int_as_float(prm[5]), keep != nullptr, win, wave_sum, [&](int cell) { return (float)keep[cell]; });
}

static int tactile_augment(const float* arena, int64_t n, int planes, int hs, int ws, const int64_t* rows, int64_t b,
                           const int32_t* params, const uint8_t* keep, int out_h, int out_w, int patch, float noise_std,
                           uint64_t seed, float* out, hipStream_t s) {
  if (!arena || !params || !out) return IGI_E_BADARG;
  TactileAugArgs a;
  if (int rc = aug_shape(a.c, n, planes, hs, ws, rows, b, keep, out_h, out_w, patch, noise_std, seed, aligned16(out)))
    return rc;
  if ((long long)out_h * out_w > TAC_MAX_PIXELS) return IGI_E_UNSUPPORTED;              // the LDS window
  a.src = arena; a.dst = out; a.params = params; a.planes = planes;
  hipLaunchKernelGGL(k_tactile_augment, dim3((unsigned)(b * planes)), dim3(256), 0, s, a);
  return (int)hipGetLastError();
}

}  // namespace igi
