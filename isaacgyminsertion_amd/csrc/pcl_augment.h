// Train-time augmentation of the online student's segmented point cloud (envs/pcl_augment.py: PclAugment; the reference's
// PointCloudAugmentations.augment, factory_utils.py:83-166, which its environment runs object by object on a boolean-masked
// subset of the envs):
//   k_pcl_augment : the environment's cloud tensor [N][P_total][3] -> a new tensor of the same shape, ONE launch.  The input
//                   is never written.
// P_total is the sum of 1..4 consecutive objects of points[o] points (the layout of pointnet_max_fwd_multi).  One workgroup
// of 256 threads per (env, object) cloud.  Env e is augmented in this call iff its hit draw says so (one draw per env,
// shared by its objects); a missed env is copied bit for bit.  A hit cloud runs the stages of `augment` in its order:
//   a  noise     per point a mask draw; per coordinate j = clamp(sigma z, +-clip); x = x + (mask ? j : 0), then
//                x = x + clamp(const_noise pn[c], +-clip), pn the env's per-episode offset.  z is evaluated only where the
//                mask is set (the same function)
//   b  rotation  (rot_deg > 0) row vector times the axis matrix of PointCloudAugmentations.random_rotate, about the origin;
//                angle = ((2u - 1) rot_deg) degrees, axis in {0, 1, 2}: per-episode
//   c  outliers  (K = int(points[o] * outlier_ratio) > 0, from the host) lo / hi = the cloud's bounding box after a and b;
//                outlier k < K replaces point ((h >> 8) * points[o]) >> 24 by, per coordinate, outlier_scale z (free) or
//                hi + |z| / lo - |z| (contour, the side drawn per coordinate).  Where two outliers pick one point the
//                higher k wins: no atomics -- the K indices sit in LDS and every point scans them, then evaluates its own
//                winner
//   d  dropout   (dropout_ratio > 0) unless the cloud's exempt draw says otherwise, a point becomes 0 iff its drop draw
//                says so -- replaced points too
// With b and c both off a cloud needs no LDS and no barrier (k_pcl_augment<false>: thread i owns elements i, i + 256, ...,
// coalesced).  Otherwise (k_pcl_augment<true>) stage a writes the cloud to LDS element by element, one thread per POINT
// rotates it in place and takes the bounding box (wave butterfly, then the four waves' values: min / max do not depend on
// order), and the store pass is element by element again: two barriers.
//
// Draws (the numbers of the planes and sites, and thr / u / the index draw: draws.h).  Every Bernoulli event is the integer
// comparison  tok_hash(...) < thr(p),  thr(p) = draw_threshold(p): fp32 and float64 restatements agree on every event.
// Per-step draws hash `seed_step`; per-episode draws hash  se = seed_episode + (episode[env] << 32)  (the
// episode number enters the hash's high word), so they are a pure function of (seed_episode, env, episode[env]).
// g = env * P_total + p is a point's number (p counted over the env's objects), g * 3 + c a coordinate's; outlier k of
// object o uses the numbers of point off[o] + k.  Refused: N * P_total * 3 >= 2^32.
//
//   site / plane   seed   element        draw
//   plane 3 (6,7)  se     env * 3 + c    pn[c], the per-episode offset
//   plane 4 (8,9)  step   g * 3 + c      jitter z
//   plane 5 (10,11) step  g * 3 + c      free outlier z
//   plane 6 (12,13) step  g * 3 + c      contour outlier |z|
//   site 14        step   env            hit
//   site 15        se     env            angle u = (h >> 8) 2^-24
//   site 16        se     env            axis = ((h >> 8) * 3) >> 24
//   site 17        step   g              noise mask
//   site 18        step   g              contour flag
//   site 19        step   g * 3 + c      contour side (hi if h < thr(0.5))
//   site 20        step   g              replaced index
//   site 21        step   env * 4 + o    cloud exempt from dropout (h >= thr(1 - no_dropout_prob))
//   site 22        step   g              drop
// tests/pcl_augment_ref.py restates all of it in float64.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aug_gauss.h"
#include "gemm_f32.h"

namespace igi {

constexpr int PCL_MAX_POINTS = 4096;   // per object: the LDS cloud is 48 KB, the index list 8 KB
constexpr int PCL_MAX_OBJECTS = 4;
constexpr int PCL_RED_FLOATS = 32;     // 4 waves x (lo[3], hi[3]), padded

struct PclAugArgs {
  const float* src;              // [N][P_total][3]
  float* dst;                    // [N][P_total][3]
  const int* episode;            // [N]
  int nobj, p_total;
  int off[PCL_MAX_OBJECTS], pts[PCL_MAX_OBJECTS], k[PCL_MAX_OBJECTS];
  float sigma, clip, const_noise, rot_deg, outlier_scale;
  int rot_on, drop_on;
  unsigned long long thr_hit, thr_mask, thr_contour, thr_side, thr_drop, thr_exempt;
  unsigned long long seed_episode, seed_step;
};

__device__ __forceinline__ int pcl_pick(const int (&v)[PCL_MAX_OBJECTS], int o) {
  return o == 0 ? v[0] : o == 1 ? v[1] : o == 2 ? v[2] : v[3];
}

__device__ __forceinline__ float pcl_clamp(float v, float c) { return fminf(fmaxf(v, -c), c); }

// Stage a of coordinate c of point number g: its value after the jitter and the env's offset.
__device__ __forceinline__ float pcl_noise(const PclAugArgs& a, float x, unsigned int g, int c, float offc) {
  float j = 0.f;
  if (a.sigma > 0.f && tok_hash(a.seed_step, PCL_SITE_MASK, g) < a.thr_mask)
    j = pcl_clamp(a.sigma * aug_gauss(a.seed_step, PCL_PLANE_JITTER, g * 3u + (unsigned int)c), a.clip);
  x = x + j;
  return x + offc;
}

// grid (N * nobj), block 256, dynamic LDS pcl_lds_bytes() for STAGED
template <bool STAGED>
__global__ __launch_bounds__(256) void k_pcl_augment(const PclAugArgs a) {
  extern __shared__ float pcl_lds[];
  const int tid = (int)threadIdx.x;
  const unsigned int env = blockIdx.x / (unsigned int)a.nobj;
  const int o = (int)(blockIdx.x - env * (unsigned int)a.nobj);
  const int off = pcl_pick(a.off, o), P = pcl_pick(a.pts, o), E = 3 * P;
  const unsigned int g0 = env * (unsigned int)a.p_total + (unsigned int)off;   // the cloud's first point number
  const long long base = (long long)g0 * 3;
  const float* __restrict__ src = a.src + base;
  float* __restrict__ dst = a.dst + base;

  if (!(tok_hash(a.seed_step, PCL_SITE_HIT, env) < a.thr_hit)) {               // missed: the cloud as it is
    for (int i = tid; i < E; i += 256) dst[i] = src[i];
    return;
  }
  // per-episode parameters: uniform over the env's workgroups
  const unsigned long long se = a.seed_episode + ((unsigned long long)(unsigned int)a.episode[env] << 32);
  float offc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    offc[c] = pcl_clamp(a.const_noise * aug_gauss(se, PCL_PLANE_PN, env * 3u + (unsigned int)c), a.clip);
  const bool drop = a.drop_on && tok_hash(a.seed_step, PCL_SITE_EXEMPT, env * 4u + (unsigned int)o) < a.thr_exempt;

  if constexpr (!STAGED) {
    for (int i = tid; i < E; i += 256) {
      const int p = i / 3, c = i - 3 * p;
      const unsigned int g = g0 + (unsigned int)p;
      float v = pcl_noise(a, src[i], g, c, c == 0 ? offc[0] : c == 1 ? offc[1] : offc[2]);
      if (drop && tok_hash(a.seed_step, PCL_SITE_DROP, g) < a.thr_drop) v = 0.f;
      dst[i] = v;
    }
  } else {
    float* __restrict__ red = pcl_lds;                             // [4][6]
    float* __restrict__ pts = pcl_lds + PCL_RED_FLOATS;            // [P][3]
    unsigned short* __restrict__ idx = reinterpret_cast<unsigned short*>(pts + E);   // [K]
    const int K = pcl_pick(a.k, o);
    for (int i = tid; i < E; i += 256) {
      const int p = i / 3, c = i - 3 * p;
      pts[i] = pcl_noise(a, src[i], g0 + (unsigned int)p, c, c == 0 ? offc[0] : c == 1 ? offc[1] : offc[2]);
    }
    for (int k = tid; k < K; k += 256)
      idx[k] = (unsigned short)draw_index(tok_hash(a.seed_step, PCL_SITE_INDEX, g0 + (unsigned int)k), (unsigned long long)P);
    __syncthreads();
    // one thread per point: rotate in place, take the bounding box
    float sn = 0.f, cs = 1.f;
    int axis = 0;
    if (a.rot_on) {
      const float deg = draw_unit(tok_hash(se, PCL_SITE_ANGLE, env)) * a.rot_deg;
      sincosf(deg * 0.017453292519943295f, &sn, &cs);
      axis = (int)draw_index(tok_hash(se, PCL_SITE_AXIS, env), 3);
    }
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int p = tid; p < P; p += 256) {
      float x = pts[3 * p], y = pts[3 * p + 1], z = pts[3 * p + 2];
      if (a.rot_on) {
        float nx = x, ny = y, nz = z;
        if (axis == 0) { ny = y * cs + z * sn; nz = z * cs - y * sn; }
        else if (axis == 1) { nx = x * cs - z * sn; nz = x * sn + z * cs; }
        else { nx = x * cs + y * sn; ny = y * cs - x * sn; }
        x = nx; y = ny; z = nz;
        pts[3 * p] = x; pts[3 * p + 1] = y; pts[3 * p + 2] = z;
      }
      lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
    }
    if (K > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
          lo[c] = fminf(lo[c], __shfl_xor(lo[c], s, 64));
          hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], s, 64));
        }
      }
      if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { red[(tid >> 6) * 6 + c] = lo[c]; red[(tid >> 6) * 6 + 3 + c] = hi[c]; }
      }
    }
    __syncthreads();
    for (int i = tid; i < E; i += 256) {
      const int p = i / 3, c = i - 3 * p;
      const unsigned int g = g0 + (unsigned int)p;
      float v = pts[i];
      int win = -1;
      for (int k = 0; k < K; ++k) win = (int)idx[k] == p ? k : win;            // the highest k wins
      if (win >= 0) {
        const unsigned int gk = g0 + (unsigned int)win, ek = gk * 3u + (unsigned int)c;
        if (tok_hash(a.seed_step, PCL_SITE_CONTOUR, gk) < a.thr_contour) {
          const float lc = fminf(fminf(red[c], red[6 + c]), fminf(red[12 + c], red[18 + c]));
          const float hc = fmaxf(fmaxf(red[3 + c], red[9 + c]), fmaxf(red[15 + c], red[21 + c]));
          const float beyond = fabsf(aug_gauss(a.seed_step, PCL_PLANE_CONTOUR, ek));
          v = tok_hash(a.seed_step, PCL_SITE_SIDE, ek) < a.thr_side ? hc + beyond : lc - beyond;
        } else {
          v = a.outlier_scale * aug_gauss(a.seed_step, PCL_PLANE_FREE, ek);
        }
      }
      if (drop && tok_hash(a.seed_step, PCL_SITE_DROP, g) < a.thr_drop) v = 0.f;
      dst[i] = v;
    }
  }
}

struct PclAugParams {            // igi_pcl_augment_params, field for field
  double sigma, noise_clip, const_noise, noise_prob, hit_prob, rot_deg, outlier_ratio, contour_prob, outlier_scale,
      dropout_ratio, no_dropout_prob;
};

static int pcl_augment(const float* clouds, int64_t n, int nobj, const int32_t* points, const int32_t* episode,
                       const PclAugParams& q, uint64_t seed_episode, uint64_t seed_step, float* out, hipStream_t s) {
  if (!clouds || !points || !episode || !out || n < 1 || nobj < 1 || nobj > PCL_MAX_OBJECTS || clouds == out)
    return IGI_E_BADARG;
  if (!draw_is_prob(q.noise_prob) || !draw_is_prob(q.hit_prob) || !draw_is_prob(q.contour_prob) ||
      !draw_is_prob(q.no_dropout_prob) || !draw_is_prob(q.outlier_ratio) || !draw_is_prob(q.dropout_ratio) ||
      !(q.sigma >= 0) || !(q.noise_clip >= 0) || !(q.rot_deg >= 0))
    return IGI_E_BADARG;
  PclAugArgs a{};
  long long total = 0;
  int max_pts = 0, max_k = 0;
  for (int o = 0; o < nobj; ++o) {
    if (points[o] < 1) return IGI_E_BADARG;
    if (points[o] > PCL_MAX_POINTS) return IGI_E_UNSUPPORTED;                   // the LDS cloud
    a.off[o] = (int)total; a.pts[o] = points[o];
    a.k[o] = (int)((double)points[o] * q.outlier_ratio);
    total += points[o];
    max_pts = points[o] > max_pts ? points[o] : max_pts;
    max_k = a.k[o] > max_k ? a.k[o] : max_k;
  }
  if ((long long)n * total * 3 >= (1ll << 32)) return IGI_E_BADARG;             // 32-bit element numbers
  a.src = clouds; a.dst = out; a.episode = episode; a.nobj = nobj; a.p_total = (int)total;
  a.sigma = (float)q.sigma; a.clip = (float)q.noise_clip; a.const_noise = (float)q.const_noise;
  a.rot_deg = (float)q.rot_deg; a.outlier_scale = (float)q.outlier_scale;
  a.rot_on = q.rot_deg > 0; a.drop_on = q.dropout_ratio > 0;
  a.thr_hit = draw_threshold(q.hit_prob); a.thr_mask = draw_threshold(q.noise_prob);
  a.thr_contour = draw_threshold(q.contour_prob); a.thr_side = draw_threshold(0.5);
  a.thr_drop = draw_threshold(q.dropout_ratio); a.thr_exempt = draw_threshold(1.0 - q.no_dropout_prob);
  a.seed_episode = seed_episode; a.seed_step = seed_step;
  const dim3 grid((unsigned)(n * nobj));
  if (!a.rot_on && max_k == 0) {
    hipLaunchKernelGGL(k_pcl_augment<false>, grid, dim3(256), 0, s, a);
  } else {
    const size_t lds = (size_t)(PCL_RED_FLOATS + 3 * max_pts) * sizeof(float) + (size_t)max_k * sizeof(unsigned short);
    hipLaunchKernelGGL(k_pcl_augment<true>, grid, dim3(256), lds, s, a);
  }
  return (int)hipGetLastError();
}

}  // namespace igi
