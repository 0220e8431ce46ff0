// The token encoder's arithmetic, each formula once: dropout, LayerNorm forward / backward of a row's elements (rows of
// 32, 64 or 128 features), erf GELU and its derivative, the register attention of one (sample, head) pair (S <= 8, heads
// of 16) and the 32 x 32 k-contiguous MFMA tile product.  The routines compute on registers only: the launch-per-operation kernels and the one-launch kernels of
// token_encoder.h load the operands from global memory or LDS, call them, and store the results, so the two paths cannot
// drift apart (the library builds with -ffp-contract=off: one expression, one rounding, wherever it is inlined).
#pragma once
#include <hip/hip_runtime.h>

#include "linear.h"
#include "tok_hash.h"

namespace igi {

constexpr int TOK_D = 32, TOK_DH = 16;   // the width and head width of the one-launch and register attention kernels
constexpr float TOK_LN_EPS = 1e-5f;

// ---- dropout: keep iff tok_hash(seed, site, index) >= p * 2^32 (tok_hash.h); kept values are scaled by 1/(1-p)
struct Drop {
  unsigned long long seed;
  unsigned int site, thresh;  // thresh = 0: no dropout
  float scale;
};
__host__ __device__ __forceinline__ Drop make_drop(float p, unsigned long long seed, unsigned int site) {
  Drop d;
  d.seed = seed; d.site = site;
  d.thresh = p > 0.f ? (unsigned int)((double)p * 4294967296.0) : 0u;
  d.scale = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
  return d;
}
__device__ __forceinline__ float drop_apply(const Drop& d, unsigned int idx, float v) {
  if (d.thresh == 0u) return v;
  return tok_hash(d.seed, d.site, idx) >= d.thresh ? v * d.scale : 0.f;
}

__device__ __forceinline__ float row16_sum(float v) {  // sum over the 16-lane DPP row, in every lane
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}
__device__ __forceinline__ float half32_sum(float v) {  // sum over 32 consecutive lanes
  v = row16_sum(v);
  return v + __shfl_xor(v, 16, 64);
}

// ---- LayerNorm over a row of D features (32, 64 or 128).  D = 32: a half wave owns the row, lane = feature.  D = 64 / 128:
// a whole wave owns the row and a lane holds the D / 64 features lane, lane + 64 (loads stay coalesced).  A row sum is
// the lane's own features in order, the DPP row sum, then the exchanges across the 16-lane rows: one fixed order.
template <int D> struct LnShape {
  static_assert(D == 32 || D == 64 || D == 128, "LayerNorm rows of 32, 64 or 128 features");
  static constexpr int LANES = D == 32 ? 32 : 64;   // lanes that own a row
  static constexpr int NV = D / LANES;              // features per lane: f = lane + LANES * u
};
template <int D>
__device__ __forceinline__ float ln_row_sum(float v) {   // sum over the lanes that own a row, in every one of them
  v = half32_sum(v);
  if constexpr (D > 32) v += __shfl_xor(v, 32, 64);
  return v;
}
// Forward: the normalised elements of v with their features' gamma / beta; mean and rstd of the row come back in every lane.
template <int D>
__device__ __forceinline__ void ln_fwd(const float (&v)[LnShape<D>::NV], const float (&gamma)[LnShape<D>::NV],
                                       const float (&beta)[LnShape<D>::NV], float (&o)[LnShape<D>::NV], float& mean,
                                       float& rstd) {
  constexpr int NV = LnShape<D>::NV;
  float s = v[0];
#pragma unroll
  for (int u = 1; u < NV; ++u) s += v[u];
  mean = ln_row_sum<D>(s) * (1.0f / D);
  float c[NV];
  c[0] = v[0] - mean;
  float q = c[0] * c[0];
#pragma unroll
  for (int u = 1; u < NV; ++u) { c[u] = v[u] - mean; q += c[u] * c[u]; }
  const float var = ln_row_sum<D>(q) * (1.0f / D);
  rstd = 1.0f / sqrtf(var + TOK_LN_EPS);
#pragma unroll
  for (int u = 0; u < NV; ++u) o[u] = c[u] * rstd * gamma[u] + beta[u];
}
// Backward + residual: dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dxn * gamma; the features' terms of
// the LayerNorm weight / bias gradients (dxn * xhat, dxn) are added to sg / sb.
template <int D>
__device__ __forceinline__ void ln_bwd(const float (&dxn)[LnShape<D>::NV], const float (&x)[LnShape<D>::NV], float mean,
                                       float rstd, const float (&gamma)[LnShape<D>::NV],
                                       const float (&dres)[LnShape<D>::NV], float (&dx)[LnShape<D>::NV],
                                       float (&sg)[LnShape<D>::NV], float (&sb)[LnShape<D>::NV]) {
  constexpr int NV = LnShape<D>::NV;
  float xhat[NV], g[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    xhat[u] = (x[u] - mean) * rstd;
    sg[u] += dxn[u] * xhat[u];
    sb[u] += dxn[u];
    g[u] = dxn[u] * gamma[u];
  }
  float s1 = g[0], s2 = g[0] * xhat[0];
#pragma unroll
  for (int u = 1; u < NV; ++u) { s1 += g[u]; s2 += g[u] * xhat[u]; }
  const float m1 = ln_row_sum<D>(s1) * (1.0f / D);
  const float m2 = ln_row_sum<D>(s2) * (1.0f / D);
#pragma unroll
  for (int u = 0; u < NV; ++u) dx[u] = dres[u] + rstd * (g[u] - m1 - xhat[u] * m2);
}
// the 32-wide row of the one-launch kernels, one feature per lane: the same routines on one-element arrays
__device__ __forceinline__ float ln_fwd(float v, float gamma, float beta, float& mean, float& rstd) {
  const float vv[1] = {v}, gm[1] = {gamma}, bt[1] = {beta};
  float o[1];
  ln_fwd<TOK_D>(vv, gm, bt, o, mean, rstd);
  return o[0];
}
__device__ __forceinline__ float ln_bwd(float dxn, float x, float mean, float rstd, float gamma, float dres, float& sg,
                                        float& sb) {
  const float dn[1] = {dxn}, xx[1] = {x}, gm[1] = {gamma}, dr[1] = {dres};
  float o[1], g1[1] = {sg}, b1[1] = {sb};
  ln_bwd<TOK_D>(dn, xx, mean, rstd, gm, dr, o, g1, b1);
  sg = g1[0]; sb = b1[0];
  return o[0];
}

// ---- exact (erf) GELU (nn.GELU default / activation="gelu") and its derivative
__device__ __forceinline__ float gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad(float x) {
  const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752f));
  const float pdf = 0.39894228040143268f * __expf(-0.5f * x * x);
  return cdf + x * pdf;
}

// ---- register attention of one (sample, head) pair, S <= 8 tokens: 16 lanes per pair, lane = head dimension, so
// q / k / v / dc hold one column of the pair's S rows and dot products over the head dimension are 16-lane DPP row sums.
// g is the global pair index b * H + h: the dropout element of probability (i, j) is (g * S + i) * S + j.
constexpr float TOK_ATTN_SCALE = 0.25f;  // 1 / sqrt(16)

// softmax row i, unnormalised: e[j] = exp(q_i . k_j / 4 - max_j); returns 1 / sum_j e[j]
template <int S>
__device__ __forceinline__ float attn_softmax_row(const float (&q)[S], const float (&k)[S], int i, float (&e)[S]) {
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < S; ++j) { e[j] = row16_sum(q[i] * k[j]) * TOK_ATTN_SCALE; mx = fmaxf(mx, e[j]); }
  float den = 0.f;
#pragma unroll
  for (int j = 0; j < S; ++j) { e[j] = __expf(e[j] - mx); den += e[j]; }
  return 1.0f / den;
}

// forward: this lane's column of context row i = sum_j drop(P_ij) v_j
template <int S>
__device__ __forceinline__ float attn_ctx_row(const float (&q)[S], const float (&k)[S], const float (&v)[S], int i,
                                              const Drop& dr, long long g) {
  float e[S];
  const float inv = attn_softmax_row<S>(q, k, i, e);
  float o = 0.f;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    const float pij = drop_apply(dr, (unsigned int)((g * S + i) * S + j), e[j] * inv);
    o += pij * v[j];
  }
  return o;
}

// backward: dq, dk, dv (this lane's column of the S rows) from dc = d(loss)/d(context); the probabilities are recomputed
template <int S>
__device__ __forceinline__ void attn_bwd(const float (&q)[S], const float (&k)[S], const float (&v)[S], const float (&dc)[S],
                                         const Drop& dr, long long g, float (&dq)[S], float (&dk)[S], float (&dv)[S]) {
#pragma unroll
  for (int s = 0; s < S; ++s) { dq[s] = 0.f; dk[s] = 0.f; dv[s] = 0.f; }
#pragma unroll
  for (int i = 0; i < S; ++i) {
    float pr[S], dp[S], dot = 0.f;
    const float inv = attn_softmax_row<S>(q, k, i, pr);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      pr[j] *= inv;
      // the mask factor m_ij in {0, 1/(1-p)}: P_drop = P * m
      const float m = drop_apply(dr, (unsigned int)((g * S + i) * S + j), 1.0f);
      dv[j] += pr[j] * m * dc[i];
      dp[j] = row16_sum(dc[i] * v[j]) * m;     // d(loss)/dP_ij
      dot += dp[j] * pr[j];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const float ds = pr[j] * (dp[j] - dot) * TOK_ATTN_SCALE;  // d(loss)/d(score_ij) incl. the 1/sqrt(dh)
      dq[i] += ds * k[j];
      dk[j] += ds * q[i];
    }
  }
}

// ---- acc += A[32][K] . W[32][K]^T on v_mfma_f32_32x32x2_f32 in the LDS-DMA GEMM kernel's k order (k = 8 c + 4 half + j at
// step j of chunk c).  ap / bp: this lane's row (lane & 31) of the two k-contiguous LDS images, + 4 * half (half = lane >> 5).
__device__ __forceinline__ void tile32_kdot(const float* ap, const float* bp, int K, f32x16& acc) {
  for (int c = 0; c < K; c += 8) {
    const f32x4 av = *reinterpret_cast<const f32x4*>(ap + c);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bp + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
  }
}

}  // namespace igi
