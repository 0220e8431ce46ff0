// Token decoder of the student: a stack of nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward,
// activation="gelu", batch_first=True, norm_first=True) over S <= 32 tokens
// (algo/models/transformer/tact.py:137-158), forward and backward.  d_model is 32, 64 or 128 with heads of 16, 32 or 64
// features; (32, 2, 128) is the reference's stock config and the only one the register attention and the one-launch
// kernels below are built for (TokenPlan::narrow).  Every other pair runs launch per operation with the LayerNorm
// kernels' <64> / <128> instantiations and the tile attention kernels at every S.
//
//   per layer:  x1 = x  + drop(out_proj(attn(in_proj(LN1(x)))))          (sa block,  norm_first)
//               x2 = x1 + drop(linear2(drop(gelu(linear1(LN2(x1))))))    (ff block)
//
// Rows are tokens, sample-major (row = b * S + s); every Linear is a row-wise product and runs on the
// MFMA GEMMs (linear.h: igi_linear_forward / backward with deterministic split sums for the weight
// gradients); everything else is a handful of small fused kernels around the routines of token_math.h:
//   k_resid_ln_fwd<D> : residual add (+ dropout of the branch) fused with the NEXT LayerNorm (ln_fwd); a 32-lane
//                    half wave owns a row of 32 features (lane = feature), a wave a row of 64 / 128 (D / 64 features per
//                    lane), statistics by DPP row sums and cross-row exchanges
//   k_attn_fwd/bwd : softmax(q k^T / sqrt(16)) v for an S x S block per (sample, head) (attn_ctx_row / attn_bwd);
//                    16 lanes own a (sample, head) pair, lane = head dimension; backward recomputes the
//                    probabilities (nothing S x S is ever stored); S <= 8, (32, 2) only
//   k_attn_tile_fwd/bwd<DH, DM> : the same with heads of DH features in a DM-wide model: a wave owns a (sample, head) pair,
//                    the S x S block is one padded 32 x 32 tile of v_mfma_f32_32x32x2_f32, S a runtime argument;
//                    <16, 32> at 9 <= S <= 32, the others at every S
//   k_gelu_fwd/bwd : exact (erf) GELU + dropout (gelu / gelu_grad)
//   k_ln_bwd<D>    : LayerNorm backward + residual gradient add (ln_bwd) + (optionally) the dropout mask of the
//                    branch below it; per-block partial sums for the LayerNorm weight / bias gradients,
//                    reduced in fixed order
// The one-launch kernels further down (k_token_fwd<S>, k_token_fwd_long, k_token_bwd<S>) carry whole samples through
// every layer in LDS and call the SAME routines: a kernel of either path only decides where operands are loaded from
// and where results go (one exception, for registers: step 7 of k_token_bwd).
// Dropout masks are a counter-based hash of (seed, site, element): backward regenerates them, nothing is stored.
// Parameter vector per layer, in nn.TransformerEncoderLayer's registration order:
//   in_proj_weight [3d][d], in_proj_bias [3d], out_proj.weight [d][d], out_proj.bias [d],
//   linear1.weight [ff][d], linear1.bias [ff], linear2.weight [d][ff], linear2.bias [d],
//   norm1.weight [d], norm1.bias [d], norm2.weight [d], norm2.bias [d]
#pragma once
#include <hip/hip_runtime.h>

#include "linear.h"
#include "prof.h"
#include "token_math.h"

namespace igi {

constexpr int TOK_MAX_S = 8;     // tokens per sample of the register attention kernels (k_attn_fwd<S>, k_token_fwd<S>)
constexpr int TOK_MAX_SEQ = 32;  // tokens per sample of the tile attention kernels (k_attn_tile_*, k_token_fwd_long)

// float offsets of a layer's parameters and saved activations: filled once by make_token_plan, handed whole to the kernels
struct TokLayout {
  long long per_layer;   // parameters per layer
  long long o_inw, o_inb, o_ow, o_ob, o_w1, o_b1, o_w2, o_b2, o_n1w, o_n1b, o_n2w, o_n2b;
  // saved activations per layer (inside a layer's slab of a_layer floats)
  long long a_x, a_st1, a_xn1, a_qkv, a_ctx, a_x1, a_st2, a_xn2, a_z, a_h, a_layer;
};
struct TokenPlan {
  int B, S, d, H, ff, L;
  int dh;                // head width d / H
  bool narrow;           // (d, H) = (32, 2): the configuration of the register attention and the one-launch kernels
  long long R;           // token rows
  float p;               // dropout probability (0 when not training)
  TokLayout lay;
  // backward scratch (float offsets after the L slabs)
  long long s_g0, s_g1, s_rA, s_rB, s_wide0, s_wide1, s_lnpart, s_lin;
  size_t lin_bytes, total_bytes;
  int ln_blocks;
  long long s_part; int bwd_samples, bwd_grid;   // fused backward (k_token_bwd)
};
constexpr int TB_ROWS = 64;                     // token rows per workgroup of the fused backward

static inline long long ru4ll(long long x) { return (x + 3) & ~3LL; }

// d_model 32, 64 or 128 with heads of 16, 32 or 64
static inline bool token_width_supported(int d, int nhead) {
  if ((d != 32 && d != 64 && d != 128) || nhead < 1 || d % nhead) return false;
  const int dh = d / nhead;
  return dh == 16 || dh == 32 || dh == 64;
}

static int make_token_plan(const igi_token_cfg* c, TokenPlan* p) {
  if (!c || c->batch < 1 || c->seq < 1 || c->layers < 1 || c->ff < 4 || c->dropout < 0.f || c->dropout >= 1.f)
    return IGI_E_BADARG;
  if (!token_width_supported(c->d_model, c->nhead) || c->seq > TOK_MAX_SEQ || (c->ff & 3) || c->layers > 8)
    return IGI_E_UNSUPPORTED;
  p->B = c->batch; p->S = c->seq; p->d = c->d_model; p->H = c->nhead; p->ff = c->ff; p->L = c->layers;
  p->dh = p->d / p->H;
  p->narrow = p->d == TOK_D && p->dh == TOK_DH;
  p->R = (long long)c->batch * c->seq;
  if (p->R > (1LL << 26)) return IGI_E_UNSUPPORTED;
  p->p = c->training ? c->dropout : 0.f;
  const int d = p->d, ff = p->ff;
  TokLayout& ly = p->lay;
  long long o = 0;
  ly.o_inw = o; o += 3LL * d * d;
  ly.o_inb = o; o += 3 * d;
  ly.o_ow = o; o += (long long)d * d;
  ly.o_ob = o; o += d;
  ly.o_w1 = o; o += (long long)ff * d;
  ly.o_b1 = o; o += ff;
  ly.o_w2 = o; o += (long long)d * ff;
  ly.o_b2 = o; o += d;
  ly.o_n1w = o; o += d;
  ly.o_n1b = o; o += d;
  ly.o_n2w = o; o += d;
  ly.o_n2b = o; o += d;
  ly.per_layer = o;
  const long long R = p->R;
  long long a = 0;
  auto take = [&](long long n) { long long r = a; a += ru4ll(n); return r; };
  ly.a_x = take(R * d); ly.a_st1 = take(R * 2); ly.a_xn1 = take(R * d); ly.a_qkv = take(R * 3 * d);
  ly.a_ctx = take(R * d); ly.a_x1 = take(R * d); ly.a_st2 = take(R * 2); ly.a_xn2 = take(R * d);
  ly.a_z = take(R * ff); ly.a_h = take(R * ff);
  ly.a_layer = a;
  long long s = a * p->L;
  auto stake = [&](long long n) { long long r = s; s += ru4ll(n); return r; };
  p->ln_blocks = (int)((R + 63) / 64 < 256 ? (R + 63) / 64 : 256);
  p->s_g0 = stake(R * d); p->s_g1 = stake(R * d); p->s_rA = stake(R * d); p->s_rB = stake(R * d);
  const int wide = 3 * d > ff ? 3 * d : ff;
  p->s_wide0 = stake(R * wide); p->s_wide1 = stake(R * wide);
  p->s_lnpart = stake((long long)p->ln_blocks * 2 * d * 2 * p->L);   // one per layer norm: the sums are deferred
  p->bwd_samples = (int)(TB_ROWS / p->S);           // fused backward: samples per workgroup (see k_token_bwd)
  if ((long long)p->bwd_samples * 256 > p->B) p->bwd_samples = (int)(p->B / 256 > 1 ? p->B / 256 : 1);
  p->bwd_grid = (int)((p->B + p->bwd_samples - 1) / p->bwd_samples);
  // one 100 KB gradient record per workgroup: beyond 1024 of them (>= 21 K samples of three tokens) the backward runs
  // launch by launch on split-row slabs instead, and no record space is reserved
  if (p->bwd_grid > 1024 || p->S > TOK_MAX_S || !p->narrow) p->bwd_grid = 0;   // (S > 8, or not (32, 2): no one-launch backward either)
  p->s_part = stake((long long)p->bwd_grid * ly.per_layer * p->L);   // one gradient record per workgroup
  p->s_lin = stake(0);
  size_t lb = linear_workspace_bytes(R, d, 3 * d);
  const size_t c1 = linear_workspace_bytes(R, d, d), c2 = linear_workspace_bytes(R, d, ff),
               c3 = linear_workspace_bytes(R, ff, d);
  if (c1 > lb) lb = c1;
  if (c2 > lb) lb = c2;
  if (c3 > lb) lb = c3;
  p->lin_bytes = lb;
  p->total_bytes = sizeof(float) * (size_t)s + lb * 4 * (size_t)p->L + 64;   // one Linear workspace per call (deferred sums)
  return 0;
}

// x_out = x_prev + drop(delta)  (delta may be null: x_out = x_prev), then xn = LN(x_out) (gamma may be
// null: residual only).  A row belongs to LnShape<D>::LANES lanes (a half wave at D = 32, a wave at 64 / 128), each with
// the features f + LANES * u.
template <int D>
__global__ __launch_bounds__(256) void k_resid_ln_fwd(const float* __restrict__ xprev, const float* __restrict__ delta,
                                                      Drop dr, float* __restrict__ xout,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ xn, float* __restrict__ stats, long long R) {
  constexpr int LANES = LnShape<D>::LANES, NV = LnShape<D>::NV;
  const int f = threadIdx.x & (LANES - 1);
  const long long hw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
  const long long nhw = ((long long)gridDim.x * blockDim.x) / LANES;
  for (long long r = hw; r < R; r += nhw) {
    const long long i = r * D + f;
    float v[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      v[u] = xprev[i + LANES * u];
      if (delta) v[u] += drop_apply(dr, (unsigned int)(i + LANES * u), delta[i + LANES * u]);
      if (xout) xout[i + LANES * u] = v[u];
    }
    if (gamma) {
      float gm[NV], bt[NV], o[NV], mean, rstd;
#pragma unroll
      for (int u = 0; u < NV; ++u) { gm[u] = gamma[f + LANES * u]; bt[u] = beta[f + LANES * u]; }
      ln_fwd<D>(v, gm, bt, o, mean, rstd);
#pragma unroll
      for (int u = 0; u < NV; ++u) xn[i + LANES * u] = o[u];
      if (f == 0) { stats[2 * r] = mean; stats[2 * r + 1] = rstd; }
    }
  }
}

// LayerNorm backward + residual:  dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dxn * gamma.
// Optionally also writes dmask = drop_mask(dx) for the branch feeding the residual BELOW this norm.
// Per-block partial sums of (dxn * xhat, dxn) per feature go to part[block][2][D], the block's row owners added in order.
template <int D>
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dxn, const float* __restrict__ x,
                                                const float* __restrict__ stats, const float* __restrict__ gamma,
                                                const float* __restrict__ dres, float* __restrict__ dx, Drop dr,
                                                float* __restrict__ dmask, float* __restrict__ part, long long R) {
  constexpr int LANES = LnShape<D>::LANES, NV = LnShape<D>::NV, OWNERS = 256 / LANES;
  __shared__ float red[2][OWNERS][D];
  const int f = threadIdx.x & (LANES - 1), hwl = threadIdx.x / LANES;
  const long long hw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / LANES;
  const long long nhw = ((long long)gridDim.x * blockDim.x) / LANES;
  float gm[NV], sg[NV], sb[NV];
#pragma unroll
  for (int u = 0; u < NV; ++u) { gm[u] = gamma[f + LANES * u]; sg[u] = 0.f; sb[u] = 0.f; }
  for (long long r = hw; r < R; r += nhw) {
    const long long i = r * D + f;
    float dn[NV], xx[NV], ds[NV], v[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) { dn[u] = dxn[i + LANES * u]; xx[u] = x[i + LANES * u]; ds[u] = dres[i + LANES * u]; }
    ln_bwd<D>(dn, xx, stats[2 * r], stats[2 * r + 1], gm, ds, v, sg, sb);
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      dx[i + LANES * u] = v[u];
      if (dmask) dmask[i + LANES * u] = drop_apply(dr, (unsigned int)(i + LANES * u), v[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < NV; ++u) {
    red[0][hwl][f + LANES * u] = sg[u];
    red[1][hwl][f + LANES * u] = sb[u];
  }
  __syncthreads();
  if (threadIdx.x < 2 * D) {
    const int w = threadIdx.x / D, ff = threadIdx.x % D;
    float a = 0.f;
    for (int q = 0; q < OWNERS; ++q) a += red[w][q][ff];
    part[((long long)blockIdx.x * 2 + w) * D + ff] = a;
  }
}

// the LayerNorm kernels' instantiation of a supported width
template <typename F>
static int width_dispatch(int d, F&& f) {
  switch (d) {
    case 32: f(std::integral_constant<int, 32>()); return 0;
    case 64: f(std::integral_constant<int, 64>()); return 0;
    case 128: f(std::integral_constant<int, 128>()); return 0;
  }
  return IGI_E_UNSUPPORTED;
}

// masked copy: dst = drop_mask(src)
__global__ __launch_bounds__(256) void k_drop_copy(const float* __restrict__ src, float* __restrict__ dst, Drop dr,
                                                   long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    dst[i] = drop_apply(dr, (unsigned int)i, src[i]);
}

// attention core (token_math.h: attn_ctx_row / attn_bwd).  16 lanes per (sample, head); lane = head dimension.
// qkv row = [q(32) | k(32) | v(32)].
template <int S>
__global__ __launch_bounds__(256) void k_attn_fwd(const float* __restrict__ qkv, float* __restrict__ ctx, Drop dr,
                                                  long long pairs, int H) {
  const int dl = threadIdx.x & 15;
  const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
  for (long long g = g0; g < pairs; g += ng) {
    const long long b = g / H;
    const int h = (int)(g - b * H);
    float q[S], k[S], v[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float* row = qkv + (b * S + s) * (3 * TOK_D) + h * TOK_DH + dl;
      q[s] = row[0]; k[s] = row[TOK_D]; v[s] = row[2 * TOK_D];
    }
#pragma unroll
    for (int i = 0; i < S; ++i) ctx[(b * S + i) * TOK_D + h * TOK_DH + dl] = attn_ctx_row<S>(q, k, v, i, dr, g);
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                  float* __restrict__ dqkv, Drop dr, long long pairs, int H) {
  const int dl = threadIdx.x & 15;
  const long long g0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
  const long long ng = ((long long)gridDim.x * blockDim.x) >> 4;
  for (long long g = g0; g < pairs; g += ng) {
    const long long b = g / H;
    const int h = (int)(g - b * H);
    float q[S], k[S], v[S], dc[S], dq[S], dk[S], dv[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
      const float* row = qkv + (b * S + s) * (3 * TOK_D) + h * TOK_DH + dl;
      q[s] = row[0]; k[s] = row[TOK_D]; v[s] = row[2 * TOK_D];
      dc[s] = dctx[(b * S + s) * TOK_D + h * TOK_DH + dl];
    }
    attn_bwd<S>(q, k, v, dc, dr, g, dq, dk, dv);
#pragma unroll
    for (int s = 0; s < S; ++s) {
      float* row = dqkv + (b * S + s) * (3 * TOK_D) + h * TOK_DH + dl;
      row[0] = dq[s]; row[TOK_D] = dk[s]; row[2 * TOK_D] = dv[s];
    }
  }
}

// ---- attention for 9 <= S <= 32 tokens: the S x S block of one (sample, head) pair as ONE 32 x 32 tile of
// v_mfma_f32_32x32x2_f32, one wave per pair, S a runtime argument.  Same semantics as k_attn_fwd / k_attn_bwd (scale
// 0.25, max-subtracted __expf softmax, dropout element ((b H + h) S + i) S + j, probabilities recomputed in the
// backward).  The scores are formed TRANSPOSED (A = K rows, B = Q rows): lane (i, half) then owns query i and its 16
// accumulator registers run over the keys j = tile_row(r, half), so the softmax is an in-register reduction plus one
// exchange between the half waves, and the probabilities already sit where the A operand of P . V wants them (k-step r
// takes key tile_row(r, 0) from the lower half wave and tile_row(r, 1) from the upper).
// Padding: a tile row >= S is read from row S - 1 instead (always inside the sample, always finite), the scores of the
// keys j >= S are set to -inf ONCE, so their probabilities are exact zeros and whatever they multiply drops out;
// queries i >= S compute a copy of row S - 1 that is never written.  (Predicates per register would each hold a lane
// mask in two SGPRs: with 16 of them alive across the routine k_token_fwd_long spilled SGPRs.)
__device__ __forceinline__ int tile_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
// the same value behind an empty asm.  The routines below take S and the lane number through these once per pair: what
// they derive from them (16 row offsets per operand, store offsets, lane masks) is invariant across the pairs and the
// layers, and hoisted out of those loops it stays alive through the whole kernel -- k_token_fwd_long then spills.  A
// comparison against a second opaque copy is not merged with the earlier ones either (whose masks would stay alive).
__device__ __forceinline__ int tok_opaque(int x) { asm volatile("" : "+s"(x)); return x; }
__device__ __forceinline__ int tok_opaque_lane(int x) { asm volatile("" : "+v"(x)); return x; }

// The tile routines are templated on the head width DH (16, 32 or 64); dm is the model width (the k / v / context column
// offsets and the context pitch), a constant wherever the caller's is.
template <int DH> struct TileShape {
  static_assert(DH == 16 || DH == 32 || DH == 64, "head widths of 16, 32 or 64");
  static constexpr int NC = DH / 8;                 // 8-wide chunks of the contraction over the head dimension
  static constexpr int CW = DH < 32 ? DH : 32;      // output columns of one pass of the 32 x 32 tile
  static constexpr int NP = DH / CW;                // column passes
  static constexpr float SCALE = DH == 16 ? 0.25f : DH == 32 ? 0.17677669529663687f : 0.125f;   // 1 / sqrt(DH)
};

// acc[r] (lane (n = lane & 31, half), row tile_row(r, half)) = sum_k a[row][k] b[n][k] over the DH columns at a / b (this
// lane's row + 4 * half): two chunks' operands at a time, so DH = 64 holds 16 operand registers like DH = 16, not 64
template <int DH>
__device__ __forceinline__ void attn_tile_headdot(const float* a, const float* b, f32x16& acc) {
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < TileShape<DH>::NC; c0 += 2) {
    f32x4 av[2], bv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      av[c] = *reinterpret_cast<const f32x4*>(a + 8 * (c0 + c));
      bv[c] = *reinterpret_cast<const f32x4*>(b + 8 * (c0 + c));
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[c][j], bv[c][j], acc, 0, 0, 0);
    if (TileShape<DH>::NC > 2) __builtin_amdgcn_sched_barrier(0);
  }
}

// probabilities of the pair: pr[r] = softmax_j(q_i . k_j / sqrt(DH)) at lane (i = lane & 31, half), j = tile_row(r, half)
// (0 for j >= S).  q: the pair's first query row (this head's DH columns), k dm floats further on, pitch ld.
template <int DH>
__device__ __forceinline__ void attn_tile_probs(const float* q, int ld, int dm, int S, int lane, f32x16& pr) {
  const int l31 = lane & 31, half = lane >> 5;
  const float* row = q + min(l31, S - 1) * ld + 4 * half;
  f32x16 acc;
  attn_tile_headdot<DH>(row + dm, row, acc);
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[r] = tile_row(r, half) < S ? acc[r] * TileShape<DH>::SCALE : -INFINITY;  // 1 / sqrt(DH); padded keys
    mx = fmaxf(mx, acc[r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // finite: key 0 is valid
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc[r] = __expf(acc[r] - mx);           // padded keys: exp(-inf) = 0
    den += acc[r];
  }
  den += __shfl_xor(den, 32, 64);
  const float inv = 1.0f / den;
#pragma unroll
  for (int r = 0; r < 16; ++r) pr[r] = acc[r] * inv;
  // (the dropout hashes that follow depend on nothing above: without this the scheduler starts all 16 of them under the
  //  matrix products and the routine no longer fits k_token_fwd_long's 128 registers)
  __builtin_amdgcn_sched_barrier(0);
}

// C[32][CW] = sum_j a[r] (row i = lane & 31, column j = tile_row(r, half)) . X[j][0..CW-1]; a is zero in the columns j >= S.
// Result at lane (d = lane & (CW - 1), half): o[r] = C[tile_row(r, half)][d] (CW = 16: lanes 16 .. 31 of a half wave repeat
// 0 .. 15).  One call is one column pass: a head of 64 takes two, X 32 columns further on.
// DROP: a[r] first passes the dropout of element e0 + j (the forward's P . V).
template <bool DROP, int CW>
__device__ __forceinline__ void attn_tile_rowmix(const f32x16& a, const float* X, int ld, int S, int lane, f32x16& o,
                                                 const Drop& dr, unsigned int e0) {
  const int half = lane >> 5;
  X += lane & (CW - 1);
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {               // four k-steps' operands at a time (registers: k_token_fwd_long has 128)
    float xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xv[u] = X[min(tile_row(4 * c + u, half), S - 1) * ld];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float av = a[4 * c + u];
      if (DROP) av = drop_apply(dr, e0 + (unsigned int)tile_row(4 * c + u, half), av);   // (padded keys: 0 stays 0)
      o = __builtin_amdgcn_mfma_f32_32x32x2f32(av, xv[u], o, 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// forward of one pair by one wave.  g: the global (sample, head) index (dropout element numbers); cl (may be null):
// context rows in LDS, pitch ldc; cg: context rows in global memory, pitch dm (both at this head's columns).
template <int DH>
__device__ __forceinline__ void attn_tile_fwd(const float* q, int ld, int dm, int S, long long g, const Drop& dr, float* cl,
                                              int ldc, float* cg) {
  constexpr int CW = TileShape<DH>::CW, NP = TileShape<DH>::NP;
  S = tok_opaque(S);
  const int lane = tok_opaque_lane(threadIdx.x & 63), l31 = lane & 31, half = lane >> 5;
  f32x16 pr, o;
  attn_tile_probs<DH>(q, ld, dm, S, lane, pr);
  const unsigned int e0 = (unsigned int)((g * S + l31) * S);
  if constexpr (NP > 1) {                     // the dropout factors once per pair, not once per column pass
#pragma unroll
    for (int r = 0; r < 16; ++r) pr[r] = drop_apply(dr, e0 + (unsigned int)tile_row(r, half), pr[r]);
  }
#pragma unroll
  for (int cp = 0; cp < NP; ++cp) {
    attn_tile_rowmix<NP == 1, CW>(pr, q + 2 * dm + 32 * cp, ld, S, lane, o, dr, e0);
    if (l31 < CW) {
      const int Sw = tok_opaque(S);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = tile_row(r, half);
        if (i < Sw) {
          if (cl) cl[i * ldc + 32 * cp + l31] = o[r];
          cg[i * dm + 32 * cp + l31] = o[r];
        }
      }
    }
  }
}

constexpr int AT_LDT = 33;                      // pitch of the 32 x 32 transposition tiles of the backward
constexpr int AT_TILE = 32 * AT_LDT;

// C[32][CW] = sum_i T[j][i] X[i][0..CW-1] for the tile T (row = key j, column = query i; zero in the columns i >= S):
// A = the tile's row (key = lane & 31), k-step t takes query 2 t + half.  Result as attn_tile_rowmix's, one column pass.
template <int CW>
__device__ __forceinline__ void attn_tile_colmix(const float* T, const float* X, int ldx, int S, int lane, f32x16& o) {
  const int l31 = lane & 31, half = lane >> 5;
  X += lane & (CW - 1);
  T += l31 * AT_LDT + half;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float av[4], xv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      av[u] = T[2 * (4 * c + u)];
      xv[u] = X[min(2 * (4 * c + u) + half, S - 1) * ldx];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) o = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], xv[u], o, 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// backward of one pair by one wave: dV = (P m)^T dC, dP = (dC V^T) m, dS = P (dP - rowsum(dP P)) / sqrt(DH), dQ = dS K,
// dK = dS^T Q (m: the dropout factors).  dP is formed transposed like the scores (A = V rows, B = dC rows), so it meets
// P register for register; dQ contracts over the keys, which the registers run over; dV and dK contract over the
// queries, which the lanes run over: P m and dS go through two 32 x 32 LDS tiles (T, this wave's own; the columns of the
// queries >= S written as zeros) to be read back as A operands with the query as the k index.  P, m and dS are formed
// once per pair; the three products run TileShape<DH>::NP column passes each off the same registers and tiles.
// q / dc / dq: first rows of the pair at this head's columns (dq: pitch ld like q; dc: pitch dm).
template <int DH>
__device__ __forceinline__ void attn_tile_bwd(const float* q, int ld, int dm, const float* dc, float* dq, int S, long long g,
                                              const Drop& dr, float* T) {
  constexpr int CW = TileShape<DH>::CW, NP = TileShape<DH>::NP;
  S = tok_opaque(S);
  const int lane = tok_opaque_lane(threadIdx.x & 63), l31 = lane & 31, half = lane >> 5;
  f32x16 pr, dp, o;
  attn_tile_probs<DH>(q, ld, dm, S, lane, pr);
  {
    const int rowi = min(l31, S - 1);
    attn_tile_headdot<DH>(q + rowi * ld + 2 * dm + 4 * half, dc + rowi * dm + 4 * half, dp);
  }
  const unsigned int e0 = (unsigned int)((g * S + l31) * S);
  const bool query = l31 < S;
  float dot = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = tile_row(r, half);
    // the mask factor m_ij in {0, 1/(1-p)}: P_drop = P * m
    const float m = drop_apply(dr, e0 + (unsigned int)j, 1.0f);
    dp[r] *= m;                               // d(loss)/dP_ij
    dot += dp[r] * pr[r];
    T[j * AT_LDT + l31] = query ? pr[r] * m : 0.f;          // (P m)^T: row = key, column = query
    if ((r & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
  dot += __shfl_xor(dot, 32, 64);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    dp[r] = pr[r] * (dp[r] - dot) * TileShape<DH>::SCALE;   // dS: d(loss)/d(score_ij) incl. the 1/sqrt(dh); zero at the padded keys
    T[AT_TILE + tile_row(r, half) * AT_LDT + l31] = query ? dp[r] : 0.f;
  }
  const int Sw = tok_opaque(S);
#pragma unroll
  for (int cp = 0; cp < NP; ++cp) {
    attn_tile_rowmix<false, CW>(dp, q + dm + 32 * cp, ld, S, lane, o, dr, 0u);  // dQ = dS K
    if (l31 < CW) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = tile_row(r, half);
        if (i < Sw) dq[i * ld + 32 * cp + l31] = o[r];
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
  for (int w = 0; w < 2; ++w) {               // dV = (P m)^T dC (dC: pitch dm), then dK = dS^T Q
#pragma unroll
    for (int cp = 0; cp < NP; ++cp) {
      attn_tile_colmix<CW>(T + w * AT_TILE, (w == 0 ? dc : q) + 32 * cp, w == 0 ? dm : ld, S, lane, o);
      if (l31 < CW) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = tile_row(r, half);
          if (j < Sw) dq[j * ld + (w == 0 ? 2 * dm : dm) + 32 * cp + l31] = o[r];
        }
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();             // the wave's next pair rewrites the tiles
}

// The tile kernels: DH the head width, DM the model width (H = DM / DH heads).  <16, 32> is the 32-wide model's kernel for
// 9 .. 32 tokens; every other instantiation is a wide configuration's attention at any S from 1 to 32.
constexpr int AT_THREADS = 256;                 // four waves, a (sample, head) pair each per step
template <int DH, int DM>
__global__ __launch_bounds__(AT_THREADS) void k_attn_tile_fwd(const float* __restrict__ qkv, float* __restrict__ ctx, Drop dr,
                                                              long long pairs, int H, int S) {
  const long long w0 = ((long long)blockIdx.x * AT_THREADS + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * AT_THREADS) >> 6;
  for (long long g = w0; g < pairs; g += nw) {
    const long long b = g / H;
    const int h = (int)(g - b * H);
    attn_tile_fwd<DH>(qkv + b * S * (3 * DM) + h * DH, 3 * DM, DM, S, g, dr, nullptr, 0, ctx + b * S * DM + h * DH);
  }
}

template <int DH, int DM>
__global__ __launch_bounds__(AT_THREADS) void k_attn_tile_bwd(const float* __restrict__ qkv, const float* __restrict__ dctx,
                                                              float* __restrict__ dqkv, Drop dr, long long pairs, int H, int S) {
  __shared__ float tiles[AT_THREADS / 64][2 * AT_TILE];
  const long long w0 = ((long long)blockIdx.x * AT_THREADS + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * AT_THREADS) >> 6;
  for (long long g = w0; g < pairs; g += nw) {
    const long long b = g / H;
    const int h = (int)(g - b * H);
    attn_tile_bwd<DH>(qkv + b * S * (3 * DM) + h * DH, 3 * DM, DM, dctx + b * S * DM + h * DH, dqkv + b * S * (3 * DM) + h * DH, S,
                      g, dr, tiles[threadIdx.x >> 6]);
  }
}

// the tile kernels' instantiation of a supported (head width, model width) pair
template <typename F>
static int tile_dispatch(int dh, int dm, F&& f) {
#define IGI_TILE_CASE(DH_, DM_) \
  if (dh == DH_ && dm == DM_) { f(std::integral_constant<int, DH_>(), std::integral_constant<int, DM_>()); return 0; }
  IGI_TILE_CASE(16, 32) IGI_TILE_CASE(32, 32)
  IGI_TILE_CASE(16, 64) IGI_TILE_CASE(32, 64) IGI_TILE_CASE(64, 64)
  IGI_TILE_CASE(16, 128) IGI_TILE_CASE(32, 128) IGI_TILE_CASE(64, 128)
#undef IGI_TILE_CASE
  return IGI_E_UNSUPPORTED;
}

// h = drop(gelu(z)), exact erf form (nn.GELU default / activation="gelu")
__global__ __launch_bounds__(256) void k_gelu_fwd(const float* __restrict__ z, float* __restrict__ h, Drop dr,
                                                  long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    h[i] = drop_apply(dr, (unsigned int)i, gelu(z[i]));
}
__global__ __launch_bounds__(256) void k_gelu_bwd(const float* __restrict__ dh, const float* __restrict__ z,
                                                  float* __restrict__ dz, Drop dr, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
  {
    const float gd = gelu_grad(z[i]);
    dz[i] = drop_apply(dr, (unsigned int)i, dh[i]) * gd;
  }
}

static inline int tok_blocks(long long n, int per_block, int cap = 2048) {
  long long b = (n + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

template <typename F>
static int attn_dispatch(int S, F&& f) {
  switch (S) {
    case 1: f(std::integral_constant<int, 1>()); return 0;
    case 2: f(std::integral_constant<int, 2>()); return 0;
    case 3: f(std::integral_constant<int, 3>()); return 0;
    case 4: f(std::integral_constant<int, 4>()); return 0;
    case 5: f(std::integral_constant<int, 5>()); return 0;
    case 6: f(std::integral_constant<int, 6>()); return 0;
    case 7: f(std::integral_constant<int, 7>()); return 0;
    case 8: f(std::integral_constant<int, 8>()); return 0;
  }
  return IGI_E_UNSUPPORTED;
}

static inline float* tok_ws(void* ws) {
  return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 15) & ~(uintptr_t)15);
}

// dropout sites of layer l
enum { SITE_ATTN = 0, SITE_SA = 1, SITE_FF_ACT = 2, SITE_FF = 3 };

// ---------------------------------------------------------------------------------------------------------------------
// The whole forward as ONE launch (round 5).  As 8 launches per layer + 1 (four GEMMs, two residual + LayerNorm kernels,
// attention, GELU) the stack was 17 launches of 4 - 8 us for ~0.15 GFLOP.  Here a workgroup (TF_THREADS) carries up to
// 128 token rows = 128 / S whole samples (at most 32 of them; 14 at S = 9, 4 at S = 32) through every layer with the residual stream,
// the LayerNorm outputs, q / k / v and the feed-forward activations in LDS; a layer's four weight matrices are brought into
// LDS once per workgroup and layer; every activation the backward pass reads (TokenPlan::a_*) is written out once.
// Arithmetic = the separate kernels', operation by operation, because both call the same routines: the Linears are fmaf
// chains on v_mfma_f32_32x32x2_f32 in the LDS-DMA kernel's k order (tile32_kdot; K = 32 and 128 are whole k-tiles), LayerNorm
// is ln_fwd on a half wave per row, attention is attn_ctx_row on 16 lanes per (sample, head) (S <= 8, k_token_fwd<S>) or
// attn_tile_fwd on the LDS rows, the (sample, head) pairs dealt over the waves (9 <= S <= 32, k_token_fwd_long), GELU is gelu,
// dropout is drop_apply on the same element indices -- outputs and saved activations are bit-identical
// (tests/test_gpu_token_encoder.py, test_gpu_token_encoder_long.py).
// Both kernels are token_fwd_body<S>; S = 0 selects the runtime-S tile attention.
// ---------------------------------------------------------------------------------------------------------------------
// Waves per workgroup of the two fused kernels.  A workgroup's time is its chain of ~20 phases per layer, each as wide as the
// workgroup: at 8192 x 2 tokens the forward ran 59.5 / 43.5 / 37.6 us with 256 / 512 / 1024 threads, the backward 95 / 64.6 /
// 69.4 (2048 x 3: 39 / 32.9 / 28.6 and 57.5 / 44.9 / 60.7: at 1024 threads the backward's attention pass has 128 registers).
#ifndef TF_THREADS_N
#define TF_THREADS_N 1024
#endif
#ifndef TB_THREADS_N
#define TB_THREADS_N 512
#endif
constexpr int TF_THREADS = TF_THREADS_N, TF_NW = TF_THREADS / 64, TF_HW = TF_THREADS / 32;   // forward
constexpr int TB_THREADS = TB_THREADS_N, TB_NW = TB_THREADS / 64, TB_HW = TB_THREADS / 32;   // backward
constexpr int TF_ROWS = 128;                 // token rows per workgroup (LDS images are this tall)
constexpr int TF_LDX = TOK_D + 4;            // 36: row pitch of the 32-wide images (16-byte reads of 16 rows: 16 bank groups)
constexpr int TF_LDZ = 128 + 4;              // 132: q|k|v (96 used) and the feed-forward activations
constexpr int TF_FF = 128;
constexpr int TF_W_FLOATS = 3 * TOK_D * TF_LDX + TOK_D * TF_LDX + TF_FF * TF_LDX + TOK_D * TF_LDZ;
constexpr int TF_LDS_FLOATS = 2 * TF_ROWS * TF_LDX + TF_ROWS * TF_LDZ + TF_W_FLOATS;

struct TokFwdArgs {
  const float* x; const float* params; float* y; float* W;   // W: the (aligned) workspace base
  long long R;
  TokLayout lay;
  int S, H, L, rows_per_wg;
  float p; unsigned long long seed;
};

// S = 0: 9 .. 32 tokens per sample, a.S at run time, attention on the matrix-pipe tile (k_token_fwd_long)
template <int S>
__device__ __forceinline__ void token_fwd_body(const TokFwdArgs& a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* bx = smem;                               // residual stream [rows][36]
  float* bn = bx + TF_ROWS * TF_LDX;              // LayerNorm output / attention context / branch outputs [rows][36]
  float* bz = bn + TF_ROWS * TF_LDX;              // q|k|v, then z / h [rows][132]
  float* win = bz + TF_ROWS * TF_LDZ;             // in_proj [96][36]
  float* wout = win + 3 * TOK_D * TF_LDX;         // out_proj [32][36]
  float* w1 = wout + TOK_D * TF_LDX;              // linear1 [128][36]
  float* w2 = w1 + TF_FF * TF_LDX;                // linear2 [32][132]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const long long r0 = (long long)blockIdx.x * a.rows_per_wg;
  const int nrows = (int)min((long long)a.rows_per_wg, a.R - r0);
  const int mtiles = (nrows + 31) >> 5;
  const int f = tid & 31, hw = tid >> 5;          // LayerNorm: half wave hw (of 8) owns rows hw, hw + 8, ...

  // C[rows][N] = A[rows][K] . Wimg[N][K]^T + bias, into LDS (pitch ldc) and, if G, to global (pitch N); tiles round-robin
  auto linear = [&](const float* A, int lda, int K, const float* Wimg, int ldw, int N, const float* bias, float* C, int ldc,
                    float* G) {
    const int ntiles = N >> 5;
    for (int t = wave; t < mtiles * ntiles; t += TF_NW) {
      const int mt = t / ntiles, nt = t - mt * ntiles;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      tile32_kdot(A + (32 * mt + l31) * lda + 4 * h, Wimg + (32 * nt + l31) * ldw + 4 * h, K, acc);
      const int n = 32 * nt + l31;
      const float b = bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h;
        const float v = acc[r] + b;
        C[row * ldc + n] = v;
        if (G && row < nrows) G[(r0 + row) * N + n] = v;
      }
    }
  };
  // bx = xout = xprev (+ drop(delta)), bn = xn = LN(xout) (ln_fwd).  xprev: global rows, or null: bx; delta: LDS rows of pitch
  // ldd, or null
  auto resid_ln = [&](const float* xprev_g, const float* delta, int ldd, const Drop& dr, float* xout_g, const float* gamma,
                      const float* beta, float* xn_g, float* stats_g) __attribute__((always_inline)) {
    for (int row = hw; row < nrows; row += TF_HW) {
      const long long i = (r0 + row) * TOK_D + f;
      float v = xprev_g ? xprev_g[i] : bx[row * TF_LDX + f];
      if (delta) v += drop_apply(dr, (unsigned int)i, delta[row * ldd + f]);
      bx[row * TF_LDX + f] = v;
      xout_g[i] = v;
      float mean, rstd;
      const float o = ln_fwd(v, gamma[f], beta[f], mean, rstd);
      bn[row * TF_LDX + f] = o;
      xn_g[i] = o;
      if (f == 0) { stats_g[2 * (r0 + row)] = mean; stats_g[2 * (r0 + row) + 1] = rstd; }
    }
  };

  const TokLayout& ly = a.lay;
  Drop pending = make_drop(0.f, a.seed, 0);
  for (int l = 0; l < a.L; ++l) {
    const float* P = a.params + (long long)l * ly.per_layer;
    float* A = a.W + (long long)l * ly.a_layer;
    // ---- this layer's weights -> LDS (coalesced 16-byte loads); the previous layer's readers are behind its last barrier
    for (int u = tid; u < 3 * TOK_D * 8; u += TF_THREADS)
      *reinterpret_cast<float4*>(win + (u >> 3) * TF_LDX + 4 * (u & 7)) = *reinterpret_cast<const float4*>(P + ly.o_inw + 4 * u);
    for (int u = tid; u < TOK_D * 8; u += TF_THREADS)
      *reinterpret_cast<float4*>(wout + (u >> 3) * TF_LDX + 4 * (u & 7)) = *reinterpret_cast<const float4*>(P + ly.o_ow + 4 * u);
    for (int u = tid; u < TF_FF * 8; u += TF_THREADS)
      *reinterpret_cast<float4*>(w1 + (u >> 3) * TF_LDX + 4 * (u & 7)) = *reinterpret_cast<const float4*>(P + ly.o_w1 + 4 * u);
    for (int u = tid; u < TOK_D * 32; u += TF_THREADS)
      *reinterpret_cast<float4*>(w2 + (u >> 5) * TF_LDZ + 4 * (u & 31)) = *reinterpret_cast<const float4*>(P + ly.o_w2 + 4 * u);
    // ---- x_l = x_{l-1} + drop(ff branch of l - 1) (l == 0: the input), xn1 = LN1(x_l)
    resid_ln(l == 0 ? a.x : nullptr, l > 0 ? bn : nullptr, TF_LDX, pending, A + ly.a_x, P + ly.o_n1w, P + ly.o_n1b, A + ly.a_xn1,
             A + ly.a_st1);
    __syncthreads();
    linear(bn, TF_LDX, TOK_D, win, TF_LDX, 3 * TOK_D, P + ly.o_inb, bz, TF_LDZ, A + ly.a_qkv);
    __syncthreads();
    if constexpr (S == 0) {
      // ---- attention: a wave per (sample, head), attn_tile_fwd on the LDS rows; context -> bn
      const Drop da = make_drop(a.p, a.seed, 4 * l + SITE_ATTN);
      const int nsamp = nrows / a.S;
      for (int g = wave; g < nsamp * a.H; g += TF_NW) {
        const int bl = g / a.H, hh = g - bl * a.H;
        attn_tile_fwd<TOK_DH>(bz + bl * a.S * TF_LDZ + hh * TOK_DH, TF_LDZ, TOK_D, a.S, (r0 / a.S + bl) * a.H + hh, da,
                              bn + bl * a.S * TF_LDX + hh * TOK_DH, TF_LDX, A + ly.a_ctx + (r0 + bl * a.S) * TOK_D + hh * TOK_DH);
      }
    } else {
      // ---- attention: 16 lanes per (sample, head), attn_ctx_row on the LDS rows; context -> bn
      const Drop da = make_drop(a.p, a.seed, 4 * l + SITE_ATTN);
      const int dl = tid & 15;
      const int nsamp = nrows / S;
      for (int g = tid >> 4; g < nsamp * a.H; g += TF_THREADS / 16) {
        const int bl = g / a.H, hh = g - bl * a.H;
        const long long gg = (r0 / S + bl) * a.H + hh;       // the global (sample, head) index: dropout element indices
        float q[S], k[S], v[S];
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
          const float* row = bz + (bl * S + s2) * TF_LDZ + hh * TOK_DH + dl;
          q[s2] = row[0]; k[s2] = row[TOK_D]; v[s2] = row[2 * TOK_D];
        }
#pragma unroll
        for (int i = 0; i < S; ++i) {
          const float o = attn_ctx_row<S>(q, k, v, i, da, gg);
          bn[(bl * S + i) * TF_LDX + hh * TOK_DH + dl] = o;
          A[ly.a_ctx + (r0 + bl * S + i) * TOK_D + hh * TOK_DH + dl] = o;
        }
      }
    }
    __syncthreads();
    linear(bn, TF_LDX, TOK_D, wout, TF_LDX, TOK_D, P + ly.o_ob, bz, TF_LDZ, nullptr);    // sa branch -> bz[:, 0..31]
    __syncthreads();
    // ---- x1 = x + drop(sa branch), xn2 = LN2(x1)   (the branch is read from bz here)
    resid_ln(nullptr, bz, TF_LDZ, make_drop(a.p, a.seed, 4 * l + SITE_SA), A + ly.a_x1, P + ly.o_n2w, P + ly.o_n2b, A + ly.a_xn2,
             A + ly.a_st2);
    __syncthreads();
    linear(bn, TF_LDX, TOK_D, w1, TF_LDX, TF_FF, P + ly.o_b1, bz, TF_LDZ, A + ly.a_z);
    __syncthreads();
    // ---- h = drop(gelu(z)), in place
    {
      const Drop dg = make_drop(a.p, a.seed, 4 * l + SITE_FF_ACT);
      for (int e = tid; e < nrows * TF_FF; e += TF_THREADS) {
        const int row = e >> 7, c = e & 127;
        const float xz = bz[row * TF_LDZ + c];
        const long long i = (r0 + row) * TF_FF + c;
        const float hv = drop_apply(dg, (unsigned int)i, gelu(xz));
        bz[row * TF_LDZ + c] = hv;
        A[ly.a_h + i] = hv;
      }
    }
    __syncthreads();
    linear(bz, TF_LDZ, TF_FF, w2, TF_LDZ, TOK_D, P + ly.o_b2, bn, TF_LDX, nullptr);      // ff branch -> bn
    __syncthreads();
    pending = make_drop(a.p, a.seed, 4 * l + SITE_FF);
  }
  // ---- y = x1_{L-1} + drop(ff branch)
  for (int row = hw; row < nrows; row += TF_HW) {
    const long long i = (r0 + row) * TOK_D + f;
    a.y[i] = bx[row * TF_LDX + f] + drop_apply(pending, (unsigned int)i, bn[row * TF_LDX + f]);
  }
}

template <int S>
__global__ __launch_bounds__(TF_THREADS) void k_token_fwd(const TokFwdArgs a) { token_fwd_body<S>(a); }
// 9 <= a.S <= 32: 128 / S whole samples per workgroup, the (sample, head) pairs dealt over the waves
__global__ __launch_bounds__(TF_THREADS) void k_token_fwd_long(const TokFwdArgs a) { token_fwd_body<0>(a); }

// Launch of a one-launch kernel: its dynamic LDS is beyond the default limit, so the attribute is set before the first launch
// (one flag per kernel instantiation).  Inside a ProfScope the launch carries the scope's events (IGI_LAUNCH).
template <auto KERNEL, typename Args>
static void tok_launch_lds(int grid, int threads, size_t lds_bytes, hipStream_t s, const Args& a) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    attr = true;
  }
  IGI_LAUNCH(KERNEL, dim3(grid), dim3(threads), lds_bytes, s, a);
}

static inline bool token_fused_enabled() {
  const char* e = getenv("IGI_TOKEN_FUSED");   // read per call (one call per forward pass): the parity test switches it
  return !e || atoi(e) != 0;
}

static int token_forward(const igi_token_cfg* c, const float* x, const float* params, float* y, void* workspace,
                         size_t workspace_bytes, unsigned long long seed, hipStream_t s) {
  TokenPlan p;
  int rc = make_token_plan(c, &p);
  if (rc) return rc;
  if (!x || !params || !y || !workspace) return IGI_E_BADARG;
  if (workspace_bytes < p.total_bytes) return IGI_E_WORKSPACE;
  float* W = tok_ws(workspace);
  const TokLayout& ly = p.lay;
  // (the alignment terms are linear_forward's conditions for the LDS-DMA kernel, whose k order the fused kernel reproduces)
  // (the one-launch kernels are (32, 2) only: a layer's weights at 64 wide are 196 KB, above LDS)
  if (token_fused_enabled() && p.ff == TF_FF && p.narrow && p.R >= 4 && aligned16(params) && !bf16_mode() &&
      ((ly.per_layer | ly.o_inw | ly.o_ow | ly.o_w1 | ly.o_w2 | ly.a_layer | ly.a_xn1 | ly.a_ctx | ly.a_xn2 | ly.a_h) & 3) == 0) {
    TokFwdArgs a;
    a.x = x; a.params = params; a.y = y; a.W = W;
    a.R = p.R; a.lay = ly;
    a.S = p.S; a.H = p.H; a.L = p.L; a.p = p.p; a.seed = seed;
    // samples per workgroup: up to 128 token rows, but no fewer than one workgroup per CU while the batch allows it (2048
    // samples x 3 tokens as 64 workgroups of 96 rows ran 78 us; a workgroup's time is its serial chain of phases)
    int samples = (int)(TF_ROWS / p.S);
    if ((long long)samples * 256 > p.B) samples = (int)(p.B / 256 > 1 ? p.B / 256 : 1);
    a.rows_per_wg = samples * p.S;
    const int grid = (int)((p.B + samples - 1) / samples);
    // algorithmic work of the stack: the four Linears of a row, the two S x S products of a (sample, head) pair
    const double tok_flops = (double)p.L * (2.0 * p.R * (4.0 * p.d * p.d + 2.0 * p.d * p.ff) + 4.0 * p.B * p.H * p.S * p.S * p.dh);
    const double tok_bytes = 4.0 * ((double)p.L * ly.a_layer + 2.0 * p.R * p.d + (double)p.L * ly.per_layer);
    if (p.S > TOK_MAX_S) {
      ProfScope ps(PC_TOKEN_FWD_LONG, s, tok_flops, tok_bytes);
      tok_launch_lds<k_token_fwd_long>(grid, TF_THREADS, sizeof(float) * TF_LDS_FLOATS, s, a);
      return (int)hipGetLastError();
    }
    rc = attn_dispatch(p.S, [&](auto sc) {
      ProfScope ps(PC_TOKEN_FWD, s, tok_flops, tok_bytes);
      tok_launch_lds<k_token_fwd<decltype(sc)::value>>(grid, TF_THREADS, sizeof(float) * TF_LDS_FLOATS, s, a);
    });
    if (rc) return rc;
    return (int)hipGetLastError();
  }
  const long long R = p.R;
  const int d = p.d, ff = p.ff;
  const int rb = tok_blocks(R, p.d == TOK_D ? 8 : 4);  // rows per 256-thread block: 8 half waves, or 4 waves beyond 32 features
  const bool tile = p.S > TOK_MAX_S || !p.narrow;     // the register attention kernels: 16-wide heads of a 32-wide model
  auto resid_ln = [&](const float* xprev, const float* delta, const Drop& dr, float* xout, const float* gamma, const float* beta,
                      float* xn, float* stats) {
    return width_dispatch(d, [&](auto dc) {
      hipLaunchKernelGGL(k_resid_ln_fwd<decltype(dc)::value>, dim3(rb), dim3(256), 0, s, xprev, delta, dr, xout, gamma, beta, xn,
                         stats, R);
    });
  };
  // layer 0 input + LN1
  const float* xin = x;
  const float* branch = nullptr;  // pending residual branch (ff output of the previous layer)
  Drop pending = make_drop(0.f, seed, 0);
  for (int l = 0; l < p.L; ++l) {
    const float* P = params + (long long)l * ly.per_layer;
    float* A = W + (long long)l * ly.a_layer;
    // x_l = x_{l-1} + drop(ff branch of l-1)  (l == 0: copy of the input), xn1 = LN1(x_l)
    if ((rc = resid_ln(xin, branch, pending, A + ly.a_x, P + ly.o_n1w, P + ly.o_n1b, A + ly.a_xn1, A + ly.a_st1))) return rc;
    if ((rc = linear_forward(A + ly.a_xn1, d, P + ly.o_inw, P + ly.o_inb, A + ly.a_qkv, 3 * d, R, d, 3 * d, LIN_NONE, s)))
      return rc;
    const long long pairs = (long long)p.B * p.H;
    const Drop da = make_drop(p.p, seed, 4 * l + SITE_ATTN);
    if (tile) {
      ProfScope ps(PC_ATTN_TILE_FWD, s, 4.0 * pairs * p.S * p.S * p.dh, 4.0 * R * (4.0 * d));
      rc = tile_dispatch(p.dh, d, [&](auto hc, auto mc) {
        IGI_LAUNCH((k_attn_tile_fwd<decltype(hc)::value, decltype(mc)::value>), dim3(tok_blocks(pairs, AT_THREADS / 64)),
                   dim3(AT_THREADS), 0, s, A + ly.a_qkv, A + ly.a_ctx, da, pairs, p.H, p.S);
      });
      if (rc) return rc;
    } else {
      rc = attn_dispatch(p.S, [&](auto sc) {
        constexpr int SS = decltype(sc)::value;
        hipLaunchKernelGGL((k_attn_fwd<SS>), dim3(tok_blocks(pairs, 16)), dim3(256), 0, s, A + ly.a_qkv, A + ly.a_ctx, da,
                           pairs, p.H);
      });
      if (rc) return rc;
    }
    float* t0 = W + p.s_g0;  // sa branch output (not needed by backward)
    if ((rc = linear_forward(A + ly.a_ctx, d, P + ly.o_ow, P + ly.o_ob, t0, d, R, d, d, LIN_NONE, s))) return rc;
    if ((rc = resid_ln(A + ly.a_x, t0, make_drop(p.p, seed, 4 * l + SITE_SA), A + ly.a_x1, P + ly.o_n2w, P + ly.o_n2b,
                       A + ly.a_xn2, A + ly.a_st2)))
      return rc;
    if ((rc = linear_forward(A + ly.a_xn2, d, P + ly.o_w1, P + ly.o_b1, A + ly.a_z, ff, R, d, ff, LIN_NONE, s))) return rc;
    hipLaunchKernelGGL(k_gelu_fwd, dim3(tok_blocks(R * ff, 256)), dim3(256), 0, s, A + ly.a_z, A + ly.a_h,
                       make_drop(p.p, seed, 4 * l + SITE_FF_ACT), R * ff);
    float* t1 = W + p.s_g1;
    if ((rc = linear_forward(A + ly.a_h, ff, P + ly.o_w2, P + ly.o_b2, t1, d, R, ff, d, LIN_NONE, s))) return rc;
    xin = A + ly.a_x1;
    branch = t1;
    pending = make_drop(p.p, seed, 4 * l + SITE_FF);
  }
  // y = x1_{L-1} + drop(ff branch)
  if ((rc = resid_ln(xin, branch, pending, y, nullptr, nullptr, nullptr, nullptr))) return rc;
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The whole backward as ONE launch + one sum (round 5).  As separate launches a backward pass was eight Linear levels
// (weight + data gradient each), four LayerNorm, two attention, two GELU kernels, a masked copy and the deferred sums:
// ~20 launches of 5 - 15 us for ~0.45 GFLOP (124 us at 2048 x 3 tokens, ~200 us at 8192 x 2).  Here a workgroup keeps the
// gradient of the residual stream of its <= 64 token rows in LDS and walks the layers top down: per layer the four
// weight matrices are staged TRANSPOSED (the data gradients then are the forward's k-contiguous MFMA loops), saved
// activations are staged once each, every weight gradient is a 32 x 32 MFMA tile over the workgroup's rows (operands
// read along the row axis of the LDS arrays), bias / LayerNorm parameter gradients are column sums of the passes that
// produce their operands.  A workgroup writes ONE record of all parameter gradients; k_slab_reduce sums the records
// in fixed order (bitwise reproducible, no atomics).  The formulas are the routines k_ln_bwd and k_gelu_bwd call (ln_bwd,
// gelu_grad, drop_apply on the same element numbers) and, restated in step 7 for its register count, k_attn_bwd's attn_bwd;
// sums associate differently (per-workgroup records instead of split-row slabs), so results agree with the
// launch-per-operation path to rounding, not bitwise.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int TB_LDW = 3 * TOK_D + 4;        // 100: row pitch of the transposed in_proj image
constexpr int TB_RED = 3 * TB_THREADS;
constexpr int TB_LDS_FLOATS = 2 * TB_ROWS * TF_LDX + 2 * TB_ROWS * TF_LDZ + TF_FF * TF_LDX + TOK_D * TF_LDZ + TOK_D * TF_LDX +
                              TOK_D * TB_LDW + TB_RED;

struct TokBwdArgs {
  const float* dy; const float* params; float* dx; float* W; float* part;
  long long R, P;        // P: floats of a workgroup's gradient record (all layers)
  TokLayout lay;
  int S, H, L, rows_per_wg;
  float p; unsigned long long seed;
};

template <int S>
__global__ __launch_bounds__(TB_THREADS) void k_token_bwd(const TokBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* bg = smem;                               // gradient w.r.t. the residual stream [rows][36]
  float* bd = bg + TB_ROWS * TF_LDX;              // 32-wide operand of the current product [rows][36]
  float* bw = bd + TB_ROWS * TF_LDX;              // wide gradient (dh / dz, dctx) [rows][132]
  float* ba = bw + TB_ROWS * TF_LDZ;              // staged activations, dqkv [rows][132]
  float* w2t = ba + TB_ROWS * TF_LDZ;             // linear2^T [128][36]
  float* w1t = w2t + TF_FF * TF_LDX;              // linear1^T [32][132]
  float* wot = w1t + TOK_D * TF_LDZ;              // out_proj^T [32][36]
  float* wit = wot + TOK_D * TF_LDX;              // in_proj^T [32][100]
  float* red = wit + TOK_D * TB_LDW;              // column-sum partials
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const long long r0 = (long long)blockIdx.x * a.rows_per_wg;
  const int nrows = (int)min((long long)a.rows_per_wg, a.R - r0);
  const int mtiles = (nrows + 31) >> 5;
  const int f = tid & 31, hw = tid >> 5;
  float* G0 = a.part + (long long)blockIdx.x * a.P;
  const TokLayout& ly = a.lay;

  // C[rows][N] = A[rows][K] . Wimg[N][K]^T (tile32_kdot like the forward's Linears, no bias)
  auto dgrad = [&](const float* A, int lda, int K, const float* Wimg, int ldw, int N, float* C, int ldc) {
    const int ntiles = N >> 5;
    for (int t = wave; t < mtiles * ntiles; t += TB_NW) {
      const int mt = t / ntiles, nt = t - mt * ntiles;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      tile32_kdot(A + (32 * mt + l31) * lda + 4 * h, Wimg + (32 * nt + l31) * ldw + 4 * h, K, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) C[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h) * ldc + 32 * nt + l31] = acc[r];
    }
  };
  // dW[M][N] = sum_r Y[r][m] X[r][n] over the workgroup's rows (rows past nrows hold zeros) -> this workgroup's record
  auto wgrad = [&](const float* Y, int ldy, int M, const float* X, int ldx, int N, float* dst) {
    const int ntiles = N >> 5;
    const int total = (M >> 5) * ntiles;
    for (int t = wave; t < total; t += TB_NW) {
      const int mt = t / ntiles, nt = t - mt * ntiles;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* yp = Y + h * ldy + 32 * mt + l31;
      const float* xp = X + h * ldx + 32 * nt + l31;
      for (int rb = 0; rb < 32 * mtiles; rb += 16) {   // eight k-steps' operands in flight in front of their MFMAs
        float ya[8], xa[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { ya[q] = yp[(rb + 2 * q) * ldy]; xa[q] = xp[(rb + 2 * q) * ldx]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ya[q], xa[q], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[(32 * mt + (r & 3) + 8 * (r >> 2) + 4 * h) * N + 32 * nt + l31] = acc[r];
    }
  };
  // rows of a saved activation [R][width] -> LDS (16-byte pieces)
  auto stage = [&](const float* g, int width, float* dst, int ld) {
    const int w4 = width >> 2;
    for (int e = tid; e < nrows * w4; e += TB_THREADS) {
      const int row = e / w4, c = e - row * w4;
      *reinterpret_cast<float4*>(dst + row * ld + 4 * c) = *reinterpret_cast<const float4*>(g + (r0 + row) * width + 4 * c);
    }
  };
  // sum of the per-half-wave partials of a 32-wide column sum -> dst[0..31]  (red + 256 * slot)
  auto put32 = [&](int slot, float v) { red[TB_THREADS * slot + hw * 32 + f] = v; };
  auto sum32 = [&](int slot, float* dst) {
    if (tid < 32) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < TB_HW; ++q) t += red[TB_THREADS * slot + q * 32 + tid];
      dst[tid] = t;
    }
  };

  for (int e = tid; e < TB_LDS_FLOATS; e += TB_THREADS) smem[e] = 0.f;   // rows past nrows stay zero for the whole kernel
  __syncthreads();
  for (int row = hw; row < nrows; row += TB_HW) bg[row * TF_LDX + f] = a.dy[(r0 + row) * TOK_D + f];

  for (int l = a.L - 1; l >= 0; --l) {
    const float* P = a.params + (long long)l * ly.per_layer;
    const float* A = a.W + (long long)l * ly.a_layer;
    float* G = G0 + (long long)l * ly.per_layer;
    // ---- the layer's weights, transposed: image[n = input feature][k = output feature]
    for (int u = tid; u < TOK_D * TF_FF; u += TB_THREADS) {
      w2t[(u & 127) * TF_LDX + (u >> 7)] = P[ly.o_w2 + u];            // linear2.weight [32][128]
      w1t[(u & 31) * TF_LDZ + (u >> 5)] = P[ly.o_w1 + u];             // linear1.weight [128][32]
    }
    for (int u = tid; u < TOK_D * TOK_D; u += TB_THREADS) wot[(u & 31) * TF_LDX + (u >> 5)] = P[ly.o_ow + u];
    for (int u = tid; u < 3 * TOK_D * TOK_D; u += TB_THREADS) wit[(u & 31) * TB_LDW + (u >> 5)] = P[ly.o_inw + u];
    // ---- 1. dff = mask_ff(dres); db2
    {
      const Drop dr = make_drop(a.p, a.seed, 4 * l + SITE_FF);
      float sb = 0.f;
      for (int row = hw; row < nrows; row += TB_HW) {
        const float v = drop_apply(dr, (unsigned int)((r0 + row) * TOK_D + f), bg[row * TF_LDX + f]);
        bd[row * TF_LDX + f] = v;
        sb += v;
      }
      put32(0, sb);
    }
    stage(A + ly.a_h, TF_FF, ba, TF_LDZ);
    __syncthreads();
    sum32(0, G + ly.o_b2);
    // ---- 2. dW2 = dff^T h; dh = dff W2
    wgrad(bd, TF_LDX, TOK_D, ba, TF_LDZ, TF_FF, G + ly.o_w2);
    dgrad(bd, TF_LDX, TOK_D, w2t, TF_LDX, TF_FF, bw, TF_LDZ);
    __syncthreads();
    stage(A + ly.a_z, TF_FF, ba, TF_LDZ);
    __syncthreads();
    // ---- 3. dz = mask_act(dh) gelu'(z); db1
    {
      const Drop dr = make_drop(a.p, a.seed, 4 * l + SITE_FF_ACT);
      const int c = tid & 127;
      float sb = 0.f;
      for (int row = tid >> 7; row < nrows; row += TB_THREADS / 128) {
        const float gd = gelu_grad(ba[row * TF_LDZ + c]);
        const float v = drop_apply(dr, (unsigned int)((r0 + row) * TF_FF + c), bw[row * TF_LDZ + c]) * gd;
        bw[row * TF_LDZ + c] = v;
        sb += v;
      }
      red[tid] = sb;
    }
    __syncthreads();
    if (tid < TF_FF) {
      float t = red[tid];
#pragma unroll
      for (int q = 1; q < TB_THREADS / 128; ++q) t += red[128 * q + tid];
      G[ly.o_b1 + tid] = t;
    }
    stage(A + ly.a_xn2, TOK_D, ba, TF_LDZ);
    __syncthreads();
    // ---- 4. dW1 = dz^T xn2; dxn2 = dz W1
    wgrad(bw, TF_LDZ, TF_FF, ba, TF_LDZ, TOK_D, G + ly.o_w1);
    dgrad(bw, TF_LDZ, TF_FF, w1t, TF_LDZ, TOK_D, bd, TF_LDX);
    __syncthreads();
    // ---- 5. LayerNorm 2 backward + residual: dx1; dsa = mask_sa(dx1); d(norm2), d(out_proj.bias)
    {
      const Drop dr = make_drop(a.p, a.seed, 4 * l + SITE_SA);
      const float gm = P[ly.o_n2w + f];
      float sg = 0.f, sb = 0.f, so = 0.f;
      for (int row = hw; row < nrows; row += TB_HW) {
        const long long i = (r0 + row) * TOK_D + f;
        const float v = ln_bwd(bd[row * TF_LDX + f], A[ly.a_x1 + i], A[ly.a_st2 + 2 * (r0 + row)], A[ly.a_st2 + 2 * (r0 + row) + 1], gm,
                               bg[row * TF_LDX + f], sg, sb);
        bg[row * TF_LDX + f] = v;
        const float ds = drop_apply(dr, (unsigned int)i, v);
        bd[row * TF_LDX + f] = ds;
        so += ds;
      }
      put32(0, sg); put32(1, sb); put32(2, so);
    }
    stage(A + ly.a_ctx, TOK_D, ba, TF_LDZ);
    __syncthreads();
    sum32(0, G + ly.o_n2w); sum32(1, G + ly.o_n2b); sum32(2, G + ly.o_ob);
    // ---- 6. dWo = dsa^T ctx; dctx = dsa Wo
    wgrad(bd, TF_LDX, TOK_D, ba, TF_LDZ, TOK_D, G + ly.o_ow);
    dgrad(bd, TF_LDX, TOK_D, wot, TF_LDX, TOK_D, bw, TF_LDZ);
    __syncthreads();
    // ---- 7. attention backward: dqkv -> ba; d(in_proj.bias).  The one place that restates token_math.h's attn_bwd instead of
    // calling it: through the routine k_token_bwd<4> allocates 238 VGPRs, written out 236 (its figure before the routines
    // existed; 256 is the ceiling).  Keep the two in step: tests/test_gpu_token_encoder_bits.py pins both.
    {
      const Drop dr = make_drop(a.p, a.seed, 4 * l + SITE_ATTN);
      const int dl = tid & 15, slot = tid >> 4;          // slot parity = head (H == 2)
      const int nsamp = nrows / S;
      float sq = 0.f, sk = 0.f, sv = 0.f;
      for (int g = slot; g < nsamp * a.H; g += TB_THREADS / 16) {
        const int bl = g / a.H, hh = g - bl * a.H;
        const long long gg = (r0 / S + bl) * a.H + hh;
        float q[S], k[S], v[S], dc[S], dq[S], dk[S], dv[S];
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
          const float* row = A + ly.a_qkv + (r0 + bl * S + s2) * (3 * TOK_D) + hh * TOK_DH + dl;
          q[s2] = row[0]; k[s2] = row[TOK_D]; v[s2] = row[2 * TOK_D];
          dc[s2] = bw[(bl * S + s2) * TF_LDZ + hh * TOK_DH + dl];
        }
        const float scale = 0.25f;
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) { dq[s2] = 0.f; dk[s2] = 0.f; dv[s2] = 0.f; }
#pragma unroll
        for (int i = 0; i < S; ++i) {
          float pr[S], mx = -INFINITY;
#pragma unroll
          for (int j = 0; j < S; ++j) { pr[j] = row16_sum(q[i] * k[j]) * scale; mx = fmaxf(mx, pr[j]); }
          float den = 0.f;
#pragma unroll
          for (int j = 0; j < S; ++j) { pr[j] = __expf(pr[j] - mx); den += pr[j]; }
          const float inv = 1.0f / den;
          float dp[S], dot = 0.f;
#pragma unroll
          for (int j = 0; j < S; ++j) {
            pr[j] *= inv;
            const float m = drop_apply(dr, (unsigned int)((gg * S + i) * S + j), 1.0f);
            dv[j] += pr[j] * m * dc[i];
            dp[j] = row16_sum(dc[i] * v[j]) * m;
            dot += dp[j] * pr[j];
          }
#pragma unroll
          for (int j = 0; j < S; ++j) {
            const float ds = pr[j] * (dp[j] - dot) * scale;
            dq[i] += ds * k[j];
            dk[j] += ds * q[i];
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < S; ++s2) {
          float* row = ba + (bl * S + s2) * TF_LDZ + hh * TOK_DH + dl;
          row[0] = dq[s2]; row[TOK_D] = dk[s2]; row[2 * TOK_D] = dv[s2];
          sq += dq[s2]; sk += dk[s2]; sv += dv[s2];
        }
      }
      red[slot * 16 + dl] = sq; red[TB_THREADS + slot * 16 + dl] = sk; red[2 * TB_THREADS + slot * 16 + dl] = sv;
    }
    __syncthreads();
    if (tid < 3 * TOK_D) {
      const int which = tid >> 5, c = tid & 31, hh = c >> 4, dl = c & 15;
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < TB_THREADS / 32; ++q) t += red[TB_THREADS * which + (2 * q + hh) * 16 + dl];   // the slots of head hh, in order
      G[ly.o_inb + tid] = t;
    }
    stage(A + ly.a_xn1, TOK_D, bw, TF_LDZ);
    __syncthreads();
    // ---- 8. dWin = dqkv^T xn1; dxn1 = dqkv Win
    wgrad(ba, TF_LDZ, 3 * TOK_D, bw, TF_LDZ, TOK_D, G + ly.o_inw);
    dgrad(ba, TF_LDZ, 3 * TOK_D, wit, TB_LDW, TOK_D, bd, TF_LDX);
    __syncthreads();
    // ---- 9. LayerNorm 1 backward + residual: the gradient of this layer's input; d(norm1)
    {
      const float gm = P[ly.o_n1w + f];
      float sg = 0.f, sb = 0.f;
      for (int row = hw; row < nrows; row += TB_HW) {
        const long long i = (r0 + row) * TOK_D + f;
        bg[row * TF_LDX + f] = ln_bwd(bd[row * TF_LDX + f], A[ly.a_x + i], A[ly.a_st1 + 2 * (r0 + row)], A[ly.a_st1 + 2 * (r0 + row) + 1],
                                      gm, bg[row * TF_LDX + f], sg, sb);
      }
      put32(0, sg); put32(1, sb);
    }
    __syncthreads();
    sum32(0, G + ly.o_n1w); sum32(1, G + ly.o_n1b);
    // (the next layer's first pass reads bg rows this thread wrote and writes red slot 0 after its weights loop; the
    //  sums above read red: one more barrier keeps them apart)
    __syncthreads();
  }
  for (int row = hw; row < nrows; row += TB_HW) a.dx[(r0 + row) * TOK_D + f] = bg[row * TF_LDX + f];
}

constexpr int TB_FUSED_MAX_S = 4;   // tokens per sample the one-launch backward takes (tests/test_host_api.py guards its registers)

static inline bool token_bwd_fused_enabled() {
  const char* e = getenv("IGI_TOKEN_FUSED_BWD");   // read per call (one call per backward pass): A/B and the parity test
  return !e || atoi(e) != 0;
}

static int token_backward(const igi_token_cfg* c, const float* dy, const float* params, float* dx, float* grads,
                          void* workspace, size_t workspace_bytes, unsigned long long seed, hipStream_t s) {
  TokenPlan p;
  int rc = make_token_plan(c, &p);
  if (rc) return rc;
  if (!dy || !params || !dx || !grads || !workspace) return IGI_E_BADARG;
  if (workspace_bytes < p.total_bytes) return IGI_E_WORKSPACE;
  float* W = tok_ws(workspace);
  const TokLayout& ly = p.lay;
  // (S <= TB_FUSED_MAX_S: with five or more tokens per sample the attention pass of k_token_bwd holds more than 256 registers
  //  -- 88 to 940 bytes of scratch per lane in the S = 5 .. 8 instantiations -- so those run the launch-per-operation
  //  backward below, which does not spill; the instantiations are not built)
  if (token_bwd_fused_enabled() && p.S <= TB_FUSED_MAX_S && p.bwd_grid > 0 && p.ff == TF_FF && p.narrow && !bf16_mode() &&
      ((ly.a_layer | ly.a_xn1 | ly.a_ctx | ly.a_xn2 | ly.a_h | ly.a_z) & 3) == 0) {
    TokBwdArgs a;
    a.dy = dy; a.params = params; a.dx = dx; a.W = W; a.part = W + p.s_part;
    a.R = p.R; a.lay = ly; a.P = ly.per_layer * p.L;
    a.S = p.S; a.H = p.H; a.L = p.L; a.p = p.p; a.seed = seed;
    a.rows_per_wg = p.bwd_samples * p.S;
    rc = attn_dispatch(p.S, [&](auto sc) {
      constexpr int SS = decltype(sc)::value;
      if constexpr (SS <= TB_FUSED_MAX_S)
        tok_launch_lds<k_token_bwd<SS>>(p.bwd_grid, TB_THREADS, sizeof(float) * TB_LDS_FLOATS, s, a);
    });
    if (rc) return rc;
    SegTable t;
    t.n = 1;
    t.wide = 1;
    Segment& sg = t.s[0];
    sg.dst = 0; sg.src = a.part; sg.stride = a.P; sg.count = (int)a.P; sg.cols = (int)a.P; sg.src_ld = 0; sg.nparts = p.bwd_grid;
    hipLaunchKernelGGL(k_slab_reduce, dim3(SLAB_GX, 1), dim3(RED_THREADS), 0, s, t, grads);
    return (int)hipGetLastError();
  }
  const long long R = p.R;
  const int d = p.d, ff = p.ff;
  float* g0 = W + p.s_g0;
  float* g1 = W + p.s_g1;
  float* rA = W + p.s_rA;   // residual-stream gradient entering a layer from above
  float* rB = W + p.s_rB;   // residual-stream gradient between the two blocks of a layer
  float* w0 = W + p.s_wide0;
  float* w1 = W + p.s_wide1;
  const bool tile = p.S > TOK_MAX_S || !p.narrow;
  auto ln_bwd_launch = [&](const float* dxn, const float* x, const float* stats, const float* gamma, const float* dres_, float* dx_,
                           const Drop& dr, float* dmask, float* part) {
    return width_dispatch(d, [&](auto dc) {
      hipLaunchKernelGGL(k_ln_bwd<decltype(dc)::value>, dim3(p.ln_blocks), dim3(256), 0, s, dxn, x, stats, gamma, dres_, dx_, dr,
                         dmask, part, R);
    });
  };
  // the sums of every split-row partial of this pass (eight Linears x (weight, bias), four layer norms) are queued and
  // run as ONE launch at the end: each producer therefore keeps its own partial buffer
  SplitSumTable sums;
  int n_lin = 0, n_ln = 0;
  auto lin_ws_next = [&]() { return (void*)(reinterpret_cast<char*>(W + p.s_lin) + (size_t)(n_lin++) * p.lin_bytes); };
  auto lnpart_next = [&]() { return W + p.s_lnpart + (long long)(n_ln++) * p.ln_blocks * 2 * d; };
  const float* dres = dy;   // gradient w.r.t. the current residual stream
  const float* dbr;         // gradient w.r.t. the branch output feeding it (after the dropout mask)
  // top: branch gradient = drop_mask(dy) with the last layer's ff site
  if (p.p > 0.f) {
    hipLaunchKernelGGL(k_drop_copy, dim3(tok_blocks(R * d, 256)), dim3(256), 0, s, dy, g1,
                       make_drop(p.p, seed, 4 * (p.L - 1) + SITE_FF), R * d);
    dbr = g1;
  } else {
    dbr = dy;
  }
  for (int l = p.L - 1; l >= 0; --l) {
    const float* P = params + (long long)l * ly.per_layer;
    float* G = grads + (long long)l * ly.per_layer;
    float* A = W + (long long)l * ly.a_layer;
    // ---- ff block: f = linear2(h)
    if ((rc = linear_backward(A + ly.a_h, ff, P + ly.o_w2, nullptr, 0, dbr, d, w0, ff, G + ly.o_w2, G + ly.o_b2, R, ff, d,
                              LIN_NONE, lin_ws_next(), p.lin_bytes, s, &sums)))
      return rc;
    hipLaunchKernelGGL(k_gelu_bwd, dim3(tok_blocks(R * ff, 256)), dim3(256), 0, s, w0, A + ly.a_z, w1,
                       make_drop(p.p, seed, 4 * l + SITE_FF_ACT), R * ff);
    if ((rc = linear_backward(A + ly.a_xn2, d, P + ly.o_w1, nullptr, 0, w1, ff, g0, d, G + ly.o_w1, G + ly.o_b1, R, d, ff,
                              LIN_NONE, lin_ws_next(), p.lin_bytes, s, &sums)))
      return rc;
    // ---- LN2 backward + residual: dx1 and its masked copy for the sa branch (g1)
    float* dx1 = rB;
    float* lnpart = lnpart_next();
    if ((rc = ln_bwd_launch(g0, A + ly.a_x1, A + ly.a_st2, P + ly.o_n2w, dres, dx1, make_drop(p.p, seed, 4 * l + SITE_SA),
                            p.p > 0.f ? g1 : (float*)nullptr, lnpart)))
      return rc;
    // norm2.weight and norm2.bias are adjacent
    if (!split_sum_defer(sums, G + ly.o_n2w, lnpart, 2LL * d, 2LL * d, p.ln_blocks))
      split_sum(G + ly.o_n2w, lnpart, 2LL * d, p.ln_blocks, 2LL * d, s);
    const float* da = p.p > 0.f ? g1 : dx1;
    // ---- sa block: a = out_proj(ctx)
    if ((rc = linear_backward(A + ly.a_ctx, d, P + ly.o_ow, nullptr, 0, da, d, g0, d, G + ly.o_ow, G + ly.o_ob, R, d, d,
                              LIN_NONE, lin_ws_next(), p.lin_bytes, s, &sums)))
      return rc;
    const long long pairs = (long long)p.B * p.H;
    const Drop datt = make_drop(p.p, seed, 4 * l + SITE_ATTN);
    if (tile) {
      ProfScope ps(PC_ATTN_TILE_BWD, s, 12.0 * pairs * p.S * p.S * p.dh, 4.0 * R * (7.0 * d));
      rc = tile_dispatch(p.dh, d, [&](auto hc, auto mc) {
        IGI_LAUNCH((k_attn_tile_bwd<decltype(hc)::value, decltype(mc)::value>), dim3(tok_blocks(pairs, AT_THREADS / 64)),
                   dim3(AT_THREADS), 0, s, A + ly.a_qkv, g0, w1, datt, pairs, p.H, p.S);
      });
      if (rc) return rc;
    } else {
      rc = attn_dispatch(p.S, [&](auto sc) {
        constexpr int SS = decltype(sc)::value;
        hipLaunchKernelGGL((k_attn_bwd<SS>), dim3(tok_blocks(pairs, 16)), dim3(256), 0, s, A + ly.a_qkv, g0, w1, datt,
                           pairs, p.H);
      });
      if (rc) return rc;
    }
    if ((rc = linear_backward(A + ly.a_xn1, d, P + ly.o_inw, nullptr, 0, w1, 3 * d, g0, d, G + ly.o_inw, G + ly.o_inb, R, d,
                              3 * d, LIN_NONE, lin_ws_next(), p.lin_bytes, s, &sums)))
      return rc;
    // ---- LN1 backward + residual: gradient of this layer's input; masked copy for the ff branch of l-1
    float* dxl = (l == 0) ? dx : rA;
    const bool mask_below = (l > 0) && p.p > 0.f;
    lnpart = lnpart_next();
    if ((rc = ln_bwd_launch(g0, A + ly.a_x, A + ly.a_st1, P + ly.o_n1w, dx1, dxl, make_drop(p.p, seed, 4 * (l - 1) + SITE_FF),
                            mask_below ? g1 : (float*)nullptr, lnpart)))
      return rc;
    // norm1.weight and norm1.bias are adjacent
    if (!split_sum_defer(sums, G + ly.o_n1w, lnpart, 2LL * d, 2LL * d, p.ln_blocks))
      split_sum(G + ly.o_n1w, lnpart, 2LL * d, p.ln_blocks, 2LL * d, s);
    dres = dxl;
    dbr = mask_below ? g1 : dxl;
  }
  split_sum_flush(sums, s);
  return (int)hipGetLastError();
}

}  // namespace igi
