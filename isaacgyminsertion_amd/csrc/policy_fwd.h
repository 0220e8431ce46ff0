// The rollout-side policy step as ONE persistent kernel per 32 environments (frozen_ppo.py:343-366 `model_act` +
// :655-665 of `play_steps`; models_split.py:120-164 `act` = env_mlp -> [obs | latent] -> actor / critic trunks -> heads
// -> Normal sample), for the reference's network shape (priv 64 -> 256 -> 128 -> 8, [obs 15 | latent 8] -> 512 -> 256 -> 128,
// <= 7 actions), with or without ground-truth contacts (below).  Other shapes keep the layer-by-layer launches (teacher.h,
// teacher_policy_step).
//
// Why: at 4096 environments the layer-by-layer step is seven dependent launches of 64 - 256 workgroups, 80 us for 3.4
// GFLOP (25 us of matrix pipe) -- every launch pays its fill, first DMA round trip, epilogue and drain with nothing to
// overlap them, and the activations go out to HBM and come back between launches.  Round 5 tried the 32-row chain kernel of
// the student's MLPs (register-staged weights, two barriers per 64-wide chunk): 103 us, a chain of global -> register ->
// LDS round trips.
//
// Shape of this kernel:
//  * a workgroup = 32 environments x ONE net (blockIdx & 1: actor | critic); both kinds run the small env_mlp for their
//    rows (22 % of a workgroup's work, twice) so that the 0.7 MB of trunk weights a workgroup streams are one net's, and
//    256 workgroups fill the chip at 4096 environments;
//  * every activation of the 32 rows stays in LDS as k-contiguous XOR-swizzled [32][32] images (the operand layout of
//    gemm_dma.h / env_mlp.h): 32 + 64 KB in two regions that the layers alternate between, nothing goes to HBM;
//  * weights are streamed by LDS-DMA in [32 outputs][16 k] chunks (2 KB) through WAVE-PRIVATE three-deep rings: wave w owns
//    output-column tile(s) w (+ 8) of the layer, requests chunk i + 2, waits (counted vmcnt) for chunk i + 1, reads its
//    fragments, and issues the eight MFMAs of chunk i -- no workgroup barrier inside a layer, one between layers;
//  * v_mfma_f32_32x32x2_f32, k order = the GEMM kernels' (k-tiles in order, pairs k, k + 4 inside every group of eight),
//    bias + tanh exactly as their epilogue: the trunk outputs are bit-identical to the per-layer launches; the 8-wide latent
//    layer and the heads are VALU dot products in another summation order (fp32 rounding apart);
//  * the heads, the Normal sample from the caller's noise, neglogp, the value de-normalisation and the seven arena writes
//    (k_heads_act_store's arithmetic) close the kernel: 2 launches per policy step (k_policy_stage + this).
//
// Contact mode (template parameter CT; the teacher with ground-truth contacts, models_split.py:166-183): xcat =
// [obs | latent 8 | embedding E] (PF_CONTACTS) or [obs | embedding 8] (PF_ONLY_CONTACT, no env_mlp), at most 32 columns.
// The encoder of contact.h runs for the block's 32 rows before env_mlp, both products on exact-fp32 MFMA:
//  * H = relu(C . W1^T + b1), C = [32][P], P a run-time value: the P / 32 k-chunks are dealt to the eight waves (wave w takes
//    chunks w, w + 8, ...; 13 chunks at P = 400), straight from global memory into the MFMA operands (float4 loads when every
//    row is 16-byte aligned, VEC; scalar loads with a column guard otherwise); the eight partial 32 x 32 tiles meet in LDS
//    and are added in WAVE ORDER (((p0 + p1) + p2) + ... + p7) by all 512 threads -- a fixed order, no atomics, so the step is
//    bit-reproducible; k_contact_fwd adds the same chunks one after the other, so the two agree at fp32 rounding only;
//  * emb = tanh(H . W2^T + b2) on one wave with H as the B operand in its accumulator layout: wave 7, while waves 0 - 3
//    compute the 128-wide env layer (waves 4 - 7 own no tile of it); wave 0 with only_contact;
//  * LDS: nothing is added.  The partials (32 KB) and the embedding (4 KB) sit in images 4 - 11 and 15 of region Q, which
//    hold nothing between the input images (0, 1) / env layer 2's output (0 - 3) and the first trunk layer's output;
//  * the actor workgroups store the contact values they loaded to the step's slot of the (T, N, P) arena (the raw contacts,
//    bit for bit: frozen_ppo.py:663-664) -- no copy is launched;
//  * the xcat image is written whole: columns >= xw as zeros.
// The instantiation without contacts is the kernel as it was (same registers, same bits).
#pragma once
#include "contact.h"
#include "dma_util.h"
#include "gemm_f32.h"

namespace igi {

struct PolicyFwdArgs {
  const float* priv; int ldp;          // [rows][64] normalised privileged input (k_policy_stage)
  const float* xcat; int ldx;          // [rows][32]: normalised obs in columns 0 .. obs - 1, zeros behind obs + 8
  int rows, obs, act;
  const float *eW1, *eb1, *eW2, *eb2, *eW3, *eb3;      // env_mlp: [256][64], [128][256], [8][128]
  const float* w1p;                                    // [2][512][32] zero-padded first trunk layer (k_policy_stage refreshes it)
  const float *tb1, *tW2, *tb2, *tW3, *tb3;            // actor trunk; critic = + ac_block floats
  long long ac_block;
  const float *Wmu, *bmu, *Wv, *bv, *logstd;
  // sampling + arena (the arguments of k_heads_act_store)
  const float* noise; const double* rms_value; float eps;
  float *actions_t, *nlp_t, *values_t, *mus_t, *sigmas_t, *actions_clamped, *values_out;
  // contact mode (PF_CONTACTS / PF_ONLY_CONTACT): the step's raw contacts [rows][ctP], their arena slot (may be NULL), the
  // encoder of contact.h (W1 [32][ctP], b1 [32], W2 [ctE][32], b2 [ctE]) and the live width of xcat
  const float* ct = nullptr; float* ct_t = nullptr; int ctP = 0, ctE = 0, xw = 0;
  const float *cW1 = nullptr, *cb1 = nullptr, *cW2 = nullptr, *cb2 = nullptr;
};

// what sits behind the observation in xcat: [latent 8] | [latent 8 | embedding ctE] | [embedding 8]
constexpr int PF_NO_CONTACTS = 0, PF_CONTACTS = 1, PF_ONLY_CONTACT = 2;

constexpr int PF_ROWS = 32;
constexpr int PF_THREADS = 512;
constexpr int PF_IMG = 32 * 32;                 // one [32 rows][32 k] activation image (floats)
constexpr int PF_P = 8 * PF_IMG;                // region P: layer-1 output (8 images), xcat, trunk-2 output
constexpr int PF_Q = 16 * PF_IMG;               // region Q: input (2), env layer 2 (4), trunk-1 output (16), trunk-3 output (4)
constexpr int PF_CH = 32 * 16;                  // one weight chunk [32 outputs][16 k]
constexpr int PF_NS = 3;                        // ring depth per wave
constexpr int PF_RING = 8 * PF_NS * PF_CH;
constexpr int PF_SMALL = 8 * 128 /* W3 */ + 8 * 128 /* head rows: mu 0.., value 7 */ + 2 * 32 * 8 /* partial dots */ + 32 * 8 /* latent | mu */;
constexpr int PF_LDS_FLOATS = PF_P + PF_Q + PF_RING + PF_SMALL;
// contact phase: images of Q that neither the privileged input (0, 1) nor env layer 2's output (0 .. 3) touches
constexpr int PF_CT_PART = 4 * PF_IMG;          // Q + this: [8 waves][16 registers][64 lanes] partial tiles (8 images); H in slot 0
constexpr int PF_CT_EMB = 15 * PF_IMG;          // Q + this: [32 rows][32] embedding, until xcat is built
static_assert(PF_CT_PART >= 4 * PF_IMG && PF_CT_PART + 8 * PF_IMG <= PF_CT_EMB && PF_CT_EMB + PF_IMG <= PF_Q, "contact phase in Q");
static_assert(PF_LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
constexpr float PF_LOG_SQRT_2PI = 0.918938533204672741780329736406f;

// xw: the live width of xcat = obs + 8 (+ embedding), or obs + embedding with only_contact
static inline bool policy_fwd_shape_ok(int obs, int priv, int act, int npl, const int* pu, int nl, const int* u, int xw) {
  return priv == 64 && npl == 3 && pu[0] == 256 && pu[1] == 128 && pu[2] == 8 && nl == 3 && u[0] == 512 && u[1] == 256 &&
         u[2] == 128 && obs >= 1 && xw > obs && xw <= 32 && act >= 1 && act <= 7;
}

// float index of accumulator element r of a lane in a k-contiguous swizzled [32][32] image: see env_img_bases (env_mlp.h)
__device__ __forceinline__ void pf_img_bases(int l31, int h, int (&ib)[4]) {
  const int sk[4] = {0, 1, 4, 5};
#pragma unroll
  for (int k = 0; k < 4; ++k) ib[k] = (4 * h * 8 + ((l31 >> 2) ^ (sk[k] + 2 * h))) * 4 + (l31 & 3);
}

template <int I, int N, class F>
__device__ __forceinline__ void pf_for(F& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    pf_for<I + 1, N>(f);
  }
}

// s_waitcnt vmcnt(N) with N a compile-time constant
template <int N>
__device__ __forceinline__ void pf_wait_vm() {
  static_assert(N >= 0 && N <= 12, "vmcnt immediates of the ring depths in use");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if constexpr (N == 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
  static_assert((N & 1) == 0, "two requests per chunk");
}

struct PfWave {
  float* ring;                 // this wave's PF_NS chunks
  int l31, h, lane, wave;
  int ib[4];
  int aoff;                    // float offset of this lane's row in an activation image: l31 * 32
  int asw;                     // (l31 >> 1) & 7
  int boff, bsw;               // chunk: l31 * 16, (l31 >> 2) & 3
};

// One Linear + Tanh layer of the block: out[32][N] = tanh(in[32][K] . W[N][K]^T + b) for THIS wave's output-column tiles
// n = wave + NW j (j < NT); waves whose first tile lies beyond N / 32 skip the layer.  `ain`: K / 32 input images;
// `aout`: N / 32 output images (another LDS region); W rows ldw floats apart.  The caller puts a workgroup barrier behind.
// NW: the waves that compute (waves 0 .. NW - 1 own tiles wave + NW j); the others return at once.
// NS: depth of the wave's ring (NS - 1 chunks in flight ahead of the one being multiplied).
// STORE (k_actor_latent's training forward): the wave also writes its output tiles, from the accumulators, to the row-major
// `gout` (rows ldg floats apart; block row 0 = row m0), rows below `rows` only.  Those stores count in vmcnt like the ring's
// requests: a later layer's counted wait can only wait longer for them, never too short (loads return in order).
template <int K, int N, int NT, int NW = 8, int NS = PF_NS, bool STORE = false>
__device__ __forceinline__ void pf_layer(const PfWave& w, const float* __restrict__ ain, const float* __restrict__ W, int ldw,
                                         const float (&bias)[NT], float* __restrict__ aout, float* __restrict__ gout = nullptr,
                                         int ldg = 0, int m0 = 0, int rows = 0) {
  constexpr int KC = K / 16, NI = KC * NT;       // items = (k-chunk c, tile j), c-major
  static_assert(K % 32 == 0 && N % 32 == 0, "whole images");
  static_assert(NT * NW * 32 >= N, "every output tile has an owner");
  if (w.wave >= NW || w.wave * 32 >= N) return;
  // the lane's two 16-byte pieces of a chunk request: DMA instruction i covers rows 16 i .. 16 i + 15, four pieces per row;
  // piece slot s of row r holds k-piece s ^ ((r >> 2) & 3) (so that the fragments' ds_read_b128 are conflict-free)
  unsigned goff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int r = 16 * i + (w.lane >> 2), p = (w.lane & 3) ^ ((r >> 2) & 3);
    goff[i] = 4u * ((unsigned)r * (unsigned)ldw + 4u * (unsigned)p);
  }
  auto issue = [&](auto item_c) {
    constexpr int I = decltype(item_c)::value;
    constexpr int c = I / NT, j = I % NT;
    float* dst = w.ring + (I % NS) * PF_CH;
    const char* base = reinterpret_cast<const char*>(uniform_ptr(W + (long long)(32 * (w.wave + NW * j)) * ldw + 16 * c));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      asm volatile("" : "+v"(goff[i]));
      dma16(reinterpret_cast<const float*>(base + goff[i]), dst + 256 * i);
    }
  };
  struct Frag { f32x4 a[2], b[2]; };
  auto read = [&](auto item_c, Frag& f) {
    constexpr int I = decltype(item_c)::value;
    constexpr int c = I / NT;
    const float* ch = w.ring + (I % NS) * PF_CH;
    const float* img = ain + (c >> 1) * PF_IMG;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int g8 = 2 * (c & 1) + g;
      f.a[g] = *reinterpret_cast<const f32x4*>(img + w.aoff + (((2 * g8 + w.h) ^ w.asw) << 2));
      f.b[g] = *reinterpret_cast<const f32x4*>(ch + w.boff + (((2 * g + w.h) ^ w.bsw) << 2));
    }
  };
  f32x16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  Frag fr[2];
  constexpr int D = NS - 1;                      // chunks in flight
  constexpr int PRO = D < NI ? D : NI;
  auto prologue = [&](auto item_c) { issue(item_c); };
  pf_for<0, PRO>(prologue);
  pf_wait_vm<2 * (PRO - 1)>();                   // item 0 has landed once only the younger requests are outstanding
  read(std::integral_constant<int, 0>{}, fr[0]);
  auto step = [&](auto item_c) {
    constexpr int I = decltype(item_c)::value;
    if constexpr (I + D < NI) issue(std::integral_constant<int, (I + D < NI ? I + D : 0)>{});
    if constexpr (I + 1 < NI) {
      // item I + 1 has landed once only the requests of the items behind it (two instructions each) are outstanding
      constexpr int last = (I + D < NI - 1) ? I + D : NI - 1;
      pf_wait_vm<2 * (last - (I + 1))>();
      read(std::integral_constant<int, (I + 1 < NI ? I + 1 : 0)>{}, fr[(I + 1) & 1]);
    }
    __builtin_amdgcn_sched_barrier(0);
    const Frag& f = fr[I & 1];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        acc[I % NT] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[g][q], f.b[g][q], acc[I % NT], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  };
  // (fully unrolled: ring slots, image addresses and the vmcnt immediates are compile-time constants)
  pf_for<0, NI>(step);
  // bias + tanh into the next layer's operand images
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    float* img = aout + (w.wave + NW * j) * PF_IMG;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float v = fast_tanh(acc[j][r] + bias[j]);
      img[w.ib[(r >> 1) & 3] + ((r & 3) + 8 * (r >> 2)) * 32] = v;
      if constexpr (STORE) {   // accumulator element r of lane (l31, h): row 4 h + (r & 3) + 8 (r >> 2), column l31 of the tile
        const int row = m0 + 4 * w.h + (r & 3) + 8 * (r >> 2);
        if (row < rows) gout[(long long)row * ldg + 32 * (w.wave + NW * j) + w.l31] = v;
      }
    }
  }
}

// dot products of the block's 32 rows (images at `img`, 4 of them = 128 k) with the eight 128-wide rows at `wrows`:
// thread (row = tid & 31, out = (tid >> 5) & 7, half = tid >> 8) sums its 64 k; the halves meet in `part`.
__device__ __forceinline__ void pf_dot8(const float* __restrict__ img, const float* __restrict__ wrows, float* __restrict__ part, int tid) {
  const int row = tid & 31, out = (tid >> 5) & 7, half = tid >> 8;
  const int sw = (row >> 1) & 7;
  float s = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t) {           // the half's two 32-k images
    const float* im = img + (2 * half + t) * PF_IMG + row * 32;
    const float* wr = wrows + out * 128 + (2 * half + t) * 32;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(im + ((p ^ sw) << 2));
      const f32x4 v = *reinterpret_cast<const f32x4*>(wr + 4 * p);
#pragma unroll
      for (int q = 0; q < 4; ++q) s = fmaf(x[q], v[q], s);
    }
  }
  part[(half * 32 + row) * 8 + out] = s;
}

// ---- contact phase (contact.h's encoder for the block's 32 rows) ----------------------------------------------------
// First product, transposed as in k_contact_fwd (Z1^T = W1 . C^T: the row on the lane, the 32 hidden units in the
// registers), with the k-chunks of 32 contact points dealt to the eight waves: wave w multiplies chunks w, w + 8, ... and
// leaves its partial tile at part[w][register][lane] (waves without a chunk leave zeros).  Rows >= rows and columns >= P
// contribute zeros.  store: this workgroup also writes what it loaded to the arena slot, bit for bit.
template <bool VEC>
__device__ __forceinline__ void pf_contact_partial(const PolicyFwdArgs& a, const PfWave& w, int m0, bool store, float* __restrict__ part) {
  const int P = a.ctP, nch = (P + 31) >> 5;
  const int grow = m0 + w.l31;
  const bool valid = grow < a.rows;
  const float* crow = a.ct + (long long)(valid ? grow : 0) * P;
  const float* wrow = a.cW1 + (long long)w.l31 * P;          // hidden unit l31
  float* trow = a.ct_t + (long long)(valid ? grow : 0) * P;
  store = store && valid && a.ct_t != nullptr;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  for (int c = w.wave; c < nch; c += 8) {
    const int k0 = 32 * c + 16 * w.h;                         // lane half h: columns k0 .. k0 + 15 of its row of C and of W1
    float cv[16], wv[16];
    if (VEC && k0 + 16 <= P) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 c4 = valid ? *reinterpret_cast<const float4*>(crow + k0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 w4 = *reinterpret_cast<const float4*>(wrow + k0 + 4 * q);
        if (store) *reinterpret_cast<float4*>(trow + k0 + 4 * q) = c4;
        cv[4 * q] = c4.x; cv[4 * q + 1] = c4.y; cv[4 * q + 2] = c4.z; cv[4 * q + 3] = c4.w;
        wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + u;
        cv[u] = (valid && k < P) ? crow[k] : 0.f;
        wv[u] = (k < P) ? wrow[k] : 0.f;
        if (store && k < P) trow[k] = cv[u];
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], cv[u], acc, 0, 0, 0);
  }
#pragma unroll
  for (int g = 0; g < 16; ++g) part[(w.wave * 16 + g) * 64 + w.lane] = acc[g];
}

// the eight partial tiles summed in wave order, + b1 (b1v: this thread's two elements), ReLU: H in slot 0 of `part`,
// in the accumulator layout [register][lane]
__device__ __forceinline__ void pf_contact_hidden(float* __restrict__ part, const float (&b1v)[2], int tid) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + PF_THREADS * i;
    float s = part[e];
#pragma unroll
    for (int v = 1; v < 8; ++v) s += part[v * 1024 + e];
    const float z1 = s + b1v[i];
    part[e] = z1 > 0.f ? z1 : 0.f;
  }
}

// second product on ONE wave, E^T = W2 . H^T with H as the B operand in its accumulator layout (k_contact_fwd), bias,
// tanh: emb[row][e]
__device__ __forceinline__ void pf_contact_emb(const PolicyFwdArgs& a, const float* __restrict__ hid, float* __restrict__ emb, int lane) {
  const int r = lane & 31, h = lane >> 5;
  float wv[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) wv[g] = r < a.ctE ? a.cW2[r * CT_HID + ct_acc_row(g, h)] : 0.f;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[g], hid[g * 64 + lane], acc, 0, 0, 0);
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const int e = ct_acc_row(g, h);
    if (e < a.ctE) emb[r * 32 + e] = tanhf(acc[g] + a.cb2[e]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the layers' counted waits see weight requests and nothing else
}

// CT: PF_NO_CONTACTS | PF_CONTACTS | PF_ONLY_CONTACT;  VEC: contact rows and W1 rows load (and store) as float4
template <int CT, bool VEC>
__global__ __launch_bounds__(PF_THREADS) void k_policy_fwd(const PolicyFwdArgs a) {
  extern __shared__ __attribute__((aligned(1024))) float smem[];
  float* P = smem;
  float* Q = P + PF_P;
  float* ring0 = Q + PF_Q;
  float* w3s = ring0 + PF_RING;          // [8][128] last env layer
  float* hws = w3s + 8 * 128;            // [8][128] head rows: mu 0 .. act - 1, value at row 7
  float* part = hws + 8 * 128;           // [2][32][8]
  float* lat = part + 2 * 32 * 8;        // [32][8]: latent, later mu
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int z = (int)blockIdx.x & 1, blk = (int)blockIdx.x >> 1;     // net (0 actor, 1 critic), row block
  const int m0 = blk * PF_ROWS;
  PfWave w;
  w.ring = ring0 + wave * (PF_NS * PF_CH);
  w.lane = lane; w.wave = wave; w.l31 = lane & 31; w.h = lane >> 5;
  pf_img_bases(w.l31, w.h, w.ib);
  w.aoff = w.l31 * 32; w.asw = (w.l31 >> 1) & 7;
  w.boff = w.l31 * 16; w.bsw = (w.l31 >> 2) & 3;
  const float* tb1 = a.tb1 + z * a.ac_block;
  const float* tW2 = a.tW2 + z * a.ac_block;
  const float* tb2 = a.tb2 + z * a.ac_block;
  const float* tW3 = a.tW3 + z * a.ac_block;
  const float* tb3 = a.tb3 + z * a.ac_block;
  const float* w1p = a.w1p + (long long)z * 512 * 32;

  // ---- everything a later phase would wait a round trip for, requested now
  const int c31 = 32 * wave + w.l31;
  float be1[1] = {a.eb1[c31]};
  float be2[1] = {a.eb2[min(c31, 127)]};
  float bt1[2] = {tb1[c31], tb1[256 + c31]};
  float bt2[1] = {tb2[c31]};
  float bt3[1] = {tb3[min(c31, 127)]};
  const int xrow = tid >> 4, xc = 2 * (tid & 15);                    // this thread's two xcat elements
  const float2 xv = *reinterpret_cast<const float2*>(a.xcat + (long long)min(m0 + xrow, a.rows - 1) * a.ldx + xc);
  float w3v[2], hwv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + PF_THREADS * i;                               // 0 .. 1023
    w3v[i] = a.eW3[e];
    const int r = e >> 7, k = e & 127;
    hwv[i] = r < a.act ? a.Wmu[r * 128 + k] : (r == 7 ? a.Wv[k] : 0.f);
  }
  if constexpr (CT != PF_ONLY_CONTACT) {  // the input block: two [32][32] images, four 1 KB pieces each, one per wave
    const int k = wave >> 2, i = wave & 3;
    const int m = 8 * i + (lane >> 3);
    const int row = min(m0 + m, a.rows - 1);
    dma16(a.priv + (long long)row * a.ldp + k * 32 + 4 * ((lane & 7) ^ ((m >> 1) & 7)), Q + k * PF_IMG + 256 * i);
  }
  float* cpart = Q + PF_CT_PART;
  float* cemb = Q + PF_CT_EMB;
  float cb1v[2] = {0.f, 0.f};
  if constexpr (CT != PF_NO_CONTACTS) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int e = tid + PF_THREADS * i;                             // element [register e >> 6][lane e & 63] of a tile
      cb1v[i] = a.cb1[ct_acc_row(e >> 6, (e >> 5) & 1)];
    }
    pf_contact_partial<VEC>(a, w, m0, z == 0, cpart);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) { w3s[tid + PF_THREADS * i] = w3v[i]; hws[tid + PF_THREADS * i] = hwv[i]; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if constexpr (CT != PF_NO_CONTACTS) pf_contact_hidden(cpart, cb1v, tid);
  if constexpr (CT == PF_ONLY_CONTACT) {
    // the privileged embedding is not used (models_split.py:176-178): no env_mlp, the embedding on wave 0
    __syncthreads();
    if (wave == 0) pf_contact_emb(a, cpart, cemb, lane);
  } else {
    // ---- env_mlp: 64 -> 256 (Q -> P), 256 -> 128 (P -> Q), 128 -> 8 (Q -> lat)
    pf_layer<64, 256, 1>(w, Q, a.eW1, 64, be1, P);
    __syncthreads();
    // (waves 4 .. 7 own no tile of the 128-wide layer: the last of them forms the contact embedding meanwhile)
    if constexpr (CT == PF_CONTACTS) { if (wave == 7) pf_contact_emb(a, cpart, cemb, lane); }
    pf_layer<256, 128, 1>(w, P, a.eW2, 256, be2, Q);
    __syncthreads();
    pf_dot8(Q, w3s, part, tid);
    __syncthreads();
    if (tid < 256) {
      const int row = tid & 31, out = tid >> 5;
      lat[row * 8 + out] = fast_tanh((part[row * 8 + out] + part[(32 + row) * 8 + out]) + a.eb3[out]);
    }
  }
  __syncthreads();
  // ---- xcat = [obs_n | latent | 0], [obs_n | latent | emb | 0] or [obs_n | emb | 0] as ONE image in P
  {
    const int sw = (xrow >> 1) & 7;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = xc + q;
      float v;
      if constexpr (CT == PF_NO_CONTACTS) {
        v = (c >= a.obs && c < a.obs + 8) ? lat[xrow * 8 + (c - a.obs)] : (q ? xv.y : xv.x);
      } else {
        // columns >= xw are written as zeros whatever the staged row holds behind them
        const int ec = a.obs + (CT == PF_CONTACTS ? 8 : 0);            // first embedding column
        if (c < a.obs) v = q ? xv.y : xv.x;
        else if (CT == PF_CONTACTS && c < ec) v = lat[xrow * 8 + (c - a.obs)];
        else v = c < a.xw ? cemb[xrow * 32 + (c - ec)] : 0.f;
      }
      P[xrow * 32 + (((c >> 2) ^ sw) << 2) + (c & 3)] = v;
    }
  }
  __syncthreads();
  // ---- trunk of net z: 32 -> 512 (P -> Q), 512 -> 256 (Q -> P), 256 -> 128 (P -> Q)
  pf_layer<32, 512, 2>(w, P, w1p, 32, bt1, Q);
  __syncthreads();
  pf_layer<512, 256, 1>(w, Q, tW2, 512, bt2, P);
  __syncthreads();
  pf_layer<256, 128, 1>(w, P, tW3, 256, bt3, Q);
  __syncthreads();
  // ---- heads: rows 0 .. act - 1 of hws = mu, row 7 = value
  pf_dot8(Q, hws, part, tid);
  __syncthreads();
  if (z == 0) {
    // thread (row, action q): k_heads_act_store's per-action arithmetic; the neglogp terms meet in action order
    const int row = tid & 31, q = tid >> 5, grow = m0 + row;
    if (tid < 256 && q < a.act && grow < a.rows) {
      const float m = (part[row * 8 + q] + part[(32 + row) * 8 + q]) + a.bmu[q];
      const float sig = expf(m * 0.f + a.logstd[q]);
      const long long ia = (long long)grow * a.act + q;
      const float av = m + sig * a.noise[ia];
      const float x = av - m;
      lat[row * 8 + q] = ((x * x) / (2.0f * (sig * sig)) + logf(sig)) + PF_LOG_SQRT_2PI;
      a.actions_t[ia] = av;
      a.mus_t[ia] = m;
      a.sigmas_t[ia] = sig;
      a.actions_clamped[ia] = fminf(fmaxf(av, -1.0f), 1.0f);
    }
    __syncthreads();
    if (tid < 32 && m0 + tid < a.rows) {
      float nlp = 0.f;
      for (int k = 0; k < a.act; ++k) nlp += lat[tid * 8 + k];
      a.nlp_t[m0 + tid] = nlp;
    }
  } else if (tid < 32 && m0 + tid < a.rows) {
    const int row = tid, grow = m0 + row;
    float v = (part[row * 8 + 7] + part[(32 + row) * 8 + 7]) + a.bv[0];
    if (a.rms_value) {
      const float vm = (float)a.rms_value[0], vd = sqrtf((float)a.rms_value[1] + a.eps);
      v = vd * fminf(fmaxf(v, -5.0f), 5.0f) + vm;
    }
    a.values_t[grow] = v;
    a.values_out[grow] = v;
  }
}

// ---- the frozen ACTOR on [obs | student latent] (models_split.py:187-216 with a `latent` entry; ext_adapt.py:684-690,
// 799-806): one workgroup = 32 rows of the actor's trunk and the mu head, built from the pieces above.  No env_mlp, no
// critic, no sampling: the caller gives the normalised observation and the latent as two row-major tensors, the kernel
// writes mu -- and, with STORE, the three post-tanh activations of the live rows for the data-gradient chain back into the
// latent (teacher_actor_latent_backward).  Same LDS carve-up as k_policy_fwd (the env_mlp's W3 slot stays unused), same
// trunk calls, so the trunk's bits are those of the per-layer launches and of k_policy_fwd.
struct ActorLatentArgs {
  const float* obs_n; const float* latent;             // [rows][obs], [rows][L]; rows need no alignment (plain loads)
  int rows, obs, L, act;
  const float* w1p;                                    // [512][32] zero-padded first layer of the ACTOR (k_pad_w1)
  const float *tb1, *tW2, *tb2, *tW3, *tb3, *Wmu, *bmu;
  float* mu;                                           // [rows][act]
  float *h1 = nullptr, *h2 = nullptr, *h3 = nullptr;   // STORE: [rows][512 | 256 | 128], rows ldh floats apart
  int ldh = 0;
};

static inline bool actor_latent_shape_ok(int obs, int L, int act, int nl, const int* u) {
  return nl == 3 && u[0] == 512 && u[1] == 256 && u[2] == 128 && obs >= 1 && L >= 1 && obs + L <= 32 && act >= 1 && act <= 7;
}

template <bool STORE>
__global__ __launch_bounds__(PF_THREADS) void k_actor_latent(const ActorLatentArgs a) {
  extern __shared__ __attribute__((aligned(1024))) float smem[];
  float* P = smem;
  float* Q = P + PF_P;
  float* ring0 = Q + PF_Q;
  float* hws = ring0 + PF_RING + 8 * 128;   // [8][128] head rows: mu 0 .. act - 1, zeros behind
  float* part = hws + 8 * 128;              // [2][32][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = (int)blockIdx.x * PF_ROWS;
  PfWave w;
  w.ring = ring0 + wave * (PF_NS * PF_CH);
  w.lane = lane; w.wave = wave; w.l31 = lane & 31; w.h = lane >> 5;
  pf_img_bases(w.l31, w.h, w.ib);
  w.aoff = w.l31 * 32; w.asw = (w.l31 >> 1) & 7;
  w.boff = w.l31 * 16; w.bsw = (w.l31 >> 2) & 3;
  const int c31 = 32 * wave + w.l31;
  float bt1[2] = {a.tb1[c31], a.tb1[256 + c31]};
  float bt2[1] = {a.tb2[c31]};
  float bt3[1] = {a.tb3[min(c31, 127)]};
  float hwv[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int e = tid + PF_THREADS * i;                               // 0 .. 1023
    const int r = e >> 7, k = e & 127;
    hwv[i] = r < a.act ? a.Wmu[r * 128 + k] : 0.f;
  }
  // ---- xcat = [obs_n | latent | 0] as ONE image in P, written whole; rows >= rows read row rows - 1
  {
    const int xrow = tid >> 4, xc = 2 * (tid & 15);
    const long long grow = min(m0 + xrow, a.rows - 1);
    const int sw = (xrow >> 1) & 7;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int c = xc + q;
      float v = 0.f;
      if (c < a.obs) v = a.obs_n[grow * a.obs + c];
      else if (c < a.obs + a.L) v = a.latent[grow * a.L + (c - a.obs)];
      P[xrow * 32 + (((c >> 2) ^ sw) << 2) + (c & 3)] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) hws[tid + PF_THREADS * i] = hwv[i];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // ---- the actor trunk: 32 -> 512 (P -> Q), 512 -> 256 (Q -> P), 256 -> 128 (P -> Q)
  pf_layer<32, 512, 2, 8, PF_NS, STORE>(w, P, a.w1p, 32, bt1, Q, a.h1, a.ldh, m0, a.rows);
  __syncthreads();
  pf_layer<512, 256, 1, 8, PF_NS, STORE>(w, Q, a.tW2, 512, bt2, P, a.h2, a.ldh, m0, a.rows);
  __syncthreads();
  pf_layer<256, 128, 1, 8, PF_NS, STORE>(w, P, a.tW3, 256, bt3, Q, a.h3, a.ldh, m0, a.rows);
  __syncthreads();
  pf_dot8(Q, hws, part, tid);
  __syncthreads();
  const int row = tid & 31, q = tid >> 5, grow = m0 + row;
  if (tid < 256 && q < a.act && grow < a.rows)
    a.mu[(long long)grow * a.act + q] = (part[row * 8 + q] + part[(32 + row) * 8 + q]) + a.bmu[q];
}

template <bool STORE>
static hipError_t actor_latent_launch(const ActorLatentArgs& a, int blocks, hipStream_t s) {
  void (*kern)(const ActorLatentArgs) = k_actor_latent<STORE>;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * PF_LDS_FLOATS));
    if (e != hipSuccess) return e;
    attr = true;
  }
  IGI_LAUNCH(kern, dim3(blocks), dim3(PF_THREADS), sizeof(float) * PF_LDS_FLOATS, s, a);
  return hipGetLastError();
}

// hipErrorInvalidValue: an operand the DMA rings cannot take (alignment) -- the caller runs the per-layer launches
static hipError_t actor_latent_forward(const ActorLatentArgs& a, hipStream_t s) {
  const bool store = a.h1 != nullptr;
  if (a.rows < 1 || !a.obs_n || !a.latent || !a.mu || a.obs < 1 || a.L < 1 || a.obs + a.L > 32 || a.act < 1 || a.act > 7 ||
      !aligned16(a.w1p) || !aligned16(a.tW2) || !aligned16(a.tW3) || (store && (!a.h2 || !a.h3 || a.ldh < 512)))
    return hipErrorInvalidValue;
  const int blocks = (a.rows + PF_ROWS - 1) / PF_ROWS;
  const double macs = (a.obs + a.L) * 512.0 + 512.0 * 256 + 256.0 * 128 + 128.0 * a.act;
  const double wbytes = 4.0 * (512.0 * 32 + 512.0 * 256 + 256.0 * 128 + 128.0 * a.act + 512 + 256 + 128 + a.act);
  ProfScope ps(PC_ACTOR_LATENT, s, 2.0 * macs * a.rows,
               4.0 * a.rows * (a.obs + a.L + a.act + (store ? 512.0 + 256 + 128 : 0.0)) + wbytes);
  return store ? actor_latent_launch<true>(a, blocks, s) : actor_latent_launch<false>(a, blocks, s);
}

template <int CT, bool VEC>
static hipError_t policy_launch(const PolicyFwdArgs& a, int blocks, hipStream_t s) {
  void (*kern)(const PolicyFwdArgs) = k_policy_fwd<CT, VEC>;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * PF_LDS_FLOATS));
    if (e != hipSuccess) return e;
    attr = true;
  }
  IGI_LAUNCH(kern, dim3(2 * blocks), dim3(PF_THREADS), sizeof(float) * PF_LDS_FLOATS, s, a);
  return hipGetLastError();
}

// mode: PF_NO_CONTACTS | PF_CONTACTS | PF_ONLY_CONTACT
static hipError_t policy_forward(const PolicyFwdArgs& a, hipStream_t s, int mode = PF_NO_CONTACTS) {
  if (a.rows < 1 || !aligned16(a.priv) || !aligned16(a.xcat) || (a.ldp & 3) || a.ldp < 64 || a.ldx != 32 || !aligned16(a.eW1) ||
      !aligned16(a.eW2) || !aligned16(a.w1p) || !aligned16(a.tW2) || !aligned16(a.tW3) || (a.ac_block & 3))
    return hipErrorInvalidValue;
  const int blocks = (a.rows + PF_ROWS - 1) / PF_ROWS;
  const int lat = mode == PF_ONLY_CONTACT ? 0 : 8, emb = mode == PF_NO_CONTACTS ? 0 : a.ctE;
  if (mode != PF_NO_CONTACTS && (!a.ct || a.ctP < 1 || emb < 1 || a.xw != a.obs + lat + emb || a.xw > 32 || !a.cW1 || !a.cb1 || !a.cW2 || !a.cb2))
    return hipErrorInvalidValue;
  const double env_macs = mode == PF_ONLY_CONTACT ? 0.0 : 64.0 * 256 + 256.0 * 128 + 128.0 * 8;
  const double ct_macs = mode == PF_NO_CONTACTS ? 0.0 : 2.0 * CT_HID * ((double)a.ctP + emb);   // both nets' workgroups encode
  const double macs = env_macs + ct_macs + 2.0 * ((a.obs + lat + emb) * 512.0 + 512.0 * 256 + 256.0 * 128) + 128.0 * (a.act + 1);
  const double ct_bytes = mode == PF_NO_CONTACTS ? 0.0 : 4.0 * a.rows * a.ctP * (a.ct_t ? 2.0 : 1.0) + 4.0 * CT_HID * ((double)a.ctP + emb);
  ProfScope ps(PC_POLICY_FWD, s, 2.0 * macs * a.rows, 4.0 * a.rows * (64.0 + 32 + 4 * a.act + 3) + 4.0 * 404501 + ct_bytes);
  if (mode == PF_NO_CONTACTS) return policy_launch<PF_NO_CONTACTS, false>(a, blocks, s);
  // float4 loads and stores of the contact rows: every row 16-byte aligned, in the input, the arena slot and W1
  const bool vec = (a.ctP & 3) == 0 && aligned16(a.ct) && aligned16(a.cW1) && (!a.ct_t || aligned16(a.ct_t));
  if (mode == PF_CONTACTS) return vec ? policy_launch<PF_CONTACTS, true>(a, blocks, s) : policy_launch<PF_CONTACTS, false>(a, blocks, s);
  return vec ? policy_launch<PF_ONLY_CONTACT, true>(a, blocks, s) : policy_launch<PF_ONLY_CONTACT, false>(a, blocks, s);
}

}  // namespace igi
