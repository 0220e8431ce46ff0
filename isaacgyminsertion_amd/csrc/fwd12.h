// Training forward of env_mlp AND the first trunk layer of both nets as ONE persistent launch (models_split.py:185-232:
// priv -> Linear+Tanh x 3 -> latent; [obs | latent] -> Linear(23 -> 512)+Tanh for actor and critic), for the reference's
// layer sizes.  VERDICT round 5, item 1(b): k_env_fwd (24 us at 0.43 of the fp32 matrix peak) + the first trunk layer's own
// launch (19 us, 0.25: one k-tile, 67 MB of tanh outputs) -> one launch.
//
// Round 2 tried this twice and got the SUM of the two launches both times: a workgroup ran env_mlp, then the first trunk
// layer of its 64 rows, then stored -- phases of one workgroup, with every store in front of a weight request holding
// that request's vmcnt wait until the store was acknowledged.  What is different here (the structure of the rollout
// kernel, policy_fwd.h, which reached 0.64 of the matrix peak on the whole network at 32 rows per workgroup):
//   * ROLES.  Waves 0-7 (two per SIMD) compute: their only memory traffic is the wave-private LDS-DMA weight rings of
//     policy_fwd.h, so their counted vmcnt waits see weight requests and nothing else.  Waves 8-11 are the data engine: they
//     copy finished operand images from LDS to global memory (e1, e2, the latent columns of xcat, the 2 x 512 first-layer
//     outputs) while the compute waves are in the next layer, bring the NEXT row block's input and observation columns in by
//     LDS-DMA (waited for with a counted vmcnt that leaves the younger stores in flight), build the [obs | latent] operand
//     image, and never wait for a store's acknowledgement (raw s_barrier + lgkmcnt only).
//   * PERSISTENT.  A workgroup walks row blocks b, b + grid, ...: the stores of a block's last unit and the next block's
//     input DMA overlap the first layer of the next block.
//   * The first trunk layer runs as four units (net, column half) of 32 x 256 outputs that ping-pong between two 32 KB
//     buffers (the regions of the dead env_mlp activations): unit u is stored while unit u + 1 is computed.
//   * 768 threads: eight compute waves (two per SIMD: one wave's epilogue, chunk requests and waits under the other's MFMAs)
//     and four data-engine waves.
// Arithmetic: the GEMM kernels' k order in every MFMA layer, the latent head as gemm_dma_head_kernel's / k_env_fwd's fmaf
// chain (pairs k, k + 4 inside every group of eight): outputs bit-identical to the launches it replaces.
#pragma once
#include "policy_fwd.h"

namespace igi {

struct Fwd12Args {
  const float* priv; int ldp;            // [M][64] normalised privileged input
  float* xcat; int ldx;                  // [M][32]: in: normalised obs in columns 0 .. obs - 1 (zeros behind obs + 8); out: latent in obs .. obs + 7
  int M, obs;
  const float *eW1, *eb1, *eW2, *eb2, *eW3, *eb3;
  const float* w1p;                      // [2][512][32] zero-padded first trunk layer
  const float* tb1; long long ac_block;  // first trunk layer's bias (actor; critic = + ac_block)
  float* e1; int lde1;                   // [M][256]
  float* e2; int lde2;                   // [M][128]
  float* h1; int ldh; long long sH;      // [2][M][512], net stride sH floats
};

constexpr int F12_NW = 8;                               // compute waves (two per SIMD), + 4 data-engine waves = 768 threads
constexpr int F12_NS = 3;                               // ring depth of a compute wave (two chunks in flight, as policy_fwd.h)
constexpr int F12_THREADS = 64 * (F12_NW + 4);
// (first version: FOUR compute waves, one per SIMD, six-deep rings -- 42.5 - 45 us, the sum of the two launches it replaces
//  once more: an in-order wave that is alone on its SIMD serialises its 20 k cycles of MFMA per row block with its own 11 k
//  of tanh epilogue, chunk requests, waits and eight barriers; profiles/r06_fwd12_ab.log)
constexpr int F12_RING = F12_NW * F12_NS * PF_CH;       // 12288 floats
constexpr int F12_PRIV = 2 * PF_IMG;                    // one input block (two images)
constexpr int F12_Q = 8 * PF_IMG;                       // region Q: env layer 2 (4 images), odd units of the first trunk layer (8)
// P | Q | ring | priv x 2 | raw xcat rows x 2 | xcat image | W3 | lat
constexpr int F12_LDS_FLOATS = PF_P + F12_Q + F12_RING + 2 * F12_PRIV + 2 * PF_IMG + PF_IMG + 8 * 128 + 32 * 8;
static_assert(F12_LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");

// The data engine's copy of NIMG [32][32] operand images (k-contiguous, swizzled) to global rows: thread st (0 .. 255) moves
// 16-byte pieces st, st + 256, ... (NIMG store instructions per thread); eight consecutive threads cover one 128-byte row
// segment.  Rows >= rows_ok are skipped (only the last row block of a ragged batch has any).
template <int NIMG>
__device__ __forceinline__ void f12_store_images(const float* __restrict__ img, float* __restrict__ g, long long ldg, int rows_ok, int st) {
#pragma unroll
  for (int i = 0; i < NIMG; ++i) {
    const int rem = st, r = rem >> 3, slot = rem & 7;     // piece st of image i
    const int p = slot ^ ((r >> 1) & 7);
    const f32x4 v = *reinterpret_cast<const f32x4*>(img + i * PF_IMG + r * 32 + slot * 4);
    if (r < rows_ok) *reinterpret_cast<f32x4*>(g + (long long)r * ldg + 32 * i + 4 * p) = v;
  }
}

// raw workgroup barrier: LDS traffic of this wave settled, global stores NOT waited for
__device__ __forceinline__ void f12_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(F12_THREADS) void k_fwd12(const Fwd12Args a) {
  extern __shared__ __attribute__((aligned(1024))) float smem[];
  float* P = smem;
  float* Q = P + PF_P;
  float* ring0 = Q + F12_Q;
  float* privb = ring0 + F12_RING;        // [2][2 images]
  float* xsb = privb + 2 * F12_PRIV;      // [2][32 rows][32]: raw xcat rows of a block
  float* X = xsb + 2 * PF_IMG;            // the xcat operand image
  float* w3s = X + PF_IMG;                // [8][128]
  float* lat = w3s + 8 * 128;             // [32][8]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool compute = wave < F12_NW;
  const int dw = compute ? wave : wave - F12_NW;     // number of the wave inside its role
  const int nblocks = (a.M + PF_ROWS - 1) / PF_ROWS;
  PfWave w;
  w.ring = ring0 + dw * (F12_NS * PF_CH);
  w.lane = lane; w.wave = wave; w.l31 = lane & 31; w.h = lane >> 5;
  pf_img_bases(w.l31, w.h, w.ib);
  w.aoff = w.l31 * 32; w.asw = (w.l31 >> 1) & 7;
  w.boff = w.l31 * 16; w.bsw = (w.l31 >> 2) & 3;
  const int st = tid - 64 * F12_NW;       // data-engine thread number (the last four waves: 0 .. 255)

  // data engine: the input block of row block `b` (two swizzled images = eight 1 KB pieces, two per wave) and its 32 raw xcat
  // rows (4 KB, one piece per wave) into buffer `buf`: three LDS-DMA instructions per wave
  auto issue_inputs = [&](int b, int buf) {
    const int m0 = b * PF_ROWS;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int piece = dw + 4 * q, k = piece >> 2, i = piece & 3;
      const int m = 8 * i + (lane >> 3);
      const int row = min(m0 + m, a.M - 1);
      dma16(a.priv + (long long)row * a.ldp + k * 32 + 4 * ((lane & 7) ^ ((m >> 1) & 7)), privb + buf * F12_PRIV + k * PF_IMG + 256 * i);
    }
    const int xr = 8 * dw + (lane >> 3);
    dma16(a.xcat + (long long)min(m0 + xr, a.M - 1) * a.ldx + 4 * (lane & 7), xsb + buf * PF_IMG + 256 * dw);
  };

  // ---- prologue: biases of this wave's tiles, the last env layer's weights, the first block's inputs
  const int c31 = 32 * (wave & 7) + w.l31;
  float be1[1] = {a.eb1[c31]};
  float be2[1] = {a.eb2[c31 & 127]};
  float bt1[4][1];
#pragma unroll
  for (int u = 0; u < 4; ++u) bt1[u][0] = a.tb1[(u >> 1) * a.ac_block + 256 * (u & 1) + c31];
  const float b3 = a.eb3[(tid >> 5) & 7];
  int b = blockIdx.x;
  if (!compute && b < nblocks) issue_inputs(b, 0);
  for (int e = tid; e < 8 * 128; e += F12_THREADS) w3s[e] = a.eW3[e];
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f12_barrier();

  int it = 0;
  for (; b < nblocks; b += gridDim.x, ++it) {
    const int m0 = b * PF_ROWS;
    const int rows_ok = min(PF_ROWS, a.M - m0);
    const bool more = b + (int)gridDim.x < nblocks;
    // ---- layer 1: 64 -> 256 (input block -> P)
    if (compute) pf_layer<64, 256, 1, F12_NW, F12_NS>(w, privb + (it & 1) * F12_PRIV, a.eW1, 64, be1, P);
    f12_barrier();                                                     // R1: e1 complete
    // ---- layer 2: 256 -> 128 (P -> Q[0 .. 4 images]) | store e1
    if (compute) pf_layer<256, 128, 1, F12_NW, F12_NS>(w, P, a.eW2, 256, be2, Q);
    else f12_store_images<8>(P, a.e1 + (long long)m0 * a.lde1, a.lde1, rows_ok, st);
    f12_barrier();                                                     // R2: e2 complete
    // ---- layer 3: the 8-wide latent, one fmaf chain per (row, output) in the GEMM head's order | store e2
    if (tid < 256) {
      const int row = tid & 31, out = tid >> 5;
      const float* xr = Q + row * 32;
      const float* wr = w3s + out * 128;
      const int sw = (row >> 1) & 7;
      float acc = 0.f;
#pragma unroll 4
      for (int c8 = 0; c8 < 128; c8 += 8) {
        const float* im = xr + (c8 >> 5) * PF_IMG;
        const int p0 = (c8 & 31) >> 2;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(im + ((p0 ^ sw) << 2)), x1 = *reinterpret_cast<const f32x4*>(im + (((p0 + 1) ^ sw) << 2));
        const f32x4 u0 = *reinterpret_cast<const f32x4*>(wr + c8), u1 = *reinterpret_cast<const f32x4*>(wr + c8 + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc = fmaf(x0[j], u0[j], acc);
          acc = fmaf(x1[j], u1[j], acc);
        }
      }
      lat[row * 8 + out] = fast_tanh(acc + b3);
    } else if (!compute) {
      f12_store_images<4>(Q, a.e2 + (long long)m0 * a.lde2, a.lde2, rows_ok, st);
    }
    f12_barrier();                                                     // R3: latent complete
    // ---- data engine: xcat image = [obs_n | latent | 0], latent columns to global, then the NEXT block's inputs
    if (!compute) {
      const int xrow = st >> 3, xc = 4 * (st & 7), sw = (xrow >> 1) & 7;
      f32x4 v = *reinterpret_cast<const f32x4*>(xsb + (it & 1) * PF_IMG + xrow * 32 + xc);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = xc + q;
        if (c >= a.obs && c < a.obs + 8) v[q] = lat[xrow * 8 + (c - a.obs)];
      }
      *reinterpret_cast<f32x4*>(X + xrow * 32 + (((xc >> 2) ^ sw) << 2)) = v;
      const int j = st & 7;
      if (xrow < rows_ok) a.xcat[(long long)(m0 + xrow) * a.ldx + a.obs + j] = lat[xrow * 8 + j];
    }
    f12_barrier();                                                     // R4: xcat image complete
    if (!compute && more) issue_inputs(b + gridDim.x, (it + 1) & 1);
    // ---- first trunk layer: units u = (net, column half), 32 x 256 outputs each, ping-pong between the halves of Q
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (compute) {
        pf_layer<32, 256, 1, F12_NW, F12_NS>(w, X, a.w1p + (long long)((u >> 1) * 512 + 256 * (u & 1)) * 32, 32, bt1[u], (u & 1) ? Q : P);
      } else if (u > 0) {
        const int v = u - 1;
        f12_store_images<8>((v & 1) ? Q : P, a.h1 + (v >> 1) * a.sH + (long long)m0 * a.ldh + 256 * (v & 1), a.ldh, rows_ok, st);
      }
      if (u == 3 && !compute && more) {
        // the next block's inputs (requested behind R4) have landed once only the 3 x 8 stores of units 0 .. 2 issued since are
        // still in flight -- a row block with a successor is a whole one, so every one of those stores was issued
        asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
      }
      f12_barrier();                                                   // R5 .. R8
    }
    if (!compute) f12_store_images<8>(Q, a.h1 + a.sH + (long long)m0 * a.ldh + 256, a.ldh, rows_ok, st);
    // (the next block's layer 1 writes P -- unit 2's buffer, stored before R8 -- and reads the other input buffer; Q is next
    //  written by that block's layer 2, behind its R1: the data engine's reads above are done by then)
  }
}

static inline bool fwd12_supported(int K1, int N1, int N2, int N3, int obs, int xld, int u0) {
  return K1 == 64 && N1 == 256 && N2 == 128 && N3 == 8 && obs >= 1 && obs + 8 <= 32 && xld == 32 && u0 == 512;
}

static hipError_t fwd12_forward(const Fwd12Args& a, hipStream_t s) {
  if (a.M < 1 || !aligned16(a.priv) || !aligned16(a.xcat) || (a.ldp & 3) || a.ldp < 64 || a.ldx != 32 || !aligned16(a.eW1) ||
      !aligned16(a.eW2) || !aligned16(a.eW3) || !aligned16(a.w1p) || !aligned16(a.e1) || !aligned16(a.e2) || !aligned16(a.h1) || (a.lde1 & 3) ||
      (a.lde2 & 3) || (a.ldh & 3) || (a.sH & 3) || a.lde1 < 256 || a.lde2 < 128 || a.ldh < 512)
    return hipErrorInvalidValue;
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fwd12, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(float) * F12_LDS_FLOATS));
    if (e != hipSuccess) return e;
    attr = true;
  }
  const int nblocks = (a.M + PF_ROWS - 1) / PF_ROWS;
  const int grid = nblocks < 256 ? nblocks : 256;
  const double fl = 2.0 * a.M * (64.0 * 256 + 256.0 * 128 + 128.0 * 8 + 2.0 * (a.obs + 8) * 512.0);
  const double by = 4.0 * a.M * (64.0 + a.obs + 256 + 128 + 8 + 1024) + 4.0 * (64.0 * 256 + 256.0 * 128 + 2 * 512.0 * 32);
  ProfScope ps(PC_FWD12, s, fl, by);
  IGI_LAUNCH(k_fwd12, dim3(grid), dim3(F12_THREADS), sizeof(float) * F12_LDS_FLOATS, s, a);
  return hipGetLastError();
}

}  // namespace igi
