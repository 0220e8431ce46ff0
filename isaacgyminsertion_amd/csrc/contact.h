// Ground-truth contact encoder of the teacher (models_split.py:41-55, ContactAE.contact_enc_mlp):
//   H = relu(C . W1^T + b1)   (rows x 32),   E = tanh(H . W2^T + b2)   (rows x emb)
// and its backward from d(pre-tanh) of the embedding.  exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), deterministic.
//
// C is the time-major contacts arena (T, N, P) that play_steps fills; minibatch row i is sample b = perm[start + i]
// (env-major id b = n*T + t, experience.py:39-46), read in place at element t*N + n -- like k_gather_normalize.
// Without perm, row i is arena row start + i (T = 1).
//
// Forward (k_contact_fwd): one wave per 32 rows.  The first product is formed transposed, H^T = W1 . C^T, so that the
// accumulator tile has the row on the lane and the 32 hidden units in its registers; the second product sums over the
// hidden units = over the registers, so the tile is the B operand of E^T = W2 . H^T as it stands (no lane movement).
// H is stored ([rows][32], 128 B per row) for the backward's ReLU mask and dW2.
//
// Backward (k_contact_bwd): one row block of CT_BWD_ROWS rows per grid column x; its small products (dH, dW2, db2,
// db1) in LDS with fixed-order sums, then dW1 = dH^T . C over the block's rows on the matrix pipe, one 32-column slice
// of C per wave (grid row y picks the slices), C read straight from the arena once per backward.  Every block writes
// one partial record [dW1 32*P | db1 32 | dW2 emb*32 | db2 emb]; the records are summed in index order by the caller
// (k_slab_reduce), so the gradient does not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prof.h"

namespace igi {

constexpr int CT_HID = 32;          // contact_enc_mlp hidden width (models_split.py:46)
constexpr int CT_MAX_EMB = 32;      // embedding width: one 32-row MFMA tile
constexpr int CT_FWD_WAVES = 2;     // 32 rows per wave
constexpr int CT_BWD_ROWS = 128;    // rows per backward block = per partial record
constexpr int CT_BWD_LD = CT_HID + 1;
typedef float ct_f32x16 __attribute__((ext_vector_type(16)));

struct ContactArgs {
  const float* C = nullptr;      // arena, rows of P floats
  const int64_t* perm = nullptr; // nullable
  long long start = 0;
  int rows = 0, N = 1, T = 1, P = 0, E = 0;
  const float *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;   // (32,P) (32) (E,32) (E)
  float* H = nullptr;            // [rows][32] relu output
  float* out = nullptr; int ldo = 0;   // embedding, row pitch ldo
  const float* dZ = nullptr; int ldz = 0;   // backward: d(pre-tanh) of the embedding, row pitch ldz
  float* part = nullptr; long long rec = 0; // backward: partial records
};

static inline long long ct_rec_floats(int P, int E) { return ((long long)CT_HID * P + CT_HID + (long long)E * CT_HID + E + 3) & ~3LL; }
static inline int ct_bwd_blocks(int rows) { return (rows + CT_BWD_ROWS - 1) / CT_BWD_ROWS; }
static inline size_t ct_bwd_lds() { return sizeof(float) * 3 * CT_BWD_ROWS * CT_BWD_LD + sizeof(long long) * CT_BWD_ROWS; }

__device__ __forceinline__ long long ct_arena_row(const ContactArgs& a, int i) {
  const long long b = a.perm ? a.perm[a.start + i] : a.start + i;
  const long long n = b / a.T;
  return (b - n * a.T) * a.N + n;
}

// accumulator register g of a 32x32 tile <-> its row: (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5)
__device__ __forceinline__ int ct_acc_row(int g, int h) { return (g & 3) + 8 * (g >> 2) + 4 * h; }

template <bool VEC>
__global__ __launch_bounds__(64 * CT_FWD_WAVES) void k_contact_fwd(const ContactArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int row0 = (blockIdx.x * CT_FWD_WAVES + wave) * 32;
  if (row0 >= a.rows) return;
  const int row = row0 + r;
  const bool valid = row < a.rows;
  const int P = a.P;
  const float* crow = a.C + (valid ? ct_arena_row(a, row) : 0LL) * P;
  const float* wrow = a.W1 + (long long)r * P;   // hidden unit r
  ct_f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  // k-chunks of 32: lane half h takes columns kb + 16h .. +15 of its row of C and of W1 row r (same k per MFMA step)
  for (int kb = 0; kb < P; kb += 32) {
    const int k0 = kb + 16 * h;
    float cv[16], wv[16];
    if (VEC && k0 + 16 <= P) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 c4 = valid ? *reinterpret_cast<const float4*>(crow + k0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 w4 = *reinterpret_cast<const float4*>(wrow + k0 + 4 * q);
        cv[4 * q] = c4.x; cv[4 * q + 1] = c4.y; cv[4 * q + 2] = c4.z; cv[4 * q + 3] = c4.w;
        wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
      }
    } else {
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k = k0 + u;
        cv[u] = (valid && k < P) ? crow[k] : 0.f;
        wv[u] = (k < P) ? wrow[k] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], cv[u], acc, 0, 0, 0);
  }
  // acc[g] = Z1[row][j], j = ct_acc_row(g, h)
  float hv[16];
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const float z = acc[g] + a.b1[ct_acc_row(g, h)];
    hv[g] = z > 0.f ? z : 0.f;
  }
  if (valid) {
    float* hr = a.H + (long long)row * CT_HID;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      *reinterpret_cast<float4*>(hr + 8 * q + 4 * h) = make_float4(hv[4 * q], hv[4 * q + 1], hv[4 * q + 2], hv[4 * q + 3]);
  }
  // E^T = W2 . H^T: MFMA step g sums over hidden unit j = ct_acc_row(g, h), which lane half h holds in register g
  const int e_lane = r;
  ct_f32x16 acc2;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc2[g] = 0.f;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    const float w = e_lane < a.E ? a.W2[e_lane * CT_HID + ct_acc_row(g, h)] : 0.f;
    acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(w, hv[g], acc2, 0, 0, 0);
  }
  if (valid) {
    float* o = a.out + (long long)row * a.ldo;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int e = ct_acc_row(g, h);
      if (e < a.E) o[e] = tanhf(acc2[g] + a.b2[e]);
    }
  }
}

__global__ __launch_bounds__(256) void k_contact_bwd(const ContactArgs a) {
  extern __shared__ float ct_lds[];
  float* sH = ct_lds;                              // [rows][33] H
  float* sD = sH + CT_BWD_ROWS * CT_BWD_LD;        // [rows][33] dH (masked)
  float* sZ = sD + CT_BWD_ROWS * CT_BWD_LD;        // [rows][33] dZ2
  long long* sRow = reinterpret_cast<long long*>(sZ + CT_BWD_ROWS * CT_BWD_LD);
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * CT_BWD_ROWS;
  const int nrows = min(CT_BWD_ROWS, a.rows - r0);
  const int E = a.E, P = a.P;
  // ---- per row: dH = (dZ2 . W2) masked by H > 0
  for (int t = tid; t < CT_BWD_ROWS; t += blockDim.x) {
    float hv[CT_HID];
    float* z = sZ + t * CT_BWD_LD;
    if (t < nrows) {
      const int row = r0 + t;
      sRow[t] = ct_arena_row(a, row);
      const float4* hr = reinterpret_cast<const float4*>(a.H + (long long)row * CT_HID);
#pragma unroll
      for (int q = 0; q < CT_HID / 4; ++q) {
        const float4 v = hr[q];
        hv[4 * q] = v.x; hv[4 * q + 1] = v.y; hv[4 * q + 2] = v.z; hv[4 * q + 3] = v.w;
      }
      for (int e = 0; e < E; ++e) z[e] = a.dZ[(long long)row * a.ldz + e];
    } else {
      sRow[t] = -1;
#pragma unroll
      for (int j = 0; j < CT_HID; ++j) hv[j] = 0.f;
      for (int e = 0; e < E; ++e) z[e] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < CT_HID; ++j) {
      float d = 0.f;
      for (int e = 0; e < E; ++e) d = fmaf(z[e], a.W2[e * CT_HID + j], d);
      sH[t * CT_BWD_LD + j] = hv[j];
      sD[t * CT_BWD_LD + j] = hv[j] > 0.f ? d : 0.f;
    }
  }
  __syncthreads();
  float* rec = a.part + (long long)blockIdx.x * a.rec;
  // ---- the small sums (grid row 0 only): db1, dW2, db2 over the block's rows in row order
  if (blockIdx.y == 0) {
    float* db1 = rec + (long long)CT_HID * P;
    float* dW2 = db1 + CT_HID;
    float* db2 = dW2 + E * CT_HID;
    for (int i = tid; i < CT_HID + E * CT_HID + E; i += blockDim.x) {
      float s = 0.f;
      if (i < CT_HID) {
        for (int t = 0; t < CT_BWD_ROWS; ++t) s += sD[t * CT_BWD_LD + i];
        db1[i] = s;
      } else if (i < CT_HID + E * CT_HID) {
        const int e = (i - CT_HID) / CT_HID, j = (i - CT_HID) % CT_HID;
        for (int t = 0; t < CT_BWD_ROWS; ++t) s = fmaf(sZ[t * CT_BWD_LD + e], sH[t * CT_BWD_LD + j], s);
        dW2[e * CT_HID + j] = s;
      } else {
        const int e = i - CT_HID - E * CT_HID;
        for (int t = 0; t < CT_BWD_ROWS; ++t) s += sZ[t * CT_BWD_LD + e];
        db2[e] = s;
      }
    }
  }
  // ---- dW1[j][k] = sum_rows dH[row][j] C[row][k]: wave w of grid row y takes the 32-column slice cb = 4y + w
  const int lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
  const int cb = blockIdx.y * (blockDim.x >> 6) + wave;
  const int col = cb * 32 + c;
  if (cb * 32 >= P) return;
  const bool cval = col < P;
  ct_f32x16 acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) acc[g] = 0.f;
  for (int t0 = 0; t0 < CT_BWD_ROWS; t0 += 32) {
    float bv[16], av[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int t = t0 + 2 * u + h;
      const long long ar = sRow[t];
      bv[u] = (ar >= 0 && cval) ? a.C[ar * P + col] : 0.f;
      av[u] = sD[t * CT_BWD_LD + c];
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
  }
  if (cval) {
#pragma unroll
    for (int g = 0; g < 16; ++g) rec[(long long)ct_acc_row(g, h) * P + col] = acc[g];
  }
}

// host launchers (pointers, pitches and sizes checked by the callers)
static inline hipError_t contact_forward(const ContactArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.P < 1 || a.E < 1 || a.E > CT_MAX_EMB) return hipErrorInvalidValue;
  const int rows_pb = 32 * CT_FWD_WAVES;
  const dim3 grid((a.rows + rows_pb - 1) / rows_pb);
  const bool vec = (a.P & 3) == 0 && (reinterpret_cast<uintptr_t>(a.C) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.W1) & 15) == 0;
  ProfScope ps(PC_OTHER, s, 2.0 * a.rows * CT_HID * ((double)a.P + a.E), 4.0 * a.rows * ((double)a.P + CT_HID + a.E));
  if (vec) IGI_LAUNCH(k_contact_fwd<true>, grid, dim3(64 * CT_FWD_WAVES), 0, s, a);
  else IGI_LAUNCH(k_contact_fwd<false>, grid, dim3(64 * CT_FWD_WAVES), 0, s, a);
  return hipGetLastError();
}

static inline hipError_t contact_backward(const ContactArgs& a, hipStream_t s) {
  if (a.rows <= 0) return hipSuccess;
  if (a.P < 1 || a.E < 1 || a.E > CT_MAX_EMB) return hipErrorInvalidValue;
  const int slices = (a.P + 31) / 32;
  const dim3 grid(ct_bwd_blocks(a.rows), (slices + 3) / 4);
  ProfScope ps(PC_OTHER, s, 2.0 * a.rows * CT_HID * ((double)a.P + 2.0 * a.E), 4.0 * a.rows * ((double)a.P + CT_HID + a.E));
  IGI_LAUNCH(k_contact_bwd, grid, dim3(256), ct_bwd_lds(), s, a);
  return hipGetLastError();
}

}  // namespace igi
